// Packed pixel formats of b64 records (input pixel formats "bgr24" / "rgba" / "bgra" / "gray"):
// the byte shuffle to interleaved RGB, defined in gale/models/preprocess.py (PixelUnpack) and
// implemented three times with the same bits - the numpy oracle there, the host twin here and the
// kernel (csrc/kernels/b64_packed.hip).
//
// An image of HS x WS pixels (any positive sizes) is B = HS*WS*P bytes, pixels in [HS][WS] order,
// P bytes per pixel:
//     bgr24  P = 3   B, G, R       RGB = (byte 2, byte 1, byte 0)
//     rgba   P = 4   R, G, B, A    RGB = (byte 0, byte 1, byte 2)    alpha ignored
//     bgra   P = 4   B, G, R, A    RGB = (byte 2, byte 1, byte 0)    alpha ignored
//     gray   P = 1   Y             RGB = (byte 0, byte 0, byte 0)
// Alpha is dropped, not composited and not un-premultiplied (PIL's convert("RGB")).
// No HIP in this header: the sanitizer programs of the host codec include it.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gale {

enum PackedFormat : int {
  PACKED_NONE = 0,
  PACKED_BGR24 = 1,
  PACKED_RGBA = 2,
  PACKED_BGRA = 3,
  PACKED_GRAY = 4
};

// Bytes per pixel; 0 for a value outside the enum (PACKED_NONE included).
constexpr int packed_bpp(int format) {
  return format == PACKED_BGR24                            ? 3
         : format == PACKED_RGBA || format == PACKED_BGRA  ? 4
         : format == PACKED_GRAY                           ? 1
                                                           : 0;
}

// Offset in a pixel's bytes of the byte that model channel c (0 = R, 1 = G, 2 = B) takes.
constexpr int packed_src_offset(int format, int c) {
  return format == PACKED_RGBA                              ? c
         : format == PACKED_BGR24 || format == PACKED_BGRA  ? 2 - c
                                                            : 0;
}

// Bytes of one image; 0 for a non-positive size or an unknown format.
inline int64_t packed_bytes(int HS, int WS, int format) {
  return HS <= 0 || WS <= 0 ? 0 : (int64_t)HS * WS * packed_bpp(format);
}

// The names of the configuration ("bgr24", ...); PACKED_NONE for anything else ("rgb" included).
inline int packed_format_of(const char* s) {
  static const char* const kNames[] = {"", "bgr24", "rgba", "bgra", "gray"};
  for (int f = PACKED_BGR24; f <= PACKED_GRAY; ++f) {
    const char *a = kNames[f], *b = s;
    while (*a && *a == *b) ++a, ++b;
    if (!*a && !*b) return f;
  }
  return PACKED_NONE;
}

namespace codec {

// The host twin of the kernel's unpack: one image's packed_bytes(HS, WS, format) bytes at src ->
// [HS][WS][3]. rgb (optional): the uint8 image. f32 (optional): the model-side floats,
// fmaf((float)RGB[c], a[c], b[c]) with the InputPrep coefficients (indexed by model channel), or
// (float)RGB[c] when a is null. false (nothing written) for non-positive sizes or an unknown
// format.
inline bool packed_to_rgb_host(const uint8_t* src, int HS, int WS, int format, uint8_t* rgb,
                               float* f32, const float* a = nullptr, const float* b = nullptr) {
  const int P = packed_bpp(format);
  if (HS <= 0 || WS <= 0 || P == 0) return false;
  const size_t hw = (size_t)HS * WS;
  for (size_t p = 0; p < hw; ++p)
    for (int c = 0; c < 3; ++c) {
      const uint8_t v = src[p * (size_t)P + (size_t)packed_src_offset(format, c)];
      if (rgb) rgb[3 * p + c] = v;
      if (f32) f32[3 * p + c] = a ? __builtin_fmaf((float)v, a[c], b[c]) : (float)v;
    }
  return true;
}

}  // namespace codec
}  // namespace gale
