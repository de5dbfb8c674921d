// YUV 4:2:0 video-frame records (input pixel formats "i420" / "nv12"): the integer conversion to
// RGB, defined in gale/models/preprocess.py (YuvConvert) and implemented three times with the
// same bits - the numpy oracle there, the host twin here and the kernel (csrc/kernels/b64_yuv.hip).
//
// A frame of HS x WS pixels (both even) is B = HS*WS*3/2 bytes:
//     I420: Y[HS][WS], U[HS/2][WS/2], V[HS/2][WS/2]        NV12: Y[HS][WS], UV[HS/2][WS/2][2]
// Pixel (y, x) takes Y[y][x] and the chroma sample (y >> 1, x >> 1) (nearest neighbour). With
// yo = 16 (limited range) or 0 (full), in signed 32-bit arithmetic, >> the arithmetic shift:
//     R = clamp((cy (Y - yo)                  + crv (V - 128) + 2^19) >> 20, 0, 255)
//     G = clamp((cy (Y - yo) + cgu (U - 128) + cgv (V - 128) + 2^19) >> 20, 0, 255)
//     B = clamp((cy (Y - yo) + cbu (U - 128)                  + 2^19) >> 20, 0, 255)
// The coefficients are the exact rationals of the matrix times 2^20, rounded half to even; the
// largest accumulator magnitude over every (Y, U, V) and table is 573 636 921 < 2^31.
// No HIP in this header: the sanitizer programs of the host codec include it.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gale {

enum YuvFormat : int { YUV_NONE = 0, YUV_I420 = 1, YUV_NV12 = 2 };
enum YuvMatrix : int { YUV_BT601 = 0, YUV_BT709 = 1 };
enum YuvRange : int { YUV_LIMITED = 0, YUV_FULL = 1 };

struct YuvCoeffs {
  int32_t cy = 1220945, crv = 1673555, cgu = -410793, cgv = -852458, cbu = 2115221;
  int32_t yo = 16;  // (the default: bt601, limited range)
};

// The table of (matrix, range); false for a value outside the enums.
inline bool yuv_coeffs(int matrix, int range, YuvCoeffs* k) {
  static const int32_t kTable[2][2][5] = {
      {{1220945, 1673555, -410793, -852458, 2115221},   // bt601 limited
       {1048576, 1470104, -360853, -748826, 1858077}},  // bt601 full
      {{1220945, 1879825, -223607, -558796, 2215014},   // bt709 limited
       {1048576, 1651297, -196424, -490864, 1945738}},  // bt709 full
  };
  if (matrix < 0 || matrix > 1 || range < 0 || range > 1) return false;
  const int32_t* t = kTable[matrix][range];
  k->cy = t[0], k->crv = t[1], k->cgu = t[2], k->cgv = t[3], k->cbu = t[4];
  k->yo = range == YUV_LIMITED ? 16 : 0;
  return true;
}

// Bytes of one frame (HS, WS even).
inline int64_t yuv420_bytes(int HS, int WS) { return (int64_t)HS * WS / 2 * 3; }

namespace codec {

inline uint8_t yuv_clamp8(int32_t acc) {
  const int32_t v = acc >> 20;
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

inline void yuv_pixel_rgb(const YuvCoeffs& k, int Y, int U, int V, uint8_t* rgb) {
  const int32_t yy = k.cy * (Y - k.yo) + (1 << 19), u = U - 128, v = V - 128;
  rgb[0] = yuv_clamp8(yy + k.crv * v);
  rgb[1] = yuv_clamp8(yy + k.cgu * u + k.cgv * v);
  rgb[2] = yuv_clamp8(yy + k.cbu * u);
}

// The host twin of the kernel's conversion: one frame's yuv420_bytes(HS, WS) bytes at src ->
// [HS][WS][3]. rgb (optional): the uint8 image. f32 (optional): the model-side floats,
// fmaf((float)RGB[c], a[c], b[c]) with the InputPrep coefficients, or (float)RGB[c] when a is
// null. false (nothing written) for odd or non-positive sizes or an unknown format.
inline bool yuv420_to_rgb_host(const uint8_t* src, int HS, int WS, int format, const YuvCoeffs& k,
                               uint8_t* rgb, float* f32, const float* a = nullptr,
                               const float* b = nullptr) {
  if (HS <= 0 || WS <= 0 || (HS & 1) || (WS & 1)) return false;
  if (format != YUV_I420 && format != YUV_NV12) return false;
  const size_t hw = (size_t)HS * WS, cw = (size_t)WS / 2;
  const uint8_t* const chroma = src + hw;
  for (int y = 0; y < HS; ++y)
    for (int x = 0; x < WS; ++x) {
      const size_t ci = (size_t)(y >> 1) * cw + (size_t)(x >> 1);
      const int U = format == YUV_NV12 ? chroma[2 * ci] : chroma[ci];
      const int V = format == YUV_NV12 ? chroma[2 * ci + 1] : chroma[hw / 4 + ci];
      uint8_t px[3];
      yuv_pixel_rgb(k, src[(size_t)y * WS + x], U, V, px);
      const size_t o = ((size_t)y * WS + x) * 3;
      for (int c = 0; c < 3; ++c) {
        if (rgb) rgb[o + c] = px[c];
        if (f32) f32[o + c] = a ? __builtin_fmaf((float)px[c], a[c], b[c]) : (float)px[c];
      }
    }
  return true;
}

}  // namespace codec
}  // namespace gale
