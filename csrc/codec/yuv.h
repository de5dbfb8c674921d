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
//
// Packed 4:2:2 frames (input pixel formats "yuyv422" / "uyvy422"; kernel csrc/kernels/yuv422.hip):
// a frame of HS x WS pixels (WS even, HS any) is B = 2*HS*WS bytes, [HS][WS/2] macropixels of 4
// bytes - yuyv422 Y0 U Y1 V, uyvy422 U Y0 V Y1. Pixel (y, x) takes Y[x & 1], U and V of
// macropixel (y, x >> 1): the horizontal half of the 4:2:0 rule. Same formulas, same tables.
//
// Planar 4:2:2 / 4:4:4 frames (input pixel formats "yuv422p" / "yuv444p", what a JPEG decoder
// hands back; kernel csrc/kernels/yuv_planar.hip): with s = 1 (4:2:2, WS even) or 0 (4:4:4, any
// WS), any HS, a frame is Y[HS][WS], U[HS][WS >> s], V[HS][WS >> s], B = HS*WS + 2 (HS*WS >> s)
// bytes. Pixel (y, x) takes Y[y][x], U[y][x >> s], V[y][x >> s]; with the linear pixel index
// p = y WS + x that is Y[p], U[p >> s], V[p >> s] of three byte streams. Same formulas and tables.
//
// 10-bit 4:2:0 frames (input pixel formats "p010le" / "yuv420p10le", raw records only; kernel
// csrc/kernels/yuv420_hi.hip): a frame of HS x WS pixels (both even) is B = 3*HS*WS bytes of
// little-endian 16-bit words:
//     p010le:      Y[HS][WS], UV[HS/2][WS/2][2]            sample = word >> 6   (low six bits ignored)
//     yuv420p10le: Y[HS][WS], U[HS/2][WS/2], V[HS/2][WS/2]  sample = word & 1023 (high six ignored)
// Pixel (y, x) takes Y[y][x] and the chroma sample (y >> 1, x >> 1). The result is in quarter
// steps of the 8-bit scale, q in [0, 1020]; with yo = 64 (limited) or 0 (full):
//     q_R = clamp((cy (Y - yo)                  + crv (V - 512) + 2^17) >> 18, 0, 1020)
//     q_G = clamp((cy (Y - yo) + cgu (U - 512) + cgv (V - 512) + 2^17) >> 18, 0, 1020)
//     q_B = clamp((cy (Y - yo) + cbu (U - 512)                  + 2^17) >> 18, 0, 1020)
// and the model input of channel c is fmaf((float)q * 0.25f, a[c], b[c]) (the product is exact).
// The coefficients are the rationals above (limited: sy = 255/219, sc = 255/224 as for 8 bits,
// 64 .. 940 being 4 x (16 .. 235); full: sy = sc = 1020/1023) times 2^18, rounded half to even -
// 2^18 because 2^20 overflows 32 bits with 10-bit samples. The accumulator is affine in
// (Y, U, V); over the 8 corners of the cube, the 4 tables and the 3 channels its largest
// magnitude, rounding term included, is 575 820 179 < 2^31. The unclamped result lies within
// 0.5 + 2047 * 2^-19 quarter steps of the real-valued matrix.
//
// Triangle-filter chroma for I420 / NV12 (input-yuv-chroma "linear", b64 records only; kernel
// csrc/kernels/b64_yuv_linear.hip): libjpeg's h2v2_fancy_upsample, a centre-sited 3:1 filter in
// both directions, in integers. For pixel (y, x) and a chroma plane C of HS/2 x WS/2:
//     cy0 = y >> 1    cyn = clamp(cy0 + (y & 1 ? +1 : -1), 0, HS/2 - 1)
//     cx0 = x >> 1    cxn = clamp(cx0 + (x & 1 ? +1 : -1), 0, WS/2 - 1)
//     col(cx) = 3 C[cy0][cx] + C[cyn][cx]                          (0 .. 1020)
//     C'(y, x) = (3 col(cx0) + col(cxn) + (x & 1 ? 7 : 8)) >> 4    (0 .. 255)
// U', V' then go with Y[y][x] through the formulas above, unchanged: a linear frame gives the
// bits of a yuv444p frame that carries (Y, U', V'), and the accumulator bound holds because
// U', V' are bytes.
// No HIP in this header: the sanitizer programs of the host codec include it.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gale {

enum YuvFormat : int {
  YUV_NONE = 0, YUV_I420 = 1, YUV_NV12 = 2, YUV_YUYV422 = 3, YUV_UYVY422 = 4,
  YUV_YUV422P = 5, YUV_YUV444P = 6, YUV_P010LE = 7, YUV_YUV420P10LE = 8
};
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

// The widest frame b64_yuv_linear_instances serves: one row pair with its chroma halo, 5 WS bytes
// and 24 of slack rounded up to 16, and the kernel's 24 KB of float staging fill 64 KB of LDS.
constexpr int kYuv420LinearMaxWS = 8186;

// Packed 4:2:2: whether `format` is one, the bytes of one frame (WS even), and the byte offsets
// of Y0 / Y1 / U / V in a macropixel (the host twin and the kernel both take them from here).
constexpr bool yuv_is_422(int format) { return format == YUV_YUYV422 || format == YUV_UYVY422; }
inline int64_t yuv422_bytes(int HS, int WS) { return (int64_t)HS * WS * 2; }
constexpr int yuv422_y0(int format) { return format == YUV_UYVY422 ? 1 : 0; }
constexpr int yuv422_y1(int format) { return format == YUV_UYVY422 ? 3 : 2; }
constexpr int yuv422_u(int format) { return format == YUV_UYVY422 ? 0 : 1; }
constexpr int yuv422_v(int format) { return format == YUV_UYVY422 ? 2 : 3; }

// Planar 4:2:2 / 4:4:4: whether `format` is one, its horizontal chroma shift s, and the bytes of
// one frame (WS even for 4:2:2).
constexpr bool yuv_is_planar(int format) { return format == YUV_YUV422P || format == YUV_YUV444P; }
constexpr int yuvp_shift(int format) { return format == YUV_YUV422P ? 1 : 0; }
inline int64_t yuvp_bytes(int HS, int WS, int format) {
  const int64_t hw = (int64_t)HS * WS;
  return hw + 2 * (hw >> yuvp_shift(format));
}

// 10-bit 4:2:0: whether `format` is one, the bytes of one frame (HS, WS even), the table of
// (matrix, range) at the scale 2^18 (false for a value outside the enums), and the 10 bits of a
// 16-bit word.
constexpr bool yuv_is_420_hi(int format) {
  return format == YUV_P010LE || format == YUV_YUV420P10LE;
}
inline int64_t yuv420p10_bytes(int HS, int WS) { return (int64_t)HS * WS * 3; }
inline bool yuv10_coeffs(int matrix, int range, YuvCoeffs* k) {
  static const int32_t kTable[2][2][5] = {
      {{305236, 418389, -102698, -213115, 528805},   // bt601 limited
       {261375, 366448, -89949, -186658, 463157}},   // bt601 full
      {{305236, 469956, -55902, -139699, 553753},    // bt709 limited
       {261375, 411614, -48962, -122356, 485008}},   // bt709 full
  };
  if (matrix < 0 || matrix > 1 || range < 0 || range > 1) return false;
  const int32_t* t = kTable[matrix][range];
  k->cy = t[0], k->crv = t[1], k->cgu = t[2], k->cgv = t[3], k->cbu = t[4];
  k->yo = range == YUV_LIMITED ? 64 : 0;
  return true;
}
constexpr int yuv10_sample(int format, int word) {
  return format == YUV_P010LE ? (word >> 6) & 1023 : word & 1023;
}

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

// One triangle-filtered chroma sample (the header's formulas): plane C with `step` bytes between
// the samples of a row and `stride` between rows (I420: 1, WS/2; NV12: 2, WS), of ch x cw samples.
inline int yuv420_linear_chroma(const uint8_t* C, size_t stride, size_t step, int ch, int cw, int y,
                                int x) {
  const int cy0 = y >> 1, cx0 = x >> 1;
  int cyn = cy0 + ((y & 1) ? 1 : -1), cxn = cx0 + ((x & 1) ? 1 : -1);
  cyn = cyn < 0 ? 0 : cyn > ch - 1 ? ch - 1 : cyn;
  cxn = cxn < 0 ? 0 : cxn > cw - 1 ? cw - 1 : cxn;
  const auto col = [&](int cx) {
    return 3 * (int)C[(size_t)cy0 * stride + (size_t)cx * step] +
           (int)C[(size_t)cyn * stride + (size_t)cx * step];
  };
  return (3 * col(cx0) + col(cxn) + ((x & 1) ? 7 : 8)) >> 4;
}

// yuv420_to_rgb_host with the triangle-filtered chroma of input-yuv-chroma "linear": the host twin
// of the b64_yuv_linear_instances kernel. Same arguments, same refusals.
inline bool yuv420_linear_to_rgb_host(const uint8_t* src, int HS, int WS, int format,
                                      const YuvCoeffs& k, uint8_t* rgb, float* f32,
                                      const float* a = nullptr, const float* b = nullptr) {
  if (HS <= 0 || WS <= 0 || (HS & 1) || (WS & 1)) return false;
  if (format != YUV_I420 && format != YUV_NV12) return false;
  const size_t hw = (size_t)HS * WS;
  const bool nv12 = format == YUV_NV12;
  const uint8_t *const up = src + hw, *const vp = nv12 ? up + 1 : up + hw / 4;
  const size_t stride = nv12 ? (size_t)WS : (size_t)WS / 2, step = nv12 ? 2 : 1;
  for (int y = 0; y < HS; ++y)
    for (int x = 0; x < WS; ++x) {
      const int U = yuv420_linear_chroma(up, stride, step, HS / 2, WS / 2, y, x);
      const int V = yuv420_linear_chroma(vp, stride, step, HS / 2, WS / 2, y, x);
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

// The same for one packed 4:2:2 frame: yuv422_bytes(HS, WS) bytes at src -> [HS][WS][3]. false
// (nothing written) for a non-positive size, an odd WS or a format that is not a 4:2:2 one.
inline bool yuv422_to_rgb_host(const uint8_t* src, int HS, int WS, int format, const YuvCoeffs& k,
                               uint8_t* rgb, float* f32, const float* a = nullptr,
                               const float* b = nullptr) {
  if (HS <= 0 || WS <= 0 || (WS & 1) || !yuv_is_422(format)) return false;
  const size_t nmp = (size_t)HS * WS / 2;
  for (size_t m = 0; m < nmp; ++m) {
    const uint8_t* mp = src + 4 * m;
    const int U = mp[yuv422_u(format)], V = mp[yuv422_v(format)];
    for (int h = 0; h < 2; ++h) {
      uint8_t px[3];
      yuv_pixel_rgb(k, mp[h ? yuv422_y1(format) : yuv422_y0(format)], U, V, px);
      const size_t o = (2 * m + h) * 3;
      for (int c = 0; c < 3; ++c) {
        if (rgb) rgb[o + c] = px[c];
        if (f32) f32[o + c] = a ? __builtin_fmaf((float)px[c], a[c], b[c]) : (float)px[c];
      }
    }
  }
  return true;
}

// The same for one planar 4:2:2 / 4:4:4 frame: yuvp_bytes(HS, WS, format) bytes at src ->
// [HS][WS][3]. false (nothing written) for a non-positive size, an odd WS with 4:2:2 or a format
// that is not a planar one.
inline bool yuvp_to_rgb_host(const uint8_t* src, int HS, int WS, int format, const YuvCoeffs& k,
                             uint8_t* rgb, float* f32, const float* a = nullptr,
                             const float* b = nullptr) {
  if (HS <= 0 || WS <= 0 || !yuv_is_planar(format)) return false;
  const int s = yuvp_shift(format);
  if (s && (WS & 1)) return false;
  const size_t hw = (size_t)HS * WS;
  const uint8_t *const up = src + hw, *const vp = up + (hw >> s);
  for (size_t p = 0; p < hw; ++p) {  // (WS even with s = 1: the chroma index of pixel p is p >> 1)
    uint8_t px[3];
    yuv_pixel_rgb(k, src[p], up[p >> s], vp[p >> s], px);
    for (int c = 0; c < 3; ++c) {
      if (rgb) rgb[3 * p + c] = px[c];
      if (f32) f32[3 * p + c] = a ? __builtin_fmaf((float)px[c], a[c], b[c]) : (float)px[c];
    }
  }
  return true;
}

inline uint16_t yuv10_clampq(int32_t acc) {
  const int32_t v = acc >> 18;
  return (uint16_t)(v < 0 ? 0 : v > 1020 ? 1020 : v);
}

// The same for one 10-bit 4:2:0 frame: yuv420p10_bytes(HS, WS) bytes at src (any alignment) ->
// [HS][WS][3]. q (optional): the quarter steps, 0 .. 1020. f32 (optional): the model-side floats,
// fmaf((float)q * 0.25f, a[c], b[c]), or (float)q * 0.25f when a is null. k: a table of
// yuv10_coeffs. false (nothing written) for odd or non-positive sizes or another format.
inline bool yuv420p10_to_rgb_host(const uint8_t* src, int HS, int WS, int format,
                                  const YuvCoeffs& k, uint16_t* q, float* f32,
                                  const float* a = nullptr, const float* b = nullptr) {
  if (HS <= 0 || WS <= 0 || (HS & 1) || (WS & 1) || !yuv_is_420_hi(format)) return false;
  const size_t hw = (size_t)HS * WS, cw = (size_t)WS / 2;
  const auto word = [&](size_t i) { return (int)src[2 * i] | (int)src[2 * i + 1] << 8; };
  for (int y = 0; y < HS; ++y)
    for (int x = 0; x < WS; ++x) {
      const size_t ci = (size_t)(y >> 1) * cw + (size_t)(x >> 1);
      const size_t iu = format == YUV_P010LE ? hw + 2 * ci : hw + ci;
      const size_t iv = format == YUV_P010LE ? hw + 2 * ci + 1 : hw + hw / 4 + ci;
      const int Y = yuv10_sample(format, word((size_t)y * WS + x));
      const int u = yuv10_sample(format, word(iu)) - 512, v = yuv10_sample(format, word(iv)) - 512;
      const int32_t yy = k.cy * (Y - k.yo) + (1 << 17);
      const uint16_t px[3] = {yuv10_clampq(yy + k.crv * v),
                              yuv10_clampq(yy + k.cgu * u + k.cgv * v),
                              yuv10_clampq(yy + k.cbu * u)};
      const size_t o = ((size_t)y * WS + x) * 3;
      for (int c = 0; c < 3; ++c) {
        const float f = (float)px[c] * 0.25f;
        if (q) q[o + c] = px[c];
        if (f32) f32[o + c] = a ? __builtin_fmaf(f, a[c], b[c]) : f;
      }
    }
  return true;
}

}  // namespace codec
}  // namespace gale
