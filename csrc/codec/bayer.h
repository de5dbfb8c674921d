// 8-bit Bayer mosaic frames (input pixel formats "bayer_rggb8" / "bayer_bggr8" / "bayer_grbg8" /
// "bayer_gbrg8", raw records only): the demosaic to interleaved RGB, defined in
// gale/models/preprocess.py (BayerConvert) and implemented three times with the same bits - the
// numpy oracle there, the host twin here and the kernel (csrc/kernels/bayer.hip).
//
// A frame of HS x WS pixels (both even, >= 2) is B = HS*WS bytes S[HS][WS]; the order names the
// colours of the tile (0,0) (0,1) / (1,0) (1,1):
//     rggb  R G / G B     bggr  B G / G R     grbg  G R / B G     gbrg  G B / R G
// Indices outside the frame are mirrored without repeating the edge sample (-1 -> 1, n -> n - 2),
// which keeps a neighbour's colour parity. With s = S[y][x] and the eight neighbours at mirrored
// indices:
//     R or B site:  own = s,  G = (N + S + E + W + 2) >> 2,  opposite = (NW + NE + SW + SE + 2) >> 2
//     G site:       G = s,  this row's colour = (W + E + 1) >> 1,  the other = (N + S + 1) >> 1
// and the model input of channel c is fmaf((float)RGB[c], a[c], b[c]). The gradient-corrected
// 5 x 5 filter (bayer_demosaic malvar) is written out at bayer_malvar_to_rgb_host below.
// No HIP in this header: the sanitizer programs of the host codec include it.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gale {

enum BayerOrder : int { BAYER_NONE = 0, BAYER_RGGB = 1, BAYER_BGGR = 2, BAYER_GRBG = 3, BAYER_GBRG = 4 };

constexpr bool bayer_is_order(int order) { return order >= BAYER_RGGB && order <= BAYER_GBRG; }
// The two choices an order is: whether site (0, 0) is green, and whether the non-green colour of
// the even rows is blue.
constexpr bool bayer_green_first(int order) { return order == BAYER_GRBG || order == BAYER_GBRG; }
constexpr bool bayer_blue_first(int order) { return order == BAYER_BGGR || order == BAYER_GBRG; }

// Bytes of one frame; 0 for odd or non-positive sizes.
inline int64_t bayer_bytes(int HS, int WS) {
  return HS <= 0 || WS <= 0 || ((HS | WS) & 1) ? 0 : (int64_t)HS * WS;
}

// The names of the configuration ("bayer_rggb8", ...); BAYER_NONE for anything else.
inline int bayer_order_of(const char* s) {
  static const char* const kNames[] = {"", "bayer_rggb8", "bayer_bggr8", "bayer_grbg8",
                                       "bayer_gbrg8"};
  for (int f = BAYER_RGGB; f <= BAYER_GBRG; ++f) {
    const char *a = kNames[f], *b = s;
    while (*a && *a == *b) ++a, ++b;
    if (!*a && !*b) return f;
  }
  return BAYER_NONE;
}

namespace codec {

// The host twin of the kernel: one frame's bayer_bytes(HS, WS) bytes at src -> [HS][WS][3].
// rgb (optional): the uint8 image. f32 (optional): the model-side floats,
// fmaf((float)RGB[c], a[c], b[c]), or (float)RGB[c] when a is null. false (nothing written) for
// odd or non-positive sizes or an unknown order.
inline bool bayer_to_rgb_host(const uint8_t* src, int HS, int WS, int order, uint8_t* rgb,
                              float* f32, const float* a = nullptr, const float* b = nullptr) {
  if (!bayer_bytes(HS, WS) || !bayer_is_order(order)) return false;
  const int gf = bayer_green_first(order), bf = bayer_blue_first(order);
  const auto at = [&](int y, int x) {
    y = y < 0 ? -y : y >= HS ? 2 * HS - 2 - y : y;
    x = x < 0 ? -x : x >= WS ? 2 * WS - 2 - x : x;
    return (int)src[(size_t)y * WS + x];
  };
  for (int y = 0; y < HS; ++y)
    for (int x = 0; x < WS; ++x) {
      const int s = at(y, x);
      const int h = (at(y, x - 1) + at(y, x + 1) + 1) >> 1;
      const int v = (at(y - 1, x) + at(y + 1, x) + 1) >> 1;
      int own, g, opp;  // own: the non-green colour of row y; opp: that of the rows next to it
      if ((((x + y) & 1) != 0) != (gf != 0)) {
        g = s, own = h, opp = v;
      } else {
        own = s;
        g = (at(y - 1, x) + at(y + 1, x) + at(y, x - 1) + at(y, x + 1) + 2) >> 2;
        opp = (at(y - 1, x - 1) + at(y - 1, x + 1) + at(y + 1, x - 1) + at(y + 1, x + 1) + 2) >> 2;
      }
      const bool blue_row = ((y & 1) != 0) != (bf != 0);
      const uint8_t px[3] = {(uint8_t)(blue_row ? opp : own), (uint8_t)g,
                             (uint8_t)(blue_row ? own : opp)};
      const size_t o = ((size_t)y * WS + x) * 3;
      for (int c = 0; c < 3; ++c) {
        if (rgb) rgb[o + c] = px[c];
        if (f32) f32[o + c] = a ? __builtin_fmaf((float)px[c], a[c], b[c]) : (float)px[c];
      }
    }
  return true;
}

// The gradient-corrected demosaic (configuration name bayer_demosaic malvar): the 5 x 5 linear
// filter of Malvar, He and Cutler (ICASSP 2004), its four kernels times 2 so that every
// coefficient is an integer over 16. HS, WS >= 4; indices are reflected two deep (-2 -> 2,
// -1 -> 1, n -> n - 2, n + 1 -> n - 3). With, at reflected indices,
//     H1 = S[y][x-1] + S[y][x+1]    H2 = S[y][x-2] + S[y][x+2]
//     V1 = S[y-1][x] + S[y+1][x]    V2 = S[y-2][x] + S[y+2][x]
//     D  = S[y-1][x-1] + S[y-1][x+1] + S[y+1][x-1] + S[y+1][x+1]
//     q(n) = clamp((n + 8) >> 4, 0, 255)          (signed, >> arithmetic)
//     R or B site:  own = s,  G = q(8 s + 4 (H1 + V1) - 2 (H2 + V2)),
//                   opposite = q(12 s + 4 D - 3 (H2 + V2))
//     G site:       G = s,  this row's colour = q(10 s + 8 H1 - 2 D - 2 H2 + V2),
//                   the other = q(10 s + 8 V1 - 2 D - 2 V2 + H2)
// Every numerator and partial sum lies in [-3060, 7140]: 16-bit lanes are exact (the kernel,
// csrc/kernels/bayer_malvar.hip). The signature and the optional outputs of bayer_to_rgb_host;
// false (nothing written) also for a size under 4.
inline bool bayer_malvar_to_rgb_host(const uint8_t* src, int HS, int WS, int order, uint8_t* rgb,
                                     float* f32, const float* a = nullptr,
                                     const float* b = nullptr) {
  if (!bayer_bytes(HS, WS) || HS < 4 || WS < 4 || !bayer_is_order(order)) return false;
  const int gf = bayer_green_first(order), bf = bayer_blue_first(order);
  const auto at = [&](int y, int x) {
    y = y < 0 ? -y : y >= HS ? 2 * HS - 2 - y : y;
    x = x < 0 ? -x : x >= WS ? 2 * WS - 2 - x : x;
    return (int)src[(size_t)y * WS + x];
  };
  const auto q = [](int n) {
    n = (n + 8) >> 4;
    return n < 0 ? 0 : n > 255 ? 255 : n;
  };
  for (int y = 0; y < HS; ++y)
    for (int x = 0; x < WS; ++x) {
      const int s = at(y, x);
      const int h1 = at(y, x - 1) + at(y, x + 1), h2 = at(y, x - 2) + at(y, x + 2);
      const int v1 = at(y - 1, x) + at(y + 1, x), v2 = at(y - 2, x) + at(y + 2, x);
      const int d = at(y - 1, x - 1) + at(y - 1, x + 1) + at(y + 1, x - 1) + at(y + 1, x + 1);
      int own, g, opp;  // own: the non-green colour of row y; opp: that of the rows next to it
      if ((((x + y) & 1) != 0) != (gf != 0)) {
        g = s;
        own = q(10 * s + 8 * h1 - 2 * d - 2 * h2 + v2);
        opp = q(10 * s + 8 * v1 - 2 * d - 2 * v2 + h2);
      } else {
        own = s;
        g = q(8 * s + 4 * (h1 + v1) - 2 * (h2 + v2));
        opp = q(12 * s + 4 * d - 3 * (h2 + v2));
      }
      const bool blue_row = ((y & 1) != 0) != (bf != 0);
      const uint8_t px[3] = {(uint8_t)(blue_row ? opp : own), (uint8_t)g,
                             (uint8_t)(blue_row ? own : opp)};
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
