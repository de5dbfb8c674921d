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
// 5 x 5 filter (bayer_demosaic malvar) is written out at bayer_malvar_to_rgb_host below, the
// edge-directed one (bayer_demosaic hamilton) at bayer_hamilton_to_rgb_host.
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

// The demosaics of the configuration name bayer_demosaic. (BILINEAR and MALVAR are 0 and 1: the
// `bool malvar` of the older signatures converts to them.)
enum BayerDemosaic : int { BAYER_BILINEAR = 0, BAYER_MALVAR = 1, BAYER_HAMILTON = 2 };

// "bilinear" | "malvar" | "hamilton"; -1 for anything else.
inline int bayer_demosaic_of(const char* s) {
  static const char* const kNames[] = {"bilinear", "malvar", "hamilton"};
  for (int f = BAYER_BILINEAR; f <= BAYER_HAMILTON; ++f) {
    const char *a = kNames[f], *b = s;
    while (*a && *a == *b) ++a, ++b;
    if (!*a && !*b) return f;
  }
  return -1;
}

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

// The edge-directed demosaic (configuration name bayer_demosaic hamilton): the adaptive colour
// plane interpolation of Hamilton and Adams (US 5,629,734) in integers. HS, WS >= 4; S is
// reflected two deep as for malvar. Green at an R or B site, s = S[y][x]:
//     dH = |W - E| + |2 s - WW - EE|            dV = |N - S| + |2 s - NN - SS|
//     gH = (2 (W + E) + 2 s - WW - EE + 2) >> 2     gV = (2 (N + S) + 2 s - NN - SS + 2) >> 2
//     gA = (2 (W + E + N + S) + 4 s - WW - EE - NN - SS + 4) >> 3      (signed, >> arithmetic)
//     G^ = clamp(dH < dV ? gH : dV < dH ? gV : gA, 0, 255)
// and G^ = s at a G site. The colour difference K[y][x] = S[y][x] - G^[y][x] (the clamped G^) is
// formed at R / B sites only, never read at a G site, and its indices are reflected one deep
// (-1 -> 1, n -> n - 2); dH / gH and dV / gV are symmetric, so that equals G^ of S reflected three
// deep. Then
//     G site:    this row's colour = clamp(s + ((K[y][x-1] + K[y][x+1] + 1) >> 1), 0, 255),
//                the other         = clamp(s + ((K[y-1][x] + K[y+1][x] + 1) >> 1), 0, 255)
//     R/B site:  own = s,  G = G^,  opposite = clamp(G^ + ((K[y-1][x-1] + K[y-1][x+1] +
//                                                K[y+1][x-1] + K[y+1][x+1] + 2) >> 2), 0, 255)
// (no diagonal direction decision). gH, gV lie in [-127, 383], K in [-255, 255], a sum of four K
// in [-1020, 1020]: 16-bit lanes are exact (the kernel, csrc/kernels/bayer_hamilton.hip). The
// signature and the optional outputs of bayer_to_rgb_host; false (nothing written) also for a size
// under 4. *choice (optional, [HS][WS]): 0 at a G site, 1 / 2 / 3 where gH / gV / gA was taken.
inline bool bayer_hamilton_to_rgb_host(const uint8_t* src, int HS, int WS, int order, uint8_t* rgb,
                                       float* f32, const float* a = nullptr,
                                       const float* b = nullptr, uint8_t* choice = nullptr) {
  if (!bayer_bytes(HS, WS) || HS < 4 || WS < 4 || !bayer_is_order(order)) return false;
  const int gf = bayer_green_first(order), bf = bayer_blue_first(order);
  const auto refl = [](int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; };
  const auto at = [&](int y, int x) { return (int)src[(size_t)refl(y, HS) * WS + refl(x, WS)]; };
  const auto clamp = [](int n) { return n < 0 ? 0 : n > 255 ? 255 : n; };
  const auto iabs = [](int n) { return n < 0 ? -n : n; };
  // G^ at the R / B site (y, x) of the frame; which: 1 / 2 / 3
  const auto green = [&](int y, int x, int* which) {
    const int s = at(y, x), w = at(y, x - 1), e = at(y, x + 1), n = at(y - 1, x), so = at(y + 1, x);
    const int hd = 2 * s - at(y, x - 2) - at(y, x + 2), vd = 2 * s - at(y - 2, x) - at(y + 2, x);
    const int dh = iabs(w - e) + iabs(hd), dv = iabs(n - so) + iabs(vd);
    *which = dh < dv ? 1 : dv < dh ? 2 : 3;
    return clamp(dh < dv   ? (2 * (w + e) + hd + 2) >> 2
                 : dv < dh ? (2 * (n + so) + vd + 2) >> 2
                           : (2 * (w + e + n + so) + hd + vd + 4) >> 3);
  };
  // K at an R / B site, its indices reflected one deep
  const auto k = [&](int y, int x) {
    int which;
    y = refl(y, HS), x = refl(x, WS);
    return (int)src[(size_t)y * WS + x] - green(y, x, &which);
  };
  for (int y = 0; y < HS; ++y)
    for (int x = 0; x < WS; ++x) {
      const int s = at(y, x);
      int own, g, opp, which = 0;  // own: the non-green colour of row y; opp: that of the rows next to it
      if ((((x + y) & 1) != 0) != (gf != 0)) {
        g = s;
        own = clamp(s + ((k(y, x - 1) + k(y, x + 1) + 1) >> 1));
        opp = clamp(s + ((k(y - 1, x) + k(y + 1, x) + 1) >> 1));
      } else {
        own = s;
        g = green(y, x, &which);
        opp = clamp(g + ((k(y - 1, x - 1) + k(y - 1, x + 1) + k(y + 1, x - 1) + k(y + 1, x + 1) + 2) >> 2));
      }
      const bool blue_row = ((y & 1) != 0) != (bf != 0);
      const uint8_t px[3] = {(uint8_t)(blue_row ? opp : own), (uint8_t)g,
                             (uint8_t)(blue_row ? own : opp)};
      const size_t o = ((size_t)y * WS + x) * 3;
      if (choice) choice[(size_t)y * WS + x] = (uint8_t)which;
      for (int c = 0; c < 3; ++c) {
        if (rgb) rgb[o + c] = px[c];
        if (f32) f32[o + c] = a ? __builtin_fmaf((float)px[c], a[c], b[c]) : (float)px[c];
      }
    }
  return true;
}

// One frame by the named demosaic (BayerDemosaic): the three twins above behind one signature.
inline bool bayer_demosaic_to_rgb_host(const uint8_t* src, int HS, int WS, int order, int demosaic,
                                       uint8_t* rgb, float* f32, const float* a = nullptr,
                                       const float* b = nullptr) {
  return demosaic == BAYER_HAMILTON ? bayer_hamilton_to_rgb_host(src, HS, WS, order, rgb, f32, a, b)
         : demosaic == BAYER_MALVAR ? bayer_malvar_to_rgb_host(src, HS, WS, order, rgb, f32, a, b)
         : demosaic == BAYER_BILINEAR ? bayer_to_rgb_host(src, HS, WS, order, rgb, f32, a, b)
                                      : false;
}

}  // namespace codec
}  // namespace gale
