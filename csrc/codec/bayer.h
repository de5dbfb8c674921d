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
// and the model input of channel c is fmaf((float)RGB[c], a[c], b[c]).
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

}  // namespace codec
}  // namespace gale
