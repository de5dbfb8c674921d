// 10-, 12- and 16-bit Bayer mosaic frames (input pixel formats "bayer_<order><form>", order rggb |
// bggr | grbg | gbrg, form 10le | 12le | 16le | 10p | 12p; raw records only): what sensors emit,
// as V4L2 and FFmpeg lay it out. The demosaics are those of bayer.h at full depth; they are
// implemented three times with the same bits - the numpy oracle (gale/models/preprocess.py
// BayerHiConvert), the host twin here and the kernel (csrc/kernels/bayer_hi.hip).
//
// A frame of HS x WS pixels (both even) holds samples S[HS][WS] of `bits` bits, M = 2^bits - 1:
//   10le 12le 16le   2 HS WS bytes: little-endian 16-bit words, S = word & M (the upper bits of a
//                    10- or 12-bit word are ignored)                       V4L2 SRGGB10/12/16
//   10p              5 HS WS / 4 bytes, WS a multiple of 4, no row padding: four pixels in five
//                    bytes, bytes 0..3 their bits 9:2, byte 4 their bits 1:0 (pixel 0 in bits
//                    1:0, pixel 3 in bits 7:6)                             V4L2 SRGGB10P
//   12p              3 HS WS / 2 bytes: two pixels in three bytes, byte 0 = p0[11:4],
//                    byte 1 = p1[11:4], byte 2 = p1[3:0] << 4 | p0[3:0]    V4L2 SRGGB12P
// Every bit pattern is a frame. RGB is bayer.h's bilinear rule on S, or its Malvar rule with
// q(n) = clamp((n + 8) >> 4, 0, M): numerators lie in [-12 M, 28 M], so int32 is exact. The model
// input of channel c is fmaf((float)RGB[c], a[c], b[c]); (float) of a value <= 65535 is exact.
// No HIP in this header: the sanitizer programs of the host codec include it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "bayer.h"

namespace gale {

enum BayerPacking : int { BAYER_PACK_NONE = 0, BAYER_PACK_LE16 = 1, BAYER_PACK_MIPI = 2 };

struct BayerHiFormat {
  int order = BAYER_NONE;  // BayerOrder; BAYER_NONE: not one of the twenty names
  int bits = 0;            // 10, 12 or 16
  int packing = BAYER_PACK_NONE;
};

// The depth / packing pairs there are: words of 10, 12 or 16 bits, MIPI groups of 10 or 12.
constexpr bool bayer_hi_is_form(int bits, int packing) {
  return packing == BAYER_PACK_LE16   ? bits == 10 || bits == 12 || bits == 16
         : packing == BAYER_PACK_MIPI ? bits == 10 || bits == 12
                                      : false;
}

// The names of the configuration ("bayer_rggb10le", "bayer_gbrg12p", ...); order BAYER_NONE for
// anything else (the 8-bit names included: bayer_order_of knows those).
inline BayerHiFormat bayer_hi_format_of(const char* s) {
  static const char* const kOrders[] = {"", "rggb", "bggr", "grbg", "gbrg"};
  static const struct {
    const char* name;
    int bits, packing;
  } kForms[] = {{"10le", 10, BAYER_PACK_LE16}, {"12le", 12, BAYER_PACK_LE16},
                {"16le", 16, BAYER_PACK_LE16}, {"10p", 10, BAYER_PACK_MIPI},
                {"12p", 12, BAYER_PACK_MIPI}};
  const auto eat = [](const char* a, const char* b) {  // b after the prefix a, null if not one
    while (*a && *a == *b) ++a, ++b;
    return *a ? nullptr : b;
  };
  const char* const t = eat("bayer_", s);
  for (int f = BAYER_RGGB; t && f <= BAYER_GBRG; ++f) {
    const char* const u = eat(kOrders[f], t);
    if (!u) continue;
    for (const auto& form : kForms) {
      const char* const e = eat(form.name, u);
      if (e && !*e) return BayerHiFormat{f, form.bits, form.packing};
    }
  }
  return BayerHiFormat{};
}

// Bytes of one frame; 0 for odd or non-positive sizes, an unknown form, or 10p with WS mod 4.
inline int64_t bayer_hi_bytes(int HS, int WS, int bits, int packing) {
  if (HS <= 0 || WS <= 0 || ((HS | WS) & 1) || !bayer_hi_is_form(bits, packing)) return 0;
  if (packing == BAYER_PACK_LE16) return (int64_t)HS * WS * 2;
  if (bits == 10) return WS & 3 ? 0 : (int64_t)HS * WS / 4 * 5;
  return (int64_t)HS * WS / 2 * 3;
}

// Sample i (= y WS + x) of a frame at src.
inline int bayer_hi_sample(const uint8_t* src, size_t i, int bits, int packing) {
  if (packing == BAYER_PACK_LE16)
    return (src[2 * i] | src[2 * i + 1] << 8) & ((1 << bits) - 1);
  if (bits == 10) {
    const uint8_t* const g = src + i / 4 * 5;
    return g[i & 3] << 2 | ((g[4] >> (2 * (i & 3))) & 3);
  }
  const uint8_t* const g = src + i / 2 * 3;
  return g[i & 1] << 4 | ((g[2] >> (4 * (i & 1))) & 15);
}

namespace codec {

// The host twin of the kernel: one frame's bayer_hi_bytes bytes at src -> [HS][WS][3]. rgb
// (optional): the uint16 image. f32 (optional): fmaf((float)RGB[c], a[c], b[c]), or (float)RGB[c]
// when a is null. malvar: the 5 x 5 filter (HS, WS >= 4). false (nothing written) for a size,
// order or form that is no frame.
inline bool bayer_hi_to_rgb_host(const uint8_t* src, int HS, int WS, int order, int bits,
                                 int packing, bool malvar, uint16_t* rgb, float* f32,
                                 const float* a = nullptr, const float* b = nullptr) {
  if (!bayer_hi_bytes(HS, WS, bits, packing) || !bayer_is_order(order)) return false;
  if (malvar && (HS < 4 || WS < 4)) return false;
  const int gf = bayer_green_first(order), bf = bayer_blue_first(order), M = (1 << bits) - 1;
  const auto at = [&](int y, int x) {
    y = y < 0 ? -y : y >= HS ? 2 * HS - 2 - y : y;
    x = x < 0 ? -x : x >= WS ? 2 * WS - 2 - x : x;
    return bayer_hi_sample(src, (size_t)y * WS + x, bits, packing);
  };
  const auto q = [M](int n) {
    n = (n + 8) >> 4;
    return n < 0 ? 0 : n > M ? M : n;
  };
  for (int y = 0; y < HS; ++y)
    for (int x = 0; x < WS; ++x) {
      const int s = at(y, x);
      const int h1 = at(y, x - 1) + at(y, x + 1), v1 = at(y - 1, x) + at(y + 1, x);
      const int d = at(y - 1, x - 1) + at(y - 1, x + 1) + at(y + 1, x - 1) + at(y + 1, x + 1);
      const bool green = (((x + y) & 1) != 0) != (gf != 0);
      int own, g, opp;  // own: the non-green colour of row y; opp: that of the rows next to it
      if (malvar) {
        const int h2 = at(y, x - 2) + at(y, x + 2), v2 = at(y - 2, x) + at(y + 2, x);
        if (green) {
          g = s;
          own = q(10 * s + 8 * h1 - 2 * d - 2 * h2 + v2);
          opp = q(10 * s + 8 * v1 - 2 * d - 2 * v2 + h2);
        } else {
          own = s;
          g = q(8 * s + 4 * (h1 + v1) - 2 * (h2 + v2));
          opp = q(12 * s + 4 * d - 3 * (h2 + v2));
        }
      } else if (green) {
        g = s, own = (h1 + 1) >> 1, opp = (v1 + 1) >> 1;
      } else {
        own = s, g = (h1 + v1 + 2) >> 2, opp = (d + 2) >> 2;
      }
      const bool blue_row = ((y & 1) != 0) != (bf != 0);
      const uint16_t px[3] = {(uint16_t)(blue_row ? opp : own), (uint16_t)g,
                              (uint16_t)(blue_row ? own : opp)};
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
