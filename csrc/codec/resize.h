// Input resize (gale/models/preprocess.py InputResize): bilinear resize of HS x WS source images
// to HR x WR (half-pixel centres, no antialiasing) and centre crop (floor offset) to the model's
// H x W, on the preprocessed fp32 NHWC values. The tables and the host resize here are the twins
// of InputResize.tables() / InputResize.apply() and of the resize_crop kernel
// (csrc/kernels/resize_crop.hip): all three give the same bits. Host code only, no HIP call.
//
// Per output row y (columns likewise), oy = (HR - H) / 2, all in integers:
//   num = (2 (y + oy) + 1) HS - HR, den = 2 HR
//   num < 0:          y0 = y1 = 0,      w = 0
//   y0 = num / den >= HS - 1: y0 = y1 = HS - 1, w = 0
//   else:             y1 = y0 + 1,      w = (float)rem / (float)den   (rem, den < 2^14: exact
//                                                                      operands, one rounding)
// lerp(a, b, w) = a for w == 0 (b is not used: a crop is a bit copy), else fmaf(w, b - a, a).
// out = lerp(lerp(v[y0][x0], v[y0][x1], wx), lerp(v[y1][x0], v[y1][x1], wx), wy) per channel.
#pragma once
#include <stdint.h>

#include <vector>

namespace gale {
namespace codec {

constexpr int kResizeMaxDim = 4096;  // every one of HS, WS, HR, WR, H, W is 1..kResizeMaxDim

struct ResizeTables {
  int HS = 0, WS = 0, HR = 0, WR = 0, H = 0, W = 0;
  std::vector<int32_t> y0, y1;  // [H]
  std::vector<float> wy;        // [H]
  std::vector<int32_t> x0, x1;  // [W]
  std::vector<float> wx;        // [W]
};

// std::invalid_argument for a dimension outside 1..kResizeMaxDim or HR < H / WR < W (no padding)
void build_resize_tables(int HS, int WS, int HR, int WR, int H, int W, ResizeTables& out);

// True when the tables have H / W entries with every index inside the source and 0 <= w < 1
bool resize_tables_ok(const ResizeTables& t);

// dst[n][H][W][C] from src[n][HS][WS][C]. The tables are checked first (resize_tables_ok): a
// table that would index outside the source throws std::invalid_argument and nothing is written.
void resize_crop_host(const float* src, int n, int C, const ResizeTables& t, float* dst);

}  // namespace codec
}  // namespace gale
