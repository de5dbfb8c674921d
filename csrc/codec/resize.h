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

// ---- antialiased form (InputResize(antialias=True); kernel: csrc/kernels/resize_crop_aa.hip) ----
// The support-scaled triangle filter of PIL / torch antialias=True on half-pixel centres, in
// integers. Per axis, off = (n_rs - n_out) / 2 and S = max(n_src, n_rs); for output i, source k:
//   u(i, k) = 2 S - |(2 k + 1) n_rs - (2 (i + off) + 1) n_src|      (2 S times the triangle)
// The taps of i are the k in [0, n_src) with u > 0: a non-empty contiguous run [start, start +
// count). U = sum of the run's u (int64, <= 2^26) and w = (float)((double)u / (double)U). Taps
// cut off at an edge are dropped; the rest renormalise through U. Each axis needs
// n_src <= 8 n_rs (kResizeAaMaxScale), so count <= 17 (kResizeAaMaxTaps).
// The tap sum of one axis: count == 1 passes the value through as a bit copy; else
// acc = w0 * v0 (one binary32 multiply), acc = fmaf(wk, vk, acc) for k = 1 .. count - 1 ascending.
// Columns first (the column sums rounded to binary32), then rows. Both axes take this form.
constexpr int kResizeAaMaxScale = 8;
constexpr int kResizeAaMaxTaps = 2 * kResizeAaMaxScale + 1;

struct ResizeAaTables {
  int HS = 0, WS = 0, HR = 0, WR = 0, H = 0, W = 0;
  std::vector<int32_t> ys, yn;  // [H] first tap and tap count of each output row
  std::vector<float> wy;        // the weights of all rows, concatenated in row order
  std::vector<int32_t> xs, xn;  // [W]
  std::vector<float> wx;
  int ty = 0, tx = 0;  // the largest tap count of a row / of a column
};

// std::invalid_argument for what build_resize_tables refuses and for HS > 8 HR or WS > 8 WR
void build_resize_aa_tables(int HS, int WS, int HR, int WR, int H, int W, ResizeAaTables& out);

// True when the tables have H / W entries, every run lies inside the source, every count is in
// 1..17 (and at most ty / tx), the weight vectors have the runs' total length and every weight
// is in (0, 1]
bool resize_aa_tables_ok(const ResizeAaTables& t);

// dst[n][H][W][C] from src[n][HS][WS][C]. The tables are checked first (resize_aa_tables_ok):
// a bad table throws std::invalid_argument and nothing is written.
void resize_crop_aa_host(const float* src, int n, int C, const ResizeAaTables& t, float* dst);

// The device layout of one axis' weights: a fixed stride of `stride` floats per entry (the
// axis' largest tap count), zero after an entry's last tap
std::vector<float> resize_aa_strided(const std::vector<int32_t>& count, const std::vector<float>& w,
                                     int stride);

// The source rows a band of `band` output rows touches (last - first + 1), the largest over all
// bands of the tables: what the kernel's launcher sizes its LDS tile from
int resize_aa_band_rows(const ResizeAaTables& t, int band);

// The band height the kernel is launched with: the largest of 8, 4, 2, 1 whose source rows and
// column weights fit the kernel's LDS budget (kResizeAaLdsRows rows of 1 KiB)
constexpr int kResizeAaLdsRows = 64;
int resize_aa_choose_band(const ResizeAaTables& t);

}  // namespace codec
}  // namespace gale
