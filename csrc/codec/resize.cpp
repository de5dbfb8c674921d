// build_resize_tables / resize_crop_host (see resize.h).
#include "resize.h"

#include <math.h>
#include <stddef.h>

#include <stdexcept>

namespace gale {
namespace codec {

namespace {

void axis_table(int n_src, int n_rs, int n_out, std::vector<int32_t>& i0,
                std::vector<int32_t>& i1, std::vector<float>& w) {
  i0.assign((size_t)n_out, 0);
  i1.assign((size_t)n_out, 0);
  w.assign((size_t)n_out, 0.f);
  const int off = (n_rs - n_out) / 2;
  const int den = 2 * n_rs;
  for (int i = 0; i < n_out; ++i) {
    // (|num| < 2 * 4096 * 4096 + 4096: fits 32 bits)
    const int num = (2 * (i + off) + 1) * n_src - n_rs;
    if (num < 0) continue;
    const int q = num / den, rem = num % den;
    if (q >= n_src - 1) {
      i0[(size_t)i] = i1[(size_t)i] = n_src - 1;
      continue;
    }
    i0[(size_t)i] = q;
    i1[(size_t)i] = q + 1;
    w[(size_t)i] = (float)rem / (float)den;
  }
}

bool axis_ok(const std::vector<int32_t>& i0, const std::vector<int32_t>& i1,
             const std::vector<float>& w, int n_out, int n_src) {
  if (i0.size() != (size_t)n_out || i1.size() != (size_t)n_out || w.size() != (size_t)n_out)
    return false;
  for (size_t i = 0; i < (size_t)n_out; ++i) {
    if (i0[i] < 0 || i0[i] >= n_src || i1[i] < 0 || i1[i] >= n_src) return false;
    if (!(w[i] >= 0.f && w[i] < 1.f)) return false;
  }
  return true;
}

bool dim_ok(int v) { return v >= 1 && v <= kResizeMaxDim; }

inline float lerp(float a, float b, float w) {
  if (w == 0.f) return a;
  const float d = b - a;
  return fmaf(w, d, a);
}

}  // namespace

void build_resize_tables(int HS, int WS, int HR, int WR, int H, int W, ResizeTables& out) {
  if (!dim_ok(HS) || !dim_ok(WS) || !dim_ok(HR) || !dim_ok(WR) || !dim_ok(H) || !dim_ok(W))
    throw std::invalid_argument("resize: a dimension outside 1..4096");
  if (HR < H || WR < W) throw std::invalid_argument("resize: resize size below the model's");
  out.HS = HS, out.WS = WS, out.HR = HR, out.WR = WR, out.H = H, out.W = W;
  axis_table(HS, HR, H, out.y0, out.y1, out.wy);
  axis_table(WS, WR, W, out.x0, out.x1, out.wx);
}

bool resize_tables_ok(const ResizeTables& t) {
  if (!dim_ok(t.HS) || !dim_ok(t.WS) || !dim_ok(t.H) || !dim_ok(t.W)) return false;
  return axis_ok(t.y0, t.y1, t.wy, t.H, t.HS) && axis_ok(t.x0, t.x1, t.wx, t.W, t.WS);
}

void resize_crop_host(const float* src, int n, int C, const ResizeTables& t, float* dst) {
  if (n < 0 || C < 1 || (n > 0 && (!src || !dst)) || !resize_tables_ok(t))
    throw std::invalid_argument("resize_crop_host: bad arguments or tables");
  const size_t sper = (size_t)t.HS * t.WS * C, dper = (size_t)t.H * t.W * C;
  for (int i = 0; i < n; ++i) {
    const float* s = src + (size_t)i * sper;
    float* d = dst + (size_t)i * dper;
    for (int y = 0; y < t.H; ++y) {
      const float* r0 = s + (size_t)t.y0[(size_t)y] * t.WS * C;
      const float* r1 = s + (size_t)t.y1[(size_t)y] * t.WS * C;
      const float wy = t.wy[(size_t)y];
      float* o = d + (size_t)y * t.W * C;
      for (int x = 0; x < t.W; ++x) {
        const size_t a = (size_t)t.x0[(size_t)x] * C, b = (size_t)t.x1[(size_t)x] * C;
        const float wx = t.wx[(size_t)x];
        for (int c = 0; c < C; ++c) {
          const float top = lerp(r0[a + c], r0[b + c], wx);
          // (wy == 0: the second row is not used, as lerp's b)
          o[(size_t)x * C + c] = wy == 0.f ? top : lerp(top, lerp(r1[a + c], r1[b + c], wx), wy);
        }
      }
    }
  }
}

// ---- antialiased form -----------------------------------------------------------------------

namespace {

void aa_axis_table(int n_src, int n_rs, int n_out, std::vector<int32_t>& start,
                   std::vector<int32_t>& count, std::vector<float>& w, int& taps) {
  start.assign((size_t)n_out, 0);
  count.assign((size_t)n_out, 0);
  w.clear();
  taps = 0;
  const int64_t off = (n_rs - n_out) / 2, S = n_src > n_rs ? n_src : n_rs;
  const int64_t d = 2 * (int64_t)n_rs;
  auto u_of = [&](int64_t k, int64_t c) {
    const int64_t a = (2 * k + 1) * n_rs - c;
    return 2 * S - (a < 0 ? -a : a);
  };
  auto floor_div = [](int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
  for (int i = 0; i < n_out; ++i) {
    const int64_t c = (2 * (i + off) + 1) * (int64_t)n_src;
    // u > 0 <=> c - 2 S < (2 k + 1) n_rs < c + 2 S
    int64_t lo = floor_div(c - 2 * S - n_rs, d) + 1;
    int64_t hi = -floor_div(n_rs - c - 2 * S, d) - 1;
    if (lo < 0) lo = 0;
    if (hi > n_src - 1) hi = n_src - 1;
    int64_t U = 0;
    for (int64_t k = lo; k <= hi; ++k) U += u_of(k, c);
    const bool run = hi >= lo && u_of(lo, c) > 0 && u_of(hi, c) > 0 &&
                     (lo == 0 || u_of(lo - 1, c) <= 0) && (hi == n_src - 1 || u_of(hi + 1, c) <= 0);
    if (!run || hi - lo + 1 > kResizeAaMaxTaps || U > ((int64_t)1 << 26))
      throw std::logic_error("resize: antialias tap run");  // (the definition's guarantees)
    start[(size_t)i] = (int32_t)lo;
    count[(size_t)i] = (int32_t)(hi - lo + 1);
    if (count[(size_t)i] > taps) taps = count[(size_t)i];
    for (int64_t k = lo; k <= hi; ++k) w.push_back((float)((double)u_of(k, c) / (double)U));
  }
}

bool aa_axis_ok(const std::vector<int32_t>& start, const std::vector<int32_t>& count,
                const std::vector<float>& w, int n_out, int n_src, int taps) {
  if (start.size() != (size_t)n_out || count.size() != (size_t)n_out) return false;
  if (taps < 1 || taps > kResizeAaMaxTaps) return false;
  size_t total = 0;
  for (size_t i = 0; i < (size_t)n_out; ++i) {
    if (count[i] < 1 || count[i] > taps) return false;
    if (start[i] < 0 || start[i] > n_src - count[i]) return false;
    total += (size_t)count[i];
  }
  if (w.size() != total) return false;
  for (float v : w)
    if (!(v > 0.f && v <= 1.f)) return false;
  return true;
}

// one axis' tap sum over values v[k * stride], k = 0 .. n - 1
inline float tap_sum(const float* v, size_t stride, const float* w, int n) {
  if (n == 1) return v[0];
  float acc = w[0] * v[0];
  for (int k = 1; k < n; ++k) acc = fmaf(w[k], v[(size_t)k * stride], acc);
  return acc;
}

}  // namespace

void build_resize_aa_tables(int HS, int WS, int HR, int WR, int H, int W, ResizeAaTables& out) {
  if (!dim_ok(HS) || !dim_ok(WS) || !dim_ok(HR) || !dim_ok(WR) || !dim_ok(H) || !dim_ok(W))
    throw std::invalid_argument("resize: a dimension outside 1..4096");
  if (HR < H || WR < W) throw std::invalid_argument("resize: resize size below the model's");
  if (HS > kResizeAaMaxScale * HR || WS > kResizeAaMaxScale * WR)
    throw std::invalid_argument("resize: input_antialias takes a downscale of at most 8x");
  out.HS = HS, out.WS = WS, out.HR = HR, out.WR = WR, out.H = H, out.W = W;
  aa_axis_table(HS, HR, H, out.ys, out.yn, out.wy, out.ty);
  aa_axis_table(WS, WR, W, out.xs, out.xn, out.wx, out.tx);
}

bool resize_aa_tables_ok(const ResizeAaTables& t) {
  if (!dim_ok(t.HS) || !dim_ok(t.WS) || !dim_ok(t.H) || !dim_ok(t.W)) return false;
  return aa_axis_ok(t.ys, t.yn, t.wy, t.H, t.HS, t.ty) &&
         aa_axis_ok(t.xs, t.xn, t.wx, t.W, t.WS, t.tx);
}

void resize_crop_aa_host(const float* src, int n, int C, const ResizeAaTables& t, float* dst) {
  if (n < 0 || C < 1 || (n > 0 && (!src || !dst)) || !resize_aa_tables_ok(t))
    throw std::invalid_argument("resize_crop_aa_host: bad arguments or tables");
  const size_t SW = (size_t)t.WS * C, RW = (size_t)t.W * C;
  const size_t sper = (size_t)t.HS * SW, dper = (size_t)t.H * RW;
  std::vector<size_t> xo((size_t)t.W), yo((size_t)t.H);  // each entry's first weight
  size_t o = 0;
  for (int x = 0; x < t.W; ++x) xo[(size_t)x] = o, o += (size_t)t.xn[(size_t)x];
  o = 0;
  for (int y = 0; y < t.H; ++y) yo[(size_t)y] = o, o += (size_t)t.yn[(size_t)y];
  // the column sums of the source rows the output rows touch (the runs' starts and ends are
  // checked individually, so take the extremes over all rows)
  int r0 = t.HS, r1 = 0;
  for (int y = 0; y < t.H; ++y) {
    const int a = t.ys[(size_t)y], b = a + t.yn[(size_t)y];
    if (a < r0) r0 = a;
    if (b > r1) r1 = b;
  }
  std::vector<float> cols((size_t)(r1 - r0) * RW);
  for (int i = 0; i < n; ++i) {
    const float* s = src + (size_t)i * sper;
    float* d = dst + (size_t)i * dper;
    for (int r = r0; r < r1; ++r) {
      const float* row = s + (size_t)r * SW;
      float* tr = cols.data() + (size_t)(r - r0) * RW;
      for (int x = 0; x < t.W; ++x) {
        const float* w = t.wx.data() + xo[(size_t)x];
        const float* v = row + (size_t)t.xs[(size_t)x] * C;
        for (int c = 0; c < C; ++c)
          tr[(size_t)x * C + c] = tap_sum(v + c, (size_t)C, w, t.xn[(size_t)x]);
      }
    }
    for (int y = 0; y < t.H; ++y) {
      const float* w = t.wy.data() + yo[(size_t)y];
      const float* v = cols.data() + (size_t)(t.ys[(size_t)y] - r0) * RW;
      for (size_t f = 0; f < RW; ++f) d[(size_t)y * RW + f] = tap_sum(v + f, RW, w, t.yn[(size_t)y]);
    }
  }
}

std::vector<float> resize_aa_strided(const std::vector<int32_t>& count, const std::vector<float>& w,
                                     int stride) {
  std::vector<float> out(count.size() * (size_t)stride, 0.f);
  size_t o = 0;
  for (size_t i = 0; i < count.size(); ++i) {
    if (count[i] < 0 || count[i] > stride || o + (size_t)count[i] > w.size())
      throw std::invalid_argument("resize_aa_strided: counts do not match the weights");
    for (int k = 0; k < count[i]; ++k) out[i * (size_t)stride + (size_t)k] = w[o + (size_t)k];
    o += (size_t)count[i];
  }
  return out;
}

int resize_aa_band_rows(const ResizeAaTables& t, int band) {
  if (band < 1 || t.ys.size() != (size_t)t.H || t.yn.size() != (size_t)t.H)
    throw std::invalid_argument("resize_aa_band_rows: bad band or tables");
  int rows = 1;
  for (int y0 = 0; y0 < t.H; y0 += band) {
    int a = t.ys[(size_t)y0], b = a + t.yn[(size_t)y0];
    for (int y = y0; y < t.H && y < y0 + band; ++y) {
      if (t.ys[(size_t)y] < a) a = t.ys[(size_t)y];
      if (t.ys[(size_t)y] + t.yn[(size_t)y] > b) b = t.ys[(size_t)y] + t.yn[(size_t)y];
    }
    if (b - a > rows) rows = b - a;
  }
  return rows;
}

int resize_aa_choose_band(const ResizeAaTables& t) {
  for (int band = 8; band > 1; band /= 2)
    if (resize_aa_band_rows(t, band) + t.tx <= kResizeAaLdsRows) return band;
  return 1;
}

}  // namespace codec
}  // namespace gale
