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

}  // namespace codec
}  // namespace gale
