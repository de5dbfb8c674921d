// InputResize, pack, bind (see resize_plan.h).
#include "resize_plan.h"

#include <string.h>

namespace gale {

InputResize InputResize::build(int HS, int WS, int HR, int WR, int H, int W, bool antialias) {
  InputResize r;
  r.aa_ = antialias;
  if (antialias) codec::build_resize_aa_tables(HS, WS, HR, WR, H, W, r.a_);
  else codec::build_resize_tables(HS, WS, HR, WR, H, W, r.t_);
  return r;
}

bool InputResize::ok() const {
  return aa_ ? codec::resize_aa_tables_ok(a_) : codec::resize_tables_ok(t_);
}

void InputResize::apply_host(const float* src, int n, int C, float* dst) const {
  if (aa_) codec::resize_crop_aa_host(src, n, C, a_, dst);
  else codec::resize_crop_host(src, n, C, t_, dst);
}

ResizeDeviceImage pack(const InputResize& r) {
  ResizeDeviceImage im;
  const void* part[6];
  size_t len[6];
  std::vector<float> wy, wx;  // antialiased: the strided weights
  auto section = [&](int i, const void* p, size_t n) { part[i] = p, len[i] = n * 4; };
  if (r.antialias()) {
    const codec::ResizeAaTables& t = r.aa_tables();
    wy = codec::resize_aa_strided(t.yn, t.wy, t.ty);
    wx = codec::resize_aa_strided(t.xn, t.wx, t.tx);
    im.ty = t.ty, im.tx = t.tx;
    im.band = codec::resize_aa_choose_band(t);
    im.band_rows = codec::resize_aa_band_rows(t, im.band);
    section(0, t.ys.data(), t.ys.size()), section(1, t.yn.data(), t.yn.size());
    section(2, wy.data(), wy.size());
    section(3, t.xs.data(), t.xs.size()), section(4, t.xn.data(), t.xn.size());
    section(5, wx.data(), wx.size());
  } else {
    const codec::ResizeTables& t = r.tables();
    section(0, t.y0.data(), t.y0.size()), section(1, t.y1.data(), t.y1.size());
    section(2, t.wy.data(), t.wy.size());
    section(3, t.x0.data(), t.x0.size()), section(4, t.x1.data(), t.x1.size());
    section(5, t.wx.data(), t.wx.size());
  }
  size_t end = 0;
  for (int i = 0; i < 6; ++i) {
    im.off[i] = end;
    end += (len[i] + 15) & ~(size_t)15;
  }
  im.bytes.assign(end, 0);
  for (int i = 0; i < 6; ++i) memcpy(im.bytes.data() + im.off[i], part[i], len[i]);
  return im;
}

BoundResize bind(const ResizeDeviceImage& image, const InputResize& r, int C,
                 const uint8_t* device_base) {
  auto ints = [&](int i) { return reinterpret_cast<const int32_t*>(device_base + image.off[i]); };
  auto floats = [&](int i) { return reinterpret_cast<const float*>(device_base + image.off[i]); };
  BoundResize b;
  b.antialias = r.antialias();
  if (b.antialias) {
    ResizeAaPlan& p = b.aa;
    p.HS = r.HS(), p.WS = r.WS(), p.HR = r.HR(), p.WR = r.WR(), p.H = r.H(), p.W = r.W(), p.C = C;
    p.ty = image.ty, p.tx = image.tx, p.band = image.band, p.band_rows = image.band_rows;
    p.ys = ints(0), p.yn = ints(1), p.wy = floats(2);
    p.xs = ints(3), p.xn = ints(4), p.wx = floats(5);
  } else {
    ResizePlan& p = b.plain;
    p.HS = r.HS(), p.WS = r.WS(), p.H = r.H(), p.W = r.W(), p.C = C;
    p.y0 = ints(0), p.y1 = ints(1), p.wy = floats(2);
    p.x0 = ints(3), p.x1 = ints(4), p.wx = floats(5);
  }
  return b;
}

}  // namespace gale
