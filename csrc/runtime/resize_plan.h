// The input resize of one engine, in either form (codec/resize.h: the two-tap bilinear tables or
// the antialiased tap tables), and the one device image of its tables: which bytes are uploaded,
// where each table stands in them, and the kernel plan that points at an uploaded copy.
// Host-only (no HIP call), in a translation unit of its own so the CPU suite
// (tests/test_resize_plan_cpu.py) and the sanitizer checker (csrc/tests/resize_plan_check.cpp)
// can drive it. The replicas (replica.h) and the bindings take the resize in this form; the
// numerics and the table builders stay in codec/resize.h.
//
// The device image: six sections in the order the plan structs name their pointers
// (y0, y1, wy, x0, x1, wx / ys, yn, wy, xs, xn, wx), each starting on a 16-byte boundary, the
// padding bytes zero. The antialiased form's weights have a fixed stride per axis
// (codec::resize_aa_strided).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../codec/resize.h"
#include "gale/kernels.h"

namespace gale {

class InputResize {
 public:
  // What codec::build_resize_tables / codec::build_resize_aa_tables (antialias) throw
  static InputResize build(int HS, int WS, int HR, int WR, int H, int W, bool antialias);
  bool antialias() const { return aa_; }
  int HS() const { return aa_ ? a_.HS : t_.HS; }
  int WS() const { return aa_ ? a_.WS : t_.WS; }
  int HR() const { return aa_ ? a_.HR : t_.HR; }
  int WR() const { return aa_ ? a_.WR : t_.WR; }
  int H() const { return aa_ ? a_.H : t_.H; }
  int W() const { return aa_ ? a_.W : t_.W; }
  // codec::resize_tables_ok / codec::resize_aa_tables_ok of the form in use
  bool ok() const;
  // the tables of the form in use (the other form's are empty)
  const codec::ResizeTables& tables() const { return t_; }
  const codec::ResizeAaTables& aa_tables() const { return a_; }
  // dst[n][H][W][C] from src[n][HS][WS][C] by the form's host twin (codec::resize_crop_host /
  // codec::resize_crop_aa_host)
  void apply_host(const float* src, int n, int C, float* dst) const;

 private:
  InputResize() = default;  // (build() is the only source: the tables are never empty)
  bool aa_ = false;
  codec::ResizeTables t_;
  codec::ResizeAaTables a_;
};

struct ResizeDeviceImage {
  std::vector<uint8_t> bytes;  // what is uploaded, once
  size_t off[6] = {};          // each section's offset in bytes (a multiple of 16)
  // antialiased form: the largest tap counts (= the weights' strides), the band height
  // (codec::resize_aa_choose_band) and its source rows (codec::resize_aa_band_rows); else 0
  int ty = 0, tx = 0, band = 0, band_rows = 0;
};

// The only place that lays the resize tables out for the device.
ResizeDeviceImage pack(const InputResize& r);

// The kernel plan of an uploaded image, in the form of its resize
struct BoundResize {
  bool antialias = false;
  ResizePlan plain;  // !antialias
  ResizeAaPlan aa;   // antialias
};

// Every pointer of the plan = device_base + the section's offset; the integer fields from the
// resize, the image and C. The only place that fills the plan structs from a layout.
BoundResize bind(const ResizeDeviceImage& image, const InputResize& r, int C,
                 const uint8_t* device_base);

}  // namespace gale
