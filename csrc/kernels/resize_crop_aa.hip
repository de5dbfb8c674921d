// Antialiased input resize on the GPU: the support-scaled triangle filter of PIL / torch
// antialias=True (half-pixel centres) + centre crop of fp32 NHWC images, src [n][HS][WS][C] ->
// dst [n][H][W][C], in the tap form of csrc/codec/resize.h by the host-built tables of a
// ResizeAaPlan. Bit-identical to codec::resize_crop_aa_host and to
// InputResize(antialias=True).apply (gale/models/preprocess.py).
//
// One launch, no intermediate in global memory. A 256-thread workgroup owns a tile: a band of
// p.band output rows (blockIdx.y) by a span of 256 consecutive floats f = x * C + c of the flat
// output row (blockIdx.x); blockIdx.z is the image.
//   Stage 1. Lane f computes, for every source row the band's taps touch (r0 .. r0 + rows - 1,
//     rows <= p.band_rows), the column sum of its (x, c) from global memory into tile[row][f] in
//     LDS. Neighbouring lanes read neighbouring source floats (the layout lesson of
//     resize_crop.hip). The lane's column weights are the same for every row; it parks them in
//     its own LDS column wl[k][f] (a register array indexed by the tap would go to scratch) and
//     takes four rows per trip through the tap loop, so four loads are in flight per weight.
//   Stage 2. After one barrier the row taps run out of LDS. The output row is uniform across a
//     wave in both store paths, so its start, count and weights are scalar loads. With 16-byte
//     stores (W * C a multiple of 4 and dst 16-byte aligned, the VEC instantiation) wave w takes
//     the band's rows w, w + 4, ... and lane l the floats 4 l .. 4 l + 3 of the span: one
//     ds_read_b128 per tap and one 16-byte store per row. Otherwise lane f takes float f of every
//     row of the band and stores it directly (one coalesced 4-byte store per lane). Consecutive
//     lanes read consecutive LDS words in both. (resize_crop's condition for 16-byte stores is
//     H * W * C % 4 == 0 on its flat output; here a tile's rows are separate pieces of the
//     output, so each row must start on a 16-byte boundary: W * C % 4 == 0.)
// Against gathering taps_y * taps_x floats per output, the column sums are computed once per band:
// the recompute factor is (band * s + 2 s + 1) / (band * s) for a downscale s.
// LDS: (p.tx + p.band_rows) KiB, dynamic, at most 64 KiB (the launcher refuses more; the host
// picks band = 8, or 4 / 2 / 1 near the 8x limit: codec::resize_aa_choose_band). At a 2x
// downscale that is 18 + 4 KiB, seven workgroups per CU by LDS. Bands of 4 and 16 rows were
// measured against 8 and lost on three of four cases each (README "Kernels").
// The tap sum is the definition's: a count of 1 copies the bits (NaN payloads, -0), else
// w0 * v0 rounded, then fmaf(wk, vk, acc) ascending. A row count beyond p.band_rows or a run
// outside the staged rows (tables that do not match the plan) is clamped into the tile, never
// read or written outside it. Per-image base offsets are 64-bit; offsets inside an image are
// 32-bit (the launcher refuses images of 2^31 floats or more). No atomics, no scratch; nothing is
// read outside src[n * HS * WS * C] or written outside dst[n * H * W * C].
#include "common.cuh"
#include "gale/kernels.h"

// the multiply and each fma of a tap sum are separate roundings by definition
#pragma clang fp contract(off)

namespace gale {
namespace {

constexpr int kAaDimMax = 4096;
constexpr int kAaSpan = 256;      // floats of the output row per workgroup
constexpr int kAaMaxScale = 8;    // n_src <= 8 n_rs per axis
constexpr int kAaMaxTaps = 17;
constexpr int kAaMaxBand = 8;
constexpr int kAaLdsRows = 64;    // tx + band_rows: 64 KiB of LDS

template <bool VEC>
__global__ __launch_bounds__(256) void resize_crop_aa_kernel(ResizeAaPlan p, const int* d_images,
                                                             const float* __restrict__ src,
                                                             float* __restrict__ dst) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int img = blockIdx.z;
  if (d_images && img >= *d_images) return;  // (the whole workgroup, before the barrier)
  const int tid = threadIdx.x;
  const int RW = p.W * p.C;  // floats per output row
  const int SW = p.WS * p.C;  // floats per source row
  const int f0 = blockIdx.x * kAaSpan;
  const int yb = blockIdx.y * p.band;
  const int tr = min(p.band, p.H - yb);  // output rows of this band
  float* wl = lds;                       // [tx][256]: lane f's column weights in column f
  float* tile = lds + p.tx * kAaSpan;    // [band_rows][256]: the column sums
  // the source rows of the band: the runs' starts and ends both grow with y
  const int r0 = p.ys[yb];
  const int rows = max(1, min(p.ys[yb + tr - 1] + p.yn[yb + tr - 1] - r0, p.band_rows));
  const int F = f0 + tid;
  const bool live = F < RW;
  if (live) {
    const int x = F / p.C, c = F - x * p.C;
    const int n = min(p.xn[x], p.tx);
    const float* w = p.wx + x * p.tx;
    for (int k = 0; k < n; ++k) wl[k * kAaSpan + tid] = w[k];
    const float* s = src + (size_t)img * ((size_t)p.HS * SW) + (r0 * SW + p.xs[x] * p.C + c);
    const float w0 = wl[tid];
    const bool copy = n == 1;
    for (int r = 0; r < rows; r += 4) {
      // (rows past the last one repeat it: loaded inside the source, not kept)
      const int ia = r * SW, ib = min(r + 1, rows - 1) * SW, ic = min(r + 2, rows - 1) * SW,
                id = min(r + 3, rows - 1) * SW;
      const float va = s[ia], vb = s[ib], vc = s[ic], vd = s[id];
      float a0 = copy ? va : w0 * va, a1 = copy ? vb : w0 * vb, a2 = copy ? vc : w0 * vc,
            a3 = copy ? vd : w0 * vd;
      for (int k = 1; k < n; ++k) {
        const float wk = wl[k * kAaSpan + tid];
        const int o = k * p.C;
        a0 = __builtin_fmaf(wk, s[ia + o], a0);
        a1 = __builtin_fmaf(wk, s[ib + o], a1);
        a2 = __builtin_fmaf(wk, s[ic + o], a2);
        a3 = __builtin_fmaf(wk, s[id + o], a3);
      }
      float* t = tile + r * kAaSpan + tid;
      t[0] = a0;
      if (r + 1 < rows) t[kAaSpan] = a1;
      if (r + 2 < rows) t[2 * kAaSpan] = a2;
      if (r + 3 < rows) t[3 * kAaSpan] = a3;
    }
  }
  __syncthreads();
  float* o = dst + (size_t)img * ((size_t)p.H * RW);
  if (VEC) {
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int len = min(kAaSpan, RW - f0);  // (a multiple of 4)
    for (int j = wave; j < tr; j += 4) {
      const int y = yb + j;
      const int n = min(min(p.yn[y], p.ty), rows);
      const int rb = max(0, min(p.ys[y] - r0, rows - n));
      const float* w = p.wy + y * p.ty;
      const float4* t = reinterpret_cast<const float4*>(tile + rb * kAaSpan) + lane;
      float4 a = t[0];
      if (n > 1) {
        const float w0 = w[0];
        a.x = w0 * a.x, a.y = w0 * a.y, a.z = w0 * a.z, a.w = w0 * a.w;
        for (int k = 1; k < n; ++k) {
          const float wk = w[k];
          const float4 v = t[k * (kAaSpan / 4)];
          a.x = __builtin_fmaf(wk, v.x, a.x);
          a.y = __builtin_fmaf(wk, v.y, a.y);
          a.z = __builtin_fmaf(wk, v.z, a.z);
          a.w = __builtin_fmaf(wk, v.w, a.w);
        }
      }
      if (4 * lane < len) *reinterpret_cast<float4*>(o + (y * RW + f0 + 4 * lane)) = a;
    }
  } else {
    for (int j = 0; j < tr; ++j) {
      const int y = yb + j;
      const int n = min(min(p.yn[y], p.ty), rows);
      const int rb = max(0, min(p.ys[y] - r0, rows - n));
      const float* w = p.wy + y * p.ty;
      const float* t = tile + rb * kAaSpan + tid;
      float a = t[0];
      if (n > 1) {
        a = w[0] * a;
        for (int k = 1; k < n; ++k) a = __builtin_fmaf(w[k], t[k * kAaSpan], a);
      }
      if (live) o[y * RW + F] = a;
    }
  }
}

hipError_t launch(int images, const int* d_images, const ResizeAaPlan& p, const float* src,
                  float* dst, hipStream_t stream) {
  if (!src || !dst || !p.ys || !p.yn || !p.wy || !p.xs || !p.xn || !p.wx)
    return hipErrorInvalidValue;
  const int dims[6] = {p.HS, p.WS, p.HR, p.WR, p.H, p.W};
  for (int d : dims)
    if (d < 1 || d > kAaDimMax) return hipErrorInvalidValue;
  if (p.HR < p.H || p.WR < p.W) return hipErrorInvalidValue;
  if (p.HS > kAaMaxScale * p.HR || p.WS > kAaMaxScale * p.WR) return hipErrorInvalidValue;
  if (p.C < 1 || images < 0 || images > 65535) return hipErrorInvalidValue;
  if ((int64_t)p.HS * p.WS * p.C >= ((int64_t)1 << 31) ||
      (int64_t)p.H * p.W * p.C >= ((int64_t)1 << 31))
    return hipErrorInvalidValue;
  if (p.ty < 1 || p.ty > kAaMaxTaps || p.tx < 1 || p.tx > kAaMaxTaps) return hipErrorInvalidValue;
  if (p.band < 1 || p.band > kAaMaxBand || p.band_rows < 1 || p.band_rows + p.tx > kAaLdsRows)
    return hipErrorInvalidValue;
  if (images == 0) return hipSuccess;
  const int64_t RW = (int64_t)p.W * p.C;
  const dim3 grid((unsigned)((RW + kAaSpan - 1) / kAaSpan), (unsigned)((p.H + p.band - 1) / p.band),
                  (unsigned)images);
  const size_t lds = (size_t)(p.tx + p.band_rows) * kAaSpan * sizeof(float);
  const bool vec = RW % 4 == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(resize_crop_aa_kernel<true>, grid, dim3(256), lds, stream, p, d_images, src,
                       dst);
  else
    hipLaunchKernelGGL(resize_crop_aa_kernel<false>, grid, dim3(256), lds, stream, p, d_images,
                       src, dst);
  return hipGetLastError();
}

}  // namespace

hipError_t resize_crop_aa(int images, const ResizeAaPlan& plan, const float* src, float* dst,
                          hipStream_t stream) {
  return launch(images, nullptr, plan, src, dst, stream);
}

hipError_t resize_crop_aa_dev(int max_images, const int* d_images, const ResizeAaPlan& plan,
                              const float* src, float* dst, hipStream_t stream) {
  if (!d_images) return hipErrorInvalidValue;
  return launch(max_images, d_images, plan, src, dst, stream);
}

}  // namespace gale
