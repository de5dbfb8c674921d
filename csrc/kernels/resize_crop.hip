// Input resize on the GPU: bilinear resize (half-pixel centres, no antialiasing) + centre crop
// of fp32 NHWC images, src [n][HS][WS][C] -> dst [n][H][W][C], by the host-built tables of a
// ResizePlan (codec::build_resize_tables; numerics: csrc/codec/resize.h). Bit-identical to
// codec::resize_crop_host and to InputResize.apply (gale/models/preprocess.py).
//
// A 256-thread workgroup produces 1024 consecutive floats g of one image's flat output
// (g = (y * W + x) * C + c), blockIdx.y is the image. The gathers outnumber the stores 2-4 to 1,
// so the work is laid out for them: in pass j = 0..3 thread t computes float 256 j + t of the
// workgroup's span, so the lanes of a wave read neighbouring source floats and neighbouring
// table entries (with a quad of 4 consecutive floats per lane every load instruction touched a
// 16-byte-strided address set, four times the cache lines: 39.8 / 76.3 us against 35.3 / 62.4 us
// for the ImageNet crop / resize batches, README "Kernels"). The stores are still 16 bytes per
// lane: when the image's float count is a multiple of 4 and dst is 16-byte aligned (the VEC
// instantiation) the four passes go through a 4 KiB LDS tile and lane t stores floats 4 t ..
// 4 t + 3 of the span; otherwise each pass stores its float directly (one coalesced 4-byte
// store per lane).
// The second pixel of a row is always loaded and dropped by a select where its weight is zero,
// so no branch separates a lane's loads; the second row is read only by lanes that have a
// non-zero row weight in one of their passes (a crop never does). Per-image base offsets are
// 64-bit; offsets inside an image are 32-bit (the launcher refuses images of 2^31 floats or
// more). No atomics, no scratch; nothing is read outside src[n * HS * WS * C] or written
// outside dst[n * H * W * C].
#include "common.cuh"
#include "gale/kernels.h"

// the subtraction and the fma of lerp are separate roundings by definition: nothing here may be
// contracted into anything else
#pragma clang fp contract(off)

namespace gale {
namespace {

constexpr int kResizeDimMax = 4096;
constexpr int kResizeSpan = 1024;  // floats per workgroup: 4 passes of 256 threads

__device__ __forceinline__ float lerp1(float a, float b, float w) {
  const float d = b - a;
  return __builtin_fmaf(w, d, a);
}

template <bool VEC>
__global__ __launch_bounds__(256) void resize_crop_kernel(ResizePlan p, const int* d_images,
                                                          const float* __restrict__ src,
                                                          float* __restrict__ dst) {
  __shared__ __attribute__((aligned(16))) float tile[VEC ? kResizeSpan : 4];
  const int img = blockIdx.y;
  if (d_images && img >= *d_images) return;  // (the whole workgroup: no barrier is left behind)
  const int RW = p.W * p.C;                  // floats per output row
  const int total = p.H * RW;                // floats per output image
  const int SW = p.WS * p.C;                 // floats per source row
  const int base = blockIdx.x * kResizeSpan;
  const float* s = src + (size_t)img * ((size_t)p.HS * SW);
  float* o = dst + (size_t)img * (size_t)total;
  // per pass: the two source offsets of the first row, the distance to the second row (0 where
  // the row weight is 0) and the weights. A float past the image's end (the last workgroup)
  // takes the image's last float's entries: loaded inside the source, never stored
  int ia[4], ib[4], dy[4];
  float wx[4], wy[4];
  bool rows2 = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int g = min(base + j * 256 + (int)threadIdx.x, total - 1);
    const int y = g / RW, f = g - y * RW;
    const int x = f / p.C, c = f - x * p.C;
    const int ya = p.y0[y] * SW;
    wy[j] = p.wy[y];
    dy[j] = wy[j] != 0.f ? p.y1[y] * SW - ya : 0;
    rows2 |= wy[j] != 0.f;
    ia[j] = ya + p.x0[x] * p.C + c;
    ib[j] = ya + p.x1[x] * p.C + c;
    wx[j] = p.wx[x];
  }
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = s[ia[j]], b = s[ib[j]];
    v[j] = wx[j] == 0.f ? a : lerp1(a, b, wx[j]);
  }
  if (rows2) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float e = s[ia[j] + dy[j]], g2 = s[ib[j] + dy[j]];
      const float u = wx[j] == 0.f ? e : lerp1(e, g2, wx[j]);
      v[j] = wy[j] == 0.f ? v[j] : lerp1(v[j], u, wy[j]);
    }
  }
  if (VEC) {
#pragma unroll
    for (int j = 0; j < 4; ++j) tile[j * 256 + threadIdx.x] = v[j];
    __syncthreads();
    // (total % 4 == 0: a quad is whole or past the end)
    const int g = base + 4 * (int)threadIdx.x;
    const float4 quad = *reinterpret_cast<const float4*>(tile + 4 * threadIdx.x);
    if (g < total) *reinterpret_cast<float4*>(o + g) = quad;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int g = base + j * 256 + (int)threadIdx.x;
      if (g < total) o[g] = v[j];
    }
  }
}

hipError_t launch(int images, const int* d_images, const ResizePlan& p, const float* src,
                  float* dst, hipStream_t stream) {
  if (!src || !dst || !p.y0 || !p.y1 || !p.wy || !p.x0 || !p.x1 || !p.wx)
    return hipErrorInvalidValue;
  const int dims[4] = {p.HS, p.WS, p.H, p.W};
  for (int d : dims)
    if (d < 1 || d > kResizeDimMax) return hipErrorInvalidValue;
  if (p.C < 1 || images < 0 || images > 65535) return hipErrorInvalidValue;
  if ((int64_t)p.HS * p.WS * p.C >= ((int64_t)1 << 31) ||
      (int64_t)p.H * p.W * p.C >= ((int64_t)1 << 31))
    return hipErrorInvalidValue;
  if (images == 0) return hipSuccess;
  const int64_t total = (int64_t)p.H * p.W * p.C;
  const dim3 grid((unsigned)((total + kResizeSpan - 1) / kResizeSpan), (unsigned)images);
  const bool vec = total % 4 == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(resize_crop_kernel<true>, grid, dim3(256), 0, stream, p, d_images, src,
                       dst);
  else
    hipLaunchKernelGGL(resize_crop_kernel<false>, grid, dim3(256), 0, stream, p, d_images, src,
                       dst);
  return hipGetLastError();
}

}  // namespace

hipError_t resize_crop(int images, const ResizePlan& plan, const float* src, float* dst,
                       hipStream_t stream) {
  return launch(images, nullptr, plan, src, dst, stream);
}

hipError_t resize_crop_dev(int max_images, const int* d_images, const ResizePlan& plan,
                           const float* src, float* dst, hipStream_t stream) {
  if (!d_images) return hipErrorInvalidValue;
  return launch(max_images, d_images, plan, src, dst, stream);
}

}  // namespace gale
