// GPU decoder of base64 YUV 4:2:0 video-frame records (gale/kernels.h: b64_yuv_instances).
//
//   {"instances":[{"b64":"<L characters>"}, ...]}      B = HS*WS*3/2 bytes, L = 4 B / 3
//
// The host scan has located every string without reading it; this kernel reads the characters,
// judges them, converts the frame to RGB with the integer matrix of csrc/codec/yuv.h and stores
// fmaf((float)RGB[c], a[c], b[c]) as fp32 NHWC - the bits b64_decode_instances gives for the
// converted image sent as an RGB record.
//
// Work split: a workgroup owns `pairs` whole row pairs of one frame: 2 * pairs luma rows and
// pairs chroma rows. Those are two (NV12) or three (I420) contiguous byte ranges of the frame,
// hence contiguous runs of base64 quads. Phase 1 decodes the quads of each range into LDS as
// bytes - a lane takes 16 characters (4 quads, 12 bytes) through the shared window of
// b64_decode.cuh (b64::load_window, which states the read bound); a range's last lane judges
// only its own characters.
// A quad that straddles two ranges (or two workgroups' ranges) is decoded by
// every owner, so each character of the string is judged by at least one workgroup. One barrier;
// phase 2 converts and stores the workgroup's 6 * pairs * WS floats, which are contiguous in the
// NHWC image: thread t of an iteration stores floats [4 q, 4 q + 4), q = 256 i + t, so a wave's
// store instruction covers 1 KB of contiguous memory. 6 * pairs * WS is a multiple of 4 and so is
// the block's offset in the image, so the 16-byte form needs only a 16-byte aligned image base;
// otherwise one float per lane and instruction, contiguous as well.
//
// Verdict: a wave with a lane that saw a character outside the alphabet stores the constant 2
// into its record's status (a plain store: every writer stores the same value). The frame is
// written anyway, inside its own slot.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "b64_decode.cuh"
#include "gale/kernels.h"

namespace gale {
namespace {

constexpr int kThreads = 256;

// one contiguous byte range [b0, b1) of the frame: its quads q0 .. q0 + nq - 1, decoded into LDS
// bytes [lds, lds + 3 nq) by nl lanes of 4 quads; byte b of the frame is at lds + (b - 3 q0)
struct Range {
  int q0, nq, nl, lds;
};
__device__ __forceinline__ Range make_range(int b0, int b1, int lds) {
  Range r;
  r.q0 = b0 / 3;
  r.nq = b1 > b0 ? (b1 - 1) / 3 - r.q0 + 1 : 0;
  r.nl = (r.nq + 3) >> 2;
  r.lds = lds;
  return r;
}
__device__ __forceinline__ int round4(int v) { return (v + 3) & ~3; }

__device__ __forceinline__ int clamp8(int acc) { return min(max(acc >> 20, 0), 255); }

using b64::prepped;

template <bool PREP>
__global__ __launch_bounds__(kThreads) void b64_yuv_kernel(const B64Image* imgs, int images,
                                                           const int* d_images,
                                                           const uint8_t* bytes, int HS, int WS,
                                                           int pairs, uint32_t ws_magic,
                                                           int nv12, float* out,
                                                           int* status, YuvCoeffs k,
                                                           InputPrep prep) {
  if (d_images) images = min(images, *d_images);
  const int img = (int)blockIdx.y;
  if (img >= images) return;  // (workgroup-uniform, before any barrier or memory access)
  extern __shared__ uint32_t lds_words[];
  const B64Image d = imgs[img];
  const int tid = (int)threadIdx.x;
  const int p0 = (int)blockIdx.x * pairs;       // the block's first row pair
  const int n = min(pairs, (HS >> 1) - p0);     // its row pairs (>= 1: the grid is exact)
  const int hw = HS * WS, cw = WS >> 1;
  // ---- the block's byte ranges: luma, then U and V (I420) or UV (NV12; no third range)
  const int yb0 = 2 * p0 * WS;
  const int ub0 = hw + (nv12 ? p0 * WS : p0 * cw);
  const int un = nv12 ? n * WS : n * cw;
  const int vb0 = ub0 + (hw >> 2);
  const Range ry = make_range(yb0, yb0 + 2 * n * WS, 0);
  const Range ru = make_range(ub0, ub0 + un, round4(3 * ry.nq));
  const Range rv = make_range(vb0, nv12 ? vb0 : vb0 + un, ru.lds + round4(3 * ru.nq));
  // ---- phase 1: base64 -> bytes in LDS
  bool bad = false;
  const int tasks = ry.nl + ru.nl + rv.nl;
  for (int task = tid; task < tasks; task += kThreads) {
    const bool in_y = task < ry.nl, in_u = task < ry.nl + ru.nl;
    const int j = in_y ? task : in_u ? task - ry.nl : task - ry.nl - ru.nl;  // lane of its range
    const int q0 = in_y ? ry.q0 : in_u ? ru.q0 : rv.q0;
    const int nq = in_y ? ry.nq : in_u ? ru.nq : rv.nq;
    const int lds = in_y ? ry.lds : in_u ? ru.lds : rv.lds;
    const int nch = min(16, 4 * nq - 16 * j);  // characters of the range in the window (4 .. 16)
    // (the window ends inside the string: a range's quads are the string's; the phase is
    // uniform over the lanes of one range; 4 q0 + 16 j < L <= 2^30)
    const b64::Window win = b64::load_window(bytes, d.off, 4 * q0 + 16 * j, nch);
    // 24 bits -> 3 bytes in memory order (byte 0 first)
    uint32_t r[4], judged = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      r[t] = __builtin_bswap32(win.v[t]) >> 8;
      // (no padding: B is a multiple of 3)
      judged |= win.inv[t] & b64::first_bytes(nch - 4 * t);
    }
    bad |= judged != 0;
    // 12 bytes = 3 dwords at a 12-byte lane stride (conflict-free); the range's last lane only
    // the dwords its quads reach into (the range's LDS extent is rounded up to 4 bytes)
    uint32_t* dst = lds_words + ((lds + 12 * j) >> 2);
    const int nb = 3 * (nch >> 2);
    dst[0] = r[0] | (r[1] << 24);
    if (nb > 4) dst[1] = (r[1] >> 8) | (r[2] << 16);
    if (nb > 8) dst[2] = (r[2] >> 16) | (r[3] << 8);
  }
  if (__ballot(bad) != 0 && (tid & 63) == 0) status[d.rec] = 2;
  __syncthreads();
  // ---- phase 2: convert and store the block's rows
  const uint8_t* const lb = reinterpret_cast<const uint8_t*>(lds_words);
  const int ay = ry.lds + (yb0 - 3 * ry.q0);
  const int au = ru.lds + (ub0 - 3 * ru.q0);
  const int av = nv12 ? au + 1 : rv.lds + (vb0 - 3 * rv.q0);
  const int cstride = nv12 ? WS : cw, cstep = nv12 ? 2 : 1;
  // pixel lp of the block (row-major over its 2 n rows) -> R, G, B
  auto pixel = [&](int lp, int* rgb) {
    // lp / WS as one multiply: ws_magic = ceil(2^32 / WS) is exact while lp * WS < 2^32, and
    // lp < 2 * pairs * WS with pairs * WS bounded by the LDS budget (b64_yuv_instances)
    const int ly = (int)__umulhi((uint32_t)lp, ws_magic), lx = lp - ly * WS;
    const int ci = (ly >> 1) * cstride + (lx >> 1) * cstep;
    const int Y = lb[ay + lp], U = lb[au + ci], V = lb[av + ci];
    const int yy = k.cy * (Y - k.yo) + (1 << 19), u = U - 128, v = V - 128;
    rgb[0] = clamp8(yy + k.crv * v);
    rgb[1] = clamp8(yy + k.cgu * u + k.cgv * v);
    rgb[2] = clamp8(yy + k.cbu * u);
  };
  const int nf = 6 * n * WS;  // the block's floats
  float* const dst = out + (int64_t)d.slot * (3 * (int64_t)hw) + 6 * (int64_t)p0 * WS;
  if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    for (int q = tid; q < (nf >> 2); q += kThreads) {
      // floats 4 q .. 4 q + 3 lie in pixels p and p + 1, from channel c of pixel p on
      const int p = (int)((unsigned)(4 * q) / 3u), c = 4 * q - 3 * p;
      int s[6];
      pixel(p, s);
      pixel(p + 1, s + 3);
      float f[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int v = c == 0 ? s[e] : c == 1 ? s[e + 1] : s[e + 2];
        const int ch = c + e >= 3 ? c + e - 3 : c + e;
        f[e] = prepped<PREP>(v, ch, prep);
      }
      reinterpret_cast<float4*>(dst)[q] = make_float4(f[0], f[1], f[2], f[3]);
    }
  } else {
    for (int e = tid; e < nf; e += kThreads) {
      const int p = (int)((unsigned)e / 3u), c = e - 3 * p;
      int s[3];
      pixel(p, s);
      dst[e] = prepped<PREP>(c == 0 ? s[0] : c == 1 ? s[1] : s[2], c, prep);
    }
  }
}

}  // namespace

int b64_yuv_pairs(int HS, int WS) {
  if (HS < 2 || WS < 2) return 0;
  // about 4096 pixels a workgroup: 2 * pairs rows of WS
  return std::min(std::max(2048 / WS, 1), HS / 2);
}

size_t b64_yuv_lds_bytes(int WS, int pairs) {
  // luma 2 * pairs * WS and chroma pairs * WS bytes, each of the three ranges widened to whole
  // quads (2 bytes at either end) and rounded up to 4
  return (size_t)3 * (size_t)pairs * (size_t)WS + 3 * 8;
}

hipError_t b64_yuv_instances(int images, const B64Image* imgs, const uint8_t* bytes, int HS,
                             int WS, int C, float* out, int* status, hipStream_t stream,
                             const int* d_images, const InputPrep* prep, int format,
                             const YuvCoeffs& coeffs, int pairs) {
  if (HS <= 0 || WS <= 0 || (HS & 1) || (WS & 1) || C != 3 || !imgs || !bytes || !out ||
      !status)
    return hipErrorInvalidValue;
  if (format != YUV_I420 && format != YUV_NV12) return hipErrorInvalidValue;
  if (prep && prep->nchw) return hipErrorInvalidValue;
  if ((int64_t)HS * WS * 3 > (1 << 30) || images > 65535) return hipErrorInvalidValue;
  if (pairs == 0) pairs = b64_yuv_pairs(HS, WS);
  if (pairs < 1 || pairs > HS / 2) return hipErrorInvalidValue;
  const size_t lds = b64_yuv_lds_bytes(WS, pairs);
  if (lds > kYuvLdsBudget) return hipErrorInvalidValue;
  if (images <= 0) return hipSuccess;
  const dim3 grid((unsigned)((HS / 2 + pairs - 1) / pairs), (unsigned)images);
  const dim3 block(kThreads);
  const int nv12 = format == YUV_NV12;
  // (2 * pairs * WS * WS <= 2 * (kYuvLdsBudget / 3) * 21845 < 2^32: see the kernel's pixel())
  const uint32_t ws_magic = (uint32_t)(0xFFFFFFFFu / (uint32_t)WS) + 1u;
  if (prep && !prep->identity())
    hipLaunchKernelGGL(b64_yuv_kernel<true>, grid, block, lds, stream, imgs, images, d_images,
                       bytes, HS, WS, pairs, ws_magic, nv12, out, status, coeffs, *prep);
  else
    hipLaunchKernelGGL(b64_yuv_kernel<false>, grid, block, lds, stream, imgs, images, d_images,
                       bytes, HS, WS, pairs, ws_magic, nv12, out, status, coeffs, InputPrep());
  return hipGetLastError();
}

}  // namespace gale
