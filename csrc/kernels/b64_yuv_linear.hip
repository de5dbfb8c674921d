// GPU decoder of base64 YUV 4:2:0 frame records with triangle-filtered chroma, input pixel formats
// "i420" / "nv12" with input-yuv-chroma "linear" (gale/kernels.h: b64_yuv_linear_instances).
//
//   {"instances":[{"b64":"<L characters>"}, ...]}      B = HS*WS*3/2 bytes, L = 4 B / 3
//
// Pixel (y, x) takes Y[y][x] and, of either chroma plane C (HS/2 x WS/2), libjpeg's
// h2v2_fancy_upsample in the integer form of csrc/codec/yuv.h:
//   cy0 = y >> 1, cyn = clamp(cy0 -+ 1), cx0 = x >> 1, cxn = clamp(cx0 -+ 1)   (- even, + odd)
//   col(cx) = 3 C[cy0][cx] + C[cyn][cx]      C' = (3 col(cx0) + col(cxn) + (x & 1 ? 7 : 8)) >> 4
// and (Y, U', V') go through the 2^20 integer matrix of yuv.h and the InputPrep fma, fp32 NHWC:
// the bits of codec::yuv420_linear_to_rgb_host.
//
// Work split: a workgroup owns `pairs` whole row pairs p0 .. p0 + n - 1 of one frame, as in
// b64_yuv.hip, and needs the chroma rows p0 - 1 .. p0 + n, clamped to the frame: the halo rows
// only lengthen the chroma byte ranges, which stay contiguous (one range for NV12, two for I420).
//   Phase 1  base64 -> bytes in LDS, range by range: a lane takes 16 characters (4 quads, 12
//            bytes) through b64::load_window, which states the read bound; a range's last lane
//            judges only its own characters. A quad that straddles two ranges or two workgroups'
//            ranges is decoded by every owner and halo rows are decoded (and judged) twice, so
//            every character of the string is judged by at least one workgroup. One barrier.
//   Phase 2  A lane owns a block of 2 rows x 8 columns, four 2 x 2 quads. It reads its 2 x 8
//            luma bytes and, of each plane, columns 4 cb - 1 .. 4 cb + 4 of the three chroma
//            rows p - 1, p, p + 1 as aligned LDS dwords realigned with v_alignbyte_b32 (6 luma
//            + 18 (I420) or 12 (NV12) dword reads for 16 pixels; no byte read). The six vertical
//            sums 3 C[p] + C[p -+ 1] of a plane and row are computed once and serve the eight
//            horizontal taps of that row; a column outside the plane is never selected (the
//            neighbour falls back to the centre column: 4 col, libjpeg's edge rule). Every pixel
//            is converted exactly once. Blocks are linearised over the workgroup's row pairs,
//            g = r nb + cb, nb = ceil(WS / 8); a 256-thread workgroup takes 256 blocks an
//            iteration (one iteration unless a single row pair is wider than 2048 pixels).
//   Stores   One image row of a wave's blocks at a time is re-staged through per-wave LDS, as in
//            yuv420_hi.hip: lane l writes floats [24 l, 24 l + 24), waits for the wave's own LDS
//            writes, reads back unit l + 64 i and stores it at the address of the block the unit
//            belongs to. 16-byte units (1 KB an instruction) when WS mod 4 == 0 and the image
//            base is 16-byte aligned, 8-byte units at 4-byte alignment otherwise; contiguous over
//            a wave except where a row ends; units past a row's end or the last block are masked.
// LDS budget (b64_yuv_linear_lds_bytes): luma 2 pairs WS bytes, chroma with halo (pairs + 2) WS,
// 8 bytes of slack per range (whole quads at either end, rounded to 4), rounded up to 16, then
// 24 KB of float staging (4 waves x 64 lanes x 24 floats) behind it - not over it, because a
// wave stages while another still reads bytes. A realigned read may run up to 12 bytes past a
// range into the next range or the staging rows; such bytes are never selected.
// (3 pairs + 2) WS + 24 + 24 576 <= 65 536: one row pair serves WS <= 8186.
//
// Verdict: a wave with a lane that saw a character outside the alphabet stores the constant 2
// into its record's status (a plain store: every writer stores the same value). The frame is
// written anyway, inside its own slot. No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "b64_decode.cuh"
#include "gale/kernels.h"

namespace gale {
namespace {

constexpr int kThreads = 256;
constexpr int kRowFloats = 24;  // a lane's floats of one image row: 8 pixels
constexpr size_t kStageBytes = (size_t)kThreads * kRowFloats * sizeof(float);

struct __attribute__((aligned(4))) F32x2a {
  float x, y;
};

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

// g -> (g / nb, g mod nb) for 0 <= g < 2^31. magic = ceil(2^32 / nb) (0 for nb == 1, where it
// does not fit): floor(g magic / 2^32) = g / nb or one more, since magic nb - 2^32 < nb.
__device__ __forceinline__ void block_rc(int g, int nb, uint32_t magic, int* r, int* cb) {
  int q = nb == 1 ? g : (int)__umulhi((uint32_t)g, magic);
  int rem = g - q * nb;
  if (rem < 0) --q, rem += nb;
  *r = q, *cb = rem;
}

// The 4 NW LDS bytes from byte a >= 0 on, any alignment: NW + 1 aligned dword reads.
template <int NW>
__device__ __forceinline__ void lds_run(const uint32_t* words, int a, uint32_t* x) {
  const uint32_t sh = (uint32_t)(a & 3);
  const uint32_t* const w = words + (a >> 2);
  uint32_t v[NW + 1];
#pragma unroll
  for (int j = 0; j <= NW; ++j) v[j] = w[j];
#pragma unroll
  for (int j = 0; j < NW; ++j) x[j] = __builtin_amdgcn_alignbyte(v[j + 1], v[j], sh);
}
// byte i (a constant after unrolling) of a little-endian dword stream
__device__ __forceinline__ int byte_of(const uint32_t* s, int i) {
  return (int)((s[i >> 2] >> (8 * (i & 3))) & 255u);
}

__device__ __forceinline__ float clamp8f(int acc) { return (float)min(max(acc >> 20, 0), 255); }

// One row of a block, 8 pixels -> 24 floats. yw: the row's 8 luma bytes; s[plane][i]: the row's
// vertical sums of chroma columns 4 cb - 1 + i (junk where the column is outside the plane).
template <bool PREP>
__device__ __forceinline__ void convert_row(const uint32_t* yw, const int (*s)[6], int cb, int cw,
                                            const YuvCoeffs& k, const InputPrep& prep, float* f) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int cx = 4 * cb + j;
    int c[2][2];  // [plane][x & 1]
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
      const int mid = s[pl][j + 1];
      const int nl = cx > 0 ? s[pl][j] : mid, nr = cx + 1 < cw ? s[pl][j + 2] : mid;
      c[pl][0] = (3 * mid + nl + 8) >> 4;
      c[pl][1] = (3 * mid + nr + 7) >> 4;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int yy = k.cy * (byte_of(yw, 2 * j + h) - k.yo) + (1 << 19);
      const int u = c[0][h] - 128, v = c[1][h] - 128;
      const float rgb[3] = {clamp8f(yy + k.crv * v), clamp8f(yy + k.cgu * u + k.cgv * v),
                            clamp8f(yy + k.cbu * u)};
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        f[3 * (2 * j + h) + ch] = PREP ? __builtin_fmaf(rgb[ch], prep.a[ch], prep.b[ch]) : rgb[ch];
    }
  }
}

// A lane's 24 floats of one row into the wave's staged row, then the wave's row to the image:
// unit lane + 64 i of UF floats goes to dst + offs[i] (offs[i] < 0: masked).
template <int UF>
__device__ __forceinline__ void stage_store_row(float* row, const float* f, bool own, int lane,
                                                float* dst, const int* offs) {
  // (the reads of the row before stay ahead of these writes: LDS serves a wave in order)
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
  if (own) {
    float4* const wl = reinterpret_cast<float4*>(row + kRowFloats * lane);
#pragma unroll
    for (int j = 0; j < kRowFloats / 4; ++j)
      wl[j] = make_float4(f[4 * j], f[4 * j + 1], f[4 * j + 2], f[4 * j + 3]);
  }
  __builtin_amdgcn_wave_barrier();  // (no code: keeps the reads behind every lane's writes)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the wave's own LDS writes)
#pragma unroll
  for (int i = 0; i < kRowFloats / UF; ++i) {
    if (offs[i] < 0) continue;
    if (UF == 4) {
      *reinterpret_cast<float4*>(dst + offs[i]) = reinterpret_cast<const float4*>(row)[lane + 64 * i];
    } else {
      const float2 v = reinterpret_cast<const float2*>(row)[lane + 64 * i];
      *reinterpret_cast<F32x2a*>(dst + offs[i]) = F32x2a{v.x, v.y};
    }
  }
}

// Both rows of the wave's blocks g0 .. g0 + 63 to the image. dst: the first float of the
// workgroup's first row. The second row is converted only after the first has left.
template <int UF, bool PREP>
__device__ __forceinline__ void emit(float* row, const uint32_t* y0, const uint32_t* y1,
                                     const int (*top)[6], const int (*bot)[6], int cb, int cw,
                                     const YuvCoeffs& k, const InputPrep& prep, bool own, int lane,
                                     int g0, int total, int nb, uint32_t magic, int WS, float* dst) {
  constexpr int NU = kRowFloats / UF;  // units of a block's row = units of a lane
  int offs[NU];
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    const int u = lane + 64 * i, gb = g0 + u / NU, ku = u % NU;
    offs[i] = -1;
    if (gb < total) {
      int r, c;
      block_rc(gb, nb, magic, &r, &c);
      // (3 ncol is 6, 12, 18 or 24 floats, UF = 4 only with 12 or 24: a unit is whole or absent)
      if (UF * ku + UF <= 3 * min(8, WS - 8 * c)) offs[i] = (2 * r * WS + 8 * c) * 3 + UF * ku;
    }
  }
  float f[kRowFloats];
  if (own) convert_row<PREP>(y0, top, cb, cw, k, prep, f);
  stage_store_row<UF>(row, f, own, lane, dst, offs);
  if (own) convert_row<PREP>(y1, bot, cb, cw, k, prep, f);
  stage_store_row<UF>(row, f, own, lane, dst + 3 * WS, offs);
}

// NV12: interleaved UV rows, else the planes of I420. PREP: fmaf(v, a[c], b[c]) where a pixel is
// converted (`prep` is never read without it). nb = ceil(WS / 8), nb_magic = ceil(2^32 / nb)
// (block_rc); stage_off: the 16-byte aligned LDS offset of the float staging rows.
// Bound to four waves a SIMD (128 VGPRs, 28 bytes of scratch a lane): other workgroups of the CU
// fill the wait at the barrier, and at 178 VGPRs and two waves the kernel measured 11-16 % slower.
template <bool NV12, bool PREP>
__global__ __launch_bounds__(kThreads, 4) void b64_yuv_linear_kernel(
    const B64Image* imgs, int images, const int* d_images, const uint8_t* bytes, int HS, int WS,
    int pairs, int nb, uint32_t nb_magic, int stage_off, float* out, int* status, YuvCoeffs k,
    InputPrep prep) {
  if (d_images) images = min(images, *d_images);
  const int img = (int)blockIdx.y;
  if (img >= images) return;  // (workgroup-uniform, before any barrier or memory access)
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_words[];
  const B64Image d = imgs[img];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int hw = HS * WS, ch = HS >> 1, cw = WS >> 1;
  const int p0 = (int)blockIdx.x * pairs;  // the block's first row pair
  const int n = min(pairs, ch - p0);       // its row pairs (>= 1: the grid is exact)
  // its chroma rows c0 .. c1: the pairs' own and one halo row either side, inside the frame
  const int c0 = max(p0 - 1, 0), c1 = min(p0 + n, ch - 1), ncr = c1 - c0 + 1;
  // ---- the block's byte ranges: luma, then U and V (I420) or UV (NV12; no third range)
  const int yb0 = 2 * p0 * WS;
  const int ub0 = hw + (NV12 ? c0 * WS : c0 * cw);
  const int un = NV12 ? ncr * WS : ncr * cw;
  const int vb0 = ub0 + (hw >> 2);
  const Range ry = make_range(yb0, yb0 + 2 * n * WS, 0);
  const Range ru = make_range(ub0, ub0 + un, round4(3 * ry.nq));
  const Range rv = make_range(vb0, NV12 ? vb0 : vb0 + un, ru.lds + round4(3 * ru.nq));
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
    // (the window ends inside the string: a range's quads are the string's, halo rows included)
    const b64::Window win = b64::load_window(bytes, d.off, 4 * q0 + 16 * j, nch);
    uint32_t r[4], judged = 0;  // 24 bits -> 3 bytes in memory order (byte 0 first)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      r[t] = __builtin_bswap32(win.v[t]) >> 8;
      // (no padding: B is a multiple of 3)
      judged |= win.inv[t] & b64::first_bytes(nch - 4 * t);
    }
    bad |= judged != 0;
    // 12 bytes = 3 dwords at a 12-byte lane stride; the range's last lane only the dwords its
    // quads reach into (the range's LDS extent is rounded up to 4 bytes)
    uint32_t* dst = lds_words + ((lds + 12 * j) >> 2);
    const int nbytes = 3 * (nch >> 2);
    dst[0] = r[0] | (r[1] << 24);
    if (nbytes > 4) dst[1] = (r[1] >> 8) | (r[2] << 16);
    if (nbytes > 8) dst[2] = (r[2] >> 16) | (r[3] << 8);
  }
  if (__ballot(bad) != 0 && lane == 0) status[d.rec] = 2;
  __syncthreads();
  // ---- phase 2: blocks of 2 rows x 8 columns (no workgroup barrier from here on)
  const int ay = ry.lds + (yb0 - 3 * ry.q0);  // LDS byte of the block's first luma byte,
  const int au = ru.lds + (ub0 - 3 * ru.q0);  // of U[c0][0]
  const int av = NV12 ? au + 1 : rv.lds + (vb0 - 3 * rv.q0);  // and of V[c0][0]
  float* const row =
      reinterpret_cast<float*>(lds_words + (stage_off >> 2)) + (tid >> 6) * (kRowFloats * 64);
  // (a later slot or row pair is 16-byte aligned with the image base when WS mod 4 == 0)
  float* const dst = out + (int64_t)d.slot * (3 * (int64_t)hw) + 6 * (int64_t)p0 * WS;
  const bool wide = (WS & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  const int total = n * nb;  // the workgroup's blocks
  for (int base = 0; base < total; base += kThreads) {
    const int g = base + tid, g0 = g - lane;
    if (g0 >= total) break;  // (wave-uniform: none of the wave's blocks is left)
    const bool own = g < total;
    uint32_t y0[2] = {0, 0}, y1[2] = {0, 0};
    int top[2][6], bot[2][6], cb = 0;
    if (own) {
      int lr;
      block_rc(g, nb, nb_magic, &lr, &cb);
      const int p = p0 + lr;  // chroma rows p - 1, p, p + 1 of the frame, as rows of the LDS copy
      const int rm = max(p - 1, 0) - c0, r1 = p - c0, rp = min(p + 1, ch - 1) - c0;
      lds_run<2>(lds_words, ay + 2 * lr * WS + 8 * cb, y0);
      lds_run<2>(lds_words, ay + (2 * lr + 1) * WS + 8 * cb, y1);
      if (NV12) {  // 12 bytes a row: U V of columns 4 cb - 1 .. 4 cb + 4 (au >= 4)
        uint32_t a[3], b[3], c[3];
        const int o = au + 8 * cb - 2;
        lds_run<3>(lds_words, o + rm * WS, a);
        lds_run<3>(lds_words, o + r1 * WS, b);
        lds_run<3>(lds_words, o + rp * WS, c);
#pragma unroll
        for (int i = 0; i < 12; ++i) {
          const int m = 3 * byte_of(b, i);
          top[i & 1][i >> 1] = m + byte_of(a, i), bot[i & 1][i >> 1] = m + byte_of(c, i);
        }
      } else {  // 6 of 8 bytes a row and plane
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
          uint32_t a[2], b[2], c[2];
          const int o = (pl ? av : au) + 4 * cb - 1;
          lds_run<2>(lds_words, o + rm * cw, a);
          lds_run<2>(lds_words, o + r1 * cw, b);
          lds_run<2>(lds_words, o + rp * cw, c);
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            const int m = 3 * byte_of(b, i);
            top[pl][i] = m + byte_of(a, i), bot[pl][i] = m + byte_of(c, i);
          }
        }
      }
    }
    if (wide)
      emit<4, PREP>(row, y0, y1, top, bot, cb, cw, k, prep, own, lane, g0, total, nb, nb_magic, WS,
                    dst);
    else
      emit<2, PREP>(row, y0, y1, top, bot, cb, cw, k, prep, own, lane, g0, total, nb, nb_magic, WS,
                    dst);
  }
}

}  // namespace

int b64_yuv_linear_pairs(int HS, int WS) {
  if (HS < 2 || WS < 2) return 0;
  // about 4096 pixels a workgroup: 2 * pairs rows of WS, 256 blocks of 2 x 8
  return std::min(std::max(2048 / WS, 1), HS / 2);
}

size_t b64_yuv_linear_lds_bytes(int WS, int pairs) {
  // luma 2 * pairs * WS, chroma with its halo (pairs + 2) * WS bytes, each of the three ranges
  // widened to whole quads and rounded up to 4; rounded up to 16 for the float staging behind it
  const size_t bytes = ((size_t)3 * (size_t)pairs + 2) * (size_t)WS + 3 * 8;
  return ((bytes + 15) & ~(size_t)15) + kStageBytes;
}
static_assert(((5 * (size_t)kYuv420LinearMaxWS + 24 + 15) & ~(size_t)15) + kStageBytes <=
                      kYuvLdsBudget &&
                  ((5 * (size_t)(kYuv420LinearMaxWS + 2) + 24 + 15) & ~(size_t)15) + kStageBytes >
                      kYuvLdsBudget,
              "kYuv420LinearMaxWS is the widest row pair that fits the LDS budget");

hipError_t b64_yuv_linear_instances(int images, const B64Image* imgs, const uint8_t* bytes, int HS,
                                    int WS, int C, float* out, int* status, hipStream_t stream,
                                    const int* d_images, const InputPrep* prep, int format,
                                    const YuvCoeffs& coeffs, int pairs) {
  if (HS <= 0 || WS <= 0 || (HS & 1) || (WS & 1) || C != 3 || !imgs || !bytes || !out ||
      !status)
    return hipErrorInvalidValue;
  if (format != YUV_I420 && format != YUV_NV12) return hipErrorInvalidValue;
  if (prep && prep->nchw) return hipErrorInvalidValue;
  // (int indices in the kernel: floats and bytes of a frame; grid y)
  if ((int64_t)HS * WS * 3 > (1 << 30) || images > 65535) return hipErrorInvalidValue;
  if (pairs == 0) pairs = b64_yuv_linear_pairs(HS, WS);
  if (pairs < 1 || pairs > HS / 2) return hipErrorInvalidValue;
  const size_t lds = b64_yuv_linear_lds_bytes(WS, pairs);
  if (lds > kYuvLdsBudget) return hipErrorInvalidValue;
  if (images <= 0) return hipSuccess;
  const dim3 grid((unsigned)((HS / 2 + pairs - 1) / pairs), (unsigned)images);
  const int nb = (WS + 7) / 8;
  const uint32_t magic = nb == 1 ? 0u : (uint32_t)(((1ull << 32) + (uint32_t)nb - 1) / (uint32_t)nb);
  const int stage_off = (int)(lds - kStageBytes);
#define GALE_YUVL_LAUNCH(NV12, PREP, P)                                                          \
  hipLaunchKernelGGL((b64_yuv_linear_kernel<NV12, PREP>), grid, dim3(kThreads), lds, stream,     \
                     imgs, images, d_images, bytes, HS, WS, pairs, nb, magic, stage_off, out,    \
                     status, coeffs, P)
  const bool id = !prep || prep->identity();
  if (format == YUV_NV12) {
    if (id) GALE_YUVL_LAUNCH(true, false, InputPrep());
    else GALE_YUVL_LAUNCH(true, true, *prep);
  } else {
    if (id) GALE_YUVL_LAUNCH(false, false, InputPrep());
    else GALE_YUVL_LAUNCH(false, true, *prep);
  }
#undef GALE_YUVL_LAUNCH
  return hipGetLastError();
}

}  // namespace gale
