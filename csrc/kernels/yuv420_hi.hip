// GPU decoder of raw 10-bit YUV 4:2:0 frame records, input pixel formats "p010le" (what every
// hardware video decoder writes) and "yuv420p10le" (what the software decoders write)
// (gale/kernels.h: raw_yuv420p10_instances).
//
//   raw   value = N frames back to back, B = 3 HS WS bytes each, no envelope
//
// A frame of HS x WS pixels (both even) is little-endian 16-bit words:
//   p010le       Y[HS][WS], UV[HS/2][WS/2][2]             sample = word >> 6
//   yuv420p10le  Y[HS][WS], U[HS/2][WS/2], V[HS/2][WS/2]   sample = word & 1023
// Pixel (y, x) takes Y[y][x] and chroma (y >> 1, x >> 1) and becomes
// fmaf((float)q[c] * 0.25f, a[c], b[c]), q the quarter steps 0 .. 1020 of yuv.h's integer matrix
// at the scale 2^18, fp32 NHWC: the bits of codec::yuv420p10_to_rgb_host.
//
// One kernel template <SEMI, PREP>. Unlike b64_yuv.hip, the other 4:2:0 kernel of the tree, no
// source byte passes through LDS, there is no workgroup barrier and no atomic, and every pixel
// is converted exactly once.
//   Work   A lane owns a block of 2 rows x 8 columns, four 2 x 2 quads: 16 bytes of row 2 r, 16
//          of row 2 r + 1 and the quads' chroma - 16 bytes of interleaved UV (p010le) or 8 + 8
//          of U and V (yuv420p10le). The three chroma products of a quad (crv v, cgu u + cgv v,
//          cbu u) are computed once and serve its four pixels. Blocks are linearised
//          g = r nb + cb, nb = ceil(WS / 8); (r, cb) come from one multiply-high by
//          ceil(2^32 / nb) and a correction by one (the product over-estimates g / nb by less
//          than 1 for g < 2^32). A wave's 64 consecutive blocks span several row pairs
//          (WS = 32: 16) or part of one (WS > 512). The last block of a row pair holds 2, 4 or 6
//          columns when WS mod 8 != 0. 256 threads: 4096 pixels a workgroup.
//   Loads  load_run<NB>: a frame sits at any byte of the staged buffer, so a 16-bit sample may
//          straddle a dword. The launcher hands over the 16-byte aligned address under the
//          caller's pointer and the pointer's phase; the kernel reads the aligned dwords that
//          hold a byte of the run - never one that holds no byte of the frame - and realigns
//          them with v_alignbyte_b32. Y rows and p010le chroma rows start at multiples of 4
//          bytes of a frame, so their phase is the frame's: a scalar operand, and when it is 0 a
//          whole block is one 16-byte load. yuv420p10le chroma rows start at multiples of WS
//          bytes: with WS mod 4 == 2 the phase alternates between row pairs, a per-lane shift
//          (8-byte loads only when WS mod 4 == 0 and the frame's phase is 0).
//   Stores A lane's 24 floats of one image row are contiguous in the image, and those of
//          neighbouring lanes are when the lanes share a row pair. One image row of the blocks
//          at a time is re-staged per wave through LDS: lane l writes [24 l, 24 l + 24), waits
//          for the wave's own LDS writes, reads back unit l + 64 i and stores it at the address
//          of the block the unit belongs to, (r, cb) of block g0 + unit / 6 recomputed the same
//          way (once: both rows use the offsets). Every store instruction of a wave writes 1 KB
//          (16-byte units: WS mod 4 == 0 and a 16-byte aligned image base) or 512 B (8-byte
//          units at 4-byte alignment: a row start is a multiple of 6 floats) that is contiguous
//          except where a row pair ends; units past a row's end or the last block are masked.
//          One row at a time: 24 KB of LDS a workgroup, 24 live floats a lane.
// LDS write side: six 16-byte writes a row at a lane stride of 96 bytes, ds_write_b128 in the
// compiled code. tools/lds_bank_model.py has no rule for that instruction; its extra() on the
// addresses 96 l + 16 j gives, with the service groups and 64 banks of its ds_read_b128 rule, 4
// extra cycles an instruction (1 per 16-lane group), and with the 16 contiguous lanes and 32 banks
// of its ds_write_b64 rule, 12. Both are stand-ins, not a rule for the instruction. A lane stride
// of 112 bytes gives 0 and 4 but breaks the contiguous units of the read side, which is
// conflict-free by the model; the natural layout is kept, as in yuv_planar.hip.
//
// A raw frame has no verdict: status is never written. Nothing is written outside
// out + slot*3*HS*WS floats of the image. Workgroups past *d_images exit as a whole before
// touching LDS or memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gale/kernels.h"

namespace gale {
namespace {

constexpr int kThreads = 256;    // four waves, one block a lane
constexpr int kRowFloats = 24;   // a lane's floats of one image row: 8 pixels

struct __attribute__((aligned(4))) U32x4a {
  uint32_t x, y, z, w;
};
struct __attribute__((aligned(4))) U32x2a {
  uint32_t x, y;
};
struct __attribute__((aligned(4))) F32x2a {
  float x, y;
};

// g -> (g / nb, g mod nb) for 0 <= g < 2^31. magic = ceil(2^32 / nb) (0 for nb == 1, where it
// does not fit): floor(g magic / 2^32) = g / nb or one more, since magic nb - 2^32 < nb.
__device__ __forceinline__ void block_rc(int g, int nb, uint32_t magic, int* r, int* cb) {
  int q = nb == 1 ? g : (int)__umulhi((uint32_t)g, magic);
  int rem = g - q * nb;
  if (rem < 0) --q, rem += nb;
  *r = q, *cb = rem;
}

// NB bytes (8 or 16) at bytes + a, of which the first n (2 .. NB) are read. bytes is 16-byte
// aligned. wide (image-uniform): a is a multiple of 4. Bytes past n are zero or the frame's own.
template <int NB>
__device__ __forceinline__ void load_run(const uint8_t* bytes, int64_t a, int n, bool wide,
                                         uint32_t* x) {
  if (wide && n == NB) {
    if constexpr (NB == 16) {
      const U32x4a v = *reinterpret_cast<const U32x4a*>(bytes + a);
      x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
    } else {
      const U32x2a v = *reinterpret_cast<const U32x2a*>(bytes + a);
      x[0] = v.x, x[1] = v.y;
    }
  } else {
    const uint32_t sh = (uint32_t)(a & 3);
    const uint8_t* const a0 = bytes + (a - sh);
    uint32_t w[NB / 4 + 1];
#pragma unroll
    for (int j = 0; j <= NB / 4; ++j)  // (a dword is loaded only when it holds a byte of the run)
      w[j] = 4 * j < (int)sh + n ? *reinterpret_cast<const uint32_t*>(a0 + 4 * j) : 0u;
#pragma unroll
    for (int j = 0; j < NB / 4; ++j) x[j] = __builtin_amdgcn_alignbyte(w[j + 1], w[j], sh);
  }
}

// The 10 bits of 16-bit word i (a constant after unrolling) of a little-endian dword stream.
template <bool SEMI>
__device__ __forceinline__ int sample_of(const uint32_t* s, int i) {
  return (int)((s[i >> 1] >> (16 * (i & 1) + (SEMI ? 6 : 0))) & 1023u);
}

// One row of a block, 8 pixels -> 24 floats. yw: the row's 8 words; cr / cg / cb: the chroma
// products of the four quads.
template <bool SEMI, bool PREP>
__device__ __forceinline__ void convert_row(const uint32_t* yw, const int* cr, const int* cg,
                                            const int* cb, const YuvCoeffs& k,
                                            const InputPrep& prep, float* f) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int yy = k.cy * (sample_of<SEMI>(yw, i) - k.yo) + (1 << 17);
    const int acc[3] = {yy + cr[i >> 1], yy + cg[i >> 1], yy + cb[i >> 1]};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float x = (float)min(max(acc[ch] >> 18, 0), 1020) * 0.25f;  // (exact)
      f[3 * i + ch] = PREP ? __builtin_fmaf(x, prep.a[ch], prep.b[ch]) : x;
    }
  }
}

// A lane's 24 floats of one row into the wave's staged row, then the wave's row to the image:
// unit lane + 64 i of UF floats goes to dst + offs[i] (offs[i] < 0: masked). dst: the image row
// of the blocks' first (or second) row, 4 UF-byte aligned where UF == 4.
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

// Both rows of the wave's blocks to the image. f0: this lane's first row; second: its second
// row, converted only after the first has left (24 live floats).
template <int UF, bool SEMI, bool PREP>
__device__ __forceinline__ void emit(float* row, float* f, const uint32_t* y1, const int* cr,
                                     const int* cg, const int* cb, const YuvCoeffs& k,
                                     const InputPrep& prep, bool own, int lane, int g0, int total,
                                     int nb, uint32_t magic, int WS, float* img_dst) {
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
  stage_store_row<UF>(row, f, own, lane, img_dst, offs);
  if (own) convert_row<SEMI, PREP>(y1, cr, cg, cb, k, prep, f);
  stage_store_row<UF>(row, f, own, lane, img_dst + 3 * WS, offs);
}

// SEMI: p010le (interleaved UV, the bits at the top), else yuv420p10le (planes, at the bottom).
// PREP: fmaf(v, a[c], b[c]) where a pixel is converted (`prep` is never read without it).
// bytes: the 16-byte aligned address under the caller's pointer and base_phase its phase.
// nb = ceil(WS / 8) and nb_magic = ceil(2^32 / nb) (block_rc).
template <bool SEMI, bool PREP>
__global__ __launch_bounds__(kThreads) void yuv420_hi_kernel(const B64Image* imgs, int images,
                                                             const int* d_images,
                                                             const uint8_t* bytes, int HS, int WS,
                                                             int nb, uint32_t nb_magic, float* out,
                                                             YuvCoeffs k, InputPrep prep,
                                                             int base_phase) {
  if (d_images) images = min(images, *d_images);
  const int img = (int)blockIdx.y;
  if (img >= images) return;  // (workgroup-uniform, before any LDS or memory access)
  __shared__ __attribute__((aligned(16))) float stage[kThreads / 64][kRowFloats * 64];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int total = (HS >> 1) * nb;  // blocks of the image
  const int g = (int)blockIdx.x * kThreads + tid, g0 = g - lane;
  if (g0 >= total) return;  // (wave-uniform: none of the wave's blocks is in the image)
  const B64Image d = imgs[img];
  const int hw = HS * WS;  // (3 hw <= 2^30)
  const bool own = g < total;
  float f[kRowFloats];
  uint32_t y1[4];
  int cr[4], cg[4], cb[4];
  if (own) {
    int r, c;
    block_rc(g, nb, nb_magic, &r, &c);
    const int ncol = min(8, WS - 8 * c);  // 2, 4, 6 or 8
    const int64_t off = d.off + base_phase;
    const bool wide = (off & 3) == 0;
    const int64_t ay = off + (int64_t)4 * r * WS + 16 * c;  // row 2 r: 2 WS bytes a row
    uint32_t y0[4];
    load_run<16>(bytes, ay, 2 * ncol, wide, y0);
    load_run<16>(bytes, ay + 2 * WS, 2 * ncol, wide, y1);
    int u[4], v[4];
    if (SEMI) {
      uint32_t uv[4];  // chroma row r: WS / 2 pairs of 4 bytes
      load_run<16>(bytes, off + (int64_t)2 * hw + (int64_t)2 * r * WS + 16 * c, 2 * ncol, wide, uv);
#pragma unroll
      for (int q = 0; q < 4; ++q) u[q] = sample_of<true>(uv, 2 * q), v[q] = sample_of<true>(uv, 2 * q + 1);
    } else {
      uint32_t ub[2], vb[2];  // chroma row r: WS / 2 words of a plane of hw / 2 bytes
      const int64_t au = off + (int64_t)2 * hw + (int64_t)r * WS + 8 * c;
      const bool cwide = wide && (WS & 3) == 0;
      load_run<8>(bytes, au, ncol, cwide, ub);
      load_run<8>(bytes, au + (hw >> 1), ncol, cwide, vb);
#pragma unroll
      for (int q = 0; q < 4; ++q) u[q] = sample_of<false>(ub, q), v[q] = sample_of<false>(vb, q);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int uu = u[q] - 512, vv = v[q] - 512;
      cr[q] = k.crv * vv, cg[q] = k.cgu * uu + k.cgv * vv, cb[q] = k.cbu * uu;
    }
    convert_row<SEMI, PREP>(y0, cr, cg, cb, k, prep, f);
  }
  float* const row = stage[tid >> 6];
  float* const img_dst = out + (int64_t)d.slot * (3 * hw);
  // (image-uniform; a later slot is 16-byte aligned with the first: 12 hw bytes, hw mod 4 == 0)
  if ((WS & 3) == 0 && (reinterpret_cast<uintptr_t>(img_dst) & 15) == 0)
    emit<4, SEMI, PREP>(row, f, y1, cr, cg, cb, k, prep, own, lane, g0, total, nb, nb_magic, WS,
                        img_dst);
  else
    emit<2, SEMI, PREP>(row, f, y1, cr, cg, cb, k, prep, own, lane, g0, total, nb, nb_magic, WS,
                        img_dst);
}

}  // namespace

hipError_t raw_yuv420p10_instances(int images, const B64Image* imgs, const uint8_t* bytes, int HS,
                                   int WS, int C, float* out, int* status, hipStream_t stream,
                                   const int* d_images, const InputPrep* prep, int format,
                                   const YuvCoeffs& coeffs) {
  if (HS <= 0 || WS <= 0 || ((HS | WS) & 1) || C != 3 || !imgs || !bytes || !out || !status)
    return hipErrorInvalidValue;
  if (!yuv_is_420_hi(format)) return hipErrorInvalidValue;
  if (prep && prep->nchw) return hipErrorInvalidValue;
  // (int indices in the kernel: floats and bytes of a frame; grid y)
  if ((int64_t)HS * WS * 3 > (1 << 30) || images > 65535) return hipErrorInvalidValue;
  if (images <= 0) return hipSuccess;
  const int nb = (WS + 7) / 8;
  const uint32_t magic = nb == 1 ? 0u : (uint32_t)(((1ull << 32) + (uint32_t)nb - 1) / (uint32_t)nb);
  const int total = HS / 2 * nb;
  const dim3 grid((unsigned)((total + kThreads - 1) / kThreads), (unsigned)images);
  // the kernel's alignment is reckoned from its byte pointer: hand it the aligned address under
  // `bytes` and let it add the pointer's own phase to every offset
  const int phase = (int)(reinterpret_cast<uintptr_t>(bytes) & 15);
  const uint8_t* const abytes = bytes - phase;
#define GALE_YUV10_LAUNCH(SEMI, PREP, P)                                                       \
  hipLaunchKernelGGL((yuv420_hi_kernel<SEMI, PREP>), grid, dim3(kThreads), 0, stream, imgs,    \
                     images, d_images, abytes, HS, WS, nb, magic, out, coeffs, P, phase)
  const bool id = !prep || prep->identity();
  if (format == YUV_P010LE) {
    if (id) GALE_YUV10_LAUNCH(true, false, InputPrep());
    else GALE_YUV10_LAUNCH(true, true, *prep);
  } else {
    if (id) GALE_YUV10_LAUNCH(false, false, InputPrep());
    else GALE_YUV10_LAUNCH(false, true, *prep);
  }
#undef GALE_YUV10_LAUNCH
  return hipGetLastError();
}

}  // namespace gale
