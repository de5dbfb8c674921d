// GPU demosaic of raw 8-bit Bayer mosaic records by the gradient-corrected linear filter of
// Malvar, He and Cutler (ICASSP 2004): configuration name bayer_demosaic malvar
// (gale/kernels.h: raw_bayer_malvar_instances). The bilinear demosaic is bayer.hip; this file
// takes over its work split, its block linearisation and its store staging and nothing else.
//
//   raw   value = N frames back to back, B = HS WS bytes each, no envelope
//
// A frame of HS x WS pixels (both even, >= 4) is S[HS][WS], one byte a pixel. Pixel (y, x) becomes
// fmaf((float)RGB[c], a[c], b[c]), fp32 NHWC, RGB the 5 x 5 filter as csrc/codec/bayer.h writes it
// in integers over 16, at indices reflected two deep (-2 -> 2, -1 -> 1, n -> n - 2,
// n + 1 -> n - 3): the bits of codec::bayer_malvar_to_rgb_host. With s = S[y][x],
//     H1 = S[y][x-1] + S[y][x+1]    H2 = S[y][x-2] + S[y][x+2]
//     V1 = S[y-1][x] + S[y+1][x]    V2 = S[y-2][x] + S[y+2][x]
//     D  = S[y-1][x-1] + S[y-1][x+1] + S[y+1][x-1] + S[y+1][x+1]
//     q(n) = clamp((n + 8) >> 4, 0, 255)
//     R or B site:  G = q(8 s + 4 (H1 + V1) - 2 (H2 + V2)),  opposite = q(12 s + 4 D - 3 (H2 + V2))
//     G site:       this row's colour = q(10 s + 8 H1 - 2 D - 2 H2 + V2),
//                   the other = q(10 s + 8 V1 - 2 D - 2 V2 + H2)
// Every numerator and every partial sum lies in [-3060, 7140], so signed 16-bit lanes are exact.
//
// One kernel template <GF, SWAP, PREP>; no source byte passes through LDS, there is no workgroup
// barrier and no atomic, and every pixel is converted once.
//   Work   bayer.hip's: a lane owns a block of 2 rows x 8 columns at even coordinates, blocks
//          linearised g = r nb + cb, nb = ceil(WS / 8), (r, cb) by one multiply-high; the last
//          block of a row pair holds 2, 4 or 6 columns when WS mod 8 != 0. 256 threads a
//          workgroup, or one wave of 64 for a frame of at most 64 blocks.
//   Loads  The block needs rows 2 r - 2 .. 2 r + 3 and columns 8 cb - 2 .. 8 cb + 9: twelve bytes
//          a row, which four aligned dwords cover at any byte phase. (The window 8 cb - 4 ..
//          8 cb + 11 of bayer.hip does not: at phase 3 its four dwords end at column 8 and this
//          filter reads column 9.) They are realigned with v_alignbyte_b32 by the row's own phase
//          into three registers, columns -2 .. 1, 2 .. 5, 6 .. 9 of the block; a dword is loaded
//          only when it holds a byte of the frame, and when all four do the row is one 16-byte
//          load, whatever the phase. Reflected rows are other rows of the same frame: an index,
//          not a path. Columns -2, -1 and WS, WS + 1 are copied from 2, 1 and WS - 2, WS - 3
//          inside the three registers, on the first and last block of a row pair only (a tail of
//          2 columns finds WS - 3 at its own column -1).
//   Sums   A row's registers are split into their even-column and odd-column bytes as 16-bit
//          pairs, E[j] = columns (4 j - 2, 4 j) and O[j] = (4 j - 1, 4 j + 1), and the pairs
//          shifted by one half, Es[k] = (4 k, 4 k + 2), Os[k] = (4 k + 1, 4 k + 3), are the
//          block's own pixels. Colour alternates with column parity, so both halves of such a
//          register are one site type and take one formula: nothing is computed to be thrown
//          away, and the site type is a compile-time fact of the unrolled loop. A row's
//              H1 of Es[k] = O[k] + Os[k]      H2 of Es[k] = E[k] + E[k+1]
//              H1 of Os[k] = Es[k] + E[k+1]    H2 of Os[k] = O[k] + O[k+1]
//          V1, V2 are adds of the centre pairs of rows y -+ 1, y -+ 2 and D is H1 of rows y - 1
//          and y + 1. The five sums are taken once a pixel pair and shared by its two formulas,
//          in packed signed 16-bit arithmetic (v_pk_add_i16, v_pk_mad_i16 / shifts,
//          v_pk_ashrrev_i16, v_pk_max_i16 / v_pk_min_i16 for the clamp); the two results of a
//          register go to float by v_cvt_f32_ubyte0 / ubyte2. The second row of a block is
//          converted after the first has been stored, so 24 floats are live, not 48.
//   Stores bayer.hip's: one image row of the blocks at a time is re-staged per wave through LDS,
//          16-byte units when WS mod 4 == 0 and the image base is 16-byte aligned, 8-byte units
//          otherwise; units past a row's end or the last block are masked. 6 KB of LDS a wave.
// Not tried: keeping the split pairs of all six rows live across both output rows (the second
// row's are recomputed from the 18 row registers instead); cross-lane moves for the halo.
//
// A raw frame has no verdict: status is never written. Nothing is written outside
// out + slot*3*HS*WS floats of the image. Workgroups past *d_images exit as a whole before
// touching LDS or memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gale/kernels.h"

namespace gale {
namespace {

constexpr int kThreads = 256;    // four waves, one block a lane (one wave for a small frame)
constexpr int kRowFloats = 24;   // a lane's floats of one image row: 8 pixels
constexpr uint32_t kLow = 0x00FF00FFu;  // the even bytes of a dword, as two 16-bit lanes

typedef short S16x2 __attribute__((ext_vector_type(2)));  // two pixels of one site type

struct __attribute__((aligned(4))) U32x4a {
  uint32_t x, y, z, w;
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

// The 12 bytes at bytes + a - 2: columns -2 .. 9 of a block whose column 0 is byte a, as
// x[0] = columns -2 .. 1, x[1] = 2 .. 5, x[2] = 6 .. 9. bytes is 16-byte aligned; [fs, fe) are
// the frame's bytes. Bytes outside the frame are zero or the buffer's own (of an aligned dword
// that also holds a byte of the frame).
__device__ __forceinline__ void load_row(const uint8_t* bytes, int64_t a, int64_t fs, int64_t fe,
                                         uint32_t* x) {
  const uint32_t sh = (uint32_t)((a - 2) & 3);
  const int64_t a0 = a - 2 - sh;  // (the four dwords at a0 cover columns -2 - sh .. 13 - sh)
  uint32_t w[4];
  if (a0 + 4 > fs && a0 + 12 < fe) {  // (all four hold a byte of the frame)
    const U32x4a v = *reinterpret_cast<const U32x4a*>(bytes + a0);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // (a dword is loaded only when it holds a byte of the frame)
      const int64_t d = a0 + 4 * j;
      w[j] = d + 4 > fs && d < fe ? *reinterpret_cast<const uint32_t*>(bytes + d) : 0u;
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) x[j] = __builtin_amdgcn_alignbyte(w[j + 1], w[j], sh);
}

// The reflected columns of a loaded row: columns -2, -1 := columns 2, 1 on the first block of a
// row pair; columns ncol, ncol + 1 := columns ncol - 2, ncol - 3 on the last (ncol = 2, 4, 6 or 8
// columns; WS >= 4, so a first block is never a tail of 2). Column k is byte (k + 2) mod 4 of
// x[(k + 2) / 4].
__device__ __forceinline__ void mirror_cols(uint32_t* x, bool first, bool last, int ncol) {
  if (first) x[0] = (x[0] & 0xFFFF0000u) | (x[1] & 0xFFu) | ((x[0] >> 16) & 0xFF00u);
  if (last) {
    if (ncol == 8) x[2] = (x[2] & 0x0000FFFFu) | ((x[2] & 0xFFu) << 16) | (x[1] & 0xFF000000u);
    else if (ncol == 6) x[2] = (x[2] & 0xFFFF0000u) | ((x[1] >> 16) & 0xFFu) | (x[1] & 0xFF00u);
    else if (ncol == 4) x[1] = (x[1] & 0x0000FFFFu) | ((x[1] & 0xFFu) << 16) | (x[0] & 0xFF000000u);
    else x[1] = (x[1] & 0xFFFF0000u) | ((x[0] >> 16) & 0xFFu) | (x[0] & 0xFF00u);
  }
}

// The pixel pairs of a row of a block and their horizontal sums. Pair t = 2 k + p: the columns
// (4 k + p, 4 k + p + 2), p the column parity. c: the samples; h1 / h2: the sums of the columns
// one / two to either side. (Sums of two or four bytes: no carry between the 16-bit lanes.)
struct RowPairs {
  uint32_t c[4], h1[4], h2[4];
};

template <bool H1, bool H2>
__device__ __forceinline__ RowPairs split_row(const uint32_t* x) {
  uint32_t e[3], o[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) e[j] = x[j] & kLow, o[j] = (x[j] >> 8) & kLow;
  RowPairs r;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint32_t es = __builtin_amdgcn_alignbyte(e[k + 1], e[k], 2);
    const uint32_t os = __builtin_amdgcn_alignbyte(o[k + 1], o[k], 2);
    r.c[2 * k] = es, r.c[2 * k + 1] = os;
    if (H1) r.h1[2 * k] = o[k] + os, r.h1[2 * k + 1] = es + e[k + 1];
    if (H2) r.h2[2 * k] = e[k] + e[k + 1], r.h2[2 * k + 1] = o[k] + o[k + 1];
  }
  return r;
}

__device__ __forceinline__ S16x2 pk(uint32_t v) { return __builtin_bit_cast(S16x2, v); }

// q(n) = clamp((n + 8) >> 4, 0, 255) of both lanes; the results are bytes 0 and 2 of the dword.
__device__ __forceinline__ uint32_t quant(S16x2 n) {
  const S16x2 v = (n + (S16x2)(8)) >> (S16x2)(4);
  return __builtin_bit_cast(
      uint32_t, __builtin_elementwise_min(__builtin_elementwise_max(v, (S16x2)(0)), (S16x2)(255)));
}

// Row J (0 or 1) of a block, 8 pixels -> 24 floats. x2n, xn, xc, xs, x2s: the rows two above, one
// above, of, one below and two below the pixels (columns reflected).
template <int J, bool GF, bool SWAP, bool PREP>
__device__ __forceinline__ void convert_row(const uint32_t* x2n, const uint32_t* xn,
                                            const uint32_t* xc, const uint32_t* xs,
                                            const uint32_t* x2s, const InputPrep& prep, float* f) {
  const RowPairs c = split_row<true, true>(xc);
  const RowPairs n = split_row<true, false>(xn), s = split_row<true, false>(xs);
  const RowPairs n2 = split_row<false, false>(x2n), s2 = split_row<false, false>(x2s);
  constexpr bool blue_row = (J == 1) != SWAP;  // the non-green colour of this row
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const S16x2 sv = pk(c.c[t]), h1 = pk(c.h1[t]), h2 = pk(c.h2[t]);
    const S16x2 v1 = pk(n.c[t] + s.c[t]), v2 = pk(n2.c[t] + s2.c[t]);
    const S16x2 d = pk(n.h1[t] + s.h1[t]);
    uint32_t own, g, opp;  // own: this row's non-green colour; opp: that of the rows next to it
    if (((((t & 1) + J) & 1) != 0) != GF) {
      const S16x2 base = sv * (S16x2)(10) - d * (S16x2)(2);
      g = c.c[t];
      own = quant(base + h1 * (S16x2)(8) - h2 * (S16x2)(2) + v2);
      opp = quant(base + v1 * (S16x2)(8) - v2 * (S16x2)(2) + h2);
    } else {
      const S16x2 far = h2 + v2;
      own = c.c[t];
      g = quant(sv * (S16x2)(8) + (h1 + v1) * (S16x2)(4) - far * (S16x2)(2));
      opp = quant(sv * (S16x2)(12) + d * (S16x2)(4) - far * (S16x2)(3));
    }
    const uint32_t px[3] = {blue_row ? opp : own, g, blue_row ? own : opp};
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int i = 4 * (t >> 1) + 2 * half + (t & 1);  // the pixel's column in the block
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float v = (float)((px[ch] >> (16 * half)) & 255u);
        f[3 * i + ch] = PREP ? __builtin_fmaf(v, prep.a[ch], prep.b[ch]) : v;
      }
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

// Both rows of the wave's blocks to the image. f: this lane's first row; the second is converted
// from x (the block's six loaded rows) only after the first has left (24 live floats).
template <int UF, bool GF, bool SWAP, bool PREP>
__device__ __forceinline__ void emit(float* row, float* f, const uint32_t (*x)[3],
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
  if (own) convert_row<1, GF, SWAP, PREP>(x[1], x[2], x[3], x[4], x[5], prep, f);
  stage_store_row<UF>(row, f, own, lane, img_dst + 3 * WS, offs);
}

// GF: site (0, 0) is green (grbg, gbrg). SWAP: the even rows' non-green colour is blue (bggr,
// gbrg). PREP: fmaf(v, a[c], b[c]) where a pixel is converted (`prep` is never read without it).
// bytes: the 16-byte aligned address under the caller's pointer and base_phase its phase.
// nb = ceil(WS / 8) and nb_magic = ceil(2^32 / nb) (block_rc). HS, WS >= 4. blockDim.x: 64 or
// 256, with 6144 bytes of dynamic LDS a wave.
template <bool GF, bool SWAP, bool PREP>
__global__ __launch_bounds__(kThreads) void bayer_malvar_kernel(
    const B64Image* imgs, int images, const int* d_images, const uint8_t* bytes, int HS, int WS,
    int nb, uint32_t nb_magic, float* out, InputPrep prep, int base_phase) {
  if (d_images) images = min(images, *d_images);
  const int img = (int)blockIdx.y;
  if (img >= images) return;  // (workgroup-uniform, before any LDS or memory access)
  extern __shared__ __attribute__((aligned(16))) float stage[];  // [waves][kRowFloats * 64]
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int total = (HS >> 1) * nb;  // blocks of the image
  const int g = (int)(blockIdx.x * blockDim.x) + tid, g0 = g - lane;
  if (g0 >= total) return;  // (wave-uniform: none of the wave's blocks is in the image)
  const B64Image d = imgs[img];
  const int hw = HS * WS;  // (3 hw <= 2^30)
  const bool own = g < total;
  float f[kRowFloats];
  uint32_t x[6][3];  // rows 2 r - 2 .. 2 r + 3, columns 8 c - 2 .. 8 c + 9
  if (own) {
    int r, c;
    block_rc(g, nb, nb_magic, &r, &c);
    const int ncol = min(8, WS - 8 * c);  // 2, 4, 6 or 8
    const int64_t fs = d.off + base_phase;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      int y = 2 * r - 2 + j;
      y = y < 0 ? -y : y >= HS ? 2 * HS - 2 - y : y;  // (reflected: another row of the same frame)
      load_row(bytes, fs + (int64_t)y * WS + 8 * c, fs, fs + hw, x[j]);
      mirror_cols(x[j], c == 0, 8 * c + ncol == WS, ncol);
    }
    convert_row<0, GF, SWAP, PREP>(x[0], x[1], x[2], x[3], x[4], prep, f);
  }
  float* const row = stage + (tid >> 6) * (kRowFloats * 64);
  float* const img_dst = out + (int64_t)d.slot * (3 * hw);
  // (image-uniform; a later slot is 16-byte aligned with the first: 12 hw bytes, hw mod 4 == 0)
  if ((WS & 3) == 0 && (reinterpret_cast<uintptr_t>(img_dst) & 15) == 0)
    emit<4, GF, SWAP, PREP>(row, f, x, prep, own, lane, g0, total, nb, nb_magic, WS, img_dst);
  else
    emit<2, GF, SWAP, PREP>(row, f, x, prep, own, lane, g0, total, nb, nb_magic, WS, img_dst);
}

}  // namespace

hipError_t raw_bayer_malvar_instances(int images, const B64Image* imgs, const uint8_t* bytes,
                                      int HS, int WS, int C, float* out, int* status,
                                      hipStream_t stream, const int* d_images,
                                      const InputPrep* prep, int order) {
  if (HS < 4 || WS < 4 || ((HS | WS) & 1) || C != 3 || !imgs || !bytes || !out || !status)
    return hipErrorInvalidValue;
  if (!bayer_is_order(order)) return hipErrorInvalidValue;
  if (prep && prep->nchw) return hipErrorInvalidValue;
  // (int indices in the kernel: floats and bytes of a frame; grid y)
  if ((int64_t)HS * WS * 3 > (1 << 30) || images > 65535) return hipErrorInvalidValue;
  if (images <= 0) return hipSuccess;
  const int nb = (WS + 7) / 8;
  const uint32_t magic = nb == 1 ? 0u : (uint32_t)(((1ull << 32) + (uint32_t)nb - 1) / (uint32_t)nb);
  const int total = HS / 2 * nb;
  const int threads = total <= 64 ? 64 : kThreads;  // (a 32 x 32 frame is one wave's worth)
  const dim3 grid((unsigned)((total + threads - 1) / threads), (unsigned)images);
  const size_t lds = (size_t)(threads / 64) * kRowFloats * 64 * sizeof(float);
  // the kernel's alignment is reckoned from its byte pointer: hand it the aligned address under
  // `bytes` and let it add the pointer's own phase to every offset
  const int phase = (int)(reinterpret_cast<uintptr_t>(bytes) & 15);
  const uint8_t* const abytes = bytes - phase;
#define GALE_MALVAR_LAUNCH(GF, SWAP, PREP, P)                                                   \
  hipLaunchKernelGGL((bayer_malvar_kernel<GF, SWAP, PREP>), grid, dim3(threads), lds, stream,   \
                     imgs, images, d_images, abytes, HS, WS, nb, magic, out, P, phase)
#define GALE_MALVAR_ORDER(GF, SWAP)                               \
  do {                                                            \
    if (id) GALE_MALVAR_LAUNCH(GF, SWAP, false, InputPrep());     \
    else GALE_MALVAR_LAUNCH(GF, SWAP, true, *prep);               \
  } while (0)
  const bool id = !prep || prep->identity();
  switch (order) {
    case BAYER_RGGB: GALE_MALVAR_ORDER(false, false); break;
    case BAYER_BGGR: GALE_MALVAR_ORDER(false, true); break;
    case BAYER_GRBG: GALE_MALVAR_ORDER(true, false); break;
    default: GALE_MALVAR_ORDER(true, true); break;
  }
#undef GALE_MALVAR_ORDER
#undef GALE_MALVAR_LAUNCH
  return hipGetLastError();
}

}  // namespace gale
