// GPU demosaic of raw 8-bit Bayer mosaic records, input pixel formats "bayer_rggb8" /
// "bayer_bggr8" / "bayer_grbg8" / "bayer_gbrg8" - what machine-vision and embedded cameras hand
// out (gale/kernels.h: raw_bayer_instances).
//
//   raw   value = N frames back to back, B = HS WS bytes each, no envelope
//
// A frame of HS x WS pixels (both even) is S[HS][WS], one byte a pixel, R, G or B by its position
// in the 2 x 2 tile the order names. Pixel (y, x) becomes fmaf((float)RGB[c], a[c], b[c]), fp32
// NHWC, RGB the rounded bilinear demosaic of csrc/codec/bayer.h over the 3 x 3 neighbourhood at
// mirrored indices (-1 -> 1, n -> n - 2): the bits of codec::bayer_to_rgb_host.
//
// One kernel template <GF, SWAP, PREP>. The only stencil among the converters of the tree; like
// yuv420_hi.hip, whose block geometry and store staging it takes over, no source byte passes
// through LDS, there is no workgroup barrier and no atomic, and every pixel is converted once.
//   Work   A lane owns a block of 2 rows x 8 columns at even coordinates, so the site pattern
//          inside a block is the same for every block of an image and an order is two
//          compile-time choices: GF, whether site (0, 0) is green (grbg, gbrg), and SWAP, whether
//          the non-green colour of the even rows is blue (bggr, gbrg). Each pixel of the unrolled
//          block knows at compile time whether it is green, so there is no divergent branch on
//          the colour and only the two sums a site needs are computed. Blocks are linearised
//          g = r nb + cb, nb = ceil(WS / 8), (r, cb) by one multiply-high; the last block of a
//          row pair holds 2, 4 or 6 columns when WS mod 8 != 0. A workgroup is 256 threads
//          (4096 pixels), or one wave of 64 for a frame of at most 64 blocks (32 x 32), where
//          three of four waves would only exit.
//   Loads  The block needs rows 2 r - 1 .. 2 r + 2 and columns 8 cb - 1 .. 8 cb + 8. A row is the
//          four aligned dwords that cover columns 8 cb - 4 .. 8 cb + 11, realigned with
//          v_alignbyte_b32 by the row's own phase ((off + y WS) mod 4: it alternates between
//          rows when WS mod 4 == 2); a dword is loaded only when it holds a byte of the frame,
//          and when the phase is 0 and all four do, the row is one 16-byte load. Rows - 1 and HS
//          are rows 1 and HS - 2 of the same frame: an index, not a path. Columns - 1 and WS are
//          copied from columns 1 and WS - 2 inside the loaded dwords, on the first and last
//          block of a row pair only. Neighbouring lanes load overlapping dwords (64 bytes a lane
//          for 16 bytes of its own); they hit the same cache lines.
//   Sums   The two-tap averages (a + b + 1) >> 1 are v_lerp_u8 on four pixels at once: two for
//          the horizontal pairs of a row (the row shifted by one byte either way) and two for
//          the vertical pairs. The four-tap sums are per-pixel 32-bit adds (two chained lerps
//          round twice and are wrong).
//   Stores yuv420_hi.hip's: one image row of the blocks at a time is re-staged per wave through
//          LDS - lane l writes its 24 floats at [24 l, 24 l + 24), waits for the wave's own LDS
//          writes, reads back unit l + 64 i and stores it at the address of the block the unit
//          belongs to. 16-byte units when WS mod 4 == 0 and the image base is 16-byte aligned,
//          8-byte units at 4-byte alignment otherwise; units past a row's end or the last block
//          are masked. 6 KB of LDS a wave (dynamic: 6 or 24 KB a workgroup).
// Not tried: fetching the halo bytes from neighbouring lanes by a cross-lane move instead of
// overlapping loads (a lane's neighbours are in another row pair at block-row ends, so the
// overlapping loads would remain as a second path); 16-bit packed adds for the four-tap sums;
// sharing the staging code with yuv420_hi.hip in a header (that file is left as it is).
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
constexpr uint32_t kOnes = 0x01010101u;  // v_lerp_u8's rounding bits

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

// The 16 bytes at bytes + a - 4: columns -4 .. 11 of a block whose column 0 is byte a. bytes is
// 16-byte aligned; [fs, fe) are the frame's bytes. Bytes outside the frame are zero or the
// buffer's own (of an aligned dword that also holds a byte of the frame).
__device__ __forceinline__ void load_row(const uint8_t* bytes, int64_t a, int64_t fs, int64_t fe,
                                         uint32_t* x) {
  const uint32_t sh = (uint32_t)((a - 4) & 3);
  const int64_t a0 = a - 4 - sh;
  if (sh == 0 && a0 >= fs && a0 + 16 <= fe) {
    const U32x4a v = *reinterpret_cast<const U32x4a*>(bytes + a0);
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
  } else {
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // (a dword is loaded only when it holds a byte of the frame)
      const int64_t d = a0 + 4 * j;
      w[j] = d + 4 > fs && d < fe ? *reinterpret_cast<const uint32_t*>(bytes + d) : 0u;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) x[j] = __builtin_amdgcn_alignbyte(w[j + 1], w[j], sh);
    x[3] = __builtin_amdgcn_alignbyte(0u, w[3], sh);  // (column 8 alone is used of it)
  }
}

// Column k (-1 .. 8, a constant after unrolling) of a loaded row.
__device__ __forceinline__ int col(const uint32_t* x, int k) {
  return (int)((x[(k + 4) >> 2] >> (8 * ((k + 4) & 3))) & 255u);
}

// The mirrored columns of a loaded row: column -1 := column 1 on the first block of a row pair,
// column ncol := column ncol - 2 on the last (ncol = 2, 4, 6 or 8 columns).
__device__ __forceinline__ void mirror_cols(uint32_t* x, bool first, bool last, int ncol) {
  if (first) x[0] = (x[0] & 0x00FFFFFFu) | ((x[1] & 0x0000FF00u) << 16);
  if (last) {
    if (ncol == 8) x[3] = (x[3] & ~0xFFu) | ((x[2] >> 16) & 0xFFu);
    else if (ncol == 6) x[2] = (x[2] & ~0x00FF0000u) | ((x[2] & 0xFFu) << 16);
    else if (ncol == 4) x[2] = (x[2] & ~0xFFu) | ((x[1] >> 16) & 0xFFu);
    else x[1] = (x[1] & ~0x00FF0000u) | ((x[1] & 0xFFu) << 16);
  }
}

// Row J (0 or 1) of a block, 8 pixels -> 24 floats. xn / xc / xs: the rows above, of and below
// the pixels (columns mirrored).
template <int J, bool GF, bool SWAP, bool PREP>
__device__ __forceinline__ void convert_row(const uint32_t* xn, const uint32_t* xc,
                                            const uint32_t* xs, const InputPrep& prep, float* f) {
  // (W + E + 1) >> 1 and (N + S + 1) >> 1 of columns 0 .. 3 and 4 .. 7
  const uint32_t h[2] = {
      __builtin_amdgcn_lerp(__builtin_amdgcn_alignbyte(xc[1], xc[0], 3),
                            __builtin_amdgcn_alignbyte(xc[2], xc[1], 1), kOnes),
      __builtin_amdgcn_lerp(__builtin_amdgcn_alignbyte(xc[2], xc[1], 3),
                            __builtin_amdgcn_alignbyte(xc[3], xc[2], 1), kOnes)};
  const uint32_t v[2] = {__builtin_amdgcn_lerp(xn[1], xs[1], kOnes),
                         __builtin_amdgcn_lerp(xn[2], xs[2], kOnes)};
  constexpr bool blue_row = (J == 1) != SWAP;  // the non-green colour of this row
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int s = col(xc, i);
    int own, g, opp;  // own: this row's non-green colour; opp: that of the rows next to it
    if ((((i + J) & 1) != 0) != GF) {
      g = s, own = (int)((h[i >> 2] >> (8 * (i & 3))) & 255u);
      opp = (int)((v[i >> 2] >> (8 * (i & 3))) & 255u);
    } else {
      own = s;
      g = (col(xn, i) + col(xs, i) + col(xc, i - 1) + col(xc, i + 1) + 2) >> 2;
      opp = (col(xn, i - 1) + col(xn, i + 1) + col(xs, i - 1) + col(xs, i + 1) + 2) >> 2;
    }
    const int px[3] = {blue_row ? opp : own, g, blue_row ? own : opp};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float x = (float)px[ch];
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

// Both rows of the wave's blocks to the image. f: this lane's first row; the second is converted
// from x (the block's four loaded rows) only after the first has left (24 live floats).
template <int UF, bool GF, bool SWAP, bool PREP>
__device__ __forceinline__ void emit(float* row, float* f, const uint32_t (*x)[4],
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
  if (own) convert_row<1, GF, SWAP, PREP>(x[1], x[2], x[3], prep, f);
  stage_store_row<UF>(row, f, own, lane, img_dst + 3 * WS, offs);
}

// GF: site (0, 0) is green (grbg, gbrg). SWAP: the even rows' non-green colour is blue (bggr,
// gbrg). PREP: fmaf(v, a[c], b[c]) where a pixel is converted (`prep` is never read without it).
// bytes: the 16-byte aligned address under the caller's pointer and base_phase its phase.
// nb = ceil(WS / 8) and nb_magic = ceil(2^32 / nb) (block_rc). blockDim.x: 64 or 256, with
// 6144 bytes of dynamic LDS a wave.
template <bool GF, bool SWAP, bool PREP>
__global__ __launch_bounds__(kThreads) void bayer_kernel(const B64Image* imgs, int images,
                                                         const int* d_images,
                                                         const uint8_t* bytes, int HS, int WS,
                                                         int nb, uint32_t nb_magic, float* out,
                                                         InputPrep prep, int base_phase) {
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
  uint32_t x[4][4];  // rows 2 r - 1 .. 2 r + 2, columns 8 c - 4 .. 8 c + 11
  if (own) {
    int r, c;
    block_rc(g, nb, nb_magic, &r, &c);
    const int ncol = min(8, WS - 8 * c);  // 2, 4, 6 or 8
    const int64_t fs = d.off + base_phase;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int y = 2 * r - 1 + j;
      y = y < 0 ? 1 : y >= HS ? HS - 2 : y;  // (mirrored: another row of the same frame)
      load_row(bytes, fs + (int64_t)y * WS + 8 * c, fs, fs + hw, x[j]);
      mirror_cols(x[j], c == 0, 8 * c + ncol == WS, ncol);
    }
    convert_row<0, GF, SWAP, PREP>(x[0], x[1], x[2], prep, f);
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

hipError_t raw_bayer_instances(int images, const B64Image* imgs, const uint8_t* bytes, int HS,
                               int WS, int C, float* out, int* status, hipStream_t stream,
                               const int* d_images, const InputPrep* prep, int order) {
  if (HS <= 0 || WS <= 0 || ((HS | WS) & 1) || C != 3 || !imgs || !bytes || !out || !status)
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
#define GALE_BAYER_LAUNCH(GF, SWAP, PREP, P)                                                    \
  hipLaunchKernelGGL((bayer_kernel<GF, SWAP, PREP>), grid, dim3(threads), lds, stream, imgs,    \
                     images, d_images, abytes, HS, WS, nb, magic, out, P, phase)
#define GALE_BAYER_ORDER(GF, SWAP)                                \
  do {                                                            \
    if (id) GALE_BAYER_LAUNCH(GF, SWAP, false, InputPrep());      \
    else GALE_BAYER_LAUNCH(GF, SWAP, true, *prep);                \
  } while (0)
  const bool id = !prep || prep->identity();
  switch (order) {
    case BAYER_RGGB: GALE_BAYER_ORDER(false, false); break;
    case BAYER_BGGR: GALE_BAYER_ORDER(false, true); break;
    case BAYER_GRBG: GALE_BAYER_ORDER(true, false); break;
    default: GALE_BAYER_ORDER(true, true); break;
  }
#undef GALE_BAYER_ORDER
#undef GALE_BAYER_LAUNCH
  return hipGetLastError();
}

}  // namespace gale
