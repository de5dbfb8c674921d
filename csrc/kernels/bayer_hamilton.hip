// GPU demosaic of raw 8-bit Bayer mosaic records by the edge-directed interpolation of Hamilton
// and Adams (US 5,629,734; "adaptive colour plane interpolation"): configuration name
// bayer_demosaic hamilton (gale/kernels.h: raw_bayer_hamilton_instances). The linear demosaics are
// bayer.hip and bayer_malvar.hip; this filter is no stencil, so neither work split carries over.
//
//   raw   value = N frames back to back, B = HS WS bytes each, no envelope
//
// A frame of HS x WS pixels (both even, >= 4) is S[HS][WS], one byte a pixel, reflected without
// repeating the edge sample (-1 -> 1, n -> n - 2, ...). Pixel (y, x) becomes
// fmaf((float)RGB[c], a[c], b[c]), fp32 NHWC: the bits of codec::bayer_hamilton_to_rgb_host
// (csrc/codec/bayer.h, where the contract is written out). With s = S[y][x], at an R or B site
//     dH = |W - E| + |2 s - WW - EE|           dV = |N - S| + |2 s - NN - SS|
//     gH = (2 (W + E) + 2 s - WW - EE + 2) >> 2,  gV alike,
//     gA = (2 (W + E + N + S) + 4 s - WW - EE - NN - SS + 4) >> 3
//     G^ = clamp(dH < dV ? gH : dV < dH ? gV : gA, 0, 255)      K = s - G^
// and at a G site G^ = s. Red and blue are interpolated as the colour difference K:
//     G site:    this row's colour = clamp(s + ((K[y][x-1] + K[y][x+1] + 1) >> 1), 0, 255),
//                the other         = clamp(s + ((K[y-1][x] + K[y+1][x] + 1) >> 1), 0, 255)
//     R/B site:  opposite = clamp(G^ + ((K at the four diagonal neighbours + 2) >> 2), 0, 255)
// K is reflected one deep, which equals G^ on S reflected three deep (dH / gH and dV / gV are
// symmetric). Numerators lie in [-510, 2044], K in [-255, 255], sums of four K in [-1020, 1020]:
// signed 16-bit lanes are exact.
//
// A pixel needs its neighbours' interpolated green: an intermediate plane with a halo. A lane of
// bayer_malvar.hip's registers-only split would interpolate 20 greens for its 8 R/B sites from a
// window of 8 rows x 14 columns, which four aligned dwords a row do not cover at every byte phase.
// So a workgroup owns a tile and works in two phases through LDS. One kernel template
// <GF, SWAP, PREP>; no atomics; a tile's ring of K is recomputed, not exchanged.
//   Work     A workgroup owns a tile of 32 rows x 32 columns of one image (blockIdx.x = tile,
//            row-major; blockIdx.y = image): 256 threads, or one wave of 64 when HS <= 8 (a tile
//            then has at most 64 pieces of phase 2). A 32 x 32 frame is one workgroup, a
//            224 x 224 one 49 whole tiles. Every loop strides by blockDim.x.
//   Stage    The tile's bytes with a halo of 3 go to LDS as dwords sb[38][10]: LDS row ly is
//            frame row y0 - 3 + ly reflected (another row of the same frame: an index, not a
//            path), dword k its columns x0 - 4 + 4 k .. + 3. A lane loads the two aligned dwords
//            around one LDS dword - each only when it holds a byte of the frame - and realigns
//            them by the row's own phase with v_alignbyte_b32; consecutive lanes, consecutive
//            dwords. On the frame's first and last tile column, after a barrier, 3 bytes a row
//            are copied to the reflected columns -1 .. -3 and WS .. WS + 2 (WS - 2 - i lies in
//            the halo when the last tile is 2 columns wide, and the tile before such a one has
//            column WS as its halo column 34). Phases 1 and 2 have no edge path.
//   Phase 1  One item a dword of rows -1 .. th, that is both R/B sites of the dword (columns
//            4 k - 4 + p and + 2, p the row's R/B column parity = (y & 1) ^ GF): the centre row's
//            three dwords are shifted by p with v_alignbyte_b32 so that the sites sit in bytes 0
//            and 2, the eight neighbours become 16-bit pairs by further byte-aligns and a mask,
//            the four rows above and below by a shift of 8 p. dH, dV, gH, gV, gA run in packed
//            signed 16-bit arithmetic (v_pk_add / sub / max / min / ashrrev_i16); |x| is
//            max(x, -x); the three-way choice is two sign masks, (dH - dV) >> 15 and
//            (dV - dH) >> 15, and bitwise selects: no branch. K = s - G^ goes to LDS as one dword
//            kb[34][10] of two 16-bit values, the dword's place that of its sites' bytes.
//   Phase 2  After one barrier a lane owns a piece of 1 row x 4 columns, one dword of sb: an R/B
//            pair and a G pair. It reads two dwords of each of the K rows y - 1, y, y + 1 (which
//            two depends on p), joins the pair in the middle with v_alignbyte_b32, and forms the
//            opposite colour of the R/B pair and both colours of the G pair, packed. p and the
//            row's colour are per-lane selects, not branches. The twelve floats are 48
//            consecutive bytes of the image and leave straight from registers: three 16-byte
//            stores when WS mod 4 == 0 and the image base is 16-byte aligned (image-uniform),
//            8-byte units otherwise, 3 of them for a piece of 2 columns.
// LDS: 38 x 40 + 34 x 40 = 2880 bytes a workgroup. Banks: rows are 10 dwords apart and 8 lanes
// read 8 consecutive dwords of a row, so the four rows of 32 lanes span 38 dwords and 6 of 32
// banks are read twice; a stride that avoids it would have to be under 8 dwords.
// Resources (the compiler's report, gfx950, all eight instantiations): 20 VGPRs (21 with PREP),
// 46 SGPRs (52), 2880 bytes of LDS, no scratch, occupancy 8.
// Measured and what was tried: README "Kernels", `bayer_hamilton`. Not tried: 16-byte global
// loads in the stage; bayer.hip's per-wave row re-staging of the floats (a store instruction here
// writes 64 pieces of 16 bytes 48 bytes apart, three of them filling the same lines); a tile of
// 16 x 64; keeping G^ of a row pair in registers and exchanging the ring by cross-lane moves.
//
// A raw frame has no verdict: status is never written. Nothing is read outside the aligned
// dwords that hold a byte of the frame, nothing written outside out + slot*3*HS*WS floats of the
// image. Workgroups past *d_images exit as a whole before touching LDS or memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gale/kernels.h"

namespace gale {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;             // a workgroup's rows and columns
constexpr int kRowDw = 10;            // dwords of an LDS row: columns -4 .. 35 of the tile
constexpr int kSRows = kTile + 6;     // halo 3
constexpr int kKRows = kTile + 2;     // ring 1
constexpr uint32_t kLow = 0x00FF00FFu;  // the even bytes of a dword, as two 16-bit lanes

typedef short S16x2 __attribute__((ext_vector_type(2)));  // two sites of one kind

struct __attribute__((aligned(4))) F32x2a {
  float x, y;
};

__device__ __forceinline__ S16x2 pk(uint32_t v) { return __builtin_bit_cast(S16x2, v); }
__device__ __forceinline__ uint32_t un(S16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ S16x2 pabs(S16x2 v) { return __builtin_elementwise_max(v, -v); }
__device__ __forceinline__ S16x2 clamp255(S16x2 v) {
  return __builtin_elementwise_min(__builtin_elementwise_max(v, (S16x2)(0)), (S16x2)(255));
}

// Stage (file header). sb: [th + 6][kRowDw]. bytes: 4-byte aligned; [fs, fe): the frame's bytes
// from there. nk: the dwords of a row that hold a column below tw + 3.
__device__ __forceinline__ void stage_tile(uint32_t* sb, const uint8_t* bytes, int64_t fs,
                                           int64_t fe, int HS, int WS, int y0, int x0, int th,
                                           int tw, int nk, int tid, int nt) {
  for (int it = tid; it < (th + 6) * kRowDw; it += nt) {
    const int ly = it / kRowDw, k = it - ly * kRowDw;
    if (k >= nk) continue;
    int ry = y0 - 3 + ly;
    ry = ry < 0 ? -ry : ry >= HS ? 2 * HS - 2 - ry : ry;  // (another row of the same frame)
    const int64_t rs = fs + (int64_t)ry * WS + x0 - 4 + 4 * k;
    const uint32_t sh = (uint32_t)(rs & 3);
    const int64_t a = rs - sh;
    // (a dword is loaded only when it holds a byte of the frame)
    const uint32_t d0 = a + 4 > fs && a < fe ? *reinterpret_cast<const uint32_t*>(bytes + a) : 0u;
    const uint32_t d1 =
        sh && a + 8 > fs && a + 4 < fe ? *reinterpret_cast<const uint32_t*>(bytes + a + 4) : 0u;
    sb[it] = __builtin_amdgcn_alignbyte(d1, d0, sh);
  }
  // the frame's end in the tile's columns: at tw on the last tile of a row, at tw + 2 = 34 on the
  // tile before a last one of 2 columns, whose halo column 34 is column WS
  const int end = WS - x0;
  const bool first = x0 == 0, last = end <= tw + 2;
  if (first || last) {  // (workgroup-uniform)
    __syncthreads();
    uint8_t* const s8 = reinterpret_cast<uint8_t*>(sb);
    for (int it = tid; it < (th + 6) * 3; it += nt) {
      const int ly = it / 3, i = it - ly * 3;
      uint8_t* const row = s8 + ly * (4 * kRowDw);  // (column c is byte 4 + c)
      if (first) row[3 - i] = row[5 + i];            // columns -1 - i := 1 + i
      if (last && end + i <= tw + 2) row[4 + end + i] = row[2 + end - i];  // end + i := end - 2 - i
    }
  }
}

// Phase 1 (file header). kb: [th + 2][kRowDw], row ky = tile row ky - 1.
template <bool GF>
__device__ __forceinline__ void green_tile(uint32_t* kb, const uint32_t* sb, int th, int nk,
                                           int tid, int nt) {
  for (int it = tid; it < (th + 2) * kRowDw; it += nt) {
    const int ky = it / kRowDw, j = it - ky * kRowDw;
    if (j >= nk) continue;
    const uint32_t p = (uint32_t)(((ky + 1) & 1) ^ (GF ? 1 : 0));  // (y0 is even)
    const uint32_t* const c = sb + (ky + 2) * kRowDw;  // the sites' own row
    // (the dwords beyond either end serve sites that are never read: any dword does)
    const uint32_t a0 = c[max(j - 1, 0)], b0 = c[j], c0 = c[min(j + 1, kRowDw - 1)];
    const uint32_t A = __builtin_amdgcn_alignbyte(b0, a0, p);  // sites at bytes 0 and 2 of B
    const uint32_t B = __builtin_amdgcn_alignbyte(c0, b0, p);
    const uint32_t Cn = c0 >> (8 * p);
    const S16x2 s = pk(B & kLow), e = pk((B >> 8) & kLow);
    const S16x2 w = pk(__builtin_amdgcn_alignbyte(B, A, 3) & kLow);
    const S16x2 ww = pk(__builtin_amdgcn_alignbyte(B, A, 2) & kLow);
    const S16x2 ee = pk(__builtin_amdgcn_alignbyte(Cn, B, 2) & kLow);
    const uint32_t vs = 8 * p;
    const S16x2 nn = pk((c[j - 2 * kRowDw] >> vs) & kLow), n = pk((c[j - kRowDw] >> vs) & kLow);
    const S16x2 so = pk((c[j + kRowDw] >> vs) & kLow), ss = pk((c[j + 2 * kRowDw] >> vs) & kLow);
    const S16x2 s2 = s + s;
    const S16x2 hs = w + e, hd = s2 - ww - ee, vsum = n + so, vd = s2 - nn - ss;
    const S16x2 dh = pabs(w - e) + pabs(hd), dv = pabs(n - so) + pabs(vd);
    const S16x2 gh = (hs + hs + hd + (S16x2)(2)) >> (S16x2)(2);
    const S16x2 gv = (vsum + vsum + vd + (S16x2)(2)) >> (S16x2)(2);
    const S16x2 ga = (hs + hs + vsum + vsum + hd + vd + (S16x2)(4)) >> (S16x2)(3);
    // (|dH - dV| <= 765: the sign fills the lane)
    const uint32_t mh = un((dh - dv) >> (S16x2)(15)), mv = un((dv - dh) >> (S16x2)(15));
    const uint32_t g = (un(gh) & mh) | (un(gv) & mv) | (un(ga) & ~(mh | mv));
    kb[it] = un(s - clamp255(pk(g)));
  }
}

// Phase 2 (file header): the piece of tile row r, dword j (columns 4 j - 4 .. 4 j - 1) to f[12].
template <bool GF, bool SWAP, bool PREP>
__device__ __forceinline__ void piece(const uint32_t* sb, const uint32_t* kb, int r, int j,
                                      const InputPrep& prep, float* f) {
  const bool p = (((r & 1) != 0) != GF);  // the R/B sites are the odd columns
  const bool blue_row = ((r & 1) != 0) != SWAP;
  const uint32_t sv = sb[(r + 3) * kRowDw + j];
  const uint32_t ev = sv & kLow, od = (sv >> 8) & kLow;
  const S16x2 srb = pk(p ? od : ev), sg = pk(p ? ev : od);
  const uint32_t* const kc = kb + (r + 1) * kRowDw + j;
  // this row: the K pairs left and right of the G sites; their sum is all that is read
  const uint32_t clo = kc[p ? -1 : 0], chi = kc[p ? 0 : 1];
  const S16x2 hsum = pk(__builtin_amdgcn_alignbyte(chi, clo, 2)) + pk(p ? chi : clo);
  const S16x2 kown = pk(p ? chi : clo);
  // the rows above and below: the pairs at the G sites' columns, and either side of the R/B ones
  const uint32_t nlo = kc[(p ? 0 : -1) - kRowDw], nhi = kc[(p ? 1 : 0) - kRowDw];
  const uint32_t slo = kc[(p ? 0 : -1) + kRowDw], shi = kc[(p ? 1 : 0) + kRowDw];
  const S16x2 nat = pk(p ? nlo : nhi), sat = pk(p ? slo : shi);
  const S16x2 dsum = pk(__builtin_amdgcn_alignbyte(nhi, nlo, 2)) + nat +
                     pk(__builtin_amdgcn_alignbyte(shi, slo, 2)) + sat;
  const S16x2 ghat = srb - kown;
  const uint32_t rb_opp = un(clamp255(ghat + ((dsum + (S16x2)(2)) >> (S16x2)(2))));
  const uint32_t g_own = un(clamp255(sg + ((hsum + (S16x2)(1)) >> (S16x2)(1))));
  const uint32_t g_opp = un(clamp255(sg + ((nat + sat + (S16x2)(1)) >> (S16x2)(1))));
  // {own, green, opposite} of the even and of the odd columns; own: this row's non-green colour
  const uint32_t rb[3] = {un(srb), un(ghat), rb_opp}, gg[3] = {g_own, un(sg), g_opp};
  uint32_t px[2][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int cc = c == 1 ? 1 : 2 - c;
    px[0][c] = p ? (blue_row ? gg[cc] : gg[c]) : (blue_row ? rb[cc] : rb[c]);
    px[1][c] = p ? (blue_row ? rb[cc] : rb[c]) : (blue_row ? gg[cc] : gg[c]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float v = (float)((px[i & 1][ch] >> (16 * (i >> 1))) & 255u);
      f[3 * i + ch] = PREP ? __builtin_fmaf(v, prep.a[ch], prep.b[ch]) : v;
    }
}

// GF: site (0, 0) is green (grbg, gbrg). SWAP: the even rows' non-green colour is blue (bggr,
// gbrg). PREP: fmaf(v, a[c], b[c]) where a pixel is converted (`prep` is never read without it).
// bytes: the 4-byte aligned address under the caller's pointer and base_phase its phase.
// ntx = ceil(WS / 32). HS, WS >= 4. blockDim.x: 64 or 256.
template <bool GF, bool SWAP, bool PREP>
__global__ __launch_bounds__(kThreads) void bayer_hamilton_kernel(
    const B64Image* imgs, int images, const int* d_images, const uint8_t* bytes, int HS, int WS,
    int ntx, float* out, InputPrep prep, int base_phase) {
  if (d_images) images = min(images, *d_images);
  const int img = (int)blockIdx.y;
  if (img >= images) return;  // (workgroup-uniform, before any LDS or memory access)
  __shared__ __attribute__((aligned(16))) uint32_t sb[kSRows * kRowDw];
  __shared__ __attribute__((aligned(16))) uint32_t kb[kKRows * kRowDw];
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const int ty = (int)blockIdx.x / ntx, tx = (int)blockIdx.x - ty * ntx;
  const int y0 = ty * kTile, x0 = tx * kTile;
  const int th = min(kTile, HS - y0), tw = min(kTile, WS - x0);
  const int nk = (tw + 10) >> 2;  // (the last byte read is that of column tw + 2: byte tw + 6)
  const B64Image d = imgs[img];
  const int hw = HS * WS;  // (3 hw <= 2^30)
  const int64_t fs = d.off + base_phase;
  stage_tile(sb, bytes, fs, fs + hw, HS, WS, y0, x0, th, tw, nk, tid, nt);
  __syncthreads();
  green_tile<GF>(kb, sb, th, nk, tid, nt);
  __syncthreads();
  float* const img_dst = out + (int64_t)d.slot * (3 * hw);
  // (image-uniform; a later slot is 16-byte aligned with the first: 12 hw bytes, hw mod 4 == 0)
  const bool wide = (WS & 3) == 0 && (reinterpret_cast<uintptr_t>(img_dst) & 15) == 0;
  for (int it = tid; it < 8 * th; it += nt) {
    const int r = it >> 3, j = (it & 7) + 1;
    const int npx = tw - 4 * (j - 1);  // the piece's columns in the frame: <= 0, 2 or >= 4
    if (npx <= 0) continue;
    float f[12];
    piece<GF, SWAP, PREP>(sb, kb, r, j, prep, f);
    float* const dst = img_dst + ((y0 + r) * WS + x0 + 4 * (j - 1)) * 3;
    if (wide) {  // (WS mod 4 == 0: a piece is whole)
#pragma unroll
      for (int u = 0; u < 3; ++u)
        reinterpret_cast<float4*>(dst)[u] =
            make_float4(f[4 * u], f[4 * u + 1], f[4 * u + 2], f[4 * u + 3]);
    } else {
#pragma unroll
      for (int u = 0; u < 6; ++u)
        if (u < 3 || npx >= 4) reinterpret_cast<F32x2a*>(dst)[u] = F32x2a{f[2 * u], f[2 * u + 1]};
    }
  }
}

}  // namespace

hipError_t raw_bayer_hamilton_instances(int images, const B64Image* imgs, const uint8_t* bytes,
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
  const int ntx = (WS + kTile - 1) / kTile, nty = (HS + kTile - 1) / kTile;
  const dim3 grid((unsigned)(ntx * nty), (unsigned)images);
  const int threads = HS <= 8 ? 64 : kThreads;  // (at most 64 pieces a tile: one wave)
  // the kernel's alignment is reckoned from its byte pointer: hand it the aligned address under
  // `bytes` and let it add the pointer's own phase to every offset
  const int phase = (int)(reinterpret_cast<uintptr_t>(bytes) & 3);
  const uint8_t* const abytes = bytes - phase;
#define GALE_HAMILTON_LAUNCH(GF, SWAP, PREP, P)                                                  \
  hipLaunchKernelGGL((bayer_hamilton_kernel<GF, SWAP, PREP>), grid, dim3(threads), 0, stream,    \
                     imgs, images, d_images, abytes, HS, WS, ntx, out, P, phase)
#define GALE_HAMILTON_ORDER(GF, SWAP)                              \
  do {                                                             \
    if (id) GALE_HAMILTON_LAUNCH(GF, SWAP, false, InputPrep());    \
    else GALE_HAMILTON_LAUNCH(GF, SWAP, true, *prep);              \
  } while (0)
  const bool id = !prep || prep->identity();
  switch (order) {
    case BAYER_RGGB: GALE_HAMILTON_ORDER(false, false); break;
    case BAYER_BGGR: GALE_HAMILTON_ORDER(false, true); break;
    case BAYER_GRBG: GALE_HAMILTON_ORDER(true, false); break;
    default: GALE_HAMILTON_ORDER(true, true); break;
  }
#undef GALE_HAMILTON_ORDER
#undef GALE_HAMILTON_LAUNCH
  return hipGetLastError();
}

}  // namespace gale
