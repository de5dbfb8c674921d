// GPU demosaic of raw 10-, 12- and 16-bit Bayer mosaic records, in 16-bit words or in the MIPI
// CSI-2 packed groups (gale/kernels.h: raw_bayer_hi_instances; csrc/codec/bayer_hi.h: the forms).
//
//   raw   value = N frames back to back, no envelope; a frame of HS x WS samples S[HS][WS] is
//     10le 12le 16le  2 HS WS bytes      little-endian words, S = word & M
//     10p             5 HS WS / 4 bytes  4 pixels in 5 bytes: bits 9:2 in bytes 0..3, 1:0 in byte 4
//     12p             3 HS WS / 2 bytes  2 pixels in 3 bytes: bits 11:4 in bytes 0, 1, 3:0 in byte 2
//
// Pixel (y, x) becomes fmaf((float)RGB[c], a[c], b[c]), fp32 NHWC, RGB at full depth by the rules
// of csrc/codec/bayer.h on S: the bilinear one, or Malvar's 5 x 5 filter with
// q(n) = clamp((n + 8) >> 4, 0, M), M = 2^bits - 1. Numerators lie in [-12 M, 28 M]: int32 is
// exact. The bits of codec::bayer_hi_to_rgb_host.
//
// The 8-bit kernels (bayer.hip, bayer_malvar.hip) keep a lane's rows in registers, a byte a pixel,
// realigned with v_alignbyte, and evaluate in packed 16-bit lanes. None of that carries over: a
// packed group straddles dwords and has no per-pixel address, a lane's window would unpack each
// group several times, and a 16-bit sample times 12 needs 32 bits. So this kernel unpacks once,
// through LDS. One template <form family, demosaic, prep>, twelve instantiations; the CFA order,
// M and the depth are wave-uniform scalars.
//   Work     A 256-thread workgroup owns a tile of 16 rows x 64 columns of one image
//            (blockIdx.x = tile, row-major; blockIdx.y = image). Workgroups past *d_images exit
//            whole, before LDS or memory.
//   Stage 1  The tile's samples with a halo of R = 2 (bilinear: 1) go to LDS once, as uint16
//            [16 + 2 R][68]: 2720 bytes. A source row y0 - R + ly, reflected (-2 -> 2, -1 -> 1,
//            n -> n - 2, n + 1 -> n - 3) to another row of the same frame, is read as the aligned
//            dwords that cover its bytes of columns x0 - R .. x0 + 64 + R, consecutive lanes
//            consecutive dwords, a dword only when it holds a byte of the frame: the frame's
//            first byte has any phase and the packed row strides 5 WS / 4 and 3 WS / 2 change
//            phase from row to row. A lane holds its dword and the next one and unpacks the
//            samples whose first byte lies in its own: a word's second byte, a group's low-bits
//            byte is at most four bytes on. It masks with M and writes the sample to its LDS
//            column, and a sample at columns 1 .. R or WS - 1 - R .. WS - 2 also to the reflected
//            column -1 .. -R or WS .. WS + R - 1, so stage 2 reads a plain window.
//   Stage 2  After one barrier a lane owns the 2 x 2 quad at (2 (tid / 32), 2 (tid mod 32)) of the
//            tile: one site of each kind, so all lanes run one instruction stream and nothing is
//            computed to be thrown away. It reads its 6 x 6 (4 x 4) window as 3 (2) dwords of
//            sample pairs a row and evaluates in int32; the horizontal pair sums of the four
//            middle rows serve H1 of the quad's rows and D of the other two, and the compiler
//            shares the rest. Green-first chooses by a wave-uniform branch which diagonal of the
//            quad takes which formula pair; blue-first is a select between two channels.
//   Stores   The quad's 2 x 6 floats go to a second LDS array, the tile as [16][192] floats
//            (12288 bytes), and after a second barrier the tile's rows leave in units of 16 bytes
//            when WS mod 4 == 0 and the image base is 16-byte aligned, of 8 bytes otherwise,
//            consecutive lanes consecutive units of an image row (image-uniform, as bayer.hip).
// LDS: 2720 + 12288 = 15008 bytes a workgroup. Banks, stage 2: the 32 lanes of a quad row read
// consecutive dwords of one sample row, conflict-free; a wave's other half reads two sample rows
// on, 68 dwords away, that is 4 banks on whether the banks number 32 or 64, so the halves collide
// only where the hardware serves all 64 lanes in one pass (not measured). The float2 writes of
// the store stage have a stride of 6 dwords between lanes (two-way conflicts at most among 32
// lanes); the reads for the global stores are consecutive.
// Measured on one MI355X (tools/bench_bayer_hi.py, profiles/bayer_hi_ab.jsonl; medians of 7 rounds
// of 200 launches, two runs within 1 - 3 %): 8 frames of 1080 x 1920 take 46 - 49 us bilinear and
// 52 - 63 us malvar (12p the slowest: a divide by 3 and two extracts a byte), 1.25 - 1.34 x and
// 1.26 - 1.53 x the 8-bit kernels and 0.63 - 0.85 x a device copy of the output's bytes; 64 frames
// of 224 x 224 take 13.6 - 15.0 us and 15.3 - 18.7 us, 1.22 - 1.49 x the 8-bit kernels.
// Tried: storing a quad's two 24-byte pieces straight from registers with 8-byte stores, no second
// LDS pass or barrier (one store instruction's 512 bytes spread over 1536): 3 - 8 % slower
// bilinear, 2 - 5 % faster malvar, so the staged form stays. Not tried: a tile of 8 x 128, two
// quads a lane, unpacking a whole 5-byte group or 3-byte pair per lane instead of a dword's bytes.
//
// No atomics, no scratch (the code object's metadata: .private_segment_fixed_size 0 for all
// twelve). A raw frame has no verdict: status is never written. Nothing is read outside the
// aligned dwords that hold a byte of the frame, nothing written outside out + slot*3*HS*WS floats
// of the image; per-image bases are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gale/kernels.h"

namespace gale {
namespace {

constexpr int kThreads = 256;
constexpr int kTileH = 16, kTileW = 64;  // a workgroup's pixels; a lane's quad: kThreads of them
constexpr int kSW = kTileW + 4;          // samples of an LDS row (halo 2 each side): 34 dwords
constexpr int kSH = kTileH + 4;
constexpr int kRowFloats = kTileW * 3;   // 192

enum Form { FORM_LE16 = 0, FORM_P10 = 1, FORM_P12 = 2 };

// Aligned dwords that cover the bytes of kSW samples of a row at any phase: 136, at most 88 and
// at most 102 bytes, plus the 3 bytes the first dword may start early.
template <int FORM>
constexpr int row_dwords() {
  return FORM == FORM_LE16 ? 35 : FORM == FORM_P10 ? 23 : 27;
}

struct __attribute__((aligned(4))) F32x2a {
  float x, y;
};

// Row bytes and the first byte of sample x within its row.
template <int FORM>
__device__ __forceinline__ int row_bytes(int WS) {
  return FORM == FORM_LE16 ? 2 * WS : FORM == FORM_P10 ? (WS >> 2) * 5 : (WS >> 1) * 3;
}
template <int FORM>
__device__ __forceinline__ int first_byte(int x) {
  return FORM == FORM_LE16 ? 2 * x : FORM == FORM_P10 ? (x >> 2) * 5 + (x & 3) : (x >> 1) * 3 + (x & 1);
}

// Stage 1 (file header). smp: [kSH][kSW] samples, row ly = frame row y0 - R + ly, column lx =
// frame column x0 - R + lx. bytes: 4-byte aligned; [fs, fe): the frame's bytes from there.
template <int FORM, int R>
__device__ __forceinline__ void unpack_tile(uint16_t* smp, const uint8_t* bytes, int64_t fs,
                                            int64_t fe, int HS, int WS, int y0, int x0, int th,
                                            int tw, uint32_t M, int tid) {
  constexpr int DW = row_dwords<FORM>();
  const int rb = row_bytes<FORM>(WS);
  const int xa = max(x0 - R, 0), xb = min(x0 + tw + R, WS);  // the frame's columns of the tile
  const int ba = first_byte<FORM>(xa);
  const bool last = x0 + tw == WS;
  for (int it = tid; it < (th + 2 * R) * DW; it += kThreads) {
    const int ly = it / DW, j = it - ly * DW;
    int ry = y0 - R + ly;
    ry = ry < 0 ? -ry : ry >= HS ? 2 * HS - 2 - ry : ry;  // (another row of the same frame)
    const int64_t rs = fs + (int64_t)ry * rb;
    const int64_t a = ((rs + ba) & ~(int64_t)3) + 4 * j;
    // (a dword is loaded only when it holds a byte of the frame; a sample's bytes all do)
    const uint32_t d0 = a + 4 > fs && a < fe ? *reinterpret_cast<const uint32_t*>(bytes + a) : 0u;
    const uint32_t d1 =
        a + 8 > fs && a + 4 < fe ? *reinterpret_cast<const uint32_t*>(bytes + a + 4) : 0u;
    const uint64_t v = (uint64_t)d1 << 32 | d0;
    uint16_t* const row = smp + ly * kSW;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int k = (int)(a + b - rs);  // the byte's place in its row (from -3)
      if (k < 0) continue;
      int x;
      uint32_t s;
      if (FORM == FORM_LE16) {
        if (k & 1) continue;
        x = k >> 1;
        s = (uint32_t)(v >> (8 * b)) & 0xFFFFu & M;
      } else if (FORM == FORM_P10) {
        const int g = (int)((uint32_t)k / 5u), m = k - 5 * g;
        if (m == 4) continue;
        x = 4 * g + m;
        const uint32_t low = (uint32_t)(v >> (8 * (b + 4 - m))) & 0xFFu;  // (b + 4 - m <= 7)
        s = ((uint32_t)(v >> (8 * b)) & 0xFFu) << 2 | ((low >> (2 * m)) & 3u);
      } else {
        const int g = (int)((uint32_t)k / 3u), m = k - 3 * g;
        if (m == 2) continue;
        x = 2 * g + m;
        const uint32_t low = (uint32_t)(v >> (8 * (b + 2 - m))) & 0xFFu;
        s = ((uint32_t)(v >> (8 * b)) & 0xFFu) << 4 | ((low >> (4 * m)) & 15u);
      }
      if (x < xa || x >= xb) continue;
      row[x - x0 + R] = (uint16_t)s;
      if (x0 == 0 && x >= 1 && x <= R) row[R - x] = (uint16_t)s;  // columns -1 .. -R
      // columns WS .. WS + R - 1, at most tw + 2 R - 1 in the tile's row
      if (last && x >= WS - 1 - R && x <= WS - 2) row[2 * (WS - 1) - x - x0 + R] = (uint16_t)s;
    }
  }
}

// One quad from its window w (rows and columns -R .. R + 1 of the quad): c[J][I] = {own, green,
// opposite} of site (J, I) - own: the non-green colour of the site's row. GF: site (0, 0) is green.
template <bool MALVAR, bool GF>
__device__ __forceinline__ void quad(const int (&w)[6][6], int M, int (&c)[2][2][3]) {
  constexpr int R = MALVAR ? 2 : 1;
  const auto q = [M](int n) { return min(max((n + 8) >> 4, 0), M); };
  int p1[4][2];  // the sums of the columns either side of the quad's, rows -1 .. 2
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int i = 0; i < 2; ++i) p1[r][i] = w[R - 1 + r][R + i - 1] + w[R - 1 + r][R + i + 1];
#pragma unroll
  for (int J = 0; J < 2; ++J)
#pragma unroll
    for (int I = 0; I < 2; ++I) {
      const int y = R + J, x = R + I, s = w[y][x];
      const int h1 = p1[J + 1][I], v1 = w[y - 1][x] + w[y + 1][x], d = p1[J][I] + p1[J + 2][I];
      const bool green = (((I + J) & 1) != 0) != GF;
      int own, g, opp;
      if (MALVAR) {
        const int h2 = w[y][x - 2] + w[y][x + 2], v2 = w[y - 2][x] + w[y + 2][x];
        if (green) {
          const int base = 10 * s - 2 * d;
          g = s;
          own = q(base + 8 * h1 - 2 * h2 + v2);
          opp = q(base + 8 * v1 - 2 * v2 + h2);
        } else {
          const int far = h2 + v2;
          own = s;
          g = q(8 * s + 4 * (h1 + v1) - 2 * far);
          opp = q(12 * s + 4 * d - 3 * far);
        }
      } else if (green) {
        g = s, own = (h1 + 1) >> 1, opp = (v1 + 1) >> 1;
      } else {
        own = s, g = (h1 + v1 + 2) >> 2, opp = (d + 2) >> 2;
      }
      c[J][I][0] = own, c[J][I][1] = g, c[J][I][2] = opp;
    }
}

// The tile's th rows of 3 tw floats from LDS to the image, UF floats a unit. dst: the image's
// float of (y0, x0), 4 UF-byte aligned where UF == 4.
template <int UF>
__device__ __forceinline__ void store_tile(const float* stage, float* dst, int WS, int th, int tw,
                                           int tid) {
  constexpr int U = kRowFloats / UF;  // units of a full tile row
  const int nu = 3 * tw / UF;         // (3 tw is a multiple of 6, and of 4 where UF == 4)
#pragma unroll
  for (int i = 0; i < kTileH * U / kThreads; ++i) {
    const int idx = tid + kThreads * i, row = idx / U, k = idx - row * U;
    if (row >= th || k >= nu) continue;
    const float* const s = stage + row * kRowFloats + UF * k;
    float* const d = dst + (int64_t)row * 3 * WS + UF * k;
    if (UF == 4) {
      *reinterpret_cast<float4*>(d) = *reinterpret_cast<const float4*>(s);
    } else {
      const float2 v = *reinterpret_cast<const float2*>(s);
      *reinterpret_cast<F32x2a*>(d) = F32x2a{v.x, v.y};
    }
  }
}

// FORM: the family of the frame's bytes. MALVAR: the 5 x 5 filter, else bilinear. PREP:
// fmaf(v, a[c], b[c]) (`prep` is never read without it). gf / bf: site (0, 0) is green / the even
// rows' non-green colour is blue. M = 2^bits - 1. bytes: the 4-byte aligned address under the
// caller's pointer and base_phase its phase. ntx = ceil(WS / 64).
template <int FORM, bool MALVAR, bool PREP>
__global__ __launch_bounds__(kThreads) void bayer_hi_kernel(
    const B64Image* imgs, int images, const int* d_images, const uint8_t* bytes, int HS, int WS,
    int ntx, float* out, InputPrep prep, int gf, int bf, uint32_t M, int base_phase) {
  if (d_images) images = min(images, *d_images);
  const int img = (int)blockIdx.y;
  if (img >= images) return;  // (workgroup-uniform, before any LDS or memory access)
  constexpr int R = MALVAR ? 2 : 1, W = 2 * R + 2;
  __shared__ __attribute__((aligned(16))) uint16_t smp[kSH * kSW];
  __shared__ __attribute__((aligned(16))) float stage[kTileH * kRowFloats];
  const int tid = (int)threadIdx.x;
  const int ty = (int)blockIdx.x / ntx, tx = (int)blockIdx.x - ty * ntx;
  const int y0 = ty * kTileH, x0 = tx * kTileW;
  const int th = min(kTileH, HS - y0), tw = min(kTileW, WS - x0);
  const B64Image d = imgs[img];
  const int64_t fs = d.off + base_phase;
  unpack_tile<FORM, R>(smp, bytes, fs, fs + (int64_t)HS * row_bytes<FORM>(WS), HS, WS, y0, x0, th,
                       tw, M, tid);
  __syncthreads();
  const int qy = tid >> 5, qx = tid & 31;
  if (2 * qy < th && 2 * qx < tw) {
    int w[6][6];
    const uint32_t* const s32 = reinterpret_cast<const uint32_t*>(smp);
#pragma unroll
    for (int r = 0; r < W; ++r)
#pragma unroll
      for (int cd = 0; cd <= R; ++cd) {
        const uint32_t v = s32[(2 * qy + r) * (kSW / 2) + qx + cd];
        w[r][2 * cd] = (int)(v & 0xFFFFu), w[r][2 * cd + 1] = (int)(v >> 16);
      }
    int c[2][2][3];
    if (gf) quad<MALVAR, true>(w, (int)M, c);  // (wave-uniform)
    else quad<MALVAR, false>(w, (int)M, c);
#pragma unroll
    for (int J = 0; J < 2; ++J) {
      const bool blue_row = (J == 1) != (bf != 0);  // the non-green colour of this row
      float f[6];
#pragma unroll
      for (int I = 0; I < 2; ++I) {
        const int px[3] = {blue_row ? c[J][I][2] : c[J][I][0], c[J][I][1],
                           blue_row ? c[J][I][0] : c[J][I][2]};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float v = (float)px[ch];
          f[3 * I + ch] = PREP ? __builtin_fmaf(v, prep.a[ch], prep.b[ch]) : v;
        }
      }
      float2* const o = reinterpret_cast<float2*>(stage + (2 * qy + J) * kRowFloats + 6 * qx);
      o[0] = make_float2(f[0], f[1]), o[1] = make_float2(f[2], f[3]), o[2] = make_float2(f[4], f[5]);
    }
  }
  __syncthreads();
  const int hw = HS * WS;  // (3 hw <= 2^30)
  float* const img_dst = out + (int64_t)d.slot * (3 * hw);
  float* const dst = img_dst + ((int64_t)y0 * WS + x0) * 3;
  // (image-uniform; a later slot is 16-byte aligned with the first: 12 hw bytes, hw mod 4 == 0)
  if ((WS & 3) == 0 && (reinterpret_cast<uintptr_t>(img_dst) & 15) == 0)
    store_tile<4>(stage, dst, WS, th, tw, tid);
  else
    store_tile<2>(stage, dst, WS, th, tw, tid);
}

}  // namespace

hipError_t raw_bayer_hi_instances(int images, const B64Image* imgs, const uint8_t* bytes, int HS,
                                  int WS, int C, float* out, int* status, hipStream_t stream,
                                  const int* d_images, const InputPrep* prep, int order, int bits,
                                  int packing, bool malvar) {
  if (HS <= 0 || WS <= 0 || ((HS | WS) & 1) || C != 3 || !imgs || !bytes || !out || !status)
    return hipErrorInvalidValue;
  if (!bayer_is_order(order) || !bayer_hi_is_form(bits, packing)) return hipErrorInvalidValue;
  if (!bayer_hi_bytes(HS, WS, bits, packing)) return hipErrorInvalidValue;  // (10p: WS mod 4)
  if (malvar && (HS < 4 || WS < 4)) return hipErrorInvalidValue;
  if (prep && prep->nchw) return hipErrorInvalidValue;
  // (int indices in the kernel: floats and bytes of a frame; grid y)
  if ((int64_t)HS * WS * 3 > (1 << 30) || images > 65535) return hipErrorInvalidValue;
  if (images <= 0) return hipSuccess;
  const int ntx = (WS + kTileW - 1) / kTileW, nty = (HS + kTileH - 1) / kTileH;
  const dim3 grid((unsigned)(ntx * nty), (unsigned)images);
  // the kernel's alignment is reckoned from its byte pointer: hand it the aligned address under
  // `bytes` and let it add the pointer's own phase to every offset
  const int phase = (int)(reinterpret_cast<uintptr_t>(bytes) & 3);
  const uint8_t* const abytes = bytes - phase;
  const int gf = bayer_green_first(order), bf = bayer_blue_first(order);
  const uint32_t M = (1u << bits) - 1;
  const bool id = !prep || prep->identity();
  const InputPrep p = id ? InputPrep() : *prep;
#define GALE_HI_LAUNCH(FORM, MALVAR, PREP)                                                       \
  hipLaunchKernelGGL((bayer_hi_kernel<FORM, MALVAR, PREP>), grid, dim3(kThreads), 0, stream, imgs, \
                     images, d_images, abytes, HS, WS, ntx, out, p, gf, bf, M, phase)
#define GALE_HI_FORM(FORM)                                 \
  do {                                                     \
    if (malvar && id) GALE_HI_LAUNCH(FORM, true, false);   \
    else if (malvar) GALE_HI_LAUNCH(FORM, true, true);     \
    else if (id) GALE_HI_LAUNCH(FORM, false, false);       \
    else GALE_HI_LAUNCH(FORM, false, true);                \
  } while (0)
  if (packing == BAYER_PACK_LE16) GALE_HI_FORM(FORM_LE16);
  else if (bits == 10) GALE_HI_FORM(FORM_P10);
  else GALE_HI_FORM(FORM_P12);
#undef GALE_HI_FORM
#undef GALE_HI_LAUNCH
  return hipGetLastError();
}

}  // namespace gale
