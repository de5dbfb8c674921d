// GPU decoder of base64 packed-pixel records (gale/kernels.h: b64_packed_instances).
//
//   {"instances":[{"b64":"<L characters>"}, ...]}      B = HS*WS*P bytes, L = 4 * ceil(B / 3)
//
// The host scan has located every string without reading it; this kernel reads the characters,
// judges them, picks each pixel's R, G and B out of its P bytes (csrc/codec/pixfmt.h: bgr24,
// rgba, bgra, gray) and stores fmaf((float)RGB[c], a[c], b[c]) as fp32 NHWC - the bits
// b64_decode_instances gives for the unpacked image sent as an RGB record. a / b are indexed by
// model channel (R, G, B), whatever the order on the wire.
//
// Work split, grid, window load and alignment are b64::b64_decode_body's. This kernel keeps its
// own copy of the ~20 lines of b64::load_window / window_bad (b64_decode.cuh): through the shared
// piece its 64x224x224 cases measured 1-2 % over this form's spread in two A/B sessions. Lane
// k of an image decodes characters [16k, 16k + 16) into bytes [12k, 12k + 12). 12 is a multiple
// of P = 1, 3 and 4, so a lane holds 12 / P whole pixels, F = 36 / P floats: no barrier and no
// cross-lane traffic. A lane loads the aligned 16-byte word under its window's first character
// and, only when the window reaches into it, the next one: at most 15 bytes before a string and
// fewer than 16 past it are read. The image's last lane holds fewer pixels; what is stored is
// bounded by the image's HS*WS*3 floats, never by the characters.
//
// Stores: a wave's 64 F floats are contiguous in the image and start 256 F bytes times the
// wave's index from the image base. They go through per-wave LDS; with a 16-byte aligned image
// base lane l of store instruction i writes floats [4 q, 4 q + 4), q = 64 i + l (1 KB contiguous
// per instruction), otherwise float 64 i + l (256 B contiguous per instruction). The wave's last
// floats stay below the image's HS*WS*3.
//
// LDS write pattern and its bank conflicts (ds_write banks are (a / 4) mod 32 per 32-lane half):
//   bgr24  F = 12  the lane's floats, three ds_write_b128 at a 12-dword lane stride: the rgb
//                  decoder's pattern (3 KB per wave)
//   rgba   F = 9   the lane's floats, nine ds_write_b32 at a 9-dword lane stride: 9 is odd, so
//   bgra           the 32 lanes of a half fall on 32 different banks - conflict-free (2.25 KB
//                  per wave)
//   gray   F = 36  NOT the lane's floats: a 36-dword lane stride puts lanes l and l + 8 on the
//                  same bank (36 mod 32 = 4: 4-way per half). The lane writes its 12 BYTES as
//                  three ds_write_b32 at a 3-dword lane stride (odd: conflict-free; 768 B per
//                  wave) and the read side replicates: a float4 of the wave's output spans two
//                  pixels, two ds_read_u8 of adjacent bytes; the lanes of a half read about 11
//                  consecutive dwords, equal addresses broadcast.
// Static LDS: 12 KB (bgr24), 9 KB (rgba / bgra), 3 KB (gray) per workgroup.
//
// Verdict: a wave with a lane that saw a character outside the alphabet in the data part, or a
// non-'=' in the padding, stores the constant 2 into its record's status (a plain vector store:
// every writer stores the same value). The image is written anyway, inside its own slot.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "b64_decode.cuh"
#include "gale/kernels.h"

namespace gale {
namespace {

constexpr int kThreads = b64::kLanesPerChunk;  // 256
constexpr int kWaves = kThreads / 64;

// dwords of one wave's LDS staging: its floats, or (gray) its bytes
template <int FMT>
constexpr int stage_dwords() {
  return FMT == PACKED_GRAY ? 64 * 3 : 64 * (36 / packed_bpp(FMT));
}

// byte i (0 .. 11) of a lane's window from its four 24-bit groups (byte 0 of a group on top)
__device__ __forceinline__ uint32_t window_byte(const uint32_t (&v)[4], int i) {
  return (v[i / 3] >> (16 - 8 * (i % 3))) & 0xFFu;
}

template <bool PREP>
__device__ __forceinline__ float prepped(uint32_t v, int ch, const InputPrep& prep) {
  const float f = (float)v;
  return PREP ? __builtin_fmaf(f, b64::prep_a(prep, ch), b64::prep_b(prep, ch)) : f;
}

// gray with prep: a lane's channel pattern is fixed up to a rotation - float e = 64 i + lane of
// the wave is channel (i + lane) mod 3, float t of float4 q = 64 i + lane channel (i + t + lane)
// mod 3 - so the lane keeps its coefficients rotated by lane mod 3 and indexes them with what is
// a constant after unrolling (a per-float select chain on the channel made this path 2.6x slower)
struct Rot {
  float a0, a1, a2, b0, b1, b2;
};
__device__ __forceinline__ Rot make_rot(const InputPrep& prep, int lane) {
  const int r = lane % 3, r1 = r == 2 ? 0 : r + 1, r2 = r == 0 ? 2 : r - 1;
  return Rot{b64::prep_a(prep, r), b64::prep_a(prep, r1), b64::prep_a(prep, r2),
             b64::prep_b(prep, r), b64::prep_b(prep, r1), b64::prep_b(prep, r2)};
}
// byte y as rotated channel j (0 .. 2)
template <bool PREP>
__device__ __forceinline__ float gray_float(uint32_t y, int j, const Rot& rot) {
  const float f = (float)y;
  return PREP ? __builtin_fmaf(f, j == 0 ? rot.a0 : j == 1 ? rot.a1 : rot.a2,
                               j == 0 ? rot.b0 : j == 1 ? rot.b1 : rot.b2)
              : f;
}

// Float e (0 .. 64 F - 1) of the wave's output from its staging row; j = (e - lane) mod 3.
template <int FMT, bool PREP>
__device__ __forceinline__ float wave_float(const uint32_t* row, int e, int j, const Rot& rot) {
  if (FMT == PACKED_GRAY)
    // (the wave's first float is channel 0 of a pixel: 64 * 36 floats a wave)
    return gray_float<PREP>(reinterpret_cast<const uint8_t*>(row)[(unsigned)e / 3u], j, rot);
  return reinterpret_cast<const float*>(row)[e];
}

// Floats [4 q, 4 q + 4) of the wave's output; i = (q - lane) mod 3.
template <int FMT, bool PREP>
__device__ __forceinline__ float4 wave_float4(const uint32_t* row, int q, int i, const Rot& rot) {
  if (FMT == PACKED_GRAY) {
    // pixel p from channel c on, then pixel p + 1 (<= 767: 4 q + 3 <= 2303)
    const int p = (int)((unsigned)(4 * q) / 3u), c = 4 * q - 3 * p;
    const uint8_t* lb = reinterpret_cast<const uint8_t*>(row);
    const uint32_t y0 = lb[p], y1 = lb[p + 1];
    float f[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) f[t] = gray_float<PREP>(c + t < 3 ? y0 : y1, (i + t) % 3, rot);
    return make_float4(f[0], f[1], f[2], f[3]);
  }
  return reinterpret_cast<const float4*>(row)[q];
}

template <int FMT, bool PREP>
__global__ __launch_bounds__(kThreads) void b64_packed_kernel(const B64Image* imgs, int images,
                                                              const int* d_images,
                                                              const uint8_t* bytes, int HS,
                                                              int WS, float* out, int* status,
                                                              InputPrep prep) {
  constexpr int P = packed_bpp(FMT);
  constexpr int NPX = 12 / P;   // whole pixels of a lane
  constexpr int F = 3 * NPX;    // its floats
  constexpr int ROW = stage_dwords<FMT>();
  if (d_images) images = min(images, *d_images);
  const int img = (int)blockIdx.y;
  if (img >= images) return;  // (workgroup-uniform)
  const B64Image d = imgs[img];
  __shared__ __attribute__((aligned(16))) uint32_t stage[kWaves][ROW];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  uint32_t* const row = stage[tid >> 6];
  const int per = HS * WS * 3;           // floats of the image (<= 2^30)
  const int B = HS * WS * P;             // bytes of the string (<= 4/3 * 2^30)
  const int L = 4 * ((B + 2) / 3);
  const int pad = (3 - B % 3) % 3;
  const int k = (int)blockIdx.x * kThreads + tid;  // this lane's 16-character group
  const int c0 = 16 * k;
  bool bad = false;
  if (c0 < L) {
    const int nch = min(16, L - c0);     // characters of the string in the window (4, 8, 12, 16)
    const int nd = L - pad - c0;         // data characters from the window's start on
    const int64_t addr = d.off + c0;
    const int ph = (int)(addr & 15);
    const uint8_t* base = bytes + (addr - ph);
    const uint4 lo = *reinterpret_cast<const uint4*>(base);
    // the second word only when the string reaches into it: it ends < 16 bytes past the string
    const uint4 hi = ph + nch > 16 ? *reinterpret_cast<const uint4*>(base + 16)
                                   : make_uint4(0, 0, 0, 0);
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const uint32_t sh = (uint32_t)(ph & 3);
    uint32_t x[4];
    switch (ph >> 2) {  // (wave-uniform: every lane of an image has the string's phase)
#define GALE_ALIGN_WORDS(D)                                \
  _Pragma("unroll") for (int t = 0; t < 4; ++t) x[t] =     \
      __builtin_amdgcn_alignbyte(w[t + (D) + 1], w[t + (D)], sh);
      case 0: GALE_ALIGN_WORDS(0) break;
      case 1: GALE_ALIGN_WORDS(1) break;
      case 2: GALE_ALIGN_WORDS(2) break;
      default: GALE_ALIGN_WORDS(3) break;
#undef GALE_ALIGN_WORDS
    }
    // 4 characters -> 4 sextets -> 24 bits: byte 0 of the group in bits 16 .. 23
    uint32_t inv[4], v[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint32_t sx = b64::b64_sextets4(x[t], &inv[t]) & 0x3F3F3F3Fu;
      const uint32_t h = ((sx & 0x003F003Fu) << 6) | ((sx >> 8) & 0x003F003Fu);
      v[t] = ((h & 0xFFFu) << 12) | (h >> 16);
    }
    if (nd >= 16) {  // every character of the window is a data character
      bad = (inv[0] | inv[1] | inv[2] | inv[3]) != 0;
    } else {         // the string's last lane: data characters, then '=', then not judged
      uint32_t j = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const uint32_t dm = b64::first_bytes(nd - 4 * t);
        j |= (inv[t] & dm) | ((x[t] ^ 0x3D3D3D3Du) & b64::first_bytes(nch - 4 * t) & ~dm);
      }
      bad = j != 0;
    }
    // (every lane writes its whole staging share; what lies past the image is never stored)
    if constexpr (FMT == PACKED_GRAY) {
      // the 12 bytes in memory order, 3 dwords at a 3-dword lane stride
      uint32_t r[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) r[t] = __builtin_bswap32(v[t]) >> 8;
      uint32_t* dst = row + 3 * lane;
      dst[0] = r[0] | (r[1] << 24);
      dst[1] = (r[1] >> 8) | (r[2] << 16);
      dst[2] = (r[2] >> 16) | (r[3] << 8);
    } else {
      float f[F];
#pragma unroll
      for (int px = 0; px < NPX; ++px)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          f[3 * px + c] =
              prepped<PREP>(window_byte(v, px * P + packed_src_offset(FMT, c)), c, prep);
      if constexpr (F == 12) {
        float4* wl = reinterpret_cast<float4*>(row);
        wl[3 * lane] = make_float4(f[0], f[1], f[2], f[3]);
        wl[3 * lane + 1] = make_float4(f[4], f[5], f[6], f[7]);
        wl[3 * lane + 2] = make_float4(f[8], f[9], f[10], f[11]);
      } else {
        float* wl = reinterpret_cast<float*>(row) + F * lane;
#pragma unroll
        for (int j = 0; j < F; ++j) wl[j] = f[j];
      }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the wave's own LDS writes)
  float* const img_dst = out + (int64_t)d.slot * per;
  // the wave's first float, F (k - lane) with k - lane a multiple of 64: a multiple of 16 bytes
  // from the image base. A wave that starts at or past the image's end has nvw <= 0 and stores
  // nothing; a float below nvw was staged by a lane whose window starts inside the string
  // (12 k' < B implies 16 k' < L)
  const int64_t wv0 = (int64_t)F * (k - lane);
  const int nvw = (int)min((int64_t)(64 * F), (int64_t)per - wv0);  // (<= 0: none)
  float* const wdst = img_dst + wv0;
  Rot rot = {};
  if constexpr (FMT == PACKED_GRAY && PREP) rot = make_rot(prep, lane);
  if ((reinterpret_cast<uintptr_t>(img_dst) & 15) == 0) {  // (wave-uniform)
#pragma unroll
    for (int i = 0; i < (F + 3) / 4; ++i) {
      const int q = 64 * i + lane;
      if (4 * q + 4 <= nvw) {
        reinterpret_cast<float4*>(wdst)[q] = wave_float4<FMT, PREP>(row, q, i % 3, rot);
      } else {
#pragma unroll
        for (int t = 0; t < 3; ++t)  // (the image's last, partial float4: at most 3 floats)
          if (4 * q + t < nvw)
            wdst[4 * q + t] = wave_float<FMT, PREP>(row, 4 * q + t, (i + t) % 3, rot);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < F; ++i) {
      const int e = 64 * i + lane;
      if (e < nvw) wdst[e] = wave_float<FMT, PREP>(row, e, i % 3, rot);
    }
  }
  if (__ballot(bad) != 0 && lane == 0) status[d.rec] = 2;
}

template <int FMT>
void launch(dim3 grid, hipStream_t stream, const B64Image* imgs, int images, const int* d_images,
            const uint8_t* bytes, int HS, int WS, float* out, int* status,
            const InputPrep* prep) {
  if (prep && !prep->identity())
    hipLaunchKernelGGL((b64_packed_kernel<FMT, true>), grid, dim3(kThreads), 0, stream, imgs,
                       images, d_images, bytes, HS, WS, out, status, *prep);
  else
    hipLaunchKernelGGL((b64_packed_kernel<FMT, false>), grid, dim3(kThreads), 0, stream, imgs,
                       images, d_images, bytes, HS, WS, out, status, InputPrep());
}

}  // namespace

hipError_t b64_packed_instances(int images, const B64Image* imgs, const uint8_t* bytes, int HS,
                                int WS, int C, float* out, int* status, hipStream_t stream,
                                const int* d_images, const InputPrep* prep, int format) {
  if (HS <= 0 || WS <= 0 || C != 3 || !imgs || !bytes || !out || !status)
    return hipErrorInvalidValue;
  const int P = packed_bpp(format);
  if (P == 0) return hipErrorInvalidValue;
  if (prep && prep->nchw) return hipErrorInvalidValue;
  if ((int64_t)HS * WS * 3 > (1 << 30) || images > 65535) return hipErrorInvalidValue;
  if (images <= 0) return hipSuccess;
  const int64_t B = (int64_t)HS * WS * P, L = 4 * ((B + 2) / 3);
  // lanes with 16 k < L: their first byte 12 k is below B (12 k >= B would mean 16 k >= L)
  const dim3 grid((unsigned)((L + kB64ChunkChars - 1) / kB64ChunkChars), (unsigned)images);
  switch (format) {
    case PACKED_BGR24:
      launch<PACKED_BGR24>(grid, stream, imgs, images, d_images, bytes, HS, WS, out, status, prep);
      break;
    case PACKED_RGBA:
      launch<PACKED_RGBA>(grid, stream, imgs, images, d_images, bytes, HS, WS, out, status, prep);
      break;
    case PACKED_BGRA:
      launch<PACKED_BGRA>(grid, stream, imgs, images, d_images, bytes, HS, WS, out, status, prep);
      break;
    default:
      launch<PACKED_GRAY>(grid, stream, imgs, images, d_images, bytes, HS, WS, out, status, prep);
      break;
  }
  return hipGetLastError();
}

}  // namespace gale
