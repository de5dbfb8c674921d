// GPU decoder of base64 typed tensor records (gale/kernels.h: b64_typed_instances).
//
//   {"instances":[{"b64":"<L characters>"}, ...]}      B = HS*WS*C*E bytes, L = 4 * ceil(B / 3)
//
// The host scan has located every string without reading it; this kernel reads the characters,
// judges them, takes the string's little-endian elements (csrc/codec/elemtype.h: u16, f16, bf16
// with E = 2, f32 with E = 4) and stores fmaf(float32(x), a[c], b[c]) as fp32 NHWC. float32(x) is
// typed_to_float_bits, the host codec's function: exact, integer operations and one multiply by
// 2^-24 between normal numbers (f16 subnormals), so no denormal mode changes it. Without a prep
// the converted bits are stored as they are: no arithmetic op touches an f32 element (-0 and
// subnormals arrive as sent).
//
// Work split, grid, window and alignment are b64::b64_decode_body's, through b64::load_window /
// window_bad (b64_decode.cuh): lane k of an image decodes characters [16k, 16k + 16) into bytes
// [12k, 12k + 12). 12 is a multiple of E = 2 and 4, so a lane holds F = 12 / E whole elements
// (6 or 3 floats): no barrier and no cross-lane traffic. At most 15 bytes before a string and
// fewer than 16 past it are read. The image's last lane holds fewer elements; what is stored and
// what is judged is bounded by the image's HS*WS*C elements, never by the characters. Byte and
// character counts are 64-bit (2^30 elements of 4 bytes are 2^32 bytes); element indices fit an
// int.
//
// Stores, NHWC:
//   F = 6 (u16, f16, bf16)  a wave's 384 floats are contiguous in the image and start 1536 bytes
//       times the wave's index from the image base. They go through per-wave LDS (1.5 KB a wave,
//       6 KB a workgroup): lane l writes its six floats as three ds_write_b64 at a 6-dword lane
//       stride. ds_write banks are (a / 4) mod 32 per group of 16 contiguous lanes: 6 l mod 32,
//       l = 0 .. 15, is 0 6 12 18 24 30 4 10 16 22 28 2 8 14 20 26 - 16 distinct even banks, the
//       second dword of each write on the odd bank above it: conflict-free. With a 16-byte
//       aligned image base lane l of store instruction i then writes floats [4 q, 4 q + 4),
//       q = 64 i + l (1 KB contiguous per instruction, 96 vectors a wave; contiguous ds_read_b128,
//       conflict-free); otherwise float 64 i + l (256 B contiguous per instruction).
//   F = 3 (f32)  a lane's 12 bytes of output abut its neighbour's, so one 12-byte store per lane
//       writes 768 contiguous bytes per wave instruction, every byte of every cache line it
//       touches but the first and last. That is what staging would produce (three ds_write_b32
//       at a 3-dword lane stride, odd, so conflict-free, then 48 float4 per wave), without the
//       LDS round trip and on any 4-byte aligned base: direct stores, no LDS.
//       Only this form was timed (1.7 - 2.0 x the device copy moving the same bytes,
//       profiles/elemtype_decode_ab.jsonl); the staged form was not built, so the choice between
//       them is by this argument, not by a measurement.
// NCHW-ordered strings ([C][H][W] elements, only with a prep) transpose at the store, one float
// per element straight to global memory, as the rgb decoder does.
//
// Verdict: a wave with a lane that saw a character outside the alphabet in the data part, a
// non-'=' in the padding or (f16, bf16, f32) an element of the image with an all-ones exponent,
// judged on the element as sent, stores the constant 2 into its record's status (a plain vector
// store: every writer stores the same value). The image is written anyway, inside its own slot.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "b64_decode.cuh"
#include "gale/kernels.h"

namespace gale {
namespace {

constexpr int kThreads = b64::kLanesPerChunk;  // 256
constexpr int kWaves = kThreads / 64;

// a lane's 12-byte store: three floats at a 4-byte aligned address (one global_store_dwordx3)
typedef float Float3 __attribute__((ext_vector_type(3)));
typedef Float3 Float3Unaligned __attribute__((aligned(4)));

// ET: the element type. PREP: fmaf(v, a[c], b[c]) at the store (`prep` is never read without
// it). NCHW (with PREP): the string's elements are ordered [C][H][W]. CT: the channel count when
// a lane's channel pattern is a compile-time one (1 or 3: F = 6 and F = 3 are whole pixels),
// 0 = general C with a running channel counter.
template <int ET, bool PREP, bool NCHW, int CT>
__global__ __launch_bounds__(kThreads) void b64_typed_kernel(const B64Image* imgs, int images,
                                                             const int* d_images,
                                                             const uint8_t* bytes, int HS,
                                                             int WS, int C, float* out,
                                                             int* status, InputPrep prep) {
  constexpr int E = elem_bytes(ET);
  constexpr int F = 12 / E;  // whole elements of a lane
  constexpr bool STAGED = F == 6 && !NCHW;
  if (d_images) images = min(images, *d_images);
  const int img = (int)blockIdx.y;
  if (img >= images) return;  // (workgroup-uniform)
  const B64Image d = imgs[img];
  __shared__ __attribute__((aligned(16))) float stage[STAGED ? kWaves : 1][STAGED ? 64 * F : 4];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int per = HS * WS * C;              // elements = floats of the image (<= 2^30)
  const int64_t B = (int64_t)per * E;       // bytes of the string (<= 2^32)
  const int64_t L = 4 * ((B + 2) / 3);
  const int pad = (int)((3 - B % 3) % 3);
  const int k = (int)blockIdx.x * kThreads + tid;  // this lane's 16-character group
  const int64_t c0 = 16 * (int64_t)k;
  const int v0 = F * k;                     // first element of this lane (<= per + F * 255)
  const int nv = min(F, per - v0);          // elements of the image in this lane (<= 0: none)
  float* const img_dst = out + (int64_t)d.slot * per;
  bool bad = false;
  if (c0 < L) {  // (then 12 k < B: v0 < per, nv >= 1)
    const int nch = (int)min((int64_t)16, L - c0);       // characters in the window (4 .. 16)
    const int nd = (int)min((int64_t)16, L - pad - c0);  // data characters from its start on
    // the window's start as (64-bit multiple of 2^30) + (int below 2^30), both multiples of 16:
    // every lane of an image keeps the string's phase
    const int clo = (int)(c0 & 0x3FFFFFFF);
    const b64::Window win = b64::load_window(bytes, d.off + (c0 - clo), clo, nch);
    bad = b64::window_bad(win, nd, nch);
    // the 12 bytes in memory order as three dwords (byte 0 of a 24-bit group is on top)
    uint32_t r[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) r[t] = __builtin_bswap32(win.v[t]) >> 8;
    const uint32_t dw[3] = {r[0] | (r[1] << 24), (r[1] >> 8) | (r[2] << 16),
                            (r[2] >> 16) | (r[3] << 8)};
    float f[F];
    bool nonfinite = false;
#pragma unroll
    for (int j = 0; j < F; ++j) {
      uint32_t raw;
      if constexpr (E == 4)
        raw = dw[j];
      else
        raw = (j & 1) ? dw[j / 2] >> 16 : dw[j / 2] & 0xFFFFu;
      nonfinite |= j < nv && typed_nonfinite<ET>(raw);
      f[j] = __uint_as_float(typed_to_float_bits<ET>(raw));
    }
    bad |= nonfinite;
    if constexpr (NCHW) {
      const int hw = HS * WS;
      int ch = v0 / hw, p = v0 - ch * hw;
#pragma unroll
      for (int j = 0; j < F; ++j) {
        if (j < nv) {
          const int cs = min(ch, 3);
          img_dst[(int64_t)p * C + ch] =
              __builtin_fmaf(f[j], b64::prep_a(prep, cs), b64::prep_b(prep, cs));
        }
        if (++p == hw) { p = 0; ++ch; }
      }
    } else {
      if constexpr (PREP) {
        int ch = CT ? 0 : v0 % C;
#pragma unroll
        for (int j = 0; j < F; ++j) {
          const int cs = CT ? j % (CT ? CT : 1) : min(ch, 3);
          f[j] = __builtin_fmaf(f[j], b64::prep_a(prep, cs), b64::prep_b(prep, cs));
          if (!CT && ++ch == C) ch = 0;
        }
      }
      if constexpr (STAGED) {
        // (every lane writes its whole staging share; what lies past the image is never stored)
        float2* wl = reinterpret_cast<float2*>(stage[tid >> 6] + F * lane);
        wl[0] = make_float2(f[0], f[1]);
        wl[1] = make_float2(f[2], f[3]);
        wl[2] = make_float2(f[4], f[5]);
      } else {
        float* dst = img_dst + v0;
        if (nv >= 3) {
          *reinterpret_cast<Float3Unaligned*>(dst) = Float3{f[0], f[1], f[2]};
        } else {
#pragma unroll
          for (int j = 0; j < 2; ++j)
            if (j < nv) dst[j] = f[j];
        }
      }
    }
  }
  if constexpr (STAGED) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the wave's own LDS writes)
    const float* const row = stage[tid >> 6];
    // the wave's first float, F (k - lane) with k - lane a multiple of 64: a multiple of 16 bytes
    // from the image base. A wave that starts at or past the image's end has nvw <= 0 and stores
    // nothing; a float below nvw was staged by a lane whose window starts inside the string
    // (12 k' < B implies 16 k' < L)
    const int wv0 = F * (k - lane);
    const int nvw = min(64 * F, per - wv0);  // (<= 0: none)
    float* const wdst = img_dst + wv0;
    if ((reinterpret_cast<uintptr_t>(img_dst) & 15) == 0) {  // (wave-uniform)
      // 64 F floats are 16 F float4: ceil(16 F / 64) passes of the wave's 64 lanes
      constexpr int kVecPasses = (64 * F / 4 + 63) / 64;
#pragma unroll
      for (int i = 0; i < kVecPasses; ++i) {
        const int q = 64 * i + lane;
        if (4 * q + 4 <= nvw) {
          reinterpret_cast<float4*>(wdst)[q] = reinterpret_cast<const float4*>(row)[q];
        } else {
#pragma unroll
          for (int t = 0; t < 3; ++t)  // (the image's last, partial float4: at most 3 floats)
            if (4 * q + t < nvw) wdst[4 * q + t] = row[4 * q + t];
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < F; ++i) {
        const int e = 64 * i + lane;
        if (e < nvw) wdst[e] = row[e];
      }
    }
  }
  if (__ballot(bad) != 0 && lane == 0) status[d.rec] = 2;
}

template <int ET>
void launch(dim3 grid, hipStream_t stream, const B64Image* imgs, int images, const int* d_images,
            const uint8_t* bytes, int HS, int WS, int C, float* out, int* status,
            const InputPrep* prep) {
#define GALE_TYPED_LAUNCH(PREP, NCHW, CT, P)                                                   \
  hipLaunchKernelGGL((b64_typed_kernel<ET, PREP, NCHW, CT>), grid, dim3(kThreads), 0, stream,  \
                     imgs, images, d_images, bytes, HS, WS, C, out, status, P)
  if (!prep || prep->identity())
    GALE_TYPED_LAUNCH(false, false, 0, InputPrep());
  else if (prep->nchw)
    GALE_TYPED_LAUNCH(true, true, 0, *prep);
  else if (C == 3)
    GALE_TYPED_LAUNCH(true, false, 3, *prep);
  else if (C == 1)
    GALE_TYPED_LAUNCH(true, false, 1, *prep);
  else
    GALE_TYPED_LAUNCH(true, false, 0, *prep);
#undef GALE_TYPED_LAUNCH
}

}  // namespace

hipError_t b64_typed_instances(int images, const B64Image* imgs, const uint8_t* bytes, int HS,
                               int WS, int C, float* out, int* status, hipStream_t stream,
                               const int* d_images, const InputPrep* prep, int type) {
  if (HS <= 0 || WS <= 0 || C <= 0 || !imgs || !bytes || !out || !status)
    return hipErrorInvalidValue;
  if (type != ELEM_U16 && type != ELEM_F16 && type != ELEM_BF16 && type != ELEM_F32)
    return hipErrorInvalidValue;
  const int64_t per = (int64_t)HS * WS * C;
  if (per > (1 << 30) || images > 65535) return hipErrorInvalidValue;  // (int indices; grid y)
  if (!b64::prep_fits(prep, C)) return hipErrorInvalidValue;
  if (images <= 0) return hipSuccess;
  const int64_t B = per * elem_bytes(type), L = 4 * ((B + 2) / 3);
  // lanes with 16 k < L: their first byte 12 k is below B (12 k >= B would mean 16 k >= L)
  const dim3 grid((unsigned)((L + kB64ChunkChars - 1) / kB64ChunkChars), (unsigned)images);
  switch (type) {
    case ELEM_U16:
      launch<ELEM_U16>(grid, stream, imgs, images, d_images, bytes, HS, WS, C, out, status, prep);
      break;
    case ELEM_F16:
      launch<ELEM_F16>(grid, stream, imgs, images, d_images, bytes, HS, WS, C, out, status, prep);
      break;
    case ELEM_BF16:
      launch<ELEM_BF16>(grid, stream, imgs, images, d_images, bytes, HS, WS, C, out, status,
                        prep);
      break;
    default:
      launch<ELEM_F32>(grid, stream, imgs, images, d_images, bytes, HS, WS, C, out, status, prep);
      break;
  }
  return hipGetLastError();
}

}  // namespace gale
