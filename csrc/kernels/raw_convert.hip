// GPU conversion of raw binary tensor records (gale/kernels.h: raw_instances).
//
//   value = N images back to back, B bytes each, no envelope      B = PixelSource::bytes(HS, WS, C)
//
// An image is HS*WS*C little-endian elements of the rgb layout (csrc/codec/elemtype.h: u8, u16,
// f16, bf16, f32; [H][W][C], or [C][H][W] with an nchw prep) or HS*WS packed pixels
// (csrc/codec/pixfmt.h: bgr24, rgba, bgra, gray). The kernel stores fmaf(float32(x), a[c], b[c])
// as fp32 NHWC: the bits the b64 decoders give for the same bytes sent as a b64 string
// (typed_to_float_bits, packed_src_offset: the host codec's functions). Without a prep the
// converted bits are stored as they are, no arithmetic op touches an f32 element.
//
// Store-driven, no LDS, no barrier. There is no decode step, so nothing ties a lane to a group of
// source bytes; the traffic is lopsided (a u8 image writes 4 bytes for each byte it reads), so the
// work is split by what is written:
//   unit q of an image = its floats [4 q, 4 q + 4), one 16-byte store.
//   A wave owns 256 consecutive units, a 256-thread workgroup 1024 (4096 floats); the grid is
//   (ceil(HS*WS*C / 4096)) x (images). Lane l of a wave takes units l, l + 64, l + 128, l + 192 of
//   the wave's share: every store instruction of a wave writes 1 KB contiguous and a lane's four
//   independent loads are in flight together.
//   The unit's source bytes, NB of them from byte sb of the image (p0 = floor(4 q / 3)):
//       u8      sb = 4 q     NB = 4        gray          sb = p0      NB = 2
//       16-bit  sb = 8 q     NB = 8        bgr24         sb = 3 p0    NB = 6
//       f32     sb = 16 q    NB = 16       rgba / bgra   sb = 4 p0    NB = 8
//   A whole unit's NB bytes lie inside the image (4 q + 3 < HS*WS*3 puts pixel p0 + 1 inside it).
// Alignment is that of the address, off + the phase of the caller's byte pointer (the launcher
// hands the kernel the 16-byte aligned address under it): the pointer may be any byte.
// Loads are aligned dwords: dword j of the aligned run that starts under byte off + sb is loaded
// only when it overlaps the unit's bytes (4 j < phase + NB), and v_alignbyte_b32 moves the bytes
// down by the phase, (off + sb) mod 4 - the image's own phase for the element kinds and rgba /
// bgra (workgroup-uniform), the lane's for gray and bgr24. A 16-bit image at an 8-byte phase and
// an f32 image at a 16-byte phase load one 8- or 16-byte vector per unit instead (a
// workgroup-uniform branch). Never an unaligned vector load, never a word that holds no byte of
// the image.
// Channels: float t of unit q is channel (4 q + t) mod C. C = 3 (and every packed format): the
// lane rotates its three coefficient pairs once by q mod 3; its four units are 64 apart and
// 64 mod 3 = 1, so float t of the lane's i-th unit takes rotated pair (i + t) mod 3, a constant
// after unrolling. C = 1: pair 0. Any other C: a running counter. The identity instantiation
// carries no fma and no channel.
// What is not a whole 16-byte store goes float by float (fetch_float: the one or two aligned
// dwords under one element): an image's last 1 - 3 floats; every float of an image whose base is
// not 16-byte aligned (float 64 j + l of the wave's share by lane l, 256 B contiguous per
// instruction); and [C][H][W]-ordered records, gathered per element from the C planes into the
// same unit or float stores.
//
// Verdict: a wave with a lane that saw an f16 / bf16 / f32 element of the image with an all-ones
// exponent, judged on the element as sent, stores the constant 2 into its record's status (a
// plain vector store: every writer stores the same value). The image is written anyway, inside
// its own slot. No atomics; nothing is written outside out + slot*HS*WS*C floats of the image.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "b64_decode.cuh"
#include "gale/kernels.h"

namespace gale {
namespace {

constexpr int kThreads = 256;
constexpr int kUnits = 4;                                // units of a lane
constexpr int kWaveFloats = 64 * kUnits * 4;             // 1024
constexpr int kGroupFloats = (kThreads / 64) * kWaveFloats;  // 4096

// What an image's bytes are: the five element types of the rgb layout, then the packed formats.
enum RawKind : int {
  RK_U8 = ELEM_U8, RK_U16 = ELEM_U16, RK_F16 = ELEM_F16, RK_BF16 = ELEM_BF16, RK_F32 = ELEM_F32,
  RK_BGR24 = kElemTypes - 1 + PACKED_BGR24, RK_RGBA = kElemTypes - 1 + PACKED_RGBA,
  RK_BGRA = kElemTypes - 1 + PACKED_BGRA, RK_GRAY = kElemTypes - 1 + PACKED_GRAY
};
constexpr bool rk_packed(int k) { return k >= kElemTypes; }
constexpr int rk_format(int k) { return rk_packed(k) ? k - (kElemTypes - 1) : (int)PACKED_NONE; }
constexpr int rk_elem(int k) { return rk_packed(k) ? (int)ELEM_U8 : k; }
// bytes of one source item: an element, or a packed pixel
constexpr int rk_item(int k) { return rk_packed(k) ? packed_bpp(rk_format(k)) : elem_bytes(k); }
// source bytes of a unit
constexpr int rk_unit_bytes(int k) {
  return k == RK_GRAY ? 2 : k == RK_BGR24 ? 6 : k == RK_RGBA || k == RK_BGRA ? 8
                                                                             : 4 * elem_bytes(k);
}

typedef uint32_t __attribute__((aligned(4))) U32a;

__device__ __forceinline__ uint32_t load_dword(const uint8_t* bytes, int64_t aligned_addr) {
  return *reinterpret_cast<const U32a*>(bytes + aligned_addr);
}

// The lane's three coefficient pairs, rotated by r = (the unit's first float's channel).
struct Rot3 {
  float a[3], b[3];
};
__device__ __forceinline__ Rot3 make_rot3(const InputPrep& prep, int r) {
  const int r1 = r == 2 ? 0 : r + 1, r2 = r == 0 ? 2 : r - 1;
  return Rot3{{b64::prep_a(prep, r), b64::prep_a(prep, r1), b64::prep_a(prep, r2)},
              {b64::prep_b(prep, r), b64::prep_b(prep, r1), b64::prep_b(prep, r2)}};
}

// One float of the image, e = its index in the NHWC output (< per): the element or pixel byte
// under it through the one or two aligned dwords that hold it. *nonfinite is raised for an
// Inf / NaN element.
template <int KIND, bool PREP, bool NCHW>
__device__ __forceinline__ float fetch_float(const uint8_t* bytes, int64_t off, int e, int hw,
                                             int C, const InputPrep& prep, bool* nonfinite) {
  constexpr int ET = rk_elem(KIND);
  constexpr int E = elem_bytes(ET);
  int c;
  int64_t sb;
  if constexpr (rk_packed(KIND)) {
    const int p = (int)((unsigned)e / 3u);
    c = e - 3 * p;
    sb = (int64_t)p * rk_item(KIND) + packed_src_offset(rk_format(KIND), c);
  } else if constexpr (NCHW) {
    const int p = (int)((unsigned)e / (unsigned)C);
    c = e - p * C;
    sb = ((int64_t)c * hw + p) * E;
  } else {
    c = PREP ? (int)((unsigned)e % (unsigned)C) : 0;
    sb = (int64_t)e * E;
  }
  const int64_t addr = off + sb;
  const uint32_t sh = (uint32_t)(addr & 3);
  const int64_t a0 = addr - sh;
  const uint32_t lo = load_dword(bytes, a0);
  // (the next dword only when the element reaches into it: then it holds a byte of the image)
  const uint32_t hi = sh + E > 4 ? load_dword(bytes, a0 + 4) : 0u;
  uint32_t raw = __builtin_amdgcn_alignbyte(hi, lo, sh);
  if constexpr (E < 4) raw &= (1u << (8 * E)) - 1u;
  *nonfinite |= typed_nonfinite<ET>(raw);
  const float f = __uint_as_float(typed_to_float_bits<ET>(raw));
  if constexpr (!PREP) return f;
  const int cs = min(c, 3);
  return __builtin_fmaf(f, b64::prep_a(prep, cs), b64::prep_b(prep, cs));
}

// The four floats of whole unit q (4 q + 4 <= per) of an NHWC-ordered image. ui: the index of the
// unit among the lane's (its channel rotation against rot, which was made for the lane's first).
template <int KIND, bool PREP, int CT>
__device__ __forceinline__ float4 convert_unit(const uint8_t* bytes, int64_t off, int q, int ui,
                                               int C, const InputPrep& prep, const Rot3& rot,
                                               bool* nonfinite) {
  constexpr int ET = rk_elem(KIND);
  constexpr int E = elem_bytes(ET);
  constexpr int NB = rk_unit_bytes(KIND);
  constexpr int NX = (NB + 3) / 4;  // dwords of the unit's bytes once realigned
  constexpr int NW = NX + 1;        // aligned dwords they can overlap
  // the unit's first source byte, and (packed) the channel of its first float
  const int p0 = (int)((unsigned)(4 * q) / 3u), r = 4 * q - 3 * p0;
  const int64_t sb = rk_packed(KIND) ? (int64_t)p0 * rk_item(KIND) : (int64_t)q * NB;
  const int64_t addr = off + sb;
  uint32_t x[NX];
  bool wide = false;
  if constexpr (!rk_packed(KIND) && NB >= 8) {
    if ((off & (NB - 1)) == 0) {  // (workgroup-uniform: sb is a multiple of NB)
      wide = true;
      if constexpr (NB == 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(bytes + addr);
        x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
      } else {
        const uint2 v = *reinterpret_cast<const uint2*>(bytes + addr);
        x[0] = v.x, x[1] = v.y;
      }
    }
  }
  if (!wide) {
    const uint32_t sh = (uint32_t)(addr & 3);
    const int64_t a0 = addr - sh;
    uint32_t w[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j)  // (a dword is loaded only when it overlaps the unit's bytes)
      w[j] = 4 * j < (int)sh + NB ? load_dword(bytes, a0 + 4 * j) : 0u;
#pragma unroll
    for (int j = 0; j < NX; ++j) x[j] = __builtin_amdgcn_alignbyte(w[j + 1], w[j], sh);
  }
  float f[4];
  if constexpr (rk_packed(KIND)) {
    // float t is channel (r + t) mod 3 of pixel p0 + (r + t) / 3: byte bi of the unit's bytes
    const uint64_t bits = NX > 1 ? ((uint64_t)x[NX > 1 ? 1 : 0] << 32) | x[0] : (uint64_t)x[0];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int idx = r + t, px = idx >= 3 ? 1 : 0, c = idx - 3 * px;
      const int bi = KIND == RK_GRAY   ? px
                     : KIND == RK_RGBA ? 4 * px + c
                                       : rk_item(KIND) * px + 2 - c;
      f[t] = (float)(uint32_t)((bits >> (8 * bi)) & 0xFFu);
    }
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint32_t raw = E == 4   ? x[t]
                           : E == 2 ? (x[t / 2] >> (16 * (t & 1))) & 0xFFFFu
                                    : (x[0] >> (8 * t)) & 0xFFu;
      *nonfinite |= typed_nonfinite<ET>(raw);
      f[t] = __uint_as_float(typed_to_float_bits<ET>(raw));
    }
  }
  if constexpr (PREP) {
    if constexpr (CT == 3) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        f[t] = __builtin_fmaf(f[t], rot.a[(ui + t) % 3], rot.b[(ui + t) % 3]);
    } else if constexpr (CT == 1) {
#pragma unroll
      for (int t = 0; t < 4; ++t) f[t] = __builtin_fmaf(f[t], prep.a[0], prep.b[0]);
    } else {
      int ch = (int)((unsigned)(4 * q) % (unsigned)C);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int cs = min(ch, 3);
        f[t] = __builtin_fmaf(f[t], b64::prep_a(prep, cs), b64::prep_b(prep, cs));
        if (++ch == C) ch = 0;
      }
    }
  }
  return make_float4(f[0], f[1], f[2], f[3]);
}

// KIND: what the bytes are. PREP: fmaf(v, a[c], b[c]) at the store (`prep` is never read without
// it). NCHW (with PREP, an element kind): the record's elements are ordered [C][H][W]. CT: the
// channel count when a unit's channel pattern is a compile-time one (1 or 3), 0 = a running
// counter.
template <int KIND, bool PREP, bool NCHW, int CT>
__global__ __launch_bounds__(kThreads) void raw_convert_kernel(const B64Image* imgs, int images,
                                                               const int* d_images,
                                                               const uint8_t* bytes, int HS,
                                                               int WS, int C, float* out,
                                                               int* status, InputPrep prep,
                                                               int base_phase) {
  if (d_images) images = min(images, *d_images);
  const int img = (int)blockIdx.y;
  if (img >= images) return;  // (workgroup-uniform)
  B64Image d = imgs[img];
  d.off += base_phase;  // (`bytes` is the 16-byte aligned address under the caller's pointer)
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int hw = HS * WS;
  const int per = hw * C;  // floats of the image (<= 2^30)
  // the wave's first float (a multiple of 1024: 16-byte aligned from the image's base)
  const int64_t wf0 = ((int64_t)blockIdx.x * (kThreads / 64) + (tid >> 6)) * kWaveFloats;
  bool bad = false;
  if (wf0 < per) {  // (wave-uniform)
    const int w0 = (int)wf0;
    float* const img_dst = out + (int64_t)d.slot * per;
    if ((reinterpret_cast<uintptr_t>(img_dst) & 15) == 0) {  // (workgroup-uniform)
      const int q0 = w0 / 4 + lane;
      Rot3 rot = {};
      if constexpr (PREP && CT == 3 && !NCHW) rot = make_rot3(prep, q0 % 3);
#pragma unroll
      for (int i = 0; i < kUnits; ++i) {
        const int q = q0 + 64 * i;  // (4 q < per + 1024 <= 2^30 + 1024)
        if (4 * q + 4 <= per) {
          float4 v;
          if constexpr (NCHW) {
            float f[4];
#pragma unroll
            for (int t = 0; t < 4; ++t)
              f[t] = fetch_float<KIND, PREP, true>(bytes, d.off, 4 * q + t, hw, C, prep, &bad);
            v = make_float4(f[0], f[1], f[2], f[3]);
          } else {
            v = convert_unit<KIND, PREP, CT>(bytes, d.off, q, i, C, prep, rot, &bad);
          }
          reinterpret_cast<float4*>(img_dst)[q] = v;
        } else {
#pragma unroll
          for (int t = 0; t < 3; ++t)  // (the image's last, partial unit: at most 3 floats)
            if (4 * q + t < per)
              img_dst[4 * q + t] =
                  fetch_float<KIND, PREP, NCHW>(bytes, d.off, 4 * q + t, hw, C, prep, &bad);
        }
      }
    } else {
#pragma unroll 4
      for (int j = 0; j < kWaveFloats / 64; ++j) {
        const int e = w0 + 64 * j + lane;
        if (e < per)
          img_dst[e] = fetch_float<KIND, PREP, NCHW>(bytes, d.off, e, hw, C, prep, &bad);
      }
    }
  }
  if (__ballot(bad) != 0 && lane == 0) status[d.rec] = 2;
}

template <int KIND>
void launch(dim3 grid, hipStream_t stream, const B64Image* imgs, int images, const int* d_images,
            const uint8_t* bytes, int HS, int WS, int C, float* out, int* status,
            const InputPrep* prep) {
#define GALE_RAW_LAUNCH(PREP, NCHW, CT, P)                                                      \
  hipLaunchKernelGGL((raw_convert_kernel<KIND, PREP, NCHW, CT>), grid, dim3(kThreads), 0,       \
                     stream, imgs, images, d_images, abytes, HS, WS, C, out, status, P, phase)
  // the kernel's alignment is reckoned from its byte pointer: hand it the aligned address under
  // `bytes` and let it add the pointer's own phase to every offset
  const int phase = (int)(reinterpret_cast<uintptr_t>(bytes) & 15);
  const uint8_t* const abytes = bytes - phase;
  if (!prep || prep->identity()) {
    GALE_RAW_LAUNCH(false, false, 0, InputPrep());
  } else if constexpr (rk_packed(KIND)) {
    GALE_RAW_LAUNCH(true, false, 3, *prep);
  } else {
    if (prep->nchw)
      GALE_RAW_LAUNCH(true, true, 0, *prep);
    else if (C == 3)
      GALE_RAW_LAUNCH(true, false, 3, *prep);
    else if (C == 1)
      GALE_RAW_LAUNCH(true, false, 1, *prep);
    else
      GALE_RAW_LAUNCH(true, false, 0, *prep);
  }
#undef GALE_RAW_LAUNCH
}

}  // namespace

hipError_t raw_instances(int images, const B64Image* imgs, const uint8_t* bytes, int HS, int WS,
                         int C, float* out, int* status, hipStream_t stream, const int* d_images,
                         const InputPrep* prep, int elem, int packed_format) {
  if (HS <= 0 || WS <= 0 || C <= 0 || !imgs || !bytes || !out || !status)
    return hipErrorInvalidValue;
  if (elem < ELEM_U8 || elem > ELEM_F32) return hipErrorInvalidValue;
  if (packed_format < PACKED_NONE || packed_format > PACKED_GRAY) return hipErrorInvalidValue;
  if (packed_format != PACKED_NONE && (elem != ELEM_U8 || C != 3 || (prep && prep->nchw)))
    return hipErrorInvalidValue;
  const int64_t per = (int64_t)HS * WS * C;
  if (per > (1 << 30) || images > 65535) return hipErrorInvalidValue;  // (int indices; grid y)
  if (!b64::prep_fits(prep, C)) return hipErrorInvalidValue;
  if (images <= 0) return hipSuccess;
  const dim3 grid((unsigned)((per + kGroupFloats - 1) / kGroupFloats), (unsigned)images);
#define GALE_RAW_KIND(K) \
  launch<K>(grid, stream, imgs, images, d_images, bytes, HS, WS, C, out, status, prep)
  switch (packed_format ? kElemTypes - 1 + packed_format : elem) {
    case RK_U8: GALE_RAW_KIND(RK_U8); break;
    case RK_U16: GALE_RAW_KIND(RK_U16); break;
    case RK_F16: GALE_RAW_KIND(RK_F16); break;
    case RK_BF16: GALE_RAW_KIND(RK_BF16); break;
    case RK_F32: GALE_RAW_KIND(RK_F32); break;
    case RK_BGR24: GALE_RAW_KIND(RK_BGR24); break;
    case RK_RGBA: GALE_RAW_KIND(RK_RGBA); break;
    case RK_BGRA: GALE_RAW_KIND(RK_BGRA); break;
    default: GALE_RAW_KIND(RK_GRAY); break;
  }
#undef GALE_RAW_KIND
  return hipGetLastError();
}

}  // namespace gale
