// GPU decoders of planar YUV 4:2:2 / 4:4:4 frame records, input pixel formats "yuv422p" and
// "yuv444p" - what a JPEG decoder hands back (gale/kernels.h: b64_yuvp_instances,
// raw_yuvp_instances).
//
//   b64   {"instances":[{"b64":"<L characters>"}, ...]}     L = 4 ceil(B / 3)
//   raw   value = N frames back to back, B bytes each, no envelope
//
// With s = 1 (4:2:2, WS even) or 0 (4:4:4) and hw = HS*WS, a frame is three linear byte streams,
// Y[hw], U[hw >> s], V[hw >> s], B = hw + 2 (hw >> s) bytes, and pixel p = y WS + x takes Y[p],
// U[p >> s], V[p >> s] (an even WS makes (y (WS/2)) + (x >> 1) = p >> 1): no row or column
// arithmetic anywhere. Every pixel becomes fmaf((float)RGB[c], a[c], b[c]) by the integer matrix
// of yuv.h, fp32 NHWC: the bits b64_decode_instances gives for the converted image as an RGB
// record.
//
// One kernel template <S, RAW, PREP>: a three-stream gather, load-driven. A lane owns a run of R
// consecutive pixels of p and converts each once, in registers; no source byte passes through LDS,
// there is no workgroup barrier and no atomic.
//   4:4:4  R = 12. The run's Y bytes [12 g, 12 g + 12) are base64 characters [16 g, 16 g + 16):
//          one 16-character window at a 16-character stride, so its phase in the staged buffer
//          is the string's. The U / V bytes start at hw + 12 g and 2 hw + 12 g: quads
//          floor(hw / 3) + 4 g and floor(2 hw / 3) + 4 g, byte phi = hw mod 3 and 2 hw mod 3 of the
//          quad. Both the buffer phase of those windows ((off + 4 floor(. / 3)) mod 16) and phi
//          are the same for every lane of an image: the alignment switch is a scalar branch and
//          the byte shift a scalar operand. 12 + phi bytes need 5 quads, so a chroma window is 20
//          characters. 256 threads, 3072 pixels a workgroup.
//   4:2:2  R = 24, the smallest run that keeps all of that uniform: the run's chroma is R / 2
//          bytes, which must be whole quads (R / 2 a multiple of 3) at a whole 16-character
//          stride (4 (R / 2) / 3 a multiple of 16), so R / 2 = 12; a run of 12 pixels would put
//          even and odd lanes 8 characters apart in phase. Y is then 24 bytes = 32 characters (8
//          quads), U 12 bytes from quad floor(hw / 3) + 4 g at phi = hw mod 3 and V 12 bytes from
//          quad hw / 2 + 4 g at phi = 0 (3 (hw / 2) is a multiple of 3). The chroma terms of a
//          pixel pair are computed once. 128 threads, 3072 pixels a workgroup again.
//   b64    load_quads<NQ>: the aligned 16-byte words that hold one of the window's characters of
//          the string (never an unaligned 16-byte load; a word past the string's last character
//          is not read, so fewer than 16 bytes past a string), realigned with v_alignbyte_b32,
//          4 characters -> sextets -> 24 bits with b64_decode.cuh's b64_sextets4, and judged the
//          way b64::window_bad judges. load_window itself is the NQ = 4, phi = 0 case; the 5- and
//          8-quad windows need the same code with another count, so there is one loader, not
//          two. Every character of a string lies in a window of some lane (the planes' windows
//          overlap in the quads two planes share; the last window of V ends at the string's
//          end) and each lane judges all of its window's characters of the string, so the
//          shared quads are judged at least once and padding is judged by V's last lane.
//   raw    load_run<NB>: the aligned dwords that hold a byte of the run, realigned by the phase of
//          the plane's *address* (workgroup-uniform: a run is a multiple of 4 bytes), or 12-byte
//          vector loads when that phase is 0. The launcher hands over the 16-byte aligned
//          address under the caller's pointer and the pointer's phase.
//
// A lane's j-th float is channel j mod 3, a constant after unrolling, so the prep's fma is applied
// where the pixel is converted and the identity instantiation carries none.
//
// Stores. A lane's 3 R floats are contiguous in the image and so are a wave's 192 R. They are
// re-staged through LDS per wave: lane l writes [3 R l, 3 R l + 3 R) of the wave's row, waits for
// its own LDS writes, and reads back 16-byte unit l + 64 i, so every store instruction of a wave
// writes 1 KB contiguous. A wave's first float of the image is a multiple of 2304: of 3 and 4,
// so 16-byte stores need only a 16-byte aligned image base; otherwise (3 hw mod 4 != 0 leaves
// later slots 4- or 8-byte aligned) lane l stores float l + 64 j, 256 B contiguous. The image's
// last, partial unit goes float by float. 36 KB of LDS a workgroup in both forms.
// LDS write side: nine 16-byte writes a half at a lane stride of 144 bytes (4:4:4) or 288
// (4:2:2), ds_write_b128 in the compiled code. tools/lds_bank_model.py has no rule for that
// instruction; its extra() on these addresses gives, with the service groups and 64 banks of its
// ds_read_b128 rule, 0 extra cycles an instruction at 144 bytes and 4 (1 per 16-lane group:
// lanes l and l + 8) at 288; with the 16 contiguous lanes and 32 banks of its ds_write_b64 rule,
// 4 and 12. Both are stand-ins, not a rule for the instruction. The natural layout is kept: a
// padded lane stride would misalign the 16-byte units of the read side, which is conflict-free
// by the model (ds_read_b128 of consecutive units), and a row moves 2 x 12 bytes a pixel where
// a CU's LDS moves 128 a clock.
//
// Verdict (b64): a wave with a lane that saw a character outside the alphabet in the data part
// or a non-'=' in the padding stores the constant 2 into its record's status, once (a plain
// vector store; every writer stores the same value). The image is written anyway. A raw frame has
// no verdict. Nothing is written outside out + slot*hw*3 floats of the image. Workgroups past
// *d_images exit as a whole before touching LDS or memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "b64_decode.cuh"
#include "gale/kernels.h"

namespace gale {
namespace {

constexpr int kGroupPixels = 3072;  // of a workgroup, either format
constexpr int kHalfFloats = 36;     // 12 pixels: what a lane converts and stages at a time

typedef uint32_t __attribute__((aligned(4))) U32a;
struct __attribute__((aligned(4))) U32x3 {
  uint32_t x, y, z;
};

__device__ __forceinline__ int clamp8(int acc) { return min(max(acc >> 20, 0), 255); }
// byte i (a constant after unrolling) of a little-endian dword stream
__device__ __forceinline__ int byte_of(const uint32_t* s, int i) {
  return (int)((s[i >> 2] >> (8 * (i & 3))) & 0xFFu);
}

// NQ quads of the string at bytes + off from character c = cu + ck on (cu: the same for every
// lane of the image; ck: a multiple of 16, so the window's phase in the buffer is visibly
// uniform and the switch below a scalar branch). c < L. r[t]: the 3 bytes of quad t, byte 0 in
// the low bits (garbage where a character is outside the alphabet or past the string). Returns
// whether one of the window's characters of the string is bad: outside the alphabet among the
// L - pad data characters, or not '=' after them.
template <int NQ>
__device__ __forceinline__ bool load_quads(const uint8_t* bytes, int64_t off, int cu, int ck,
                                           int L, int pad, uint32_t* r) {
  constexpr int NV = (4 * NQ + 30) / 16;  // 16-byte words a window can touch: 2, 3 (NQ 5), 3 (8)
  const int c = cu + ck;
  const int nch = min(4 * NQ, L - c);  // characters of the string in the window (4, 8, ...)
  const int nd = L - pad - c;          // data characters from the window's start on
  const int ph = (int)((off + cu) & 15);
  const uint8_t* const base = bytes + (off + c - ph);
  uint32_t w[4 * NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {  // (a word is read only when a character of the string is in it)
    const uint4 v = i == 0 || 16 * i < ph + nch ? *reinterpret_cast<const uint4*>(base + 16 * i)
                                                 : make_uint4(0, 0, 0, 0);
    w[4 * i] = v.x, w[4 * i + 1] = v.y, w[4 * i + 2] = v.z, w[4 * i + 3] = v.w;
  }
  const uint32_t sh = (uint32_t)(ph & 3);
  uint32_t x[NQ];
  switch (ph >> 2) {
#define GALE_ALIGN_WORDS(D)                                \
  _Pragma("unroll") for (int t = 0; t < NQ; ++t) x[t] =    \
      __builtin_amdgcn_alignbyte(w[t + (D) + 1], w[t + (D)], sh);
    case 0: GALE_ALIGN_WORDS(0) break;
    case 1: GALE_ALIGN_WORDS(1) break;
    case 2: GALE_ALIGN_WORDS(2) break;
    default: GALE_ALIGN_WORDS(3) break;
#undef GALE_ALIGN_WORDS
  }
  const bool all_data = nd >= 4 * NQ;
  uint32_t j = 0;
#pragma unroll
  for (int t = 0; t < NQ; ++t) {
    uint32_t inv;
    const uint32_t sx = b64::b64_sextets4(x[t], &inv) & 0x3F3F3F3Fu;
    const uint32_t h = ((sx & 0x003F003Fu) << 6) | ((sx >> 8) & 0x003F003Fu);
    r[t] = __builtin_bswap32(((h & 0xFFFu) << 12) | (h >> 16)) >> 8;
    const uint32_t dm = b64::first_bytes(nd - 4 * t);
    j |= all_data ? inv
                  : (inv & dm) | ((x[t] ^ 0x3D3D3D3Du) & b64::first_bytes(nch - 4 * t) & ~dm);
  }
  return j != 0;
}

// Dword m (a constant after unrolling) of the byte stream of NQ 3-byte groups.
template <int NQ>
__device__ __forceinline__ uint32_t stream_dword(const uint32_t* r, int m) {
  const int t = 4 * m / 3, s = 4 * m % 3;
  uint32_t d = r[t] >> (8 * s);
  if (t + 1 < NQ) d |= r[t + 1] << (24 - 8 * s);
  return d;
}

// 12 bytes of a chroma plane of a string: 5 quads from character cu + ck on, from byte phi of the
// first quad (phi: 0, 1 or 2, the same for every lane of the image).
__device__ __forceinline__ bool load_chroma_b64(const uint8_t* bytes, int64_t off, int cu, int ck,
                                                int L, int pad, uint32_t phi, uint32_t* o) {
  uint32_t r[5], d[4];
  const bool bad = load_quads<5>(bytes, off, cu, ck, L, pad, r);
#pragma unroll
  for (int m = 0; m < 4; ++m) d[m] = stream_dword<5>(r, m);
#pragma unroll
  for (int m = 0; m < 3; ++m) o[m] = __builtin_amdgcn_alignbyte(d[m + 1], d[m], phi);
  return bad;
}

// NB bytes (12 or 24) at bytes + au + ag, of which the first n (1 .. NB) are read: au the same
// for every lane of the image, ag a multiple of 4, so the phase au & 3 is workgroup-uniform.
// bytes is 16-byte aligned. Bytes past n are zero or the frame's own.
template <int NB>
__device__ __forceinline__ void load_run(const uint8_t* bytes, int64_t au, int64_t ag, int n,
                                         uint32_t* x) {
  const uint32_t sh = (uint32_t)(au & 3);
  if (sh == 0 && n == NB) {  // (the phase test is workgroup-uniform)
#pragma unroll
    for (int i = 0; i < NB / 12; ++i) {
      const U32x3 v = *reinterpret_cast<const U32x3*>(bytes + au + ag + 12 * i);
      x[3 * i] = v.x, x[3 * i + 1] = v.y, x[3 * i + 2] = v.z;
    }
  } else {
    const uint8_t* const a0 = bytes + (au - sh + ag);
    uint32_t w[NB / 4 + 1];
#pragma unroll
    for (int j = 0; j <= NB / 4; ++j)  // (a dword is loaded only when it holds a byte of the run)
      w[j] = 4 * j < (int)sh + n ? *reinterpret_cast<const U32a*>(a0 + 4 * j) : 0u;
#pragma unroll
    for (int j = 0; j < NB / 4; ++j) x[j] = __builtin_amdgcn_alignbyte(w[j + 1], w[j], sh);
  }
}

// Pixels [12 h, 12 h + 12) of a lane's run -> 36 floats. yb / ub / vb: the run's byte streams.
template <int S, bool PREP>
__device__ __forceinline__ void convert12(const uint32_t* yb, const uint32_t* ub,
                                          const uint32_t* vb, int h, const YuvCoeffs& k,
                                          const InputPrep& prep, float* f) {
#pragma unroll
  for (int c = 0; c < (12 >> S); ++c) {
    const int u = byte_of(ub, (12 >> S) * h + c) - 128, v = byte_of(vb, (12 >> S) * h + c) - 128;
    // (with 4:2:2 the chroma terms are shared by the two pixels)
    const int cr = k.crv * v, cg = k.cgu * u + k.cgv * v, cb = k.cbu * u;
#pragma unroll
    for (int e = 0; e < (1 << S); ++e) {
      const int i = (c << S) + e;
      const int yy = k.cy * (byte_of(yb, 12 * h + i) - k.yo) + (1 << 19);
      const int rgb[3] = {clamp8(yy + cr), clamp8(yy + cg), clamp8(yy + cb)};
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float x = (float)rgb[ch];
        f[3 * i + ch] = PREP ? __builtin_fmaf(x, prep.a[ch], prep.b[ch]) : x;
      }
    }
  }
}

// The wave's staged row (NF floats, written by the wave's own lanes) to the image:
// row[0 .. nvw) -> wdst[0 .. nvw), nvw <= NF the wave's floats of the image. wdst is 16-byte
// aligned iff `aligned` (wave-uniform).
template <int NF>
__device__ __forceinline__ void store_row(const float* row, float* wdst, int nvw, int lane,
                                          bool aligned) {
  __builtin_amdgcn_wave_barrier();  // (no code: keeps the reads behind every lane's writes)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the wave's own LDS writes)
  if (aligned) {
#pragma unroll
    for (int i = 0; i < NF / 256; ++i) {  // (NF / 4 units, a multiple of 64)
      const int q = 64 * i + lane;
      if (4 * q + 4 <= nvw) {
        reinterpret_cast<float4*>(wdst)[q] = reinterpret_cast<const float4*>(row)[q];
      } else {
        for (int e = 4 * q; e < nvw; ++e) wdst[e] = row[e];  // (the image's last 1 - 3 floats)
      }
    }
  } else {
#pragma unroll 6
    for (int j = 0; j < NF / 64; ++j) {
      const int e = 64 * j + lane;
      if (e < nvw) wdst[e] = row[e];
    }
  }
}

// S: the chroma shift (1: yuv422p, 0: yuv444p). RAW: the frames' bytes, else base64 strings.
// PREP: fmaf(v, a[c], b[c]) where a pixel is converted (`prep` is never read without it).
// bytes: RAW, the 16-byte aligned address under the caller's pointer and base_phase its phase.
template <int S, bool RAW, bool PREP>
__global__ __launch_bounds__(256 >> S) void yuvp_kernel(const B64Image* imgs, int images,
                                                        const int* d_images, const uint8_t* bytes,
                                                        int hw, float* out, int* status,
                                                        YuvCoeffs k, InputPrep prep,
                                                        int base_phase) {
  constexpr int T = 256 >> S, R = 12 << S, NF = 3 * R;  // threads, pixels and floats of a lane
  static_assert(T * R == kGroupPixels, "a workgroup's pixels");
  if (d_images) images = min(images, *d_images);
  const int img = (int)blockIdx.y;
  if (img >= images) return;  // (workgroup-uniform, before any LDS or memory access)
  __shared__ float stage[T / 64][NF * 64];
  const B64Image d = imgs[img];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int per = 3 * hw;   // floats of the image (<= 2^30)
  const int hc = hw >> S;   // bytes of a chroma plane
  const int g = (int)blockIdx.x * T + tid;  // this lane's run of the image
  const int n = min(R, hw - R * g);         // its pixels of the image (<= 0: none)
  float* const row = stage[tid >> 6];
  bool bad = false;
  if (n > 0) {
    uint32_t yb[R / 4], ub[3], vb[3];
    if (RAW) {
      const int64_t off = d.off + base_phase;
      const int nc = (n + S) >> S;  // the run's chroma bytes
      load_run<R>(bytes, off, (int64_t)R * g, n, yb);
      load_run<12>(bytes, off + hw, (int64_t)12 * g, nc, ub);
      load_run<12>(bytes, off + hw + hc, (int64_t)12 * g, nc, vb);
    } else {
      const int B = hw + 2 * hc;  // (<= 2^30)
      const int L = 4 * ((B + 2) / 3), pad = (3 - B % 3) % 3;
      uint32_t r[2 * R / 6];  // 4 quads (4:4:4), 8 (4:2:2)
      bad = load_quads<2 * R / 6>(bytes, d.off, 0, (16 << S) * g, L, pad, r);
#pragma unroll
      for (int m = 0; m < R / 4; ++m) yb[m] = stream_dword<2 * R / 6>(r, m);
      const int bu = hw, bv = hw + hc;  // the planes' first bytes
      bad |= load_chroma_b64(bytes, d.off, 4 * (bu / 3), 16 * g, L, pad, (uint32_t)(bu % 3), ub);
      bad |= load_chroma_b64(bytes, d.off, 4 * (bv / 3), 16 * g, L, pad, (uint32_t)(bv % 3), vb);
    }
#pragma unroll
    for (int h = 0; h < R / 12; ++h) {
      float f[kHalfFloats];
      convert12<S, PREP>(yb, ub, vb, h, k, prep, f);
      // 144 bytes a half, 16-byte aligned: nine 16-byte writes
      float4* const wl = reinterpret_cast<float4*>(row + NF * lane + kHalfFloats * h);
#pragma unroll
      for (int j = 0; j < kHalfFloats / 4; ++j)
        wl[j] = make_float4(f[4 * j], f[4 * j + 1], f[4 * j + 2], f[4 * j + 3]);
    }
  }
  // the wave's first float of the image and its floats of it (<= 0: none, wave-uniform; lanes
  // past the image wrote nothing and a lane's pixels past it were converted from bytes of no
  // pixel: both lie past nvw)
  const int64_t wf0 = (int64_t)NF * (g - lane);
  const int nvw = (int)min((int64_t)NF * 64, per - wf0);
  if (nvw > 0) {
    float* const img_dst = out + (int64_t)d.slot * per;
    store_row<NF * 64>(row, img_dst + wf0, nvw, lane,
                       (reinterpret_cast<uintptr_t>(img_dst) & 15) == 0);
  }
  if (!RAW && __ballot(bad) != 0 && lane == 0) status[d.rec] = 2;
}

template <bool RAW>
hipError_t launch(int images, const B64Image* imgs, const uint8_t* bytes, int HS, int WS, int C,
                  float* out, int* status, hipStream_t stream, const int* d_images,
                  const InputPrep* prep, int format, const YuvCoeffs& coeffs) {
  if (HS <= 0 || WS <= 0 || C != 3 || !imgs || !bytes || !out || !status)
    return hipErrorInvalidValue;
  if (!yuv_is_planar(format) || (yuvp_shift(format) && (WS & 1))) return hipErrorInvalidValue;
  if (prep && prep->nchw) return hipErrorInvalidValue;
  // (int indices in the kernel: floats, bytes and characters of a frame; grid y)
  if ((int64_t)HS * WS * 3 > (1 << 30) || images > 65535) return hipErrorInvalidValue;
  if (images <= 0) return hipSuccess;
  const int hw = HS * WS;
  const dim3 grid((unsigned)((hw + kGroupPixels - 1) / kGroupPixels), (unsigned)images);
  // RAW: the kernel's alignment is reckoned from its byte pointer: hand it the aligned address
  // under `bytes` and let it add the pointer's own phase to every offset
  const int phase = RAW ? (int)(reinterpret_cast<uintptr_t>(bytes) & 15) : 0;
  const uint8_t* const abytes = bytes - phase;
#define GALE_YUVP_LAUNCH(S, PREP, P)                                                        \
  hipLaunchKernelGGL((yuvp_kernel<S, RAW, PREP>), grid, dim3(256 >> S), 0, stream, imgs,    \
                     images, d_images, abytes, hw, out, status, coeffs, P, phase)
  const bool id = !prep || prep->identity();
  if (yuvp_shift(format)) {
    if (id) GALE_YUVP_LAUNCH(1, false, InputPrep());
    else GALE_YUVP_LAUNCH(1, true, *prep);
  } else {
    if (id) GALE_YUVP_LAUNCH(0, false, InputPrep());
    else GALE_YUVP_LAUNCH(0, true, *prep);
  }
#undef GALE_YUVP_LAUNCH
  return hipGetLastError();
}

}  // namespace

hipError_t b64_yuvp_instances(int images, const B64Image* imgs, const uint8_t* bytes, int HS,
                              int WS, int C, float* out, int* status, hipStream_t stream,
                              const int* d_images, const InputPrep* prep, int format,
                              const YuvCoeffs& coeffs) {
  return launch<false>(images, imgs, bytes, HS, WS, C, out, status, stream, d_images, prep,
                       format, coeffs);
}

hipError_t raw_yuvp_instances(int images, const B64Image* imgs, const uint8_t* bytes, int HS,
                              int WS, int C, float* out, int* status, hipStream_t stream,
                              const int* d_images, const InputPrep* prep, int format,
                              const YuvCoeffs& coeffs) {
  return launch<true>(images, imgs, bytes, HS, WS, C, out, status, stream, d_images, prep,
                      format, coeffs);
}

}  // namespace gale
