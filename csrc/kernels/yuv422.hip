// GPU decoders of packed YUV 4:2:2 video-frame records, input pixel formats "yuyv422" and
// "uyvy422" (gale/kernels.h: b64_yuv422_instances, raw_yuv422_instances).
//
//   b64   {"instances":[{"b64":"<L characters>"}, ...]}     B = 2*HS*WS bytes, L = 4 ceil(B / 3)
//   raw   value = N frames back to back, B bytes each, no envelope
//
// A frame is [HS][WS/2] macropixels of 4 bytes (csrc/codec/yuv.h: Y0 U Y1 V, or U Y0 V Y1); a
// macropixel is two whole pixels and needs nothing else of the frame. Both kernels convert with
// the integer matrix of yuv.h and store fmaf((float)RGB[c], a[c], b[c]) as fp32 NHWC: the bits
// b64_decode_instances gives for the converted image sent as an RGB record.
//
// Load-driven. A lane owns whole macropixels and converts each pixel exactly once:
//   b64: the shared 16-character -> 12-byte window of b64_decode.cuh (load_window, window_bad).
//        Windows start at multiples of 12 bytes of the frame, so a lane holds 3 macropixels:
//        6 pixels, 18 floats. A 4096-character chunk (256 lanes) is 1536 pixels; the grid is
//        (chunks per image) x (images).
//   raw: 16 source bytes, 4 macropixels: 8 pixels, 24 floats. Aligned dword loads, realigned with
//        v_alignbyte_b32 by the image's byte phase (off mod 4, workgroup-uniform), or one aligned
//        16-byte vector load when the phase is 0 modulo 16; a word is loaded only when it holds a
//        byte of the image. A 256-thread workgroup covers 2048 pixels; the grid is
//        ceil(HS*WS / 2048) x (images).
// A lane's j-th float is channel j mod 3, a constant after unrolling, so the prep's fma is applied
// where the pixel is converted: no per-lane rotation of the coefficient pairs is needed, and the
// identity instantiation carries no fma.
//
// Stores. A lane's floats are 72 (b64) or 96 (raw) bytes apart from its neighbour's, so they are
// re-staged through LDS, per wave: lane l writes its floats at [F l, F l + F) of the wave's own
// F*64-float row (F = 18 or 24), the wave waits for its own LDS writes, and lane l reads back
// unit l + 64 i (16 bytes at 16 (l + 64 i): contiguous over the wave) and stores it, so every
// store instruction of a wave writes 1 KB contiguous. A wave's first float of the image is a
// multiple of 1152 or 1536, of both 3 and 4: 16-byte stores need only a 16-byte aligned image
// base. Otherwise (HS*WS*3 mod 4 != 0 leaves every second slot 8-byte aligned) float 64 j + l of
// the row is read and stored by lane l, 256 B contiguous per instruction. An image's last,
// partial unit goes float by float. There is no workgroup barrier - a wave reads only what it
// wrote - and the byte values never pass through LDS.
// LDS write side: the natural layout above. b64 writes 8-byte pairs at a 72-byte lane stride:
// tools/lds_bank_model.py's ds_write_b64 rule (16 contiguous lanes, 32 banks) puts the 16 lanes'
// dwords 18 l + {0, 1} on 32 distinct banks, no conflict. raw writes 16-byte vectors at a 96-byte
// stride; the model has no rule for 16-byte writes, so those conflicts were not counted. The
// read side (ds_read_b128 of consecutive 16-byte units) is conflict-free by the model.
//
// Verdict (b64): a wave with a lane that saw a character outside the alphabet in the data part
// or a non-'=' in the padding stores the constant 2 into its record's status (a plain vector
// store: every writer stores the same value). The image is written anyway. A raw frame has no
// verdict: every byte pattern is a frame. No atomics; nothing is written outside
// out + slot*HS*WS*3 floats of the image. Workgroups past *d_images exit as a whole before
// touching LDS or memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "b64_decode.cuh"
#include "gale/kernels.h"

namespace gale {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kB64LaneFloats = 18, kRawLaneFloats = 24;
constexpr int kRawLaneBytes = 16;
constexpr int kRawGroupPixels = kThreads * kRawLaneBytes / 2;  // 2048

typedef uint32_t __attribute__((aligned(4))) U32a;

__device__ __forceinline__ int clamp8(int acc) { return min(max(acc >> 20, 0), 255); }

// One macropixel (its 4 bytes, byte 0 in the low bits) -> the 6 floats of its two pixels.
template <int FORMAT, bool PREP>
__device__ __forceinline__ void convert_macropixel(uint32_t mp, const YuvCoeffs& k,
                                                   const InputPrep& prep, float* f) {
  const int u = (int)((mp >> (8 * yuv422_u(FORMAT))) & 0xFFu) - 128;
  const int v = (int)((mp >> (8 * yuv422_v(FORMAT))) & 0xFFu) - 128;
  // the chroma terms are shared by the two pixels
  const int cr = k.crv * v, cg = k.cgu * u + k.cgv * v, cb = k.cbu * u;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int Y = (int)((mp >> (8 * (h ? yuv422_y1(FORMAT) : yuv422_y0(FORMAT)))) & 0xFFu);
    const int yy = k.cy * (Y - k.yo) + (1 << 19);
    const int rgb[3] = {clamp8(yy + cr), clamp8(yy + cg), clamp8(yy + cb)};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float x = (float)rgb[c];
      f[3 * h + c] = PREP ? __builtin_fmaf(x, prep.a[c], prep.b[c]) : x;
    }
  }
}

// The wave's staged row (NF floats: NF / 64 per lane, written by the wave's own lanes) to the
// image: row[0 .. nvw) -> wdst[0 .. nvw), nvw <= NF the wave's floats of the image. wdst is
// 16-byte aligned iff `aligned` (wave-uniform).
template <int NF>
__device__ __forceinline__ void store_row(const float* row, float* wdst, int nvw, int lane,
                                          bool aligned) {
  __builtin_amdgcn_wave_barrier();  // (no code: keeps the reads behind every lane's writes)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the wave's own LDS writes)
  if (aligned) {
    constexpr int NU = NF / 4;  // 16-byte units of the row
#pragma unroll
    for (int i = 0; i < (NU + 63) / 64; ++i) {
      const int q = 64 * i + lane;
      if (NU % 64 != 0 && q >= NU) break;  // (the last round of 288 units is a half round)
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

// FORMAT: YUV_YUYV422 or YUV_UYVY422. PREP: fmaf(v, a[c], b[c]) where a pixel is converted
// (`prep` is never read without it).
template <int FORMAT, bool PREP>
__global__ __launch_bounds__(kThreads) void b64_yuv422_kernel(const B64Image* imgs, int images,
                                                              const int* d_images,
                                                              const uint8_t* bytes, int hw,
                                                              float* out, int* status,
                                                              YuvCoeffs k, InputPrep prep) {
  if (d_images) images = min(images, *d_images);
  const int img = (int)blockIdx.y;
  if (img >= images) return;  // (workgroup-uniform, before any LDS or memory access)
  __shared__ float stage[kWaves][kB64LaneFloats * 64];
  const B64Image d = imgs[img];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int per = 3 * hw;                      // floats of the image (<= 2^30)
  const int B = 2 * hw;                        // bytes of the frame: whole macropixels
  const int L = 4 * ((B + 2) / 3), pad = (3 - B % 3) % 3;
  const int lk = (int)blockIdx.x * b64::kLanesPerChunk + tid;  // this lane's 16-character group
  const int c0 = 16 * lk;                      // (<= L + 4096 < 2^30)
  float* const row = stage[tid >> 6];
  bool bad = false;
  if (c0 < L) {
    const int nch = min(16, L - c0);  // characters of the string in the window (4, 8, 12, 16)
    const int nd = L - pad - c0;      // data characters from the window's start on
    // (every lane of an image has the string's phase)
    const b64::Window win = b64::load_window(bytes, d.off, c0, nch);
    bad = b64::window_bad(win, nd, nch);
    // 24 bits -> 3 bytes in memory order (byte 0 in the low bits), then 12 bytes = 3 macropixels.
    // Bytes past B (decoded from the padding) lie in no macropixel of the image: B is a
    // multiple of 4 and so is 12 lk.
    uint32_t r[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) r[t] = __builtin_bswap32(win.v[t]) >> 8;
    const uint32_t mp[3] = {r[0] | (r[1] << 24), (r[1] >> 8) | (r[2] << 16),
                            (r[2] >> 16) | (r[3] << 8)};
    float f[kB64LaneFloats];
#pragma unroll
    for (int m = 0; m < 3; ++m) convert_macropixel<FORMAT, PREP>(mp[m], k, prep, f + 6 * m);
    // 72 bytes a lane: 8-byte aligned, nine 8-byte writes
    float2* const wl = reinterpret_cast<float2*>(row) + 9 * lane;
#pragma unroll
    for (int j = 0; j < 9; ++j) wl[j] = make_float2(f[2 * j], f[2 * j + 1]);
  }
  // the wave's first float of the image and its floats of it (<= 0: none, wave-uniform; lanes
  // past the string wrote nothing and their floats are past nvw)
  const int wf0 = kB64LaneFloats * (lk - lane);
  const int nvw = min(kB64LaneFloats * 64, per - wf0);
  if (nvw > 0) {
    float* const img_dst = out + (int64_t)d.slot * per;
    store_row<kB64LaneFloats * 64>(row, img_dst + wf0, nvw, lane,
                                   (reinterpret_cast<uintptr_t>(img_dst) & 15) == 0);
  }
  if (__ballot(bad) != 0 && lane == 0) status[d.rec] = 2;
}

template <int FORMAT, bool PREP>
__global__ __launch_bounds__(kThreads) void raw_yuv422_kernel(const B64Image* imgs, int images,
                                                              const int* d_images,
                                                              const uint8_t* bytes, int hw,
                                                              float* out, YuvCoeffs k,
                                                              InputPrep prep, int base_phase) {
  if (d_images) images = min(images, *d_images);
  const int img = (int)blockIdx.y;
  if (img >= images) return;  // (workgroup-uniform, before any LDS or memory access)
  __shared__ float stage[kWaves][kRawLaneFloats * 64];
  const B64Image d = imgs[img];
  // (`bytes` is the 16-byte aligned address under the caller's pointer)
  const int64_t off = d.off + base_phase;
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int per = 3 * hw;  // floats of the image (<= 2^30)
  const int nmp = hw >> 1;  // macropixels of the frame
  const int g = (int)blockIdx.x * kThreads + tid;  // this lane's 16-byte group of the frame
  const int nm = min(4, nmp - 4 * g);              // its macropixels of the frame (<= 0: none)
  float* const row = stage[tid >> 6];
  if (nm > 0) {
    const int64_t addr = off + (int64_t)kRawLaneBytes * g;
    uint32_t x[4];
    if ((off & 15) == 0 && nm == 4) {  // (the phase test is workgroup-uniform)
      const uint4 v = *reinterpret_cast<const uint4*>(bytes + addr);
      x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
    } else {
      const uint32_t sh = (uint32_t)(off & 3);  // (addr's phase: 16 g is a multiple of 4)
      const int64_t a0 = addr - sh;
      uint32_t w[5];
#pragma unroll
      for (int j = 0; j < 5; ++j)  // (a dword is loaded only when it holds a byte of the lane's)
        w[j] = 4 * j < (int)sh + 4 * nm ? *reinterpret_cast<const U32a*>(bytes + a0 + 4 * j) : 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = __builtin_amdgcn_alignbyte(w[j + 1], w[j], sh);
    }
    float f[kRawLaneFloats];
#pragma unroll
    for (int m = 0; m < 4; ++m) convert_macropixel<FORMAT, PREP>(x[m], k, prep, f + 6 * m);
    // 96 bytes a lane: six 16-byte writes
    float4* const wl = reinterpret_cast<float4*>(row) + 6 * lane;
#pragma unroll
    for (int j = 0; j < 6; ++j)
      wl[j] = make_float4(f[4 * j], f[4 * j + 1], f[4 * j + 2], f[4 * j + 3]);
  }
  // (lanes past the frame wrote nothing and their floats are past nvw; a lane's macropixels
  // past the frame were converted from zeros and lie past nvw as well)
  const int64_t wf0 = (int64_t)kRawLaneFloats * (g - lane);
  const int nvw = (int)min((int64_t)kRawLaneFloats * 64, per - wf0);
  if (nvw > 0) {
    float* const img_dst = out + (int64_t)d.slot * per;
    store_row<kRawLaneFloats * 64>(row, img_dst + wf0, nvw, lane,
                                   (reinterpret_cast<uintptr_t>(img_dst) & 15) == 0);
  }
}

// What both launchers refuse before any launch.
bool refused(const B64Image* imgs, const uint8_t* bytes, int HS, int WS, int C, const float* out,
             int images, const InputPrep* prep, int format) {
  if (HS <= 0 || WS <= 0 || (WS & 1) || C != 3 || !imgs || !bytes || !out) return true;
  if (!yuv_is_422(format)) return true;
  if (prep && prep->nchw) return true;
  return (int64_t)HS * WS * 3 > (1 << 30) || images > 65535;  // (int indices; grid y)
}

}  // namespace

hipError_t b64_yuv422_instances(int images, const B64Image* imgs, const uint8_t* bytes, int HS,
                                int WS, int C, float* out, int* status, hipStream_t stream,
                                const int* d_images, const InputPrep* prep, int format,
                                const YuvCoeffs& coeffs) {
  if (refused(imgs, bytes, HS, WS, C, out, images, prep, format) || !status)
    return hipErrorInvalidValue;
  if (images <= 0) return hipSuccess;
  const int hw = HS * WS;
  const int64_t L = 4 * (((int64_t)2 * hw + 2) / 3);
  const dim3 grid((unsigned)((L + kB64ChunkChars - 1) / kB64ChunkChars), (unsigned)images);
#define GALE_YUV422_LAUNCH(FORMAT, PREP, P)                                                    \
  hipLaunchKernelGGL((b64_yuv422_kernel<FORMAT, PREP>), grid, dim3(kThreads), 0, stream, imgs, \
                     images, d_images, bytes, hw, out, status, coeffs, P)
  const bool id = !prep || prep->identity();
  if (format == YUV_YUYV422) {
    if (id) GALE_YUV422_LAUNCH(YUV_YUYV422, false, InputPrep());
    else GALE_YUV422_LAUNCH(YUV_YUYV422, true, *prep);
  } else {
    if (id) GALE_YUV422_LAUNCH(YUV_UYVY422, false, InputPrep());
    else GALE_YUV422_LAUNCH(YUV_UYVY422, true, *prep);
  }
#undef GALE_YUV422_LAUNCH
  return hipGetLastError();
}

hipError_t raw_yuv422_instances(int images, const B64Image* imgs, const uint8_t* bytes, int HS,
                                int WS, int C, float* out, int* status, hipStream_t stream,
                                const int* d_images, const InputPrep* prep, int format,
                                const YuvCoeffs& coeffs) {
  if (refused(imgs, bytes, HS, WS, C, out, images, prep, format) || !status)
    return hipErrorInvalidValue;
  if (images <= 0) return hipSuccess;
  const int hw = HS * WS;
  const dim3 grid((unsigned)((hw + kRawGroupPixels - 1) / kRawGroupPixels), (unsigned)images);
  // the kernel's alignment is reckoned from its byte pointer: hand it the aligned address under
  // `bytes` and let it add the pointer's own phase to every offset
  const int phase = (int)(reinterpret_cast<uintptr_t>(bytes) & 15);
  const uint8_t* const abytes = bytes - phase;
#define GALE_YUV422_LAUNCH(FORMAT, PREP, P)                                                    \
  hipLaunchKernelGGL((raw_yuv422_kernel<FORMAT, PREP>), grid, dim3(kThreads), 0, stream, imgs, \
                     images, d_images, abytes, hw, out, coeffs, P, phase)
  const bool id = !prep || prep->identity();
  if (format == YUV_YUYV422) {
    if (id) GALE_YUV422_LAUNCH(YUV_YUYV422, false, InputPrep());
    else GALE_YUV422_LAUNCH(YUV_YUYV422, true, *prep);
  } else {
    if (id) GALE_YUV422_LAUNCH(YUV_UYVY422, false, InputPrep());
    else GALE_YUV422_LAUNCH(YUV_UYVY422, true, *prep);
  }
#undef GALE_YUV422_LAUNCH
  return hipGetLastError();
}

}  // namespace gale
