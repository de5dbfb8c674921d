// GPU decoder of base64 uint8 image records (gale/kernels.h: b64_decode_instances).
//
//   {"instances":[{"b64":"<L characters>"}, ...]}      L = 4 * ceil(H*W*C / 3)
//
// The host scan (codec::scan_instances_b64) has checked the element list and located every
// string without reading it; this kernel reads the characters, judges them and stores the
// pixels as fp32 NHWC. It is a streaming kernel: 1 byte in, 3 bytes out per character, no
// number conversion, no token counting.
//
// Work split: lane k of an image decodes characters [16k, 16k + 16) into bytes [12k, 12k + 12),
// 12 floats (48 contiguous bytes). A 256-thread workgroup covers kB64ChunkChars = 4096
// characters (one 32x32x3 image); grid = (chunks per image, images). The floats of a wave are
// staged in LDS (3 KB per wave, no other LDS) so that its store instructions are contiguous;
// NCHW-ordered strings transpose at the store, straight to global memory.
//
// Alignment: a string starts at an arbitrary phase modulo 16 of the staged buffer (the replica's
// span copy preserves the phase the record had in the fetch buffer). A lane reads its 16
// characters through b64::load_window (b64_decode.cuh, which states the read bound): aligned
// 16-byte words, byte-aligned in registers (v_alignbyte_b32 behind a wave-uniform switch on the
// dword phase, as the JSON parser aligns its windows). No unaligned 16-byte load is issued.
//
// Verdict: b64::window_bad per lane, branch-free but for the string's last lane; a wave with a
// bad lane stores the constant 2 into its record's status once (every wave of a bad record
// stores the same value, so a plain store is enough). Images of a bad record are still written,
// inside their own slot.
//
// The decode of one chunk is b64::b64_decode_body (b64_decode.cuh), shared with the fetch ingest
// (b64_ingest.hip); the window under it is shared with the YUV decoder as well. The kernels
// here map the 2-D grid onto the body and raise the record status.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "b64_decode.cuh"
#include "gale/kernels.h"

namespace gale {
namespace {

// grid = (chunks per image, images); the decode itself is b64::b64_decode_body (b64_decode.cuh)
template <bool PREP, bool NCHW, int CT>
__device__ __forceinline__ void b64_decode_grid(const B64Image* imgs, int images,
                                                const int* d_images, const uint8_t* bytes, int H,
                                                int W, int C, float* out, int* status,
                                                const InputPrep& prep) {
  if (d_images) images = min(images, *d_images);
  const int img = (int)blockIdx.y;
  if (img >= images) return;  // (workgroup-uniform)
  const B64Image d = imgs[img];
  __shared__ b64::Stage stage[b64::kStageWaves];
  const bool bad = b64::b64_decode_body<PREP, NCHW, CT>(d, (int)blockIdx.x, (int)threadIdx.x,
                                                        bytes, H, W, C, out, prep, stage);
  if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) status[d.rec] = 2;
}

__global__ __launch_bounds__(256) void b64_decode_kernel(const B64Image* imgs, int images,
                                                         const int* d_images,
                                                         const uint8_t* bytes, int H, int W,
                                                         int C, float* out, int* status) {
  b64_decode_grid<false, false, 0>(imgs, images, d_images, bytes, H, W, C, out, status,
                                   InputPrep());
}

// With input preprocessing: `prep` arrives by value in the kernel arguments, so it is captured
// into the step graph with the other scalars.
template <bool NCHW, int CT>
__global__ __launch_bounds__(256) void b64_decode_prep_kernel(const B64Image* imgs, int images,
                                                              const int* d_images,
                                                              const uint8_t* bytes, int H, int W,
                                                              int C, float* out, int* status,
                                                              InputPrep prep) {
  b64_decode_grid<true, NCHW, CT>(imgs, images, d_images, bytes, H, W, C, out, status, prep);
}

}  // namespace

hipError_t b64_decode_instances(int images, const B64Image* imgs, const uint8_t* bytes, int H,
                                int W, int C, float* out, int* status, hipStream_t stream,
                                const int* d_images, const InputPrep* prep) {
  if (images <= 0) return hipSuccess;
  if (H <= 0 || W <= 0 || C <= 0 || !imgs || !bytes || !out || !status)
    return hipErrorInvalidValue;
  const int64_t per = (int64_t)H * W * C;
  if (per > (1 << 30) || images > 65535) return hipErrorInvalidValue;  // (int indices; grid y)
  const bool with_prep = prep && !prep->identity();
  if (with_prep && C > 4)  // a channel index past the four coefficient slots
    for (int i = 1; i < 4; ++i)
      if (prep->a[i] != prep->a[0] || prep->b[i] != prep->b[0]) return hipErrorInvalidValue;
  const int64_t L = 4 * ((per + 2) / 3);
  // lanes with 16 k < L: their first value 12 k is below per (12 k >= per would mean 16 k >= L)
  const dim3 grid((unsigned)((L + kB64ChunkChars - 1) / kB64ChunkChars), (unsigned)images);
  const dim3 block(kB64ChunkChars / 16);
#define GALE_B64_LAUNCH(KERNEL)                                                              \
  hipLaunchKernelGGL(KERNEL, grid, block, 0, stream, imgs, images, d_images, bytes, H, W, C, \
                     out, status, *prep)
  if (!with_prep)
    hipLaunchKernelGGL(b64_decode_kernel, grid, block, 0, stream, imgs, images, d_images, bytes,
                       H, W, C, out, status);
  else if (prep->nchw)
    GALE_B64_LAUNCH((b64_decode_prep_kernel<true, 0>));
  else if (C == 3)
    GALE_B64_LAUNCH((b64_decode_prep_kernel<false, 3>));
  else if (C == 1)
    GALE_B64_LAUNCH((b64_decode_prep_kernel<false, 1>));
  else
    GALE_B64_LAUNCH((b64_decode_prep_kernel<false, 0>));
#undef GALE_B64_LAUNCH
  return hipGetLastError();
}

}  // namespace gale
