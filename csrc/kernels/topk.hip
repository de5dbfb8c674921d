// Top-k prediction output on the GPU: of each softmax row the k best classes, as class indices
// and Java Float.toString text slots (java_float.cuh), in score order.
//
// The order is the one codec/json_codec.h defines ("Score order"): entries descend by
// key(v) = bits(v) ^ (bits(v) >> 31 ? 0xffffffff : 0x80000000) compared as unsigned, ties to
// the lower class index. A row entry is the 64-bit word (key << 32) | ~index, so "better" is one
// unsigned comparison and no two entries of a row are equal; every valid word is > 0
// (index <= 4095, so ~index >= 0xfffff000).
//
// One wave per row, 4 rows per 256-thread workgroup. Lane l owns entries l, l + 64, ...: it
// stores their keys in the wave's LDS region once (classes * 4 bytes) and only ever reads back
// its own, so there is no cross-lane LDS hazard and no barrier. Round j takes the lane's best
// word below round j - 1's winner (nothing is retired or rewritten), then a 64-lane __shfl_xor
// max-reduction; lane j keeps the winner. After k rounds lanes [0, k) hold the row's result in
// order: each formats its value and the wave stores k contiguous 16-byte slots and k contiguous
// indices. No atomics, no per-lane arrays, nothing read past x[rows * classes].
#include "common.cuh"
#include "gale/kernels.h"
#include "java_float.cuh"

namespace gale {
namespace {

constexpr int kTopkWaves = 4;       // rows per workgroup
constexpr int kTopkMaxK = 64;       // one winner per lane
constexpr int kTopkMaxClasses = 4096;

__device__ __forceinline__ uint32_t score_key(uint32_t bits) {
  return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);
}

__device__ __forceinline__ uint32_t score_bits(uint32_t key) {  // score_key's inverse
  return (key >> 31) ? key ^ 0x80000000u : ~key;
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64);
    const uint32_t hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    const uint64_t w = ((uint64_t)hi << 32) | lo;
    v = w > v ? w : v;
  }
  return v;
}

__global__ __launch_bounds__(256) void topk_kernel(int rows, const int* d_rows, int classes, int k,
                                                   const float* __restrict__ x,
                                                   uint4* __restrict__ text,
                                                   int* __restrict__ idx, const int* d_nrec,
                                                   int* status, int* status_out) {
  extern __shared__ uint32_t s_keys[];  // [kTopkWaves][classes]
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (d_nrec && i < *d_nrec) {  // the parse verdicts: to the host, cleared for the next batch
    status_out[i] = status[i];
    status[i] = 0;
  }
  if (d_rows) rows = min(rows, *d_rows);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.x * kTopkWaves + wave;
  if (r >= rows) return;  // (wave-uniform; no barrier follows)
  const float* xr = x + (size_t)r * classes;
  uint32_t* keys = s_keys + wave * classes;
  for (int c = lane; c < classes; c += 64) keys[c] = score_key(__float_as_uint(xr[c]));
  uint64_t below = 0;  // the previous round's winner
  uint64_t mine = 0;
  for (int j = 0; j < k; ++j) {
    uint64_t best = 0;  // (below every entry: a lane without candidates left)
    for (int c = lane; c < classes; c += 64) {
      const uint64_t w = ((uint64_t)keys[c] << 32) | (uint32_t)~c;
      // (round 0 takes every entry: NaN 0x7fffffff at class 0 is the all-ones word)
      best = ((j == 0 || w < below) && w > best) ? w : best;
    }
    below = wave_max_u64(best);
    if (lane == j) mine = below;
  }
  if (lane >= k) return;
  const size_t o = (size_t)r * k + lane;
  text[o] = java_float_slot(__uint_as_float(score_bits((uint32_t)(mine >> 32))));
  idx[o] = (int)~(uint32_t)mine;
}

hipError_t launch(int rows, const int* d_rows, int classes, int k, const float* x, void* text16,
                  int32_t* idx, const int* d_nrec, int* status, int* status_out,
                  hipStream_t stream) {
  if (k < 1 || k > kTopkMaxK || k > classes || classes > kTopkMaxClasses)
    return hipErrorInvalidValue;
  if (rows <= 0) return hipSuccess;
  const unsigned blocks = (unsigned)((rows + kTopkWaves - 1) / kTopkWaves);
  const size_t lds = sizeof(uint32_t) * kTopkWaves * (size_t)classes;  // <= 64 KiB
  hipLaunchKernelGGL(topk_kernel, dim3(blocks), dim3(256), lds, stream, rows, d_rows, classes, k,
                     x, static_cast<uint4*>(text16), idx, d_nrec, status, status_out);
  return hipGetLastError();
}

}  // namespace

hipError_t topk_java(int rows, int classes, int k, const float* x, void* text16, int32_t* idx,
                     hipStream_t stream) {
  return launch(rows, nullptr, classes, k, x, text16, idx, nullptr, nullptr, nullptr, stream);
}

hipError_t topk_java_dev(int max_rows, const int* d_rows, int classes, int k, const float* x,
                         void* text16, int32_t* idx, hipStream_t stream) {
  if (!d_rows) return hipErrorInvalidValue;
  return launch(max_rows, d_rows, classes, k, x, text16, idx, nullptr, nullptr, nullptr, stream);
}

hipError_t topk_java_step(int max_rows, const int* d_rows, int classes, int k, const float* x,
                          void* text16, int32_t* idx, const int* d_nrec, int* status,
                          int* status_out, hipStream_t stream) {
  if (!d_rows || !d_nrec || !status || !status_out) return hipErrorInvalidValue;
  return launch(max_rows, d_rows, classes, k, x, text16, idx, d_nrec, status, status_out, stream);
}

}  // namespace gale
