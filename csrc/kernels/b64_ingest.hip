// The GPU ingest of one fetch of base64 image records in ONE launch (gale/kernels.h:
// ingest_crc_b64): the batches' CRC32C windows and the decode of every image's string into the
// fetch's image arena.
//
// The host scan (codec::scan_instances_b64) knows every record's image count and every string's
// offset before anything is launched, so unlike the JSON ingest there is no token count, no
// second pass and no look-back: workgroups [0, crc_blocks) fold CRC windows (crc::crc_windows,
// as ingest_crc_count), workgroup crc_blocks + g decodes chunk g % chunks_per_image of image
// g / chunks_per_image with b64::b64_decode_body - the batch step's decoder, same loads, same
// verdict rules, same store paths - from the fetch's device mirror into arena + slot * H*W*C.
//
// Verdicts: every decode workgroup stores exactly one word, wg_bad[g] = 2 (a lane saw a bad
// character or bad padding) or 0, by a plain vector store, so the array is never zeroed, nothing
// is atomic, and it may be host-mapped memory; the host takes the max over a record's words.
//
// LDS: a workgroup is either a CRC workgroup (4.25 KB of tables) or a decode workgroup (12 KB of
// staging), so both views share one 12 KB allocation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "b64_decode.cuh"
#include "crc32c.cuh"
#include "gale/kernels.h"

namespace gale {
namespace {

static_assert(sizeof(b64::Stage) * b64::kStageWaves >= sizeof(uint32_t) * crc::kTableWords,
              "the CRC tables fit in the decode staging");
static_assert(b64::kStageWaves == crc::kCrcWaves, "one workgroup shape for both roles");

template <bool PREP, bool NCHW, int CT>
__global__ __launch_bounds__(256) void ingest_crc_b64_kernel(
    const uint8_t* bytes, const CrcChunk* chunks, int nchunks, const uint32_t* tables,
    uint32_t* crc_out, int crc_blocks, const B64Image* imgs, int chunks_per_image, int H, int W,
    int C, float* arena, int* wg_bad, InputPrep prep) {
  __shared__ b64::Stage stage[b64::kStageWaves];
  if ((int)blockIdx.x < crc_blocks) {  // (workgroup-uniform)
    uint32_t* T = reinterpret_cast<uint32_t*>(&stage[0][0]);
    crc::crc_stage_tables(tables, T);
    crc::crc_windows(bytes, chunks, nchunks, T, crc_out, (int)blockIdx.x, crc_blocks);
    return;
  }
  __shared__ int wave_bad[b64::kStageWaves];
  const int g = (int)blockIdx.x - crc_blocks;
  const int img = g / chunks_per_image;
  const int chunk = g - img * chunks_per_image;
  const B64Image d = imgs[img];
  const bool bad = b64::b64_decode_body<PREP, NCHW, CT>(d, chunk, (int)threadIdx.x, bytes, H, W,
                                                        C, arena, prep, stage);
  const bool wbad = __ballot(bad) != 0;
  if ((threadIdx.x & 63) == 0) wave_bad[threadIdx.x >> 6] = wbad ? 2 : 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    int v = 0;
#pragma unroll
    for (int i = 0; i < b64::kStageWaves; ++i) v |= wave_bad[i];
    wg_bad[g] = v;
  }
}

}  // namespace

hipError_t ingest_crc_b64(const uint8_t* bytes, const CrcChunk* chunks, int nchunks,
                          const uint32_t* tables, uint32_t* crc_out, int images,
                          const B64Image* imgs, int H, int W, int C, float* arena, int* wg_bad,
                          hipStream_t stream, const InputPrep* prep) {
  if (nchunks < 0) nchunks = 0;
  if (images < 0) images = 0;
  if (nchunks == 0 && images == 0) return hipSuccess;
  if (!bytes) return hipErrorInvalidValue;
  if (nchunks > 0 && (!chunks || !tables || !crc_out)) return hipErrorInvalidValue;
  int crc_blocks = (nchunks + crc::kCrcWaves - 1) / crc::kCrcWaves;
  if (crc_blocks > 1024) crc_blocks = 1024;  // (windows loop: the table load is amortised)
  int64_t cpi = 1;
  if (images > 0) {
    if (H <= 0 || W <= 0 || C <= 0 || !imgs || !arena || !wg_bad) return hipErrorInvalidValue;
    const int64_t per = (int64_t)H * W * C;
    if (per > (1 << 30)) return hipErrorInvalidValue;  // (int indices)
    const int64_t L = 4 * ((per + 2) / 3);
    // lanes with 16 k < L: their first value 12 k is below per (12 k >= per would mean 16 k >= L)
    cpi = (L + kB64ChunkChars - 1) / kB64ChunkChars;
  }
  if (!b64::prep_fits(prep, C)) return hipErrorInvalidValue;
  const int64_t blocks = (int64_t)images * cpi + crc_blocks;
  if (blocks > 0x7fffffffll) return hipErrorInvalidValue;  // (the 1-D grid limit)
  const bool with_prep = images > 0 && prep && !prep->identity();
  const InputPrep p = with_prep ? *prep : InputPrep();
#define GALE_B64_INGEST_LAUNCH(KERNEL)                                                         \
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)blocks), dim3(b64::kLanesPerChunk), 0, stream,     \
                     bytes, chunks, nchunks, tables, crc_out, crc_blocks, imgs, (int)cpi, H, W, \
                     C, arena, wg_bad, p)
  if (!with_prep)
    GALE_B64_INGEST_LAUNCH((ingest_crc_b64_kernel<false, false, 0>));
  else if (p.nchw)
    GALE_B64_INGEST_LAUNCH((ingest_crc_b64_kernel<true, true, 0>));
  else if (C == 3)
    GALE_B64_INGEST_LAUNCH((ingest_crc_b64_kernel<true, false, 3>));
  else if (C == 1)
    GALE_B64_INGEST_LAUNCH((ingest_crc_b64_kernel<true, false, 1>));
  else
    GALE_B64_INGEST_LAUNCH((ingest_crc_b64_kernel<true, false, 0>));
#undef GALE_B64_INGEST_LAUNCH
  return hipGetLastError();
}

}  // namespace gale
