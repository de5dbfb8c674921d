// The host plan of one fetch's base64 device ingest (GpuIngest::run_b64, ingest_crc_b64): CRC
// windows, one B64Image per image of every record that scanned OK, dense arena slots, and the
// layout of the plan and result sections. Host-only (no HIP call), in a translation unit of its
// own so the CPU suite and the sanitizer checker (csrc/tests/b64_plan_check.cpp) can drive it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "gale/kernels.h"

namespace gale {

// The CRC windows of the byte range [rs, re) (a record batch from its attributes on), aligned to
// its end: the first window is the short one. Appends to `chunks`, returns how many.
size_t append_crc_windows(int64_t rs, int64_t re, std::vector<CrcChunk>& chunks);

struct B64PlanRecord {
  int32_t status = 0;     // codec::Status of the host scan (0 = OK)
  int32_t images = 0;     // images the scan counted
  int64_t value_off = 0;  // the record value's offset in the fetch buffer, and its length
  int64_t value_len = 0;
  int64_t arr_off = 0;    // the instances array's offset inside the value
};

struct B64IngestPlan {
  std::vector<CrcChunk> chunks;
  std::vector<std::pair<size_t, size_t>> batch_chunks;  // (first window, count) per batch
  std::vector<B64Image> imgs;   // off: the string's offset in the fetch buffer; slot: dense
  std::vector<int32_t> slot0;   // per record: its first arena slot, -1 = none
  std::vector<int32_t> img0;    // per record: its first descriptor in imgs, -1 = none
  int chunks_per_image = 1;     // decode workgroups per image
  size_t lo = 0, hi = 0;        // the byte span holding the batches and the OK records' values
  size_t ok_records = 0;        // records with status OK (resident in the mirror after the copy)
  // plan sections [CrcChunk x nc][B64Image x ni], result sections [crc u32 x nc]
  // [wg_bad i32 x ni * chunks_per_image]; every offset a multiple of 16
  size_t o_chunks = 0, o_imgs = 0, plan_bytes = 0;
  size_t o_crc = 0, o_bad = 0, result_bytes = 0;
};

// batches: (offset, length) of every record batch in the fetch buffer; attr_off: where a batch's
// CRC'd part starts (kafka::kBatchAttrOffset). offs: for every OK record in order, `images`
// offsets of its strings' first characters relative to its instances array
// (codec::b64_image_offsets). A record gets arena slots only if all its images fit in
// arena_bytes; that record and every later one is otherwise left without (not an error: the
// replica decodes them from the resident mirror). Throws std::invalid_argument when the inputs
// contradict each other (a string outside its record's value, too few offsets).
void plan_b64_ingest(const std::vector<std::pair<int64_t, int64_t>>& batches, int64_t attr_off,
                     bool check_crcs, const std::vector<B64PlanRecord>& recs,
                     const std::vector<uint32_t>& offs, int H, int W, int C, size_t arena_bytes,
                     size_t fetch_size, B64IngestPlan& out);

}  // namespace gale
