// The host plans of one fetch's device ingest: plan_json_ingest / fill_json_ingest for JSON
// number records (GpuIngest::run, ingest_crc_count + json_parse_instances) and plan_b64_ingest
// for base64 image records (GpuIngest::run_b64, ingest_crc_b64). A plan is every byte offset the
// ingest kernels are handed: the CRC windows, the span that crosses the link, the record tables,
// arena slots, and the layout of the plan and result sections. Host-only (no HIP call), in a
// translation unit of its own so the CPU suite and the sanitizer checkers
// (csrc/tests/json_plan_check.cpp, csrc/tests/b64_plan_check.cpp) can drive it.
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

// ---- JSON number records ------------------------------------------------------------------------

struct JsonPlanRecord {
  int32_t status = 0;     // codec::Status of the host envelope scan (0 = OK)
  int64_t value_off = 0;  // the record value's offset in the fetch buffer, and its length
  int64_t value_len = 0;
  int64_t arr_off = 0;    // the instances array's extent inside the value
  int64_t arr_len = 0;
};

// Phase 1, the layout. The plan sections (what fill_json_ingest writes, what one DMA carries):
//   [pack tab u32 x 2 x ng][CrcChunk x nc][int2 group x ngroups][JsonRecord x nr]
//   [parse JsonRecord x np][parse tile -> parse record i32 x ptiles]
// and the result sections behind them (stored by the kernels, never copied):
//   [group sum i32 x ngroups][crc u32 x nc][group verdict i32 x ngroups]
//   [parse tile verdict i32 x ptiles]
// Every section offset is a multiple of 16.
struct JsonIngestPlan {
  std::vector<CrcChunk> chunks;                         // nc CRC windows
  std::vector<std::pair<size_t, size_t>> batch_chunks;  // (first window, count) per batch
  std::vector<int> rec_of;  // counted record j -> record index (the records that scanned OK)
  std::vector<int> pjs;     // parse record k -> counted record j (the ones parsed at ingest)
  int ntiles = 0, ngroups = 0;  // tiles and tile groups of the counted records
  int ptiles = 0;               // tiles of the parsed records
  // what crosses the link: the span [lo, lo + span) holding batches and records, raw, or (packed:
  // the source's PackTap, text_pack.h) the whole body as its packed stream of `link` bytes with
  // ng pack groups, expanded in the device mirror. The copy moves [c_lo, c_lo + c_len).
  bool packed = false;
  size_t lo = 0, span = 0, link = 0, ng = 0;
  size_t c_lo = 0, c_len = 0;
  size_t tab_off = 0;  // packed: where the pack group table (ng x 2 words) stands in the chunk
  size_t used = 0;  // end of the bytes the device mirror holds (text, or the packed stream)
  // the per-tile token counts stay with the fetch buffer: at the end of its device mirror when
  // they fit behind `used`, so the parse - at ingest or in the replica that later takes these
  // records - reuses them instead of counting again. -1: they do not fit (lane scratch, no parse)
  int64_t cnt_base = -1;
  size_t o_chunks = 0, o_groups = 0, o_recs = 0, o_precs = 0, o_ptr = 0;
  size_t o_gsum = 0;  // the end of the plan sections: the prefix [0, o_gsum) is what is DMA'd
  size_t o_crc = 0, o_gbad = 0, o_pbad = 0, io_bytes = 0;
  // the plan rides behind the fetch in its own pinned chunk at plan_off (past every byte of the
  // fetch: host code may still read records this plan skips) when it fits before the counts
  // and stays clear of a packed body's group table at tab_off
  size_t plan_off = 0;
  bool plan_in_chunk = false;
  int64_t per = 0;  // H * W * C; a record's arena slots start at ceil(off / (2 * per))

  size_t nc() const { return chunks.size(); }
  size_t nr() const { return rec_of.size(); }
  size_t np() const { return pjs.size(); }
  bool empty() const { return chunks.empty() && rec_of.empty(); }  // nothing to copy or launch
  // where a counted record's count block sits in the device mirror (cnt_base >= 0)
  int64_t cnt_off(const JsonRecord& r) const {
    return cnt_base + ((int64_t)r.tile0 + r.grp0) * (int64_t)sizeof(int);
  }
};

// batches: (offset, length) of every record batch in the fetch buffer; attr_off: where a batch's
// CRC'd part starts (kafka::kBatchAttrOffset). arena_bytes 0: no parse at ingest; otherwise every
// counted record whose arena slots fit is parsed - one that does not fit is left out alone, later
// ones that fit are still parsed (slots derive from text offsets, not from a running count).
// dev_cap: the size of the pinned chunk and its device mirror. tap_result: the packed stream's
// size, < 0 = the body is raw. plan_separate: never ride in the chunk. Throws
// std::invalid_argument when the inputs contradict each other (a batch or an OK record's value
// outside the fetch, an array outside its value, negative extents, H * W * C <= 0). `out` is
// overwritten; its vectors keep their capacity, so a caller that reuses it allocates nothing.
void plan_json_ingest(const std::vector<std::pair<int64_t, int64_t>>& batches, int64_t attr_off,
                      bool check_crcs, const std::vector<JsonPlanRecord>& recs, int H, int W,
                      int C, size_t arena_bytes, size_t fetch_size, size_t dev_cap,
                      int64_t tap_result, bool plan_separate, JsonIngestPlan& out);

// Phase 2: writes the windows, the group table, the count and parse JsonRecords and the parse
// tile map of `plan` (made from the same `recs`) straight into dst + o_*: the fetch's pinned
// chunk at plan_off, or a lane buffer. Touches nothing outside those sections, all of which lie
// in [o_chunks, o_gsum); the pack group table in front of them is the caller's.
void fill_json_ingest(const JsonIngestPlan& plan, const std::vector<JsonPlanRecord>& recs,
                      uint8_t* dst);

// ---- base64 image records -----------------------------------------------------------------------

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
  size_t c_lo = 0, c_len = 0;   // the copy: that span from its 16-byte-aligned start, raw
  size_t plan_off = 0;          // where the plan rides in the fetch's chunk, when it fits there
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
