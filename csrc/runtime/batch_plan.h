// The host plan of one batch in the GPU replica (GpuReplica::submit): where every record's text
// stands in the slot's device bytes, what is copied there from which buffer, and every byte of the
// slot's parser metadata. Host-only (no HIP call), in a translation unit of its own so the CPU
// suite (tests/test_batch_plan_cpu.py) and the sanitizer checker
// (csrc/tests/batch_plan_check.cpp) can drive it.
//
// The slot's metadata, pinned on the host and mirrored on the device:
//   [64-byte header][JsonRecord x max_batch][float* x max_batch][tile -> record i32 x tiles_cap]
// base64 image records (b64) put [B64Image x max_batch][status i32 x max_batch] in the record
// table's place; they have no tile map.
//
// Two phases. plan_batch needs no slot address: it lays the text out relative to the slot's
// device buffer and counts, so the caller can grow the slot's buffers to fit before a byte is
// written. A record's tile count depends on its offset only through `off & 15`; a record staged
// or copied here keeps its source phase, and a resident record's offset is the distance from the
// slot's buffer to its device address, whose phase is the address's own because the slot's buffer
// is a 256-byte-aligned allocation. So the tile count is known before the buffer exists.
// fill_batch then writes the metadata for the buffer's final address.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "gale/kernels.h"

namespace gale {

// The header's words; the rest of its 64 bytes is never written.
enum MetaHeader { kHdrRecords = 0, kHdrTiles = 1, kHdrImages = 2, kHdrB64 = 3 };

// How the replica launches its step, as far as the metadata is concerned:
//   OpByOp    counts passed from the host; the record table onwards is copied, the header is not
//             used; verdicts come back in the table
//   Captured  one graph replay that copies the whole allocation and reads the counts from the
//             header; verdicts come back in the table
//   Kernels   the used prefix is copied ahead of kernels that read the counts from the header;
//             verdicts are raised elsewhere (a status array of the slot's own)
enum class StepForm { OpByOp, Captured, Kernels };

struct MetaRange {
  size_t off = 0, bytes = 0;
  size_t end() const { return off + bytes; }
};

struct BatchPlan;

struct MetaLayout {
  static constexpr size_t kHeaderBytes = 64;
  int max_batch = 0, tiles_cap = 0;
  size_t hdr = 0, recs = 0, xs = 0, tiles = 0;  // header, record table, input pointers, tile map
  size_t b64_table = 0, b64_status = 0;         // b64: descriptors and status words (in `recs`)
  size_t total = 0;
  MetaLayout() = default;
  MetaLayout(int max_batch, int tiles_cap);
  // The metadata bytes the planned batch's step copies to the device; fill_batch writes nothing
  // outside them.
  MetaRange used(const BatchPlan& p) const;
};

struct BatchPlanRecord {
  uint64_t buf = 0;     // id of its fetch buffer: records with the same id may share one copy
  int64_t arr_off = 0;  // the instances array's offset in that buffer, and its length
  int64_t arr_len = 0;
  int32_t images = 0;
  bool pinned = false;     // the buffer is page-locked: copied from where it is
  bool resident = false;   // the text is in this replica's device memory already
  bool preparsed = false;  // so are its parsed images: the step runs the forward alone for it
  uint64_t dev_text = 0;    // resident: the array's device address
  uint64_t dev_counts = 0;  // resident: its tile counts' device address, 0 = none
  uint64_t dev_image = 0;   // preparsed: its first image's device address
  // b64: its strings start at offs[b64_first + k], k < b64_n, relative to the array (b64_n is
  // what the scan found: not `images` = the record does not match its scan)
  int32_t b64_first = 0, b64_n = 0;
};

struct BatchPlan {
  struct Span {  // buffer bytes [lo, lo + len), lo a multiple of 16, copied to device offset dev
    uint64_t buf;
    size_t lo, len, dev;
  };
  struct Staged {  // record rec's array, gathered at `host` in the pinned staging buffer
    int rec;
    size_t host, len;
  };
  std::vector<Span> spans;
  std::vector<Staged> staged;
  std::vector<int> parse_idx;  // per record: its index among those the step parses, -1 = none
  std::vector<int64_t> off;    // per parsed record not resident: its array's device offset
  size_t staged_bytes = 0;     // the staging buffer's used bytes, copied to device offset staged_dev
  size_t staged_dev = 0;
  size_t dev_total = 0;  // device bytes the batch needs (the caller adds the parser's read slack)
  int nrec = 0, ntiles = 0, img = 0, b64n = 0;  // records, tiles, images, b64 descriptors
  int npre = 0, resident = 0;                   // preparsed / resident records
  bool count_pass = false;  // some parsed record has no tile counts yet
  // what the plan was made for (plan_batch's arguments)
  StepForm form = StepForm::OpByOp;
  bool ptr_input = false, b64 = false;
  int64_t per = 0;  // H * W * C
  // a batch the step parses nothing of (every record preparsed, each its own verdict)
  void all_preparsed(size_t records) { parse_idx.assign(records, -1); }
};

// Phase 1. offs: the b64 records' string offsets (see BatchPlanRecord). ptr_input: the forward
// reads each image through the input pointer table. Throws std::logic_error when the images
// exceed max_batch or a b64 record does not match its scan. `out` is overwritten; its vectors
// keep their capacity, so a caller that reuses it allocates nothing.
void plan_batch(const std::vector<BatchPlanRecord>& recs, int max_batch, int64_t per,
                StepForm form, bool ptr_input, bool b64, BatchPlan& out);

// Phase 2: the header, the record table (status zeroed) or the dense descriptor table and the
// parsed records' zeroed status words, the input pointer table (ptr_input) and the tile map of
// `plan` (made from the same `recs`), written at dst + the layout's offsets, for a device text
// buffer at d_bytes and the slot's own input buffer at input_base. Touches nothing outside
// layout.used(plan); layout.tiles_cap >= plan.ntiles.
void fill_batch(const BatchPlan& plan, const std::vector<BatchPlanRecord>& recs,
                const std::vector<uint32_t>& offs, const MetaLayout& layout, uint64_t d_bytes,
                uint64_t input_base, uint8_t* dst);

}  // namespace gale
