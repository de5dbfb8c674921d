// plan_b64_ingest (see b64_ingest_plan.h).
#include "b64_ingest_plan.h"

#include <algorithm>
#include <stdexcept>

namespace gale {

namespace {
size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
}  // namespace

size_t append_crc_windows(int64_t rs, int64_t re, std::vector<CrcChunk>& chunks) {
  const int64_t len = re - rs;
  if (len <= 0) return 0;
  const int64_t n = (len + kCrcChunkBytes - 1) / kCrcChunkBytes;
  for (int64_t k = 0; k < n; ++k) {
    CrcChunk c;
    c.end = re - (int64_t)kCrcChunkBytes * (n - 1 - k);
    c.len = k == 0 ? (int32_t)(len - (int64_t)kCrcChunkBytes * (n - 1)) : kCrcChunkBytes;
    c.pad_ = 0;
    chunks.push_back(c);
  }
  return (size_t)n;
}

void plan_b64_ingest(const std::vector<std::pair<int64_t, int64_t>>& batches, int64_t attr_off,
                     bool check_crcs, const std::vector<B64PlanRecord>& recs,
                     const std::vector<uint32_t>& offs, int H, int W, int C, size_t arena_bytes,
                     size_t fetch_size, B64IngestPlan& out) {
  out = B64IngestPlan();
  if (H <= 0 || W <= 0 || C <= 0) throw std::invalid_argument("b64 ingest plan: bad image shape");
  const int64_t per = (int64_t)H * W * C;
  if (per > (1 << 30)) throw std::invalid_argument("b64 ingest plan: image too large");
  const int64_t L = 4 * ((per + 2) / 3);
  out.chunks_per_image = (int)((L + kB64ChunkChars - 1) / kB64ChunkChars);
  size_t lo = fetch_size, hi = 0;
  for (const auto& b : batches) {
    if (b.first < 0 || b.second < 0 || (uint64_t)b.first + (uint64_t)b.second > fetch_size)
      throw std::invalid_argument("b64 ingest plan: batch outside the fetch");
    lo = std::min(lo, (size_t)b.first);
    hi = std::max(hi, (size_t)(b.first + b.second));
    if (!check_crcs) continue;
    const size_t first = out.chunks.size();
    const size_t n = append_crc_windows(b.first + attr_off, b.first + b.second, out.chunks);
    out.batch_chunks.emplace_back(first, n);
  }
  out.slot0.assign(recs.size(), -1);
  out.img0.assign(recs.size(), -1);
  size_t next_off = 0;    // into offs
  int64_t next_slot = 0;  // dense, in record order
  bool cut = false;       // a record did not fit: it and every later one stay without slots
  for (size_t i = 0; i < recs.size(); ++i) {
    const B64PlanRecord& r = recs[i];
    if (r.status != 0) continue;
    if (r.images <= 0 || r.value_off < 0 || r.value_len < 0 || r.arr_off < 0 ||
        r.arr_off > r.value_len || (uint64_t)r.value_off + (uint64_t)r.value_len > fetch_size)
      throw std::invalid_argument("b64 ingest plan: record outside the fetch");
    if (offs.size() - next_off < (size_t)r.images)
      throw std::invalid_argument("b64 ingest plan: fewer string offsets than images");
    ++out.ok_records;
    lo = std::min(lo, (size_t)r.value_off);
    hi = std::max(hi, (size_t)(r.value_off + r.value_len));
    const uint32_t* ro = offs.data() + next_off;
    next_off += (size_t)r.images;
    // every string inside its record's value (the kernel's read bounds rest on this)
    for (int32_t k = 0; k < r.images; ++k)
      if (r.arr_off + (int64_t)ro[k] + L > r.value_len)
        throw std::invalid_argument("b64 ingest plan: string outside its record");
    if (!cut && ((uint64_t)(next_slot + r.images) * (uint64_t)per * sizeof(float) > arena_bytes ||
                 next_slot + r.images > 0x7fffffffll))  // (B64Image::slot is an int32)
      cut = true;
    if (cut) continue;
    out.slot0[i] = (int32_t)next_slot;
    out.img0[i] = (int32_t)out.imgs.size();
    for (int32_t k = 0; k < r.images; ++k) {
      B64Image d;
      d.off = r.value_off + r.arr_off + (int64_t)ro[k];
      d.slot = (int32_t)(next_slot + k);
      d.rec = (int32_t)i;  // (not read by the kernel)
      out.imgs.push_back(d);
    }
    next_slot += r.images;
  }
  if (hi < lo) lo = hi = 0;
  out.lo = lo;
  out.hi = hi;
  const size_t nc = out.chunks.size(), ni = out.imgs.size();
  out.o_chunks = 0;
  out.o_imgs = out.o_chunks + align16(nc * sizeof(CrcChunk));
  out.plan_bytes = out.o_imgs + align16(ni * sizeof(B64Image));
  out.o_crc = 0;
  out.o_bad = out.o_crc + align16(nc * sizeof(uint32_t));
  out.result_bytes = out.o_bad + align16(ni * (size_t)out.chunks_per_image * sizeof(int32_t));
}

}  // namespace gale
