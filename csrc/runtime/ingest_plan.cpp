// plan_json_ingest / fill_json_ingest / plan_b64_ingest (see ingest_plan.h).
#include "ingest_plan.h"

#include <string.h>

#include <algorithm>
#include <stdexcept>

#include "../codec/text_pack.h"

namespace gale {

namespace {

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// What both plans do with the record batches: widen the span [lo, hi) over them and, with
// check_crcs, append each batch's CRC windows (from its attributes on).
void plan_batches(const std::vector<std::pair<int64_t, int64_t>>& batches, int64_t attr_off,
                  bool check_crcs, size_t fetch_size, std::vector<CrcChunk>& chunks,
                  std::vector<std::pair<size_t, size_t>>& batch_chunks, size_t& lo, size_t& hi) {
  for (const auto& b : batches) {
    if (b.first < 0 || b.second < 0 || (uint64_t)b.first + (uint64_t)b.second > fetch_size)
      throw std::invalid_argument("ingest plan: batch outside the fetch");
    lo = std::min(lo, (size_t)b.first);
    hi = std::max(hi, (size_t)(b.first + b.second));
    if (!check_crcs) continue;
    const size_t first = chunks.size();
    const size_t n = append_crc_windows(b.first + attr_off, b.first + b.second, chunks);
    batch_chunks.emplace_back(first, n);
  }
}

// H * W * C, refusing shapes no plan takes
int64_t image_elements(int H, int W, int C) {
  if (H <= 0 || W <= 0 || C <= 0) throw std::invalid_argument("ingest plan: bad image shape");
  const int64_t per = (int64_t)H * W * C;
  if (per > (1 << 30)) throw std::invalid_argument("ingest plan: image too large");
  return per;
}

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

void plan_json_ingest(const std::vector<std::pair<int64_t, int64_t>>& batches, int64_t attr_off,
                      bool check_crcs, const std::vector<JsonPlanRecord>& recs, int H, int W,
                      int C, size_t arena_bytes, size_t fetch_size, size_t dev_cap,
                      int64_t tap_result, bool plan_separate, JsonIngestPlan& out) {
  {
    JsonIngestPlan fresh;  // (the vectors keep their capacity)
    fresh.chunks.swap(out.chunks);
    fresh.batch_chunks.swap(out.batch_chunks);
    fresh.rec_of.swap(out.rec_of);
    fresh.pjs.swap(out.pjs);
    fresh.chunks.clear();
    fresh.batch_chunks.clear();
    fresh.rec_of.clear();
    fresh.pjs.clear();
    out = std::move(fresh);
  }
  const int64_t per = out.per = image_elements(H, W, C);
  // ---- CRC windows (aligned to each batch's end) and the records to count
  size_t lo = fetch_size, hi = 0;
  plan_batches(batches, attr_off, check_crcs, fetch_size, out.chunks, out.batch_chunks, lo, hi);
  for (size_t i = 0; i < recs.size(); ++i) {
    const JsonPlanRecord& r = recs[i];
    if (r.status != 0) continue;
    if (r.value_off < 0 || r.value_len < 0 || r.arr_off < 0 || r.arr_len < 0 ||
        r.arr_len > 0x7fffffffll ||  // (JsonRecord::len is an int32)
        (uint64_t)r.value_off + (uint64_t)r.value_len > fetch_size)
      throw std::invalid_argument("ingest plan: record outside the fetch");
    if ((uint64_t)r.arr_off + (uint64_t)r.arr_len > (uint64_t)r.value_len)
      throw std::invalid_argument("ingest plan: array outside its record");
    out.rec_of.push_back((int)i);
    const int nt = json_tile_count(r.value_off + r.arr_off, (int32_t)r.arr_len);
    out.ntiles += nt;
    out.ngroups += (nt + kGroupTiles - 1) / kGroupTiles;
    lo = std::min(lo, (size_t)r.value_off);
    hi = std::max(hi, (size_t)(r.value_off + r.value_len));
  }
  if (out.empty()) return;
  const size_t nc = out.nc(), nr = out.nr();
  // packed body: the whole body crosses the link packed and is expanded in its device mirror;
  // otherwise the span holding batches and records, raw
  out.packed = tap_result >= 0;
  if (out.packed) {
    lo = 0;
    hi = fetch_size;
  }
  lo &= ~(size_t)15;
  const size_t span = hi - lo;
  out.lo = lo;
  out.span = span;
  out.ng = out.packed ? codec::pack_groups(span) : 0;
  out.link = out.packed ? (size_t)tap_result : span;
  out.c_lo = out.packed ? codec::pack_offset(span) : lo;
  out.c_len = out.link;
  out.tab_off = out.packed ? codec::tab_offset(span) : 0;
  out.used = out.c_lo + out.c_len;
  if (out.used > dev_cap) throw std::invalid_argument("ingest plan: the copy ends past the mirror");
  // the count block: per record its tile counts, then its group sums
  const size_t ncnt = (size_t)out.ntiles + (size_t)out.ngroups;
  if (out.ntiles > 0) {
    const size_t cb = align256(ncnt * sizeof(int));
    if (dev_cap > cb + 256 && ((dev_cap - cb) & ~(size_t)255) >= align256(out.used + 64))
      out.cnt_base = (int64_t)((dev_cap - cb) & ~(size_t)255);
  }
  // parse at ingest: every counted record whose arena slots fit
  if (arena_bytes > 0 && out.cnt_base >= 0) {
    const int64_t S = 2 * per;
    for (size_t j = 0; j < nr; ++j) {
      const JsonPlanRecord& r = recs[(size_t)out.rec_of[j]];
      const int64_t off = r.value_off + r.arr_off;
      const int64_t slot = (off + S - 1) / S, cap = r.arr_len / S;
      if (cap <= 0 || (slot + cap) * per * (int64_t)sizeof(float) > (int64_t)arena_bytes) continue;
      out.pjs.push_back((int)j);
      out.ptiles += json_tile_count(off, (int32_t)r.arr_len);
    }
  }
  const size_t np = out.np(), ngroups = (size_t)out.ngroups, ptiles = (size_t)out.ptiles;
  out.o_chunks = align16(out.ng * 2 * sizeof(uint32_t));  // (the pack group table first)
  out.o_groups = out.o_chunks + align16(nc * sizeof(CrcChunk));
  out.o_recs = out.o_groups + align16(ngroups * sizeof(int2));
  out.o_precs = out.o_recs + nr * sizeof(JsonRecord);  // (JsonRecord is 48 bytes)
  out.o_ptr = out.o_precs + np * sizeof(JsonRecord);
  out.o_gsum = out.o_ptr + align16(ptiles * sizeof(int));
  out.o_crc = out.o_gsum + align16(ngroups * 4);
  out.o_gbad = out.o_crc + align16(nc * 4);
  out.o_pbad = out.o_gbad + align16(ngroups * 4);
  out.io_bytes = out.o_pbad + align16(ptiles * 4);
  out.plan_off = align256(std::max(fetch_size, out.used));
  const size_t plan_lim = out.cnt_base >= 0 ? (size_t)out.cnt_base : dev_cap;
  // (a packed body's group table still stands in the chunk, at tab_off, while the plan is
  // written: the caller copies it in front of the plan afterwards. A plan that would reach it -
  // a fetch of very many tiny records - takes the lane's buffer instead.)
  const bool on_tab = out.packed && out.plan_off < out.tab_off + out.ng * 2 * sizeof(uint32_t) &&
                      out.tab_off < out.plan_off + out.o_gsum;
  out.plan_in_chunk = !plan_separate && !on_tab && out.plan_off + out.o_gsum <= plan_lim;
}

void fill_json_ingest(const JsonIngestPlan& p, const std::vector<JsonPlanRecord>& recs,
                      uint8_t* dst) {
  const size_t nc = p.nc(), nr = p.nr(), np = p.np();
  if (nc) memcpy(dst + p.o_chunks, p.chunks.data(), nc * sizeof(CrcChunk));
  int2* hg = reinterpret_cast<int2*>(dst + p.o_groups);
  JsonRecord* hr = reinterpret_cast<JsonRecord*>(dst + p.o_recs);
  int tile = 0, grp = 0;
  for (size_t j = 0; j < nr; ++j) {
    const JsonPlanRecord& r = recs[(size_t)p.rec_of[j]];
    JsonRecord& jr = hr[j];
    jr.off = r.value_off + r.arr_off;
    jr.len = (int32_t)r.arr_len;
    jr.slot = 0;
    jr.images = 0;
    jr.status = 0;
    jr.tile0 = tile;
    jr.has_cnt = 0;
    jr.cnt_off = 0;
    jr.grp0 = grp;
    const int nt = json_tile_count(jr.off, jr.len);
    for (int t0 = 0; t0 < nt; t0 += kGroupTiles) {
      hg[grp].x = (int)j;
      hg[grp].y = t0;
      ++grp;
    }
    tile += nt;
  }
  JsonRecord* hp = reinterpret_cast<JsonRecord*>(dst + p.o_precs);
  int* hpt = reinterpret_cast<int*>(dst + p.o_ptr);
  const int64_t S = 2 * p.per;
  int pt = 0;
  for (size_t k = 0; k < np; ++k) {
    const JsonRecord& jr = hr[p.pjs[k]];
    JsonRecord& pr = hp[k];
    pr = jr;
    pr.slot = (int32_t)((jr.off + S - 1) / S);
    pr.images = -1;  // from the counts, on the device
    pr.status = 0;
    pr.tile0 = pt;
    pr.has_cnt = 1;
    pr.cnt_off = p.cnt_off(jr);
    pr.grp0 = 0;
    const int nt = json_tile_count(pr.off, pr.len);
    for (int t = 0; t < nt; ++t) hpt[pt + t] = (int)k;
    pt += nt;
  }
}

void plan_b64_ingest(const std::vector<std::pair<int64_t, int64_t>>& batches, int64_t attr_off,
                     bool check_crcs, const std::vector<B64PlanRecord>& recs,
                     const std::vector<uint32_t>& offs, int H, int W, int C, size_t arena_bytes,
                     size_t fetch_size, B64IngestPlan& out) {
  out = B64IngestPlan();
  const int64_t per = image_elements(H, W, C);
  const int64_t L = 4 * ((per + 2) / 3);
  out.chunks_per_image = (int)((L + kB64ChunkChars - 1) / kB64ChunkChars);
  size_t lo = fetch_size, hi = 0;
  plan_batches(batches, attr_off, check_crcs, fetch_size, out.chunks, out.batch_chunks, lo, hi);
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
  out.c_lo = lo & ~(size_t)15;
  out.c_len = hi - out.c_lo;
  out.plan_off = align256(fetch_size);
  const size_t nc = out.chunks.size(), ni = out.imgs.size();
  out.o_chunks = 0;
  out.o_imgs = out.o_chunks + align16(nc * sizeof(CrcChunk));
  out.plan_bytes = out.o_imgs + align16(ni * sizeof(B64Image));
  out.o_crc = 0;
  out.o_bad = out.o_crc + align16(nc * sizeof(uint32_t));
  out.result_bytes = out.o_bad + align16(ni * (size_t)out.chunks_per_image * sizeof(int32_t));
}

}  // namespace gale
