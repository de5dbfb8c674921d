// MetaLayout / plan_batch / fill_batch (see batch_plan.h).
#include "batch_plan.h"

#include <algorithm>
#include <stdexcept>

namespace gale {

namespace {

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

template <typename T>
T* at(uint8_t* base, size_t off) {
  return reinterpret_cast<T*>(base + off);
}

}  // namespace

MetaLayout::MetaLayout(int mb, int cap) : max_batch(mb), tiles_cap(cap) {
  hdr = 0;
  recs = kHeaderBytes;
  xs = recs + sizeof(JsonRecord) * (size_t)mb;
  tiles = xs + sizeof(float*) * (size_t)mb;
  b64_table = recs;
  b64_status = b64_table + sizeof(B64Image) * (size_t)mb;
  total = tiles + sizeof(int) * (size_t)cap;
}

MetaRange MetaLayout::used(const BatchPlan& p) const {
  const size_t map_end = tiles + sizeof(int) * (size_t)p.ntiles;
  switch (p.form) {
    case StepForm::OpByOp:  // (b64: the descriptor table and the status words behind it)
      return {recs, (p.b64 ? b64_status + sizeof(int) * (size_t)max_batch : map_end) - recs};
    case StepForm::Captured:
      return {hdr, total};
    case StepForm::Kernels:
      break;
  }
  // the header, the batch's records, the input pointer table, its tile map
  if (p.ntiles > 0) return {hdr, map_end};
  if (p.ptr_input) return {hdr, tiles};
  if (p.b64) return {hdr, b64_table + sizeof(B64Image) * (size_t)p.b64n};
  return {hdr, recs + sizeof(JsonRecord) * (size_t)p.nrec};
}

void plan_batch(const std::vector<BatchPlanRecord>& recs, int max_batch, int64_t per,
                StepForm form, bool ptr_input, bool b64, BatchPlan& out) {
  {
    BatchPlan fresh;  // (the vectors keep their capacity)
    fresh.spans.swap(out.spans);
    fresh.staged.swap(out.staged);
    fresh.parse_idx.swap(out.parse_idx);
    fresh.off.swap(out.off);
    fresh.spans.clear();
    fresh.staged.clear();
    out = std::move(fresh);
  }
  out.form = form;
  out.ptr_input = ptr_input;
  out.b64 = b64;
  out.per = per;
  out.parse_idx.assign(recs.size(), -1);
  out.off.assign(recs.size(), 0);
  // what crosses the link: one span per pinned fetch buffer over its records' extent (the few
  // bytes between them ride along), and the pageable records gathered in the staging buffer,
  // each at its source's position modulo 16 so the parser's aligned 16-byte loads see the same
  // layout as on the host
  size_t hoff = 0;
  for (size_t i = 0; i < recs.size(); ++i) {
    const BatchPlanRecord& r = recs[i];
    if (r.resident) continue;  // already in device memory: nothing to copy
    const size_t lo = (size_t)r.arr_off, len = (size_t)r.arr_len;
    if (!r.pinned) {
      const size_t host = hoff + (lo & 15);
      out.staged.push_back({(int)i, host, len});
      hoff = align16(host + len);
      continue;
    }
    BatchPlan::Span* sp = nullptr;
    for (BatchPlan::Span& x : out.spans)
      if (x.buf == r.buf) sp = &x;
    if (!sp) {
      out.spans.push_back({r.buf, lo, len, 0});
    } else {
      const size_t hi = std::max(sp->lo + sp->len, lo + len);
      sp->lo = std::min(sp->lo, lo);
      sp->len = hi - sp->lo;
    }
  }
  // device layout: [span 0][span 1]...[staged records]
  size_t doff = 0;
  for (BatchPlan::Span& x : out.spans) {
    x.len += x.lo & 15;
    x.lo &= ~(size_t)15;
    x.dev = doff;
    doff += align16(x.len);
  }
  out.staged_dev = doff;
  out.staged_bytes = hoff;
  out.dev_total = 16 + doff + hoff;
  size_t next_staged = 0;
  for (size_t i = 0; i < recs.size(); ++i) {
    const BatchPlanRecord& r = recs[i];
    if (out.img + r.images > max_batch)
      throw std::logic_error("GpuReplica: batch exceeds max_batch");
    out.resident += r.resident ? 1 : 0;
    out.img += r.images;
    if (r.preparsed) {  // the forward reads its images where the ingest parsed them
      ++out.npre;
      continue;
    }
    out.parse_idx[i] = out.nrec++;
    // where the record's instances array stands in the slot's device bytes: resident in a
    // mirror (placed by fill_batch; its phase is its address's), inside a pinned span, or
    // staged behind the spans
    int64_t phase = (int64_t)(r.dev_text & 15);
    if (!r.resident) {
      if (r.pinned) {
        size_t k = 0;
        while (out.spans[k].buf != r.buf) ++k;
        out.off[i] = (int64_t)(out.spans[k].dev + ((size_t)r.arr_off - out.spans[k].lo));
      } else {
        out.off[i] = (int64_t)(out.staged_dev + out.staged[next_staged++].host);
      }
      phase = out.off[i];
    }
    if (b64) {
      if (r.b64_n != r.images)
        throw std::logic_error("GpuReplica: b64 record does not match its scan");
      out.b64n += r.images;
      continue;
    }
    if (!(r.resident && r.dev_counts)) out.count_pass = true;
    out.ntiles += json_tile_count(phase, (int32_t)r.arr_len);
  }
}

void fill_batch(const BatchPlan& p, const std::vector<BatchPlanRecord>& recs,
                const std::vector<uint32_t>& offs, const MetaLayout& L, uint64_t d_bytes,
                uint64_t input_base, uint8_t* dst) {
  const size_t end = L.used(p).end();
  if (p.form != StepForm::OpByOp) {
    int32_t* hdr = at<int32_t>(dst, L.hdr);
    hdr[kHdrRecords] = p.nrec;
    hdr[kHdrTiles] = p.ntiles;
    hdr[kHdrImages] = p.img;
    hdr[kHdrB64] = p.b64n;
  }
  JsonRecord* jrecs = at<JsonRecord>(dst, L.recs);
  B64Image* tab = at<B64Image>(dst, L.b64_table);
  int32_t* b64_status = at<int32_t>(dst, L.b64_status);
  uint64_t* xs = at<uint64_t>(dst, L.xs);
  int32_t* tile_rec = at<int32_t>(dst, L.tiles);
  const uint64_t image_bytes = (uint64_t)p.per * sizeof(float);
  int img = 0, ntiles = 0, b64n = 0;
  for (size_t i = 0; i < recs.size(); ++i) {
    const BatchPlanRecord& r = recs[i];
    const int k = p.parse_idx[i];
    if (p.ptr_input)  // per image: the ingest's arena, or the slot's input the step parses into
      for (int j = 0; j < r.images; ++j)
        xs[img + j] = k < 0 ? r.dev_image + (uint64_t)j * image_bytes
                            : input_base + (uint64_t)(img + j) * image_bytes;
    if (k >= 0) {
      // offsets are relative to the slot's buffer; a mirror elsewhere in device memory is a
      // (signed) distance in the flat address space
      const int64_t off = r.resident ? (int64_t)(r.dev_text - d_bytes) : p.off[i];
      if (p.b64) {
        // one descriptor per image the step decodes: the table is dense over those, not over
        // the batch's images (preparsed records have none)
        for (int j = 0; j < r.images; ++j)
          tab[b64n + j] = B64Image{off + (int64_t)offs[(size_t)(r.b64_first + j)], img + j, k};
        b64n += r.images;
        // (the steps that raise verdicts elsewhere do not copy the status words)
        if (L.b64_status + sizeof(int32_t) * (size_t)(k + 1) <= end) b64_status[k] = 0;
      } else {
        JsonRecord& jr = jrecs[k];
        jr.off = off;
        jr.len = (int32_t)r.arr_len;
        jr.slot = img;
        jr.images = r.images;
        jr.status = 0;
        jr.tile0 = ntiles;
        // counted by the ingest pass: no counting pass over this record
        jr.has_cnt = r.resident && r.dev_counts ? 1 : 0;
        jr.cnt_off = jr.has_cnt ? (int64_t)(r.dev_counts - d_bytes) : 0;
        jr.grp0 = 0;
        const int nt = json_tile_count(jr.off, jr.len);
        for (int t = 0; t < nt; ++t) tile_rec[ntiles + t] = k;
        ntiles += nt;
      }
    }
    img += r.images;
  }
}

}  // namespace gale
