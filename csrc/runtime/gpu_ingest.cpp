// GpuIngest (see gpu_ingest.h / ingest.h).
#include "gpu_ingest.h"
#include "metrics.h"

#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <stdexcept>
#include <thread>

#include "../codec/json_codec.h"
#include "gale/executor.h"
#include "replica.h"

namespace gale {

GpuIngest::GpuIngest(int device, int lanes, int poll_us)
    : device_(device), poll_us_(poll_us), shift_chunk_(kCrcChunkBytes) {
  check_hip(hipSetDevice(device_), "ingest: hipSetDevice");
  std::vector<uint32_t> t(kafka::kCrcDeviceTableWords);
  kafka::crc32c_device_tables(t.data());
  check_hip(hipMalloc(reinterpret_cast<void**>(&d_tables_), t.size() * 4), "ingest: tables");
  check_hip(hipMemcpy(d_tables_, t.data(), t.size() * 4, hipMemcpyHostToDevice),
            "ingest: tables H2D");
  // (ingest lanes at the highest stream priority were measured and dropped: the replicas' batch
  // kernels then queue behind every fetch's ingest, ResNet-20 device time per batch 0.4 -> 2 ms,
  // profiles/archive/r4_ab_ingest_priority.jsonl)
  for (int i = 0; i < std::max(1, lanes); ++i) {
    auto L = std::make_unique<Lane>();
    check_hip(hipStreamCreateWithFlags(&L->stream, hipStreamNonBlocking), "ingest: stream");
    check_hip(hipEventCreateWithFlags(&L->done, hipEventDisableTiming), "ingest: event");
    lanes_.push_back(std::move(L));
  }
  if (const char* e = getenv("GALE_INGEST_DEV_TIMING")) dev_every_ = std::max(0, atoi(e));
  // (tests: the plan's own DMA, the path of a fetch whose plan does not fit behind it)
  if (const char* e = getenv("GALE_INGEST_PLAN_SEPARATE")) plan_separate_ = atoi(e) != 0;
  if (dev_every_ > 0)
    for (auto& L : lanes_)
      for (hipEvent_t& ev : L->tev) check_hip(hipEventCreate(&ev), "ingest: timing event");
}

GpuIngest::~GpuIngest() {
  hipSetDevice(device_);
  for (auto& L : lanes_) {
    if (L->stream) hipStreamSynchronize(L->stream);
    if (L->h_io) hipHostFree(L->h_io);
    if (L->d_io) hipFree(L->d_io);
    if (L->d_counts) hipFree(L->d_counts);
    if (L->done) hipEventDestroy(L->done);
    for (hipEvent_t ev : L->tev)
      if (ev) hipEventDestroy(ev);
    if (L->stream) hipStreamDestroy(L->stream);
  }
  if (d_tables_) hipFree(d_tables_);
}

// Before a run's first write into the lane's buffers: the device of the calling thread, and
// room for the plan + results and for the scratch counts.
void GpuIngest::grow(Lane& L, size_t io_bytes, size_t tiles) {
  check_hip(hipSetDevice(device_), "ingest: hipSetDevice");
  auto up = [](size_t want, size_t have) {
    return (std::max(want, have * 2) + 4095) & ~(size_t)4095;
  };
  if (io_bytes > L.io_cap) {
    if (L.h_io) hipHostFree(L.h_io);
    if (L.d_io) hipFree(L.d_io);
    L.io_cap = up(io_bytes, L.io_cap);
    check_hip(hipMalloc(reinterpret_cast<void**>(&L.d_io), L.io_cap), "ingest: d_io");
    // the plan (DMA'd to d_io) and the results (stored here by the kernel): host-mapped
    check_hip(hipHostMalloc(reinterpret_cast<void**>(&L.h_io), L.io_cap, hipHostMallocMapped),
              "ingest: h_io");
    void* dp = nullptr;
    check_hip(hipHostGetDevicePointer(&dp, L.h_io, 0), "ingest: h_io device pointer");
    if (dp != L.h_io) throw std::runtime_error("ingest: mapped plan buffer has another address");
  }
  if (tiles * sizeof(int) > L.counts_cap) {
    if (L.d_counts) hipFree(L.d_counts);
    L.counts_cap = up(tiles * sizeof(int), L.counts_cap);
    check_hip(hipMalloc(reinterpret_cast<void**>(&L.d_counts), L.counts_cap), "ingest: counts");
  }
}

void GpuIngest::wait(Lane& L) {
  if (poll_us_ <= 0) {
    check_hip(hipEventSynchronize(L.done), "ingest: hipEventSynchronize");
    return;
  }
  for (;;) {
    const hipError_t e = hipEventQuery(L.done);
    if (e == hipSuccess) return;
    if (e != hipErrorNotReady) check_hip(e, "ingest: hipEventQuery");
    std::this_thread::sleep_for(std::chrono::microseconds(poll_us_));
  }
}

void GpuIngest::mark(Lane& L, const Stamps& ts, int k) {
  if (ts.timed) check_hip(hipEventRecord(L.tev[k], L.stream), "ingest: timing event");
}

// The copies of a run: the text (with the plan behind it, in ONE DMA, when the plan rides in the
// fetch's chunk), else the text and then the plan from the lane's buffer. A run without plan
// sections copies the text alone.
void GpuIngest::begin(Lane& L, Stamps& ts, const kafka::Fetched& f, uint8_t* dev,
                      const Transfer& t) {
  hipStream_t st = L.stream;
  ts.plan = mono_ns();  // plan built; the HIP calls follow
  ts.timed = dev_every_ > 0 && L.nrun++ % dev_every_ == 0;
  mark(L, ts, 0);
  if (t.tab_bytes) memcpy(t.hpl, t.tab, t.tab_bytes);
  const bool has_plan = t.plan_bytes > 0;
  if (t.in_chunk && has_plan) {
    check_hip(hipMemcpyAsync(dev + t.lo, f.buf.get() + t.lo, t.plan_off + t.plan_bytes - t.lo,
                             hipMemcpyHostToDevice, st),
              "ingest: H2D text + plan");
  } else {
    check_hip(hipMemcpyAsync(dev + t.lo, f.buf.get() + t.lo, t.len, hipMemcpyHostToDevice, st),
              "ingest: H2D text");
    if (has_plan)
      check_hip(hipMemcpyAsync(L.d_io, L.h_io, t.plan_bytes, hipMemcpyHostToDevice, st),
                "ingest: H2D plan");
  }
  plan_in_chunk_ += t.in_chunk && has_plan;
  mark(L, ts, 1);
  text_bytes_ += (int64_t)t.text_bytes;
  link_bytes_ += (int64_t)t.link_bytes;
}

// Returns the time the device was done (the host's verdict work is timed from it).
int64_t GpuIngest::end(Lane& L, const Stamps& ts, bool parsed) {
  mark(L, ts, 3);
  check_hip(hipEventRecord(L.done, L.stream), "ingest: event");
  const int64_t t_wait = mono_ns();
  wait(L);
  const int64_t t_post = mono_ns();
  ++runs_;
  prep_ns_ += t_wait - ts.start;
  plan_ns_ += ts.plan - ts.start;
  wait_ns_ += t_post - t_wait;
  if (ts.timed) {
    float ms[3] = {0.f, 0.f, 0.f};  // copies, count (or b64) launch, parse launch
    for (int k = 0; k < (parsed ? 3 : 2); ++k)
      check_hip(hipEventElapsedTime(&ms[k], L.tev[k], L.tev[k + 1]), "ingest: event time");
    ++dev_runs_;
    dev_copy_ns_ += (int64_t)(ms[0] * 1e6);
    dev_count_ns_ += (int64_t)(ms[1] * 1e6);
    dev_parse_ns_ += (int64_t)(ms[2] * 1e6);
    dev_wait_ns_ += t_post - t_wait;
  }
  return t_post;
}

// Joins the window CRCs of each batch and compares with the batch header's (io.batch_ok).
void GpuIngest::join_batch_crcs(const kafka::Fetched& f,
                                const std::vector<std::pair<size_t, size_t>>& batch_chunks,
                                const uint32_t* crc, IngestIO& io) {
  for (size_t b = 0; b < batch_chunks.size(); ++b) {
    const kafka::BatchSpan& bs = f.batches[b];
    uint32_t raw = 0;
    for (size_t k = 0; k < batch_chunks[b].second; ++k) {
      const uint32_t c = crc[batch_chunks[b].first + k];
      raw = k == 0 ? c : shift_chunk_(raw) ^ c;
    }
    // standard CRC32C = raw ^ (initial ~0 carried over the message) ^ final ~0
    const uint64_t len = bs.len - (size_t)kafka::kBatchAttrOffset;
    const uint32_t got = raw ^ kafka::crc32c_shift(0xffffffffu, len) ^ 0xffffffffu;
    kafka::Reader cr(f.buf.get() + bs.off + kafka::kBatchCrcOffset, 4);
    io.batch_ok[b] = got == cr.u32();
  }
}

// The ingest of a fetch of base64 image records: ONE DMA (text + plan) and ONE launch
// (ingest_crc_b64). The host scan already knows every image count and string offset, so there
// is no counting pass, no count block in the mirror and no second launch.
void GpuIngest::run_b64(int lane, const kafka::Fetched& f, uint8_t* dev, size_t dev_cap,
                        bool check_crcs, int H, int W, int C, IngestIO& io, float* arena,
                        size_t arena_bytes) {
  Lane& L = *lanes_[(size_t)lane % lanes_.size()];
  std::lock_guard<std::mutex> lk(L.mu);
  Stamps ts;
  ts.start = mono_ns();
  const size_t nrec_all = f.records.size();
  io.cnt_off.assign(nrec_all, -1);
  io.batch_ok.assign(f.batches.size(), 1);
  io.img.assign(nrec_all, nullptr);
  // ---- plan
  std::vector<std::pair<int64_t, int64_t>> batches;
  for (const kafka::BatchSpan& b : f.batches) batches.emplace_back((int64_t)b.off, (int64_t)b.len);
  std::vector<B64PlanRecord> recs(nrec_all);
  for (size_t i = 0; i < nrec_all; ++i) {
    const kafka::RecordRef& rr = f.records[i];
    B64PlanRecord& r = recs[i];
    r.status = io.status[i];
    r.images = io.images[i];
    r.value_off = rr.value_off;
    r.value_len = rr.value_len;
    r.arr_off = io.arr_off[i];
  }
  B64IngestPlan plan;
  plan_b64_ingest(batches, kafka::kBatchAttrOffset, check_crcs, recs, io.b64_offs, H, W, C,
                  arena ? arena_bytes : 0, f.size, plan);
  const size_t nc = plan.chunks.size(), ni = plan.imgs.size();
  if (nc == 0 && plan.ok_records == 0) return;
  grow(L, plan.plan_bytes + plan.result_bytes + 16, 1);
  // ---- fill. The plan: behind the fetch's bytes in its own pinned chunk when it fits (the chunk
  // is pinned and mirrored at the same offsets), so ONE DMA carries text and plan; else the
  // lane's buffer and a second copy. There is no packed body in this mode, so the plan cannot
  // land on a pack table behind the body (the overlap the JSON plan's `used` guards against does
  // not exist here). The span holding batches and records crosses raw (base64 text does not
  // nibble-pack).
  Transfer t;
  t.lo = plan.c_lo;
  t.len = t.text_bytes = t.link_bytes = plan.c_len;
  t.plan_off = plan.plan_off;
  t.plan_bytes = plan.plan_bytes;
  t.in_chunk = !plan_separate_ && t.plan_off + plan.plan_bytes <= dev_cap;
  t.hpl = t.in_chunk ? f.buf.get() + t.plan_off : L.h_io;
  const uint8_t* dpl = t.in_chunk ? dev + t.plan_off : L.d_io;
  if (nc) memcpy(t.hpl + plan.o_chunks, plan.chunks.data(), nc * sizeof(CrcChunk));
  if (ni) memcpy(t.hpl + plan.o_imgs, plan.imgs.data(), ni * sizeof(B64Image));
  // the results behind the lane's plan area, host-mapped: the kernel stores them over the link
  uint8_t* res = L.h_io + plan.plan_bytes;
  int* wg_bad = reinterpret_cast<int*>(res + plan.o_bad);
  // ---- device
  begin(L, ts, f, dev, t);
  check_hip(ingest_crc_b64(dev, reinterpret_cast<const CrcChunk*>(dpl + plan.o_chunks), (int)nc,
                           d_tables_, reinterpret_cast<uint32_t*>(res + plan.o_crc), (int)ni,
                           reinterpret_cast<const B64Image*>(dpl + plan.o_imgs), H, W, C, arena,
                           wg_bad, L.stream, &input_prep_),
            "ingest: crc32c + b64 decode");
  mark(L, ts, 2);
  const int64_t t_post = end(L, ts, /*parsed=*/false);  // (no parse launch)
  // ---- host: batch CRCs; a record's verdict is the worst of its images' workgroup words
  join_batch_crcs(f, plan.batch_chunks, reinterpret_cast<const uint32_t*>(res + plan.o_crc), io);
  const int64_t per = (int64_t)H * W * C;
  const int cpi = plan.chunks_per_image;
  for (size_t i = 0; i < nrec_all; ++i) {
    if (plan.img0[i] < 0) continue;
    const int* w = wg_bad + (size_t)plan.img0[i] * cpi;
    int v = 0;
    for (int64_t g = 0; g < (int64_t)io.images[i] * cpi; ++g) v = std::max(v, w[g]);
    if (v == 2) io.status[i] = codec::BAD_NUMBER;
    else io.img[i] = arena + (int64_t)plan.slot0[i] * per;
  }
  post_ns_ += mono_ns() - t_post;
}

// The ingest of a fetch of JSON number records: one or two DMAs (text, plan) and two launches,
// ingest_crc_count and - for the records whose arena slots fit - json_parse_instances.
void GpuIngest::run(int lane, const kafka::Fetched& f, uint8_t* dev, size_t dev_cap,
                    bool check_crcs, int H, int W, int C, IngestIO& io, float* arena,
                    size_t arena_bytes) {
  Lane& L = *lanes_[(size_t)lane % lanes_.size()];
  std::lock_guard<std::mutex> lk(L.mu);
  Stamps ts;
  ts.start = mono_ns();
  const size_t nrec_all = f.records.size();
  io.images.assign(nrec_all, 0);
  io.cnt_off.assign(nrec_all, -1);
  io.batch_ok.assign(f.batches.size(), 1);
  io.img.assign(nrec_all, nullptr);
  // ---- plan: CRC windows, the records to count and to parse, the span that crosses the link,
  // the count block and every section offset (ingest_plan.h)
  L.batches.clear();
  for (const kafka::BatchSpan& b : f.batches)
    L.batches.emplace_back((int64_t)b.off, (int64_t)b.len);
  L.recs.resize(nrec_all);
  for (size_t i = 0; i < nrec_all; ++i) {
    const kafka::RecordRef& rr = f.records[i];
    JsonPlanRecord& r = L.recs[i];
    r.status = io.status[i];
    r.value_off = rr.value_off;
    r.value_len = rr.value_len;
    r.arr_off = io.arr_off[i];
    r.arr_len = io.arr_len[i];
  }
  const JsonIngestPlan& p = L.plan;
  plan_json_ingest(L.batches, kafka::kBatchAttrOffset, check_crcs, L.recs, H, W, C,
                   arena ? arena_bytes : 0, f.size, dev_cap, f.tap_result, plan_separate_, L.plan);
  if (p.empty()) return;
  const size_t nc = p.nc(), nr = p.nr(), np = p.np();
  grow(L, p.io_bytes + 16, (size_t)p.ntiles + (size_t)p.ngroups + 1);
  // ---- fill. The plan part [0, o_gsum): written into the fetch's own pinned chunk, behind the
  // bytes the copy moves anyway, when it fits before the counts (the chunk is pinned and
  // mirrored at the same offsets), so ONE DMA carries text and plan; else into the lane's
  // buffer, its own DMA.
  // (Sampled device timing, GALE_INGEST_DEV_TIMING: the copies were the largest device span of
  // a fetch, 40-60 us, mostly per-DMA latency - profiles/r6_ingest_device_split.jsonl)
  uint8_t* hpl = p.plan_in_chunk ? f.buf.get() + p.plan_off : L.h_io;  // host view of the plan
  uint8_t* dpl = p.plan_in_chunk ? dev + p.plan_off : L.d_io;          // device view
  fill_json_ingest(p, L.recs, hpl);
  const JsonRecord* hr = reinterpret_cast<const JsonRecord*>(hpl + p.o_recs);
  const JsonRecord* hp = reinterpret_cast<const JsonRecord*>(hpl + p.o_precs);
  // ---- device: text span -> mirror (packed: ONE H2D of the packed stream, expanded in place),
  // plan H2D, CRC windows, token counts [, parse]; the kernels store their results (window CRCs,
  // group sums and verdicts, parse tile verdicts) straight into the lane's host-mapped buffer,
  // so no D2H copy follows. Both copies are DMAs (SDMA engines, no CU time). Kernel READS of
  // host memory stay out of this path: under the serving load the link is busy with these DMAs
  // and every read waits behind them - expanding the packed text straight from the host-mapped
  // chunk made text_unpack 15x slower (device time per batch 0.34 -> 2.9 ms), and reading only
  // the plan and the step's metadata that way still stretched every kernel by 25-40 %
  // (profiles/r5_step_ab.txt).
  Transfer t;
  t.lo = p.c_lo;
  t.len = p.c_len;
  t.plan_off = p.plan_off;
  t.plan_bytes = p.o_gsum;
  t.in_chunk = p.plan_in_chunk;
  t.hpl = hpl;
  if (p.packed) {
    t.tab = f.buf.get() + p.tab_off;
    t.tab_bytes = p.ng * 2 * sizeof(uint32_t);
  }
  t.text_bytes = p.span;
  t.link_bytes = p.link;
  begin(L, ts, f, dev, t);
  uint32_t* d_crc = reinterpret_cast<uint32_t*>(L.h_io + p.o_crc);   // (host-mapped results)
  int* d_gsum = reinterpret_cast<int*>(L.h_io + p.o_gsum);
  int* d_gbad = reinterpret_cast<int*>(L.h_io + p.o_gbad);
  int* d_pbad = reinterpret_cast<int*>(L.h_io + p.o_pbad);
  int* d_cnt = p.cnt_base >= 0 ? reinterpret_cast<int*>(dev + p.cnt_base) : L.d_counts;
  // CRC windows and token counts: one launch, one pass of workgroups over the buffer. Packed,
  // the same launch expands the text: CRC and counting waves read the packed stream, and the
  // counting waves store each record's text into the mirror for the parse (r4 ran a separate
  // text_unpack pass over the whole body first: a third of the ingest launches, 16 % of the
  // GPU's busy time under the serving load, profiles/r5_step_ab.txt)
  check_hip(ingest_crc_count(dev, reinterpret_cast<const CrcChunk*>(dpl + p.o_chunks), (int)nc,
                             d_tables_, d_crc, (int)nr, p.ngroups,
                             reinterpret_cast<JsonRecord*>(dpl + p.o_recs),
                             reinterpret_cast<const int2*>(dpl + p.o_groups), d_cnt, d_gsum,
                             d_gbad, L.stream, p.packed ? dev + p.c_lo : nullptr,
                             p.packed ? reinterpret_cast<const uint32_t*>(dpl) : nullptr,
                             p.packed ? dev : nullptr),
            "ingest: crc32c + count");
  mark(L, ts, 2);
  // the parse right behind it, same stream (the counts are in place when it starts): the text
  // -> fp32 images in the fetch's arena, so the batch step later runs only the forward
  if (np > 0)
    check_hip(json_parse_instances((int)np, p.ptiles,
                                   reinterpret_cast<JsonRecord*>(dpl + p.o_precs),
                                   reinterpret_cast<const int*>(dpl + p.o_ptr), dev, H, W, C,
                                   L.d_counts, arena, L.stream, /*count_pass=*/false, nullptr,
                                   nullptr, d_pbad, &input_prep_),
              "ingest: parse");
  const int64_t t_post = end(L, ts, /*parsed=*/true);
  // ---- host: join the windows of each batch and compare; images from the element counts
  join_batch_crcs(f, p.batch_chunks, d_crc, io);
  // a record's tokens: the sums of its tile groups (and its verdict: the worst group's)
  size_t k = 0;  // the next parse record (pjs ascends)
  for (size_t j = 0; j < nr; ++j) {
    const size_t i = (size_t)p.rec_of[j];
    const bool parsed = k < np && (size_t)p.pjs[k] == j;
    const JsonRecord* pr = parsed ? &hp[k++] : nullptr;
    const int64_t g1 = j + 1 < nr ? hr[j + 1].grp0 : p.ngroups;
    int64_t tok = 0;
    int bad = 0;
    for (int64_t g = hr[j].grp0; g < g1; ++g) {
      tok += d_gsum[g];
      bad |= d_gbad[g];
    }
    if (bad != 0) {
      io.status[i] = codec::BAD_NUMBER;
    } else if (tok == 0) {
      io.status[i] = codec::EMPTY;
    } else if (tok % p.per != 0) {
      io.status[i] = codec::BAD_SHAPE;
    } else {
      io.images[i] = (int32_t)(tok / p.per);
      if (p.cnt_base >= 0) io.cnt_off[i] = p.cnt_off(hr[j]);
      if (pr) {
        // the parse's verdict (structure, element count, numbers): the worst of its tiles
        const int nt = json_tile_count(pr->off, pr->len);
        int v = 0;
        for (int t0 = 0; t0 < nt; ++t0) v = std::max(v, d_pbad[pr->tile0 + t0]);
        const int32_t verdict = device_verdict_status(v);
        if (verdict != codec::OK) io.status[i] = verdict;
        else io.img[i] = arena + (int64_t)pr->slot * p.per;
      }
    }
  }
  post_ns_ += mono_ns() - t_post;
}

}  // namespace gale
