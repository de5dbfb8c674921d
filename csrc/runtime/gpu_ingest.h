// GpuIngest: the HIP implementation of Ingest (see ingest.h). Kept out of engine.cpp so the
// sanitizer build of the host pipeline links no GPU kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "gale/kernels.h"
#include "ingest.h"
#include "ingest_plan.h"

namespace gale {

class GpuIngest : public Ingest {
 public:
  // lanes: decode threads that may call run() concurrently; poll_us: sleep between completion
  // polls (0 = hipEventSynchronize)
  GpuIngest(int device, int lanes, int poll_us);
  ~GpuIngest() override;
  int device() const override { return device_; }
  void run(int lane, const kafka::Fetched& f, uint8_t* dev, size_t dev_cap, bool check_crcs,
           int H, int W, int C, IngestIO& io, float* arena = nullptr,
           size_t arena_bytes = 0) override;
  void run_b64(int lane, const kafka::Fetched& f, uint8_t* dev, size_t dev_cap, bool check_crcs,
               int H, int W, int C, IngestIO& io, float* arena = nullptr,
               size_t arena_bytes = 0) override;
  void link_bytes(int64_t& text, int64_t& link) const override {
    text = text_bytes_.load();
    link = link_bytes_.load();
  }
  // input preprocessing of the ingest parse (InputPrep, gale/kernels.h); before the first run()
  void set_input_prep(const InputPrep& p) { input_prep_ = p; }
  Timing timing() const override {
    Timing t;
    t.runs = runs_.load();
    t.prep_ns = prep_ns_.load();
    t.plan_ns = plan_ns_.load();
    t.wait_ns = wait_ns_.load();
    t.post_ns = post_ns_.load();
    t.dev_runs = dev_runs_.load();
    t.dev_copy_ns = dev_copy_ns_.load();
    t.dev_count_ns = dev_count_ns_.load();
    t.dev_parse_ns = dev_parse_ns_.load();
    t.dev_wait_ns = dev_wait_ns_.load();
    t.plan_in_chunk = plan_in_chunk_.load();
    return t;
  }

 private:
  struct Lane {
    std::mutex mu;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    // one host-mapped pinned buffer and a device image of its plan part, laid out by the
    // fetch's plan (ingest_plan.h):
    //   run (JsonIngestPlan): the plan sections [0, o_gsum) - pack tab, o_chunks, o_groups,
    //   o_recs, o_precs, o_ptr - then the result sections o_gsum, o_crc, o_gbad, o_pbad
    //   run_b64 (B64IngestPlan): the plan sections [0, plan_bytes) - o_chunks, o_imgs - then,
    //   from plan_bytes on, the result sections o_crc, o_bad
    // The host writes the plan sections - here, or behind the fetch in its own pinned chunk, when
    // they fit there - ONE H2D copies them into d_io (or carries them with the text), and the
    // kernels store the result sections straight into the host buffer: no D2H copy
    uint8_t* h_io = nullptr;
    uint8_t* d_io = nullptr;
    size_t io_cap = 0;
    int* d_counts = nullptr;  // per-tile token counts (scratch)
    size_t counts_cap = 0;
    hipEvent_t tev[4] = {nullptr, nullptr, nullptr, nullptr};  // sampled device timing
    int64_t nrun = 0;
    // run()'s plan and its inputs, kept for their capacity: a fetch allocates nothing
    std::vector<std::pair<int64_t, int64_t>> batches;
    std::vector<JsonPlanRecord> recs;
    JsonIngestPlan plan;
  };
  // What begin() moves to the device: the fetch's bytes [lo, lo + len) into its mirror and the
  // plan sections, `plan_bytes` at hpl - in the fetch's chunk at plan_off (in_chunk: one DMA
  // carries both) or in the lane's buffer (its own DMA into d_io).
  struct Transfer {
    size_t lo = 0, len = 0;
    size_t plan_off = 0, plan_bytes = 0;
    bool in_chunk = false;
    uint8_t* hpl = nullptr;
    // packed body: its pack group table, copied in front of the plan sections
    const uint8_t* tab = nullptr;
    size_t tab_bytes = 0;
    size_t text_bytes = 0, link_bytes = 0;  // for the link counters
  };
  struct Stamps {  // of one lane transaction (mono_ns)
    int64_t start = 0, plan = 0;
    bool timed = false;  // this run is in the device timing sample
  };
  void grow(Lane& L, size_t io_bytes, size_t tiles);
  void wait(Lane& L);
  // One lane transaction around a run's launches (the caller holds the lane and has grown it):
  // begin() issues the copies, mark() records timing event k between launches, end() records the
  // rest, waits for the device and does the accounting; a run with one launch (parsed false)
  // leaves the parse span out.
  void begin(Lane& L, Stamps& ts, const kafka::Fetched& f, uint8_t* dev, const Transfer& t);
  void mark(Lane& L, const Stamps& ts, int k);
  int64_t end(Lane& L, const Stamps& ts, bool parsed);
  void join_batch_crcs(const kafka::Fetched& f,
                       const std::vector<std::pair<size_t, size_t>>& batch_chunks,
                       const uint32_t* crc, IngestIO& io);
  int device_, poll_us_;
  InputPrep input_prep_;
  std::atomic<int64_t> text_bytes_{0}, link_bytes_{0};
  std::atomic<int64_t> runs_{0}, prep_ns_{0}, plan_ns_{0}, wait_ns_{0}, post_ns_{0};
  std::atomic<int64_t> dev_runs_{0}, dev_copy_ns_{0}, dev_count_ns_{0}, dev_parse_ns_{0},
      dev_wait_ns_{0};
  int dev_every_ = 0;  // GALE_INGEST_DEV_TIMING
  bool plan_separate_ = false;  // GALE_INGEST_PLAN_SEPARATE
  std::atomic<int64_t> plan_in_chunk_{0};
  uint32_t* d_tables_ = nullptr;
  std::vector<std::unique_ptr<Lane>> lanes_;
  kafka::CrcShift shift_chunk_;
};

}  // namespace gale
