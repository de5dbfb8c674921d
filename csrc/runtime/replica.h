// Inference replicas driven by the serving engine.
//
// A replica is the InferenceBolt's model + session (InferenceBolt.java:43-62) and its per-tuple
// execute (:70-99), generalised to micro-batches: the engine hands it a Batch of Kafka records
// (already envelope-validated by codec::scan_instances), the replica turns their JSON text into
// softmax rows. Replicas are asynchronous with a fixed depth so that host staging of batch k+1
// overlaps device work on batch k:
//   submit(b)  — enqueue (returns immediately for the GPU replica)
//   wait(b)    — block until b's outputs and per-record statuses are on the host
// Both replicas take the engine's input resize as one InputResize (resize_plan.h), in either form.
#pragma once
#include <stdint.h>

#include <atomic>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "../codec/json_codec.h"
#include "../codec/pixel_source.h"
#include "batch_plan.h"
#include "gale/executor.h"
#include "gale/kernels.h"
#include "resize_plan.h"

namespace gale {

// The device parsers' verdict word (json_parse_instances' record status or the worst of a
// record's tile verdicts: 0 ok, 1 number-count mismatch, 2 malformed number, 3 bad structure) as
// the codec::Status the engine reports - one mapping for the replica's parse and the ingest's.
inline int32_t device_verdict_status(int v) {
  return v == 1 || v == 3 ? codec::BAD_SHAPE : v == 2 ? codec::BAD_NUMBER : codec::OK;
}

struct InRecord;
// A record with more images than one micro-batch holds (InstObj N > max_batch): it is served as
// consecutive fragments of <= max_batch images, each a record of its own in the batcher, and the
// prediction rows are joined back into ONE {"predictions": [...]} record for the input offset.
struct SplitRecord;

struct InRecord {
  std::shared_ptr<uint8_t> buf;  // keeps the fetch buffer alive
  const uint8_t* value = nullptr;
  int32_t len = -1;              // -1 = null value
  const uint8_t* key = nullptr;  // record key (inside buf), key_len -1 = null
  int32_t key_len = -1;
  int32_t partition = -1;
  int64_t offset = -1;
  int64_t timestamp_ms = -1;     // Kafka record CreateTime
  int64_t t_fetch_ns = 0;        // host receive time
  int64_t t_take_ns = 0, t_done_ns = 0;  // its batch's dispatch / device-done time (sink metas)
  int64_t t_ready_ns = 0;                // decoded / ingested: handed to the batcher
  int64_t arr_off = 0, arr_len = 0;  // instances array inside the value (scan result)
  int32_t images = 0;
  int32_t status = 0;            // codec::Status (scan, then device parse)
  int32_t source = 0;
  bool pinned = false;           // buf is page-locked: the GPU replica DMAs straight from it
  // GPU ingest (ingest.h): the value's bytes are already in device memory, in the mirror of
  // the fetch pool of locality slot dev_locality (its key: the device, or the split slot)
  const uint8_t* dev_value = nullptr;
  int32_t dev_locality = -1;
  // its per-tile token counts, left on the device by the ingest pass (null: none)
  const uint8_t* dev_counts = nullptr;
  // its images, already parsed by the ingest pass: fp32 [H][W][C] each, contiguous, in the
  // fetch's device image arena (null: the replica parses the text)
  const float* dev_image = nullptr;
  const float* dev_arena = nullptr;  // the arena dev_image lies in (its fetch's)
  // fragment `split_index` of an oversized record (null for ordinary records)
  std::shared_ptr<SplitRecord> split;
  int32_t split_index = -1;
};

struct Batch {
  std::vector<InRecord> recs;
  int images = 0;
  int slot = 0;
  const float* probs = nullptr;  // [images, classes] after wait()
  // [images, classes] Java Float.toString slots (kFloatTextSlot bytes each) when the replica
  // formats on the device (GpuReplica gpu_encode), else null: the engine formats `probs`
  const uint8_t* pred_text = nullptr;
  // top-k output selected on the device (GpuReplica gpu_encode with top_k): pred_text then holds
  // [images, k] score slots and pred_idx the [images, k] class indices; else null
  const int32_t* pred_idx = nullptr;
  std::vector<int32_t> dev_status;  // per-record codec::Status found by the replica's parser
  int64_t t_take_ns = 0, t_submit_ns = 0, t_done_ns = 0;
  bool step_graph = false;  // (GpuReplica) submitted as one replay of the slot's step graph
};

class Replica {
 public:
  virtual ~Replica() = default;
  virtual std::string name() const = 0;
  virtual int max_images() const = 0;
  virtual int depth() const = 0;  // batches that may be in flight
  virtual void submit(Batch& b) = 0;
  virtual void wait(Batch& b) = 0;
  virtual int device() const { return -1; }
  // locality slot key: replicas with the same key share a batcher and fetch-buffer pool (the
  // device for GPU replicas; stub replicas take a tag so the scheme is testable on CPU)
  virtual int locality() const { return device(); }
  // Supervisor restart after submit/wait threw (its in-flight batches were already re-queued):
  // bring the replica back to an idle, usable state or throw if it cannot be.
  virtual void recover() {}
  // records whose text this replica parsed from device memory already holding it (GPU ingest
  // mirror of its own locality slot) vs. copied over the host link (pinned or staged)
  virtual int64_t resident_records() const { return 0; }
  virtual int64_t host_records() const { return 0; }
  // batches run as ONE captured step graph (parse + forward + format + status) / with a
  // graph-captured forward only (the rest launched directly)
  virtual int64_t graph_step_batches() const { return 0; }
  virtual int64_t graph_forward_batches() const { return 0; }
  // records whose images the GPU ingest had parsed (the step ran only the forward for them)
  virtual int64_t preparsed_records() const { return 0; }
  // batches whose step was the forward alone with its inputs in the kernel arguments
  virtual int64_t table_batches() const { return 0; }
  // images that went through the input resize (the resize_crop kernel or its host twin)
  virtual int64_t resized_images() const { return 0; }
};

// CPU stub (SURVEY.md §4 "stub replica for plumbing tests on GPU-less hosts"): parses on the
// host and computes a fixed deterministic classifier, logits[k] = (k+1) * mean(x[..., k % C]),
// followed by softmax. An optional per-batch delay emulates device time.
class StubReplica : public Replica {
 public:
  StubReplica(int H, int W, int C, int classes, int max_images, int delay_us, bool compute = true,
              int locality = -1);
  std::string name() const override { return "stub"; }
  int locality() const override { return locality_; }
  int max_images() const override { return max_images_; }
  int depth() const override { return 1; }
  void submit(Batch& b) override;
  void wait(Batch& b) override;
  // input preprocessing (InputPrep, gale/kernels.h) on the host-parsed images; before submit()
  void set_input_prep(const InputPrep& p) { prep_ = p; }
  // base64 image records (EngineConfig::input_b64) whose strings carry `src`
  // (EngineConfig::pixels): decoded, and converted to RGB, by the source's host parser
  // (PixelSource::parse_host); before submit()
  void set_input_b64(bool on, const PixelSource& src = PixelSource()) {
    b64_ = on, pixels_ = src;
  }
  // input resize (resize_plan.h, either form): the records carry r.HS() x r.WS() images, parsed
  // and preprocessed at that size into a source buffer and resized into the model-size images by
  // the form's host twin (InputResize::apply_host); the logits stay the function of the
  // model-size image. Before submit(); r.H() / r.W() must be the replica's
  void set_input_resize(const InputResize& r);
  int64_t resized_images() const override { return resized_; }

 private:
  InputPrep prep_;
  bool b64_ = false;
  PixelSource pixels_;
  std::optional<InputResize> resize_;
  std::vector<float> src_;  // resize_: the batch's images at the source size
  std::atomic<int64_t> resized_{0};
  int H_, W_, C_, classes_, max_images_, delay_us_;
  bool compute_;
  int locality_ = -1;  // false: a "null" replica (uniform softmax, no parsing) to measure host paths
  std::vector<float> x_, probs_;
};

// One model replica on one GPU: staged JSON bytes -> GPU JSON parser -> hipGraph forward ->
// softmax rows, all on the replica's own stream. `slots` I/O buffer sets pipeline host staging
// with device work (the executor's per-slot graphs, csrc/runtime/executor.cpp).
class GpuReplica : public Replica {
 public:
  // wait_poll_us > 0: wait() first sleeps until ~85 % of the batch's expected submit -> done
  // time (a running average of the replica's recent batches), then polls the completion event
  // every wait_poll_us (the worker thread costs ~no CPU while the GPU works, and polls only
  // around the expected completion); 0: hipEventSynchronize (the HIP runtime busy-waits, lowest
  // wake-up latency, one core per waiting replica); < 0: blocking-sync completion events (the
  // thread sleeps on the device interrupt)
  // gpu_encode: the softmax rows are also formatted as prediction text on the device
  // locality: the replica's locality slot key (-1 = its device). Records ingested by another
  // slot - a steal - are not resident for this replica even on the same device: their text is
  // DMA'd from the host-pinned fetch buffer, as it would be across GPUs (--locality-split
  // exercises the multi-GPU dispatch on one device)
  // step_graph: with use_graph and a whole-network plan (Executor::device_batch_ok), each batch
  // is ONE hipGraphLaunch of the slot's captured step (the sequence and its forms: emit_step in
  // gpu_replica.cpp), so one graph per slot serves every batch size
  // high_priority: the replica's stream at the device's highest stream priority, so its step
  // kernels are dispatched ahead of the GPU ingest's when both wait for CUs
  // top_k > 0 (EngineConfig::top_k) with gpu_encode: the step ends with the selection kernel
  // (topk.hip) where it formatted the whole rows: k score slots and k class indices per image
  // come back instead of `classes` slots (whole-network plans keep the verdict hand-off in the
  // forward's epilogue and leave its text out). Without gpu_encode the probabilities come back
  // as ever and the engine selects
  GpuReplica(std::shared_ptr<Executor> exec, int H, int W, int C, int classes, bool use_graph,
             int wait_poll_us = 0, bool gpu_encode = false, int locality = -1,
             bool step_graph = true, bool high_priority = false, bool step_direct = false,
             int top_k = 0);
  ~GpuReplica() override;
  std::string name() const override;
  int max_images() const override { return exec_->max_batch(); }
  int depth() const override { return exec_->slots(); }
  int device() const override { return exec_->device(); }
  int locality() const override { return locality_ >= 0 ? locality_ : exec_->device(); }
  void submit(Batch& b) override;
  void wait(Batch& b) override;
  void recover() override;
  int64_t resident_records() const override { return resident_; }
  int64_t host_records() const override { return host_; }
  int64_t graph_step_batches() const override { return step_batches_; }
  int64_t graph_forward_batches() const override { return fwd_graph_batches_; }
  int64_t preparsed_records() const override { return preparsed_; }
  int64_t table_batches() const override { return table_batches_; }
  bool step_graph() const { return step_graph_; }
  // input preprocessing of every parse this replica launches (InputPrep, gale/kernels.h): by
  // value in the parse's kernel arguments, so it is part of a captured step; before submit()
  void set_input_prep(const InputPrep& p) { prep_ = p; }
  // base64 uint8 image records (EngineConfig::input_b64): the step runs b64_decode_instances
  // where it runs json_parse_instances otherwise. The batch's image descriptor table and (for
  // the steps that copy verdicts back) its status words take the place of the JsonRecord table
  // in the slot's metadata allocation: [B64Image x max_batch][int status x max_batch]. No tile
  // map, no count pass. The strings carry `src` (EngineConfig::pixels): the one decode launch is
  // the source's (b64_source_instances: b64_yuv_instances, b64_packed_instances or
  // b64_typed_instances for YUV frames, packed pixels or typed tensors) - same descriptor table,
  // status words and output tensor, strings of src.bytes(recH_, recW_, C_) bytes; for the first
  // two C must be 3 and the prep not nchw (the launchers refuse otherwise). Before submit()
  void set_input_b64(bool on, const PixelSource& src = PixelSource()) {
    b64_ = on, pixels_ = src;
  }
  // input resize (resize_plan.h, either form): the records carry r.HS() x r.WS() images. The
  // tables' device image (pack) is uploaded once and every slot gets a source tensor of
  // max_batch * HS * WS * C floats that never moves (captured steps stay valid); the step's
  // parse / b64 decode writes it at the source size and resize_crop, or resize_crop_aa for the
  // antialiased form, follows into the executor's input (emit_step). Before submit(), once;
  // r.H() / r.W() must be the replica's
  void set_input_resize(const InputResize& r);
  int64_t resized_images() const override { return resized_; }

 private:
  struct Slot {
    float* d_src = nullptr;      // input resize: the batch's images at the source size
    uint8_t* h_bytes = nullptr;  // pinned staging for records that arrived in pageable memory
    uint8_t* d_bytes = nullptr;  // device copy of the batch's JSON text
    size_t h_cap = 0, d_cap = 0;
    // parser metadata: header, records, input pointer table (per batch image its fp32 input on
    // the device, ptr_input_), tile map, laid out by `meta` (batch_plan.h). Pinned and
    // host-mapped, and its device mirror
    uint8_t* h_meta = nullptr;
    uint8_t* d_meta = nullptr;
    MetaLayout meta;
    hipGraphExec_t step[2] = {nullptr, nullptr};  // captured steps (without / with count pass)
    int* d_tiles = nullptr;      // per-tile token counts (parser scratch)
    float* h_out = nullptr;      // pinned softmax rows
    uint8_t* h_text = nullptr;   // pinned, device-mapped prediction text slots (gpu_encode)
    int32_t* h_idx = nullptr;    // top_k: the class indices, behind the k slots per image in h_text
    // the kernels-only step (gpu_encode) raises verdicts in d_status; its last kernel hands
    // them to h_status (host-mapped)
    int* d_status = nullptr;
    int* h_status = nullptr;
    // the batch in flight: its records as the plan sees them, their b64 string offsets, and
    // the plan (its form says where wait() finds the verdicts)
    std::vector<BatchPlanRecord> recs;
    std::vector<uint32_t> b64_offs, b64_scan;  // (b64_scan: one record's, scratch)
    BatchPlan plan;
    hipEvent_t done = nullptr;
    int64_t t_submit_ns = 0;
  };
  struct StepDesc;   // how the step's sequence is emitted (gpu_replica.cpp)
  struct StepError;  // what failed in it
  void ensure_host(Slot& s, size_t bytes);
  void ensure_device(Slot& s, size_t bytes);
  void ensure_tiles(Slot& s, int ntiles);
  void drop_steps(Slot& s);  // (buffers moved: the captured steps point at the old ones)
  // the record's text is in this replica's device memory (GPU ingest, its own locality slot) /
  // so are its images, already parsed there (the ingest's arena)
  bool resident(const InRecord& r) const {
    return r.dev_value != nullptr && r.dev_locality == my_loc_;
  }
  bool preparsed(const InRecord& r) const { return ptr_input_ && resident(r) && r.dev_image; }
  void describe(const Batch& b, Slot& s);
  bool table_step(Batch& b, Slot& s, int slot);
  void stage_text(const Batch& b, Slot& s);
  void launch_step(Batch& b, Slot& s, int slot);
  hipGraphExec_t step_for(Slot& s, int slot, bool count_pass);
  StepDesc step_desc() const;
  StepError emit_step(Slot& s, int slot, hipStream_t st, const StepDesc& d, bool count_pass,
                      bool parse);
  static StepError launch_resize(const BoundResize& r, int images, const int* d_images,
                                 const float* src, float* dst, hipStream_t st);
  static void* mapped_alloc(size_t bytes, const char* what);
  std::shared_ptr<Executor> exec_;
  InputPrep prep_;
  bool b64_ = false;
  PixelSource pixels_;  // what the b64 strings carry
  // input resize: the tables' device image (one allocation; null = off, the records carry
  // model-size images, recH_ / recW_ == H_ / W_) and the kernel plan bound to it
  uint8_t* d_resize_ = nullptr;
  BoundResize resize_;
  std::atomic<int64_t> resized_{0};
  int H_, W_, C_, classes_;
  int recH_, recW_;  // the size the records' images arrive in (parsers, b64 string length)
  bool use_graph_;
  int wait_poll_us_ = 0;
  bool gpu_encode_ = false;
  int top_k_ = 0;  // > 0 with gpu_encode_: the device selects (else 0, whatever the engine's is)
  // H2D of the batch's metadata (and of any text not already resident) + parse + forward + D2H,
  // in order on ONE stream: with GPU ingest the text is resident, so a separate copy stream
  // bought no overlap, and its cross-stream wait (hipStreamWaitEvent) was where rocprofv3's
  // kernel tracing crashed under the default 6-replica concurrency; overlap comes from the
  // replicas' streams running side by side
  hipStream_t stream_ = nullptr;
  std::vector<Slot> slots_;
  int next_slot_ = 0;
  int locality_ = -1;
  int my_loc_ = -1;  // locality(), fixed at construction
  std::atomic<int64_t> resident_{0}, host_{0};
  std::atomic<int64_t> step_batches_{0}, fwd_graph_batches_{0};
  bool step_graph_ = false;
  bool step_direct_ = false;  // the kernels-only step launched directly, not as a graph replay
  StepForm form_ = StepForm::OpByOp;  // the form every batch is submitted in (batch_plan.h)
  // batches whose records the GPU ingest already parsed (InRecord::dev_image) run the forward
  // only, reading each image through the slot's input pointer table (direct-launch step of a
  // whole-network plan with the epilogue outputs); records without parse as before
  bool ptr_input_ = false;
  std::atomic<int64_t> preparsed_{0};
  std::atomic<int64_t> table_batches_{0};  // batches launched with a kernel-argument input table
  int64_t expect_ns_ = 0;  // running average of submit -> done (adaptive sleep-poll)
};

}  // namespace gale
