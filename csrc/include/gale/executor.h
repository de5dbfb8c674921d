// Model plan executor: runs a flat list of gale kernels on one device/stream and replays each
// (batch bucket, I/O slot) pair from a captured hipGraph.
//
// Replaces the reference's per-tuple `sess.runner().feed("input:0").fetch("output/Softmax:0")
// .run()` (InferenceBolt.java:81-85): the model is a static plan built once (R6 prepare,
// InferenceBolt.java:43-62) and every micro-batch is one graph launch.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "gale/forward_plan.h"
#include "gale/kernels.h"

namespace gale {

class Executor {
 public:
  // validate_plan(spec) and the stem_pool geometry check come first: a refused plan throws
  // std::invalid_argument before any HIP call
  Executor(int device, PlanSpec spec);
  ~Executor();
  Executor(const Executor&) = delete;
  Executor& operator=(const Executor&) = delete;

  int device() const { return device_; }
  int max_batch() const { return spec_.max_batch; }
  int slots() const { return spec_.slots; }
  const std::vector<int>& buckets() const { return buckets_; }
  int bucket_for(int batch) const;

  // Device I/O buffers of a slot (input fp32 [max_batch, ...], output fp32 [max_batch, classes]).
  void* input(int slot) const { return bufs_[slot][0]; }
  void* output(int slot) const { return bufs_[slot][1]; }
  long long input_bytes_per_image() const { return spec_.buf_bytes_per_image[0]; }
  long long output_bytes_per_image() const { return spec_.buf_bytes_per_image[1]; }

  // Enqueue the forward for `batch` images of `slot` on `stream`. use_graph replays (capturing on
  // first use) the graph of the smallest bucket >= batch; otherwise launches kernels eagerly.
  // Plans of at most kMaxDirectOps kernels (the whole-network ResNet-20 kernel) always launch
  // directly: a graph saves nothing there, runs the padded bucket batch, and every replay costs
  // CPU on the HIP runtime's worker thread (~0.9 core at the serving rate, -> 0.16 with direct
  // launches, measured in round 3).
  static constexpr size_t kMaxDirectOps = 2;
  bool graph_pays() const { return spec_.ops.size() > kMaxDirectOps; }
  void run(int slot, int batch, hipStream_t stream, bool use_graph);
  // Eager forward on caller-provided device buffers (tests / ops API; no graph).
  void run_on(int batch, const void* in, void* out, hipStream_t stream);
  void capture_all(hipStream_t stream);  // pre-capture every (bucket, slot) graph
  int graphs_captured() const;
  // Plans whose every op reads its image count from device memory (the whole-network kernels):
  // launch_device_batch enqueues the forward of `slot` sized for max_batch images, the count
  // taken from *d_batch when the kernels run - what a captured per-slot step graph replays
  // for every batch size (GpuReplica step graphs).
  // so (optional): the step outputs the forward kernel writes in its own epilogue (prediction
  // text, parse verdicts; gale/kernels.h StepOut) - only when step_out_ok()
  bool device_batch_ok() const;
  bool step_out_ok() const { return device_batch_ok() && spec_.ops.size() == 1; }
  // xs (optional, device memory): image i's fp32 input at xs[i] instead of the slot's input
  // buffer - images the GPU ingest already parsed (whole-network plans: device_batch_ok())
  void launch_device_batch(int slot, const int* d_batch, hipStream_t stream,
                           const StepOut* so = nullptr, const float* const* xs = nullptr);
  // The forward of `batch` images taken from an input table in the kernel arguments (images the
  // GPU ingest parsed): no metadata in device memory, one launch (step_out_ok() plans)
  void launch_table(int slot, int batch, const InputTable& tab, hipStream_t stream,
                    const StepOut* so = nullptr);

 private:
  void launch_all(int batch, void* const* bufs, hipStream_t stream,
                  const int* d_batch = nullptr, const StepOut* so = nullptr,
                  const float* const* xs = nullptr);
  // ops [begin, end) for images [c0, c0 + batch) of the buffers (c0 > 0: a chunk)
  void launch_ops(size_t begin, size_t end, int batch, void* const* bufs, hipStream_t stream,
                  int c0 = 0, const int* d_batch = nullptr, const StepOut* so = nullptr,
                  const float* const* xs = nullptr, const InputTable* tab = nullptr);
  int device_;
  PlanSpec spec_;
  std::vector<int> buckets_;
  std::vector<std::vector<void*>> bufs_;  // [slot][buffer id]
  void* shared_ws_ = nullptr;             // activation buffers shared by every slot
  std::map<std::pair<int, int>, hipGraphExec_t> graphs_;
  mutable std::mutex mu_;
  std::mutex capture_mu_;
};

void check_hip(hipError_t e, const char* what);

}  // namespace gale
