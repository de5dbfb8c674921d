// Plan executor (see gale/executor.h).
#include "gale/executor.h"

#include <algorithm>
#include <stdexcept>

namespace gale {

void check_hip(hipError_t e, const char* what) {
  if (e != hipSuccess) {
    throw std::runtime_error(std::string("HIP error in ") + what + ": " + hipGetErrorString(e));
  }
}

Executor::Executor(int device, PlanSpec spec) : device_(device), spec_(std::move(spec)) {
  validate_plan(spec_);
  buckets_ = spec_.buckets;
  if (buckets_.empty()) {
    for (int b = 1; b < spec_.max_batch; b *= 2) buckets_.push_back(b);
    buckets_.push_back(spec_.max_batch);
  }
  std::sort(buckets_.begin(), buckets_.end());
  buckets_.erase(std::unique(buckets_.begin(), buckets_.end()), buckets_.end());
  if (buckets_.back() < spec_.max_batch) buckets_.push_back(spec_.max_batch);

  check_hip(hipSetDevice(device_), "hipSetDevice");
  const size_t nb = spec_.buf_bytes_per_image.size();
  // activation workspace (ids >= 2) shared by all slots: one compute stream per executor
  size_t ws_total = 0;
  std::vector<size_t> ws_off(nb, 0);
  for (size_t i = 2; i < nb; ++i) {
    ws_off[i] = ws_total;
    const size_t bytes = (size_t)spec_.buf_bytes_per_image[i] * spec_.max_batch;
    ws_total += (bytes + 255) & ~size_t(255);
  }
  if (ws_total) check_hip(hipMalloc(&shared_ws_, ws_total), "hipMalloc(workspace)");
  bufs_.resize(spec_.slots);
  for (int s = 0; s < spec_.slots; ++s) {
    bufs_[s].assign(nb, nullptr);
    for (int i = 0; i < 2; ++i) {
      const size_t bytes = (size_t)spec_.buf_bytes_per_image[i] * spec_.max_batch;
      check_hip(hipMalloc(&bufs_[s][i], bytes ? bytes : 256), "hipMalloc(io)");
      check_hip(hipMemset(bufs_[s][i], 0, bytes ? bytes : 256), "hipMemset(io)");
    }
    for (size_t i = 2; i < nb; ++i) bufs_[s][i] = static_cast<char*>(shared_ws_) + ws_off[i];
  }
}

Executor::~Executor() {
  hipSetDevice(device_);
  for (auto& kv : graphs_) hipGraphExecDestroy(kv.second);
  for (auto& s : bufs_) {
    if (s.size() >= 2) {
      hipFree(s[0]);
      hipFree(s[1]);
    }
  }
  if (shared_ws_) hipFree(shared_ws_);
}

int Executor::bucket_for(int batch) const {
  for (int b : buckets_)
    if (b >= batch) return b;
  return -1;
}

void Executor::launch_all(int batch, void* const* bufs, hipStream_t stream, const int* d_batch,
                          const StepOut* so, const float* const* xs) {
  size_t begin = 0;
  const int ch = spec_.chunk_images;
  if (spec_.chunk_ops > 0 && ch > 0 && batch > ch) {
    for (int c0 = 0; c0 < batch; c0 += ch)
      launch_ops(0, spec_.chunk_ops, std::min(ch, batch - c0), bufs, stream, c0);
    begin = spec_.chunk_ops;
  }
  launch_ops(begin, spec_.ops.size(), batch, bufs, stream, 0, d_batch, so, xs);
}

bool Executor::device_batch_ok() const {
  if (spec_.ops.empty() || spec_.chunk_ops > 0) return false;
  for (const PlanOp& op : spec_.ops)
    if (op.kind() != OP_RESNET20 && op.kind() != OP_LENET5) return false;
  return true;
}

void Executor::launch_device_batch(int slot, const int* d_batch, hipStream_t stream,
                                   const StepOut* so, const float* const* xs) {
  if (!device_batch_ok()) throw std::logic_error("plan does not take a device batch count");
  if (so && !step_out_ok()) throw std::logic_error("plan cannot write the step outputs");
  if (xs && spec_.ops.size() != 1) throw std::logic_error("plan cannot read an input table");
  if (slot < 0 || slot >= spec_.slots) throw std::invalid_argument("bad slot");
  launch_all(spec_.max_batch, bufs_[slot].data(), stream, d_batch, so, xs);
}

void Executor::launch_table(int slot, int batch, const InputTable& tab, hipStream_t stream,
                            const StepOut* so) {
  if (!step_out_ok()) throw std::logic_error("plan cannot read an input table");
  if (slot < 0 || slot >= spec_.slots) throw std::invalid_argument("bad slot");
  if (batch <= 0 || batch > spec_.max_batch || batch > kInputTableImages)
    throw std::invalid_argument("bad table batch");
  launch_ops(0, 1, batch, bufs_[slot].data(), stream, 0, nullptr, so, nullptr, &tab);
}

namespace {

// One op's launch: the operands of this launch, and per kind the launcher with the op's fields.
struct Launch {
  int batch;
  const void* in;
  void* out;
  const void* res;
  hipStream_t stream;
  const int* d_batch;
  const StepOut* so;
  const float* const* xs;
  const InputTable* tab;

  hipError_t operator()(const ConvOp& o) const {
    return conv2d(o.conv, batch, in, o.w, o.bias, o.wscale, res, out, stream);
  }
  hipError_t operator()(const MaxPoolOp& o) const {
    const PoolGeom& g = o.g;
    return maxpool2d(batch, g.H, g.W, g.C, g.k, g.s, g.pad, g.Ho, g.Wo, in, out, o.et, stream);
  }
  hipError_t operator()(const AvgPoolOp& o) const {
    return avgpool_global(batch, o.HW, o.C, in, out, o.et, stream);
  }
  hipError_t operator()(const HeadOp& o) const {
    return head_pool_dense_softmax(batch, o.HW, o.C, o.N, in, o.et, o.in_scale, o.w, o.bias,
                                   static_cast<float*>(out), stream);
  }
  hipError_t operator()(const SoftmaxOp& o) const {
    return softmax_rows(batch, o.N, o.ld, static_cast<const float*>(in),
                        static_cast<float*>(out), stream);
  }
  hipError_t operator()(const StemPackOp& o) const {
    return stem_pack(batch, o.H, o.W, o.C, o.Wp, o.lp, static_cast<const float*>(in), out, stream);
  }
  hipError_t operator()(const BnActOp& o) const {
    return bn_act(batch, o.HW, o.Wo, o.C, in, o.scale, o.shift, res, o.res_H, o.res_W, o.res_C,
                  o.res_stride, o.relu, out, stream, o.et);
  }
  // the whole-network kernels: the plan's struct with this launch's members set on a copy
  template <typename Params>
  Params per_launch(Params p) const {
    p.batch_dev = d_batch;
    p.xs = xs;
    if (so) p.so = *so;
    return p;
  }
  hipError_t operator()(const ResNet20Params& p) const {
    return resnet20_fused_forward(per_launch(p), batch, static_cast<const float*>(in),
                                  static_cast<float*>(out), stream, tab);
  }
  hipError_t operator()(const LeNet5Params& p) const {
    return lenet5_fused_forward(per_launch(p), batch, static_cast<const float*>(in),
                                static_cast<float*>(out), stream, tab);
  }
  hipError_t operator()(const BottleneckParams& p) const {
    return bottleneck56(p, batch, in, out, stream);
  }
  hipError_t operator()(const StemPoolOp& o) const {
    return stem_pool(batch, in, o.w, o.bias, out, stream);
  }
  hipError_t operator()(const ConvProjOp& o) const {
    return conv2d_gemm_proj(o.conv, batch, in, o.w, o.bias, res, o.H2, o.W2, o.Cin2, o.stride2,
                            o.Kpad2, o.wd, o.bd, out, stream);
  }
};

}  // namespace

// Every id and field was checked when the executor was built (validate_plan).
void Executor::launch_ops(size_t begin, size_t end, int batch, void* const* bufs,
                          hipStream_t stream, int c0, const int* d_batch, const StepOut* so,
                          const float* const* xs, const InputTable* tab) {
  auto at = [&](int id, long long bpi) -> void* {
    return static_cast<char*>(bufs[id]) + (size_t)c0 * (size_t)bpi;
  };
  for (size_t oi = begin; oi < end; ++oi) {
    const PlanOp& op = spec_.ops[oi];
    const Launch launch{batch, at(op.in, op.bpi[0]), at(op.out, op.bpi[1]),
                        op.res >= 0 ? at(op.res, op.bpi[2]) : nullptr,
                        stream, d_batch, so, xs, tab};
    check_hip(std::visit(launch, op.params), "plan op launch");
  }
}

void Executor::run_on(int batch, const void* in, void* out, hipStream_t stream) {
  if (batch > spec_.max_batch) throw std::invalid_argument("batch > max_batch");
  std::vector<void*> b = bufs_[0];
  b[0] = const_cast<void*>(in);
  b[1] = out;
  launch_all(batch, b.data(), stream);
}

void Executor::run(int slot, int batch, hipStream_t stream, bool use_graph) {
  if (slot < 0 || slot >= spec_.slots) throw std::invalid_argument("bad slot");
  if (batch <= 0) return;
  if (batch > spec_.max_batch) throw std::invalid_argument("batch > max_batch");
  if (!use_graph || !graph_pays()) {
    launch_all(batch, bufs_[slot].data(), stream);
    return;
  }
  const int bucket = bucket_for(batch);
  hipGraphExec_t exec = nullptr;
  {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = graphs_.find({bucket, slot});
    if (it != graphs_.end()) exec = it->second;
  }
  if (!exec) {
    // capture on a private non-blocking stream (the legacy null stream cannot capture) that
    // lives only for the capture: serving keeps one stream per replica and per ingest lane, so
    // every stream can own a hardware queue (GPU_MAX_HW_QUEUES) - rocprofv3's queue
    // interception crashed on queues shared by concurrently submitting threads. The
    // instantiated graph is launched on the caller's stream.
    std::lock_guard<std::mutex> cap(capture_mu_);
    hipStream_t cs = nullptr;
    check_hip(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking), "capture stream");
    hipGraph_t graph = nullptr;
    hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
      try {
        launch_all(bucket, bufs_[slot].data(), cs);
      } catch (...) {
        hipStreamEndCapture(cs, &graph);
        if (graph) hipGraphDestroy(graph);
        hipStreamDestroy(cs);
        throw;
      }
      e = hipStreamEndCapture(cs, &graph);
    }
    hipStreamDestroy(cs);
    check_hip(e, "graph capture");
    check_hip(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0), "GraphInstantiate");
    hipGraphDestroy(graph);
    std::lock_guard<std::mutex> lk(mu_);
    graphs_[{bucket, slot}] = exec;
  }
  check_hip(hipGraphLaunch(exec, stream), "hipGraphLaunch");
}

void Executor::capture_all(hipStream_t stream) {
  if (!graph_pays()) return;
  for (int s = 0; s < spec_.slots; ++s)
    for (int b : buckets_) run(s, b, stream, true);
  check_hip(hipStreamSynchronize(stream), "capture_all sync");
}

int Executor::graphs_captured() const {
  std::lock_guard<std::mutex> lk(mu_);
  return (int)graphs_.size();
}

}  // namespace gale
