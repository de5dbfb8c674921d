// GpuReplica (see replica.h): staged JSON bytes -> GPU JSON parser -> hipGraph forward ->
// softmax rows on the replica's own streams. Kept apart from the host-only replicas so the
// sanitizer build of the host pipeline (make tsan / make asan) links no GPU code. What a batch's
// metadata holds and how the input resize's tables lie on the device are decided by host-only
// plans (batch_plan.h, resize_plan.h); this file allocates, copies and launches.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <thread>
#include <vector>
#include <stdexcept>

#include "../codec/json_codec.h"
#include "b64_source.h"
#include "metrics.h"
#include "replica.h"

namespace gale {

namespace {

// a section of a slot's metadata (host copy or device mirror) at its MetaLayout offset
template <typename T>
T* meta_at(uint8_t* base, size_t off) {
  return reinterpret_cast<T*>(base + off);
}

}  // namespace

// How a site emits the step's sequence (emit_step)
struct GpuReplica::StepDesc {
  bool device_counts;  // the kernels read the batch's counts from the metadata header, their
                       // launches sized for the largest batch; else the host passes them
  bool meta_h2d;       // the metadata's copy is part of the sequence (else: ahead of it)
  // the prediction text / the text and the verdicts, from the forward's epilogue or the
  // formatting kernel / the probabilities copied back
  enum { Text, TextVerdicts, Probs } out;
  bool verdict_d2h;  // the verdicts are copied back from the metadata
};

struct GpuReplica::StepError {
  hipError_t code;
  const char* what;
};

// ---------------------------------------------------------------------------------------------
// GpuReplica
// ---------------------------------------------------------------------------------------------

GpuReplica::GpuReplica(std::shared_ptr<Executor> exec, int H, int W, int C, int classes,
                       bool use_graph, int wait_poll_us, bool gpu_encode, int locality,
                       bool step_graph, bool high_priority, bool step_direct, int top_k)
    : exec_(std::move(exec)), H_(H), W_(W), C_(C), classes_(classes), recH_(H), recW_(W),
      use_graph_(use_graph),
      wait_poll_us_(wait_poll_us), gpu_encode_(gpu_encode), top_k_(gpu_encode ? top_k : 0),
      locality_(locality), step_direct_(step_direct) {
  // (the selection kernel's limits, topk.hip; the engine's configuration is checked before)
  if (top_k_ < 0 || top_k_ > std::min(classes, 64) || (top_k_ > 0 && classes > 4096))
    throw std::invalid_argument("GpuReplica: top_k must be 1 .. min(classes, 64), classes <= "
                                "4096");
  step_graph_ = step_graph && use_graph && exec_->device_batch_ok();
  ptr_input_ = step_graph_ && gpu_encode_ && step_direct_ && exec_->step_out_ok();
  my_loc_ = this->locality();
  form_ = !step_graph_ ? StepForm::OpByOp : gpu_encode_ ? StepForm::Kernels : StepForm::Captured;
  if (exec_->input_bytes_per_image() != (long long)H * W * C * 4)
    throw std::invalid_argument("GpuReplica: executor input is not fp32 [H, W, C]");
  if (exec_->output_bytes_per_image() != (long long)classes * 4)
    throw std::invalid_argument("GpuReplica: executor output is not fp32 [classes]");
  check_hip(hipSetDevice(exec_->device()), "hipSetDevice");
  if (high_priority) {
    int least = 0, greatest = 0;
    check_hip(hipDeviceGetStreamPriorityRange(&least, &greatest), "stream priority range");
    check_hip(hipStreamCreateWithPriority(&stream_, hipStreamNonBlocking, greatest),
              "hipStreamCreateWithPriority");
  } else if (const char* e = getenv("GALE_REPLICA_CU_RESERVE"); e && atoi(e) > 0) {
    // (A/B) the replica's kernels kept off the last N CUs, which the GPU ingest's passes then
    // find free instead of queueing behind whole-chip forward batches
    hipDeviceProp_t prop;
    check_hip(hipGetDeviceProperties(&prop, exec_->device()), "hipGetDeviceProperties");
    const int cus = prop.multiProcessorCount, keep = std::max(1, cus - atoi(e));
    std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0u);
    for (int i = 0; i < keep; ++i) mask[(size_t)i / 32] |= 1u << (i % 32);
    check_hip(hipExtStreamCreateWithCUMask(&stream_, (uint32_t)mask.size(), mask.data()),
              "hipExtStreamCreateWithCUMask");
  } else {
    check_hip(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
  }
  const int mb = exec_->max_batch();
  slots_.resize((size_t)exec_->slots());
  for (Slot& s : slots_) {
    check_hip(hipHostMalloc(reinterpret_cast<void**>(&s.h_out), sizeof(float) * mb * classes),
              "hipHostMalloc(out)");
    if (gpu_encode_) {
      // top_k: k slots per image and, behind them in the same allocation, k class indices
      const size_t per = top_k_ > 0 ? (size_t)top_k_ : (size_t)classes;
      const size_t tb = (size_t)kFloatTextSlot * mb * per;
      const size_t ib = top_k_ > 0 ? sizeof(int32_t) * mb * per : 0;
      check_hip(hipHostMalloc(reinterpret_cast<void**>(&s.h_text), tb + ib, hipHostMallocMapped),
                "hipHostMalloc(text)");
      if (top_k_ > 0) s.h_idx = reinterpret_cast<int32_t*>(s.h_text + tb);
      check_hip(hipMalloc(reinterpret_cast<void**>(&s.d_status), sizeof(int) * mb),
                "hipMalloc(status)");
      check_hip(hipMemset(s.d_status, 0, sizeof(int) * mb), "hipMemset(status)");
      s.h_status = static_cast<int*>(mapped_alloc(sizeof(int) * mb, "status"));
    }
    check_hip(hipEventCreateWithFlags(&s.done, hipEventDisableTiming |
                                                   (wait_poll_us_ < 0 ? hipEventBlockingSync : 0)),
              "hipEventCreate");
    // initial text capacity: ~12 bytes per number (Java Float.toString + ",") x a full batch
    ensure_device(s, (size_t)mb * H * W * C * 12 + 4096);
    ensure_tiles(s, (int)(((size_t)mb * H * W * C * 12) / kJsonTileBytes) + 2 * mb);
  }
}

GpuReplica::~GpuReplica() {
  hipSetDevice(exec_->device());
  if (stream_) hipStreamSynchronize(stream_);
  for (Slot& s : slots_) {
    drop_steps(s);
    if (s.h_bytes) hipHostFree(s.h_bytes);
    if (s.d_bytes) hipFree(s.d_bytes);
    if (s.h_meta) hipHostFree(s.h_meta);
    if (s.d_meta) hipFree(s.d_meta);
    if (s.d_tiles) hipFree(s.d_tiles);
    if (s.h_out) hipHostFree(s.h_out);
    if (s.h_text) hipHostFree(s.h_text);
    if (s.h_status) hipHostFree(s.h_status);
    if (s.d_status) hipFree(s.d_status);
    if (s.done) hipEventDestroy(s.done);
    if (s.d_src) hipFree(s.d_src);
  }
  if (d_resize_) hipFree(d_resize_);
  if (stream_) hipStreamDestroy(stream_);
}

// The input resize of this replica's step: the tables' device image (pack, resize_plan.h) in one
// device allocation with the kernel plan bound to it and, per slot, the source tensor the parse
// writes. Both are allocated here, once, and never move.
void GpuReplica::set_input_resize(const InputResize& r) {
  if (d_resize_) throw std::logic_error("GpuReplica: input resize set twice");
  if (r.H() != H_ || r.W() != W_ || !r.ok())
    throw std::invalid_argument("GpuReplica: resize tables do not match the model input");
  check_hip(hipSetDevice(exec_->device()), "hipSetDevice");
  const ResizeDeviceImage image = pack(r);
  check_hip(hipMalloc(reinterpret_cast<void**>(&d_resize_), image.bytes.size()),
            "hipMalloc(resize tables)");
  check_hip(hipMemcpy(d_resize_, image.bytes.data(), image.bytes.size(), hipMemcpyHostToDevice),
            "H2D resize tables");
  resize_ = bind(image, r, C_, d_resize_);
  const int mb = exec_->max_batch(), HS = r.HS(), WS = r.WS();
  const size_t bytes = sizeof(float) * (size_t)mb * HS * WS * C_;
  for (Slot& s : slots_) {
    check_hip(hipMalloc(reinterpret_cast<void**>(&s.d_src), bytes), "hipMalloc(resize source)");
    // the text of a full batch at the source size (as the constructor sized it for the model's)
    ensure_device(s, (size_t)mb * HS * WS * C_ * 12 + 4096);
    ensure_tiles(s, (int)(((size_t)mb * HS * WS * C_ * 12) / kJsonTileBytes) + 2 * mb);
  }
  fprintf(stderr, "[gale %s] input resize%s %dx%d -> %dx%d -> crop %dx%d: %zu source bytes per "
                  "slot, %zu slots\n",
          name().c_str(), r.antialias() ? " (antialiased)" : "", HS, WS, r.HR(), r.WR(), H_, W_,
          bytes, slots_.size());
  recH_ = HS, recW_ = WS;
}

// The resize of the step in the bound plan's form: with d_images the count is read on the device
// and `images` is the launch size (the step graph's form)
GpuReplica::StepError GpuReplica::launch_resize(const BoundResize& r, int images,
                                                const int* d_images, const float* src, float* dst,
                                                hipStream_t st) {
  if (r.antialias)
    return d_images ? StepError{resize_crop_aa_dev(images, d_images, r.aa, src, dst, st),
                                "resize_crop_aa_dev"}
                    : StepError{resize_crop_aa(images, r.aa, src, dst, st), "resize_crop_aa"};
  return d_images ? StepError{resize_crop_dev(images, d_images, r.plain, src, dst, st),
                              "resize_crop_dev"}
                  : StepError{resize_crop(images, r.plain, src, dst, st), "resize_crop"};
}

std::string GpuReplica::name() const { return "gpu" + std::to_string(exec_->device()); }

// Host-mapped pinned memory that kernels address with the host pointer (ROCm maps it at the
// same virtual address; anything else is refused rather than silently copied).
void* GpuReplica::mapped_alloc(size_t bytes, const char* what) {
  void* h = nullptr;
  check_hip(hipHostMalloc(&h, bytes, hipHostMallocMapped), what);
  void* d = nullptr;
  check_hip(hipHostGetDevicePointer(&d, h, 0), what);
  if (d != h) {
    hipHostFree(h);
    throw std::runtime_error(std::string("GpuReplica: mapped ") + what +
                             " buffer has another device address");
  }
  return h;
}

void GpuReplica::ensure_host(Slot& s, size_t bytes) {
  if (bytes <= s.h_cap) return;
  const size_t cap = (std::max(bytes, s.h_cap * 2) + 4095) & ~(size_t)4095;
  if (s.h_bytes) {
    check_hip(hipEventSynchronize(s.done), "hipEventSynchronize");
    hipHostFree(s.h_bytes);
  }
  check_hip(hipHostMalloc(reinterpret_cast<void**>(&s.h_bytes), cap), "hipHostMalloc(bytes)");
  s.h_cap = cap;
}

void GpuReplica::drop_steps(Slot& s) {
  for (hipGraphExec_t& g : s.step) {
    if (g) hipGraphExecDestroy(g);
    g = nullptr;
  }
}

// Per-slot parser metadata (MetaLayout, batch_plan.h), pinned on the host and mirrored on the
// device (one H2D per batch), plus the per-tile token counts. Grown before the batch's metadata
// is written (the plan knows the tile count first), so nothing is carried over.
void GpuReplica::ensure_tiles(Slot& s, int ntiles) {
  if (ntiles <= s.meta.tiles_cap) return;
  const MetaLayout m(exec_->max_batch(), std::max(ntiles, s.meta.tiles_cap * 2));
  if (s.h_meta) {
    check_hip(hipEventSynchronize(s.done), "hipEventSynchronize");
    drop_steps(s);
    hipHostFree(s.h_meta);
    hipFree(s.d_meta);
    hipFree(s.d_tiles);
    s.h_meta = s.d_meta = nullptr;
    s.d_tiles = nullptr;
    s.meta = MetaLayout();
  }
  // host-mapped: the copy-free step graph's kernels read the metadata from here
  s.h_meta = static_cast<uint8_t*>(mapped_alloc(m.total, "meta"));
  memset(s.h_meta, 0, MetaLayout::kHeaderBytes);
  check_hip(hipMalloc(reinterpret_cast<void**>(&s.d_meta), m.total), "hipMalloc(meta)");
  check_hip(hipMalloc(reinterpret_cast<void**>(&s.d_tiles), sizeof(int) * (size_t)m.tiles_cap),
            "hipMalloc(tiles)");
  s.meta = m;
}

void GpuReplica::ensure_device(Slot& s, size_t bytes) {
  if (bytes <= s.d_cap) return;
  const size_t cap = (std::max(bytes, s.d_cap * 2) + 4095) & ~(size_t)4095;
  if (s.d_bytes) {
    check_hip(hipEventSynchronize(s.done), "hipEventSynchronize");
    drop_steps(s);
    hipFree(s.d_bytes);
  }
  check_hip(hipMalloc(reinterpret_cast<void**>(&s.d_bytes), cap), "hipMalloc(bytes)");
  s.d_cap = cap;
}

// The batch as the plan sees it (BatchPlanRecord): where each record's instances array lies,
// whether this replica's device memory holds its text (GPU ingest, its own locality slot) and
// its parsed images, and for b64 records where their strings start.
void GpuReplica::describe(const Batch& b, Slot& s) {
  s.recs.assign(b.recs.size(), BatchPlanRecord());
  s.b64_offs.clear();
  for (size_t i = 0; i < b.recs.size(); ++i) {
    const InRecord& r = b.recs[i];
    BatchPlanRecord& p = s.recs[i];
    p.arr_len = r.arr_len;
    p.images = r.images;
    p.pinned = r.pinned;
    p.resident = resident(r);
    p.preparsed = preparsed(r);
    if (p.resident) {
      p.dev_text = reinterpret_cast<uint64_t>(r.dev_value + r.arr_off);
      p.dev_counts = reinterpret_cast<uint64_t>(r.dev_counts);
      p.dev_image = reinterpret_cast<uint64_t>(r.dev_image);
    } else {
      p.buf = reinterpret_cast<uint64_t>(r.buf.get());
      p.arr_off = (r.value + r.arr_off) - r.buf.get();
    }
    if (b64_ && !p.preparsed) {
      p.b64_first = (int32_t)s.b64_offs.size();
      p.b64_n = codec::b64_image_offsets_bytes(r.value + r.arr_off, (size_t)r.arr_len,
                                               pixels_.bytes(recH_, recW_, C_), s.b64_scan)
                    ? (int32_t)s.b64_scan.size()
                    : -1;
      s.b64_offs.insert(s.b64_offs.end(), s.b64_scan.begin(), s.b64_scan.end());
    }
  }
}

// One batch: its step is the forward alone when the ingest parsed every record (table_step);
// otherwise the plan (batch_plan.h) says where every record's text goes on the device and what
// the parser's metadata holds, the slot's buffers grow to fit, the text and the metadata are
// written, and the step is launched in the replica's form.
void GpuReplica::submit(Batch& b) {
  const int slot = next_slot_;
  next_slot_ = (next_slot_ + 1) % (int)slots_.size();
  b.slot = slot;
  Slot& s = slots_[(size_t)slot];
  if (!(ptr_input_ && table_step(b, s, slot))) {
    BatchPlan& p = s.plan;
    describe(b, s);
    plan_batch(s.recs, exec_->max_batch(), (int64_t)H_ * W_ * C_, form_, ptr_input_, b64_, p);
    resident_ += p.resident;
    host_ += (int64_t)b.recs.size() - p.resident;
    preparsed_ += p.npre;
    b.images = p.img;
    ensure_device(s, p.dev_total + 16);
    if (p.staged_bytes) ensure_host(s, p.staged_bytes + 16);
    ensure_tiles(s, p.ntiles);
    stage_text(b, s);
    fill_batch(p, s.recs, s.b64_offs, s.meta, reinterpret_cast<uint64_t>(s.d_bytes),
               reinterpret_cast<uint64_t>(exec_->input(slot)), s.h_meta);
    launch_step(b, s, slot);
    if (d_resize_) resized_ += p.img;
  }
  check_hip(hipEventRecord(s.done, stream_), "hipEventRecord");
  s.t_submit_ns = mono_ns();
}

// The batch's text on the device. Records that arrived in pinned fetch buffers are DMA'd straight
// from them: one hipMemcpyAsync per fetch buffer covering the records' span (the few Kafka
// record-header bytes between values ride along); records in pageable memory are first gathered
// into the slot's pinned staging buffer.
void GpuReplica::stage_text(const Batch& b, Slot& s) {
  const BatchPlan& p = s.plan;
  for (const BatchPlan::Span& x : p.spans)
    check_hip(hipMemcpyAsync(s.d_bytes + x.dev, reinterpret_cast<const uint8_t*>(x.buf) + x.lo,
                             x.len, hipMemcpyHostToDevice, stream_),
              "H2D span");
  if (!p.staged_bytes) return;
  for (const BatchPlan::Staged& g : p.staged) {
    const InRecord& r = b.recs[(size_t)g.rec];
    memcpy(s.h_bytes + g.host, r.value + r.arr_off, g.len);
  }
  check_hip(hipMemcpyAsync(s.d_bytes + p.staged_dev, s.h_bytes, p.staged_bytes,
                           hipMemcpyHostToDevice, stream_),
            "H2D staged");
}

// The planned batch's step: ONE replay of the slot's captured graph, or its sequence enqueued
// here (step_direct: the same kernels launched directly, no graph-launch bookkeeping in the
// runtime; without a step graph: op by op).
void GpuReplica::launch_step(Batch& b, Slot& s, int slot) {
  const BatchPlan& p = s.plan;
  const bool captured =
      form_ == StepForm::Captured || (form_ == StepForm::Kernels && !step_direct_);
  hipGraphExec_t g = captured ? step_for(s, slot, p.count_pass) : nullptr;
  if (form_ == StepForm::Kernels) {
    // the metadata this batch uses (header, its records, the input pointer table, its tile
    // map) as one DMA ahead of the kernels
    const MetaRange m = s.meta.used(p);
    check_hip(hipMemcpyAsync(s.d_meta + m.off, s.h_meta + m.off, m.bytes, hipMemcpyHostToDevice,
                             stream_),
              "H2D step metadata");
  }
  if (g) {
    check_hip(hipGraphLaunch(g, stream_), "hipGraphLaunch(step)");
  } else {
    const StepError e = emit_step(s, slot, stream_, step_desc(), p.count_pass,
                                  form_ == StepForm::OpByOp || p.nrec > 0);
    check_hip(e.code, e.what);
  }
  if (form_ == StepForm::OpByOp) {
    if (use_graph_ && exec_->graph_pays()) ++fwd_graph_batches_;
  } else {
    b.step_graph = true;
    ++step_batches_;
  }
}

// Every record of the batch parsed by the ingest pass (into at most kInputTableBases arenas):
// the step is ONE launch - the forward, each image addressed through an InputTable in its kernel
// arguments - with no metadata copy (the H2D of a step's metadata ran as a CU blit kernel, ~12 us
// of device time per batch, profiles/r6_e2e_kernel_stats.txt) and no verdict hand-off (the
// ingest judged the records). With top_k the forward writes no text and the selection kernel
// follows it: two launches.
bool GpuReplica::table_step(Batch& b, Slot& s, int slot) {
  InputTable tab;
  memset(&tab, 0, sizeof(tab));
  const int64_t per = (int64_t)H_ * W_ * C_;
  int nb = 0, img = 0;
  for (const InRecord& r : b.recs) {
    if (!preparsed(r) || !r.dev_arena || img + r.images > kInputTableImages) return false;
    int bi = 0;
    while (bi < nb && tab.base[bi] != r.dev_arena) ++bi;
    if (bi == nb) {
      if (nb == kInputTableBases) return false;
      tab.base[nb++] = r.dev_arena;
    }
    const int64_t s0 = (r.dev_image - r.dev_arena) / per;
    if (s0 < 0 || s0 + r.images > 0xffffff) return false;
    for (int k = 0; k < r.images; ++k) tab.code[img + k] = ((uint32_t)bi << 24) | (uint32_t)(s0 + k);
    img += r.images;
  }
  if (img <= 0 || img > exec_->max_batch()) return false;
  s.plan.all_preparsed(b.recs.size());
  StepOut so;
  so.text = top_k_ > 0 ? nullptr : s.h_text;  // (no status hand-off: status_out null)
  exec_->launch_table(slot, img, tab, stream_, &so);
  if (top_k_ > 0)  // a second launch: the selection reads the rows the forward left on the device
    check_hip(topk_java(img, classes_, top_k_, static_cast<const float*>(exec_->output(slot)),
                        s.h_text, s.h_idx, stream_),
              "topk_java");
  b.images = img;
  b.step_graph = true;
  ++step_batches_;
  ++table_batches_;
  preparsed_ += (int64_t)b.recs.size();
  resident_ += (int64_t)b.recs.size();
  return true;
}

// The step's sequence, enqueued on `st`: [metadata H2D] -> [count] -> parse -> forward -> output
// -> [verdicts D2H]; parse false: a batch of records the ingest already parsed, the forward
// alone. Three sites emit it, each in the replica's form (step_desc):
//   op by op (no step graph): the counts come from the host (the slot's plan), the forward is
//     the executor's own run, the text or the probabilities and the verdicts come back by copy;
//   the captured step without gpu_encode: the same with every launch sized for the largest batch
//     and the counts read from the metadata header, so one graph per slot serves every batch
//     (the parse covers tiles_cap tiles and the forward max_batch images, their waves past the
//     header's counts exit at once; the status copy-back is max_batch records);
//   the kernels-only step (gpu_encode), captured or launched directly: the batch's metadata is
//     DMA'd just before (submit(): an SDMA copy of the used part only), the prediction text and
//     the verdicts leave in the forward's epilogue (other plans end with the formatting kernel).
//     The r4 step captured a metadata H2D and a status D2H as graph nodes, which this runtime
//     runs as CU blit kernels (two per batch, 68 us average under the serving load); reading the
//     metadata from host memory instead stretched every kernel by 25-40 % under the link's DMA
//     load (profiles/r5_step_ab.txt).
GpuReplica::StepDesc GpuReplica::step_desc() const {
  const bool kernels = form_ == StepForm::Kernels;
  return {form_ != StepForm::OpByOp, !kernels,
          kernels       ? StepDesc::TextVerdicts
          : gpu_encode_ ? StepDesc::Text
                        : StepDesc::Probs,
          !kernels};
}

GpuReplica::StepError GpuReplica::emit_step(Slot& s, int slot, hipStream_t st, const StepDesc& d,
                                            bool count_pass, bool parse) {
  const MetaLayout& L = s.meta;
  const BatchPlan& p = s.plan;
  const int mb = exec_->max_batch();
  const bool dev = d.device_counts;
  const int32_t* hdr = meta_at<int32_t>(s.d_meta, L.hdr);
  float* in = static_cast<float*>(exec_->input(slot));
  // input resize: the parse writes the slot's source tensor at the records' size and resize_crop
  // follows into the executor's input
  float* parsed = d_resize_ ? s.d_src : in;
  const float* out = static_cast<const float*>(exec_->output(slot));
  int* status = d.out == StepDesc::TextVerdicts ? s.d_status : nullptr;  // (null: in the table)
  hipError_t c = hipSuccess;
  if (d.meta_h2d) {
    const MetaRange m = L.used(p);
    c = hipMemcpyAsync(s.d_meta + m.off, s.h_meta + m.off, m.bytes, hipMemcpyHostToDevice, st);
    if (c != hipSuccess) return {c, "H2D step metadata"};
  }
  if (parse && b64_) {
    // one decode launch, chosen by what the strings carry: the same table, status words and
    // output for every source
    const char* which = nullptr;
    c = b64_source_instances(dev ? mb : p.b64n, meta_at<B64Image>(s.d_meta, L.b64_table),
                             s.d_bytes, recH_, recW_, C_, parsed,
                             status ? status : meta_at<int>(s.d_meta, L.b64_status), st,
                             dev ? hdr + kHdrB64 : nullptr, &prep_, pixels_, &which);
    if (c != hipSuccess) return {c, which};
  } else if (parse) {
    c = json_parse_instances(dev ? mb : p.nrec, dev ? L.tiles_cap : p.ntiles,
                             meta_at<JsonRecord>(s.d_meta, L.recs), meta_at<int>(s.d_meta, L.tiles),
                             s.d_bytes, recH_, recW_, C_, s.d_tiles, parsed, st, count_pass,
                             dev ? hdr + kHdrTiles : nullptr, status, nullptr, &prep_);
    if (c != hipSuccess) return {c, "json_parse_instances"};
  }
  if (parse && d_resize_) {
    const StepError e = launch_resize(resize_, dev ? mb : p.img, dev ? hdr + kHdrImages : nullptr,
                                      s.d_src, in, st);
    if (e.code != hipSuccess) return e;
  }
  // the forward: the executor's run with the host's count for plans that are not one device
  // batch, else sized for max_batch with the count read from the header
  const bool epilogue = d.out == StepDesc::TextVerdicts && exec_->step_out_ok();
  if (!dev) {
    exec_->run(slot, p.img, st, use_graph_);
  } else {
    StepOut so;
    so.text = top_k_ > 0 ? nullptr : s.h_text;  // (top_k: the selection launch below writes it)
    so.status = s.d_status;
    so.status_out = s.h_status;
    so.nrec = hdr + kHdrRecords;
    try {
      exec_->launch_device_batch(slot, hdr + kHdrImages, st, epilogue ? &so : nullptr,
                                 ptr_input_ ? meta_at<const float*>(s.d_meta, L.xs) : nullptr);
    } catch (const std::exception&) {
      return {hipErrorLaunchFailure, "step forward"};
    }
  }
  const int rows = dev ? mb : p.img;
  switch (d.out) {
    case StepDesc::Text:
      // the prediction text (Java Float.toString per value) is formatted on the stream and
      // comes back instead of the probabilities, so the emitting thread only concatenates slots
      // (format.hip: ~6 us per 256-image batch). The kernel stores the 16-byte slots straight
      // into the pinned (device-mapped, coherent) host buffer: no separate D2H copy.
      // With top_k the selection kernel (topk.hip) stands in its place: k slots and k class
      // indices per row.
      c = top_k_ > 0 ? topk_java(rows, classes_, top_k_, out, s.h_text, s.h_idx, st)
                     : format_floats_java(rows * classes_, out, s.h_text, st);
      if (c != hipSuccess) return {c, top_k_ > 0 ? "topk_java" : "format_floats_java"};
      break;
    case StepDesc::TextVerdicts:
      if (top_k_ > 0) {
        // the epilogue handed the verdicts over and wrote no text: the selection follows it with
        // the header's image count; other plans end with the selection's step form (its launch
        // has 64 threads per row of max_batch, enough for max_batch verdicts)
        c = epilogue ? topk_java_dev(mb, hdr + kHdrImages, classes_, top_k_, out, s.h_text,
                                     s.h_idx, st)
                     : topk_java_step(mb, hdr + kHdrImages, classes_, top_k_, out, s.h_text,
                                      s.h_idx, hdr + kHdrRecords, s.d_status, s.h_status, st);
        if (c != hipSuccess) return {c, epilogue ? "topk_java_dev" : "topk_java_step"};
        break;
      }
      if (!epilogue)
        c = format_floats_java_step(std::max(mb * classes_, mb), hdr + kHdrImages, classes_, out,
                                    s.h_text, hdr + kHdrRecords, s.d_status, s.h_status, st);
      if (c != hipSuccess) return {c, "format_floats_java_step"};
      break;
    case StepDesc::Probs:
      c = hipMemcpyAsync(s.h_out, out, sizeof(float) * rows * classes_, hipMemcpyDeviceToHost, st);
      if (c != hipSuccess) return {c, "D2H probs"};
      break;
  }
  if (d.verdict_d2h) {
    const size_t n = (size_t)(dev ? mb : p.nrec);
    c = b64_ ? hipMemcpyAsync(s.h_meta + L.b64_status, s.d_meta + L.b64_status, sizeof(int) * n,
                              hipMemcpyDeviceToHost, st)
             : hipMemcpyAsync(s.h_meta + L.recs, s.d_meta + L.recs, sizeof(JsonRecord) * n,
                              hipMemcpyDeviceToHost, st);
    if (c != hipSuccess) return {c, "D2H status"};
  }
  return {hipSuccess, ""};
}

// The slot's step graph, captured on first use (and after its buffers moved), on a private
// stream (as Executor::run does) and replayed on the replica's stream.
hipGraphExec_t GpuReplica::step_for(Slot& s, int slot, bool count_pass) {
  hipGraphExec_t& g = s.step[count_pass ? 1 : 0];
  if (g) return g;
  hipStream_t cs = nullptr;
  check_hip(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking), "capture stream");
  hipGraph_t graph = nullptr;
  hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
  if (e == hipSuccess) {
    const hipError_t c = emit_step(s, slot, cs, step_desc(), count_pass, true).code;
    e = hipStreamEndCapture(cs, &graph);
    if (e == hipSuccess) e = c;
  }
  hipStreamDestroy(cs);
  if (e != hipSuccess && graph) hipGraphDestroy(graph);
  check_hip(e, "step graph capture");
  e = hipGraphInstantiate(&g, graph, nullptr, nullptr, 0);
  hipGraphDestroy(graph);
  check_hip(e, "step graph instantiate");
  return g;
}

void GpuReplica::wait(Batch& b) {
  Slot& s = slots_[(size_t)b.slot];
  if (wait_poll_us_ > 0) {
    // sleep-poll: the thread sleeps while the GPU works (the engine's timer slack is set to
    // 1 us on replica threads, so a sleep is not stretched by the default 50 us slack). It
    // sleeps through most of the expected batch time at once and polls only near the end:
    // polling every 20 us through a 0.5 ms batch cost ~0.25 core per replica (6 replicas:
    // 1.5 of a 16-core host share, which then tipped it into CFS throttling)
    const int64_t due = s.t_submit_ns + expect_ns_ * 85 / 100;
    const int64_t now = mono_ns();
    if (expect_ns_ > 0 && due - now > 2000ll * wait_poll_us_)
      std::this_thread::sleep_for(std::chrono::nanoseconds(due - now));
    for (;;) {
      const hipError_t e = hipEventQuery(s.done);
      if (e == hipSuccess) break;
      if (e != hipErrorNotReady) check_hip(e, "hipEventQuery(batch)");
      std::this_thread::sleep_for(std::chrono::microseconds(wait_poll_us_));
    }
    const int64_t took = mono_ns() - s.t_submit_ns;
    expect_ns_ = expect_ns_ > 0 ? (expect_ns_ * 7 + took) / 8 : took;
  } else {
    check_hip(hipEventSynchronize(s.done), "hipEventSynchronize(batch)");
  }
  b.dev_status.assign(b.recs.size(), codec::OK);
  // the verdicts are where the form the batch was submitted in leaves them
  const int* words = s.plan.form == StepForm::Kernels ? s.h_status
                     : b64_ ? meta_at<int>(s.h_meta, s.meta.b64_status)
                            : nullptr;
  const JsonRecord* recs = meta_at<JsonRecord>(s.h_meta, s.meta.recs);
  for (size_t i = 0; i < b.recs.size(); ++i) {
    const int k = i < s.plan.parse_idx.size() ? s.plan.parse_idx[i] : (int)i;
    if (k < 0) continue;  // parsed (and judged) by the ingest pass
    b.dev_status[i] = device_verdict_status(words ? words[k] : recs[k].status);
  }
  b.probs = gpu_encode_ ? nullptr : s.h_out;
  b.pred_text = gpu_encode_ ? s.h_text : nullptr;
  b.pred_idx = gpu_encode_ && top_k_ > 0 ? s.h_idx : nullptr;
}

void GpuReplica::recover() {
  // drain whatever the failed batches left queued on both streams, then clear the (non-sticky)
  // error state; a sticky device fault makes these calls fail and the supervisor gives up
  check_hip(hipSetDevice(exec_->device()), "recover: hipSetDevice");
  check_hip(hipStreamSynchronize(stream_), "recover: compute stream");
  (void)hipGetLastError();
  next_slot_ = 0;
}

}  // namespace gale
