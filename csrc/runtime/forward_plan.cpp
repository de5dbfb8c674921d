// Forward-plan validation (see gale/forward_plan.h). Host only.
#include "gale/forward_plan.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace gale {

const char* op_kind_name(int kind) {
  static const char* const kNames[kOpKinds] = {
      "conv",       "maxpool", "avgpool", "head",       "softmax",   "resnet20",
      "stem_pack",  "bn_act",  "lenet5",  "bottleneck", "stem_pool", "conv_proj"};
  return kind >= 0 && kind < kOpKinds ? kNames[kind] : "?";
}

namespace {

// The checks of one op: need() refuses with the op's index, its kind and the field at fault.
struct OpCheck {
  size_t index;
  int kind;
  int batch;     // the largest batch the executor launches this op with
  bool has_res;  // the op has a residual buffer

  [[noreturn]] void fail(const std::string& what) const {
    throw std::invalid_argument("plan op " + std::to_string(index) + " (" + op_kind_name(kind) +
                                "): " + what);
  }
  void need(bool ok, const char* what) const {
    if (!ok) fail(what);
  }
  void ptr(const void* p, const char* field) const {
    if (p == nullptr) fail(std::string(field) + " is null");
  }
  void elem_type(int et) const {
    need(et == ET_BF16 || et == ET_FP8 || et == ET_F32, "et is not an ElemType (0, 1 or 2)");
  }
  void per_launch_null(const int* batch_dev, const float* const* xs, const StepOut& so) const {
    need(!batch_dev && !xs && !so.text && !so.status && !so.status_out && !so.nrec,
         "batch_dev / xs / so are set per launch, not in the plan");
  }

  void operator()(const ConvOp& o) const {
    ptr(o.w, "w");
    ptr(o.bias, "bias");
    if (o.conv.fp8) ptr(o.wscale, "wscale");
    const ConvRoute r = conv_route(o.conv, batch, has_res && o.conv.has_res);
    if (r.kernel == CONV_NONE) fail(std::string("no conv kernel takes it: ") + r.refusal);
  }
  void operator()(const MaxPoolOp& o) const { elem_type(o.et); }
  void operator()(const AvgPoolOp& o) const { elem_type(o.et); }
  void operator()(const HeadOp& o) const {
    elem_type(o.et);
    ptr(o.w, "w");
    ptr(o.bias, "bias");
  }
  void operator()(const SoftmaxOp&) const {}
  void operator()(const StemPackOp&) const {}
  void operator()(const BnActOp& o) const {
    elem_type(o.et);
    ptr(o.scale, "scale");
    ptr(o.shift, "shift");
  }
  void operator()(const ResNet20Params& p) const {
    for (int i = 0; i < 19; ++i) {
      ptr(p.w[i], "w[]");
      ptr(p.b[i], "b[]");
      if (p.fp8) ptr(p.ws[i], "ws[]");
    }
    ptr(p.fc_w, "fc_w");
    ptr(p.fc_b, "fc_b");
    per_launch_null(p.batch_dev, p.xs, p.so);
  }
  void operator()(const LeNet5Params& p) const {
    const void* const all[10] = {p.w1, p.b1, p.w2, p.b2, p.w3, p.b3, p.w4, p.b4, p.w5, p.b5};
    static const char* const names[10] = {"w1", "b1", "w2", "b2", "w3",
                                          "b3", "w4", "b4", "w5", "b5"};
    for (int i = 0; i < 10; ++i) ptr(all[i], names[i]);
    per_launch_null(p.batch_dev, p.xs, p.so);
  }
  void operator()(const BottleneckParams& p) const {
    ptr(p.w1, "w1");
    ptr(p.b1, "b1");
    ptr(p.w2, "w2");
    ptr(p.b2, "b2");
    ptr(p.w3, "w3");
    ptr(p.b3, "b3");
    if (p.down) {
      ptr(p.wd, "wd");
      ptr(p.bd, "bd");
    }
    need(bottleneck56_supported(kBneckH, kBneckW, p.cin, kBneckMid, kBneckOut, p.down),
         "cin is not the 56x56 bottleneck's (256, or 64 with down)");
  }
  void operator()(const StemPoolOp& o) const {
    ptr(o.w, "w");
    ptr(o.bias, "bias");
    const PoolGeom& g = o.g;
    need(stem_pool_supported(o.conv, g.H, g.W, g.C, g.k, g.s, g.pad, g.Ho, g.Wo),
         "unsupported geometry (not the 224x224 stem + 3x3/2 max-pool)");
  }
  void operator()(const ConvProjOp& o) const {
    ptr(o.w, "w");
    ptr(o.bias, "bias");
    ptr(o.wd, "wd");
    ptr(o.bd, "bd");
    need(conv_gemm_proj_supported(o.conv, batch, o.H2, o.W2, o.Cin2, o.stride2, o.Kpad2),
         "unsupported geometry (conv3 + projection as one GEMM)");
  }
};

}  // namespace

void validate_plan(const PlanSpec& spec) {
  const std::vector<long long>& bytes = spec.buf_bytes_per_image;
  if (bytes.size() < 2) throw std::invalid_argument("plan needs >= 2 buffers");
  if (spec.max_batch <= 0 || spec.slots <= 0) throw std::invalid_argument("bad max_batch/slots");
  if (spec.chunk_ops < 0 || spec.chunk_ops > (int)spec.ops.size() || spec.chunk_images < 0)
    throw std::invalid_argument("bad chunk_ops / chunk_images");
  const int nb = (int)bytes.size();
  for (size_t i = 0; i < spec.ops.size(); ++i) {
    const PlanOp& op = spec.ops[i];
    const bool chunked = spec.chunk_images > 0 && (int)i < spec.chunk_ops;
    const OpCheck c{i, op.kind(),
                    chunked ? std::min(spec.chunk_images, spec.max_batch) : spec.max_batch,
                    op.res >= 0};
    c.need(op.in >= 0 && op.in < nb, "in is outside the buffer table");
    c.need(op.out >= 0 && op.out < nb, "out is outside the buffer table");
    c.need(op.res >= -1 && op.res < nb, "res is outside the buffer table");
    c.need(op.kind() != OP_CONV_PROJ || op.res >= 0, "res is missing (the projection's source)");
    const int ids[3] = {op.in, op.out, op.res};
    static const char* const over[3] = {"bpi[0] exceeds the in buffer",
                                        "bpi[1] exceeds the out buffer",
                                        "bpi[2] exceeds the res buffer"};
    for (int k = 0; k < 3; ++k) {
      c.need(op.bpi[k] >= 0, "bpi is negative");
      if (ids[k] >= 0) c.need(op.bpi[k] <= bytes[ids[k]], over[k]);
    }
    if (chunked)
      c.need(op.bpi[0] > 0 && op.bpi[1] > 0 && (op.res < 0 || op.bpi[2] > 0),
             "chunked without per-image operand bytes (bpi)");
    std::visit(c, op.params);
  }
}

}  // namespace gale
