// The forward plan of a model: a flat list of typed ops over numbered buffers, checked once by
// validate_plan before the executor (gale/executor.h) makes any HIP call. Host only: no HIP call
// here or in forward_plan.cpp, so the plan is testable (and sanitizer-checked) without a GPU.
#pragma once
#include <variant>
#include <vector>

#include "gale/kernels.h"

namespace gale {

// One struct per op kind, holding exactly what its launcher takes besides the op's buffers.
struct ConvOp {  // conv2d (also dense layers as 1x1 convs)
  ConvDesc conv{};
  const void* w = nullptr;
  const float* bias = nullptr;
  const float* wscale = nullptr;  // fp8 only
};
struct PoolGeom {
  int H = 0, W = 0, C = 0, k = 0, s = 0, pad = 0, Ho = 0, Wo = 0;
};
struct MaxPoolOp {
  PoolGeom g;
  int et = 0;  // ElemType of the activations
};
struct AvgPoolOp {
  int HW = 0, C = 0, et = 0;
};
struct HeadOp {  // pool + dense (fp32 w) + softmax
  int HW = 0, C = 0, N = 0, et = 0;
  float in_scale = 1.f;  // fp8: the input's activation scale
  const float* w = nullptr;
  const float* bias = nullptr;
};
struct SoftmaxOp {
  int N = 0, ld = 0;
};
struct StemPackOp {  // fp32 input -> packed-stem bf16 image
  int H = 0, W = 0, C = 0, Wp = 0, lp = 0;
};
struct BnActOp {  // unfolded-BN plan: standalone BatchNorm + residual add + ReLU
  int HW = 0, Wo = 0, C = 0, relu = 0, res_H = 0, res_W = 0, res_C = 0, res_stride = 1, et = 0;
  const float* scale = nullptr;
  const float* shift = nullptr;
};
struct StemPoolOp {  // ResNet-50 stem conv + max-pool (stem_pool): the stem's desc and weights,
  ConvDesc conv{};   // the max-pool's geometry
  const void* w = nullptr;
  const float* bias = nullptr;
  PoolGeom g;
};
struct ConvProjOp {  // bottleneck conv3 + projection shortcut as one GEMM (conv2d_gemm_proj):
  ConvDesc conv{};   // conv = conv3's desc, in = its input, res = the block input (the
  const void* w = nullptr;  // projection's source, [H2][W2][Cin2] sampled at stride2)
  const float* bias = nullptr;
  const void* wd = nullptr;
  const float* bd = nullptr;
  int H2 = 0, W2 = 0, Cin2 = 0, stride2 = 0, Kpad2 = 0;
};

// The alternatives in OpKind order: PlanOp::kind() is the variant's index. The whole-network
// kernels and the 56x56 bottleneck hold their launcher's struct (gale/kernels.h), filled once;
// the per-launch members (batch_dev, xs, so) stay null in the plan.
enum OpKind : int {
  OP_CONV = 0,
  OP_MAXPOOL = 1,
  OP_AVGPOOL = 2,
  OP_HEAD = 3,
  OP_SOFTMAX = 4,
  OP_RESNET20 = 5,
  OP_STEM_PACK = 6,
  OP_BN_ACT = 7,
  OP_LENET5 = 8,
  OP_BOTTLENECK = 9,
  OP_STEM_POOL = 10,
  OP_CONV_PROJ = 11,
};
using OpParams = std::variant<ConvOp, MaxPoolOp, AvgPoolOp, HeadOp, SoftmaxOp, ResNet20Params,
                              StemPackOp, BnActOp, LeNet5Params, BottleneckParams, StemPoolOp,
                              ConvProjOp>;
constexpr int kOpKinds = (int)std::variant_size_v<OpParams>;
const char* op_kind_name(int kind);  // "conv", "maxpool", ...; "?" outside [0, kOpKinds)

// Buffer ids: 0 = network input (fp32 NHWC), 1 = network output (fp32 [B, classes]),
// >= 2 = activation workspace.
struct PlanOp {
  OpParams params;
  int in = 0, out = 0, res = -1;
  long long bpi[3] = {0, 0, 0};  // bytes per image of the in / out / res tensors (chunking)
  int layer = 0;                 // the last model layer the op covers (chunk_ops is counted by it)
  int kind() const { return (int)params.index(); }
};

struct PlanSpec {
  std::vector<PlanOp> ops;
  std::vector<long long> buf_bytes_per_image;  // indexed by buffer id (ids 0 and 1 included)
  int max_batch = 256;
  int slots = 2;                               // independent I/O buffer sets (pipelining depth)
  std::vector<int> buckets;                    // graph batch buckets (ascending); empty = powers of 2
  // Batch chunking of the leading ops: ops [0, chunk_ops) run once per chunk of chunk_images
  // images (operands offset by the first image of the chunk times their PlanOp::bpi; activations
  // are batch-major), the
  // rest once over the whole batch. Keeps the wide early tensors (ResNet-50 56x56x256 at batch
  // 256: 411 MB each) small enough to stay in the 256 MB Infinity Cache between producer and
  // consumer. 0 = off. The plan must keep every tensor that outlives the prefix in a buffer no
  // other prefix tensor uses (a later chunk would overwrite it): build_plan(chunk_layers=...).
  int chunk_ops = 0;
  int chunk_images = 0;
};

// Throws std::invalid_argument ("plan op <index> (<kind>): <field> ...") unless every op can be
// launched as it stands: in / out / res inside buf_bytes_per_image (a conv_proj has a res), every
// pointer its kind needs non-null, et an ElemType, bpi within its buffer; and max_batch / slots /
// chunk_ops / chunk_images sane, every chunked op with the bpi of its operands. Every conv is
// routed (gale/conv_route.h) at the largest batch the executor launches it with - chunk_images for
// a chunked op, else max_batch - and refused with the route's refusal when no kernel takes it;
// a conv_proj, a bottleneck and a stem_pool must have the geometry their kernel is compiled for.
void validate_plan(const PlanSpec& spec);

}  // namespace gale
