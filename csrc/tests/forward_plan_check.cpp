// Sanitizer run of the forward plan's validation (gale/forward_plan.h): a fixed seed, plans
// holding every op kind over a random buffer table, then random corruption - buffer ids in and
// out of range, null pointers, element types, bytes per image, chunking figures, conv and fused-op
// geometry no kernel takes. validate_plan must refuse by std::invalid_argument exactly the plans the second derivation below calls
// unlaunchable, so an accepted plan has every id inside the table.
//   build/asan/forward_plan_check [iterations]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "gale/forward_plan.h"

using namespace gale;

namespace {

int failures = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      ++failures;                                          \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                        \
      fprintf(stderr, "\n");                               \
    }                                                      \
  } while (0)

float storage[4];  // (addresses for the plan's pointers; nothing reads through them)
const float* kPtr = storage;

// The conv geometries of the valid plans: a 3x3 16 -> 16 conv on 8x8 (bf16 or fp8: the MFMA
// kernel), the ResNet-50 packed stem, and conv3 of its first bottleneck (1x1 64 -> 256 on 56x56).
ConvDesc conv3x3(int fp8) {
  ConvDesc d{};
  d.H = d.W = d.Ho = d.Wo = 8, d.Cin = d.Cout = d.Npad = 16;
  d.KH = d.KW = 3, d.stride = d.pad = 1, d.K = 144, d.Kpad = 160;
  d.fp8 = fp8, d.in_scale = d.out_scale = d.res_scale = 0.5f;
  return d;
}
ConvDesc stem_desc() {
  ConvDesc d{};
  d.H = 224, d.W = 230, d.Cin = 4, d.Ho = d.Wo = 112, d.Cout = d.Npad = 64;
  d.KH = d.KW = 8, d.stride = 2, d.pad = 3, d.K = d.Kpad = 256, d.relu = 1, d.stem = 1;
  return d;
}
ConvDesc conv3_desc() {
  ConvDesc d{};
  d.H = d.W = d.Ho = d.Wo = 56, d.Cin = d.K = d.Kpad = 64, d.Cout = d.Npad = 256;
  d.KH = d.KW = d.stride = 1, d.relu = 1;
  return d;
}
const PoolGeom kStemPool = {112, 112, 64, 3, 2, 1, 56, 56};

OpParams valid_params(int kind, std::mt19937& rng) {
  switch (kind) {
    case OP_CONV: {
      ConvOp o;
      o.conv = conv3x3(rng() % 2);
      o.w = o.bias = kPtr;
      if (o.conv.fp8) o.wscale = kPtr;
      return o;
    }
    case OP_MAXPOOL: {
      MaxPoolOp o;
      o.et = rng() % 3;
      return o;
    }
    case OP_AVGPOOL: {
      AvgPoolOp o;
      o.et = rng() % 3;
      return o;
    }
    case OP_HEAD: {
      HeadOp o;
      o.et = rng() % 3;
      o.w = o.bias = kPtr;
      return o;
    }
    case OP_SOFTMAX: return SoftmaxOp{};
    case OP_RESNET20: {
      ResNet20Params p{};
      p.fp8 = rng() % 2;
      for (int i = 0; i < 19; ++i) {
        p.w[i] = p.b[i] = kPtr;
        if (p.fp8) p.ws[i] = kPtr;
      }
      p.fc_w = p.fc_b = kPtr;
      return p;
    }
    case OP_STEM_PACK: return StemPackOp{};
    case OP_BN_ACT: {
      BnActOp o;
      o.et = rng() % 3;
      o.scale = o.shift = kPtr;
      return o;
    }
    case OP_LENET5: {
      LeNet5Params p{};
      p.w1 = p.w2 = p.w3 = p.w4 = kPtr;
      p.b1 = p.b2 = p.b3 = p.b4 = p.w5 = p.b5 = kPtr;
      return p;
    }
    case OP_BOTTLENECK: {
      BottleneckParams p;
      p.w1 = p.w2 = p.w3 = kPtr;
      p.b1 = p.b2 = p.b3 = kPtr;
      p.down = rng() % 2;
      p.cin = p.down ? 64 : 256;
      if (p.down) p.wd = p.bd = kPtr;
      return p;
    }
    case OP_STEM_POOL: {
      StemPoolOp o;
      o.conv = stem_desc();
      o.g = kStemPool;
      o.w = o.bias = kPtr;
      return o;
    }
    default: {
      ConvProjOp o;
      o.conv = conv3_desc();
      o.H2 = o.W2 = 56, o.Cin2 = o.Kpad2 = 64, o.stride2 = 1;
      o.w = o.wd = kPtr;
      o.bias = o.bd = kPtr;
      return o;
    }
  }
}

// null one pointer of the op (whichever the draw picks; possibly one the kind does not need)
void null_a_pointer(OpParams& params, std::mt19937& rng) {
  const unsigned r = rng();
  if (auto* o = std::get_if<ConvOp>(&params)) {
    switch (r % 3) {
      case 0: o->w = nullptr; break;
      case 1: o->bias = nullptr; break;
      default: o->wscale = nullptr;
    }
  } else if (auto* o = std::get_if<HeadOp>(&params)) {
    (r % 2 ? o->w : o->bias) = nullptr;
  } else if (auto* o = std::get_if<BnActOp>(&params)) {
    (r % 2 ? o->scale : o->shift) = nullptr;
  } else if (auto* p = std::get_if<ResNet20Params>(&params)) {
    switch (r % 5) {
      case 0: p->w[(r >> 8) % 19] = nullptr; break;
      case 1: p->b[(r >> 8) % 19] = nullptr; break;
      case 2: p->ws[(r >> 8) % 19] = nullptr; break;
      case 3: p->fc_w = nullptr; break;
      default: p->fc_b = nullptr;
    }
  } else if (auto* p = std::get_if<LeNet5Params>(&params)) {
    const float** f[6] = {&p->b1, &p->b2, &p->b3, &p->b4, &p->w5, &p->b5};
    const void** v[4] = {&p->w1, &p->w2, &p->w3, &p->w4};
    if (r % 10 < 6) *f[r % 10] = nullptr; else *v[r % 10 - 6] = nullptr;
  } else if (auto* p = std::get_if<BottleneckParams>(&params)) {
    const float** f[4] = {&p->b1, &p->b2, &p->b3, &p->bd};
    const void** v[4] = {&p->w1, &p->w2, &p->w3, &p->wd};
    if (r % 8 < 4) *f[r % 8] = nullptr; else *v[r % 8 - 4] = nullptr;
  } else if (auto* o = std::get_if<StemPoolOp>(&params)) {
    if (r % 2) o->w = nullptr; else o->bias = nullptr;
  } else if (auto* o = std::get_if<ConvProjOp>(&params)) {
    switch (r % 4) {
      case 0: o->w = nullptr; break;
      case 1: o->bias = nullptr; break;
      case 2: o->wd = nullptr; break;
      default: o->bd = nullptr;
    }
  }
}

// one field of the op's geometry set to a value no kernel takes (ops without geometry: nothing)
void break_geometry(OpParams& params, std::mt19937& rng) {
  const unsigned r = rng();
  if (auto* o = std::get_if<ConvOp>(&params)) {
    switch (r % 6) {
      case 0: o->conv.Cout = 18; break;                   // Cout % 4
      case 1: o->conv.Kpad = 144; break;                  // Kpad % 32
      case 2: o->conv.Npad = 24; break;                   // Npad % (16 nt)
      case 3: o->conv.out_f32 = 1; break;                 // fp32 out outside a 1x1
      case 4: o->conv.fp8 = 1, o->conv.in_scale = 0.f; break;
      default: o->conv.H = o->conv.W = 1 << 14; break;    // max_batch*H*W*Cin >= 2^31
    }
  } else if (auto* p = std::get_if<BottleneckParams>(&params)) {
    p->cin = 128;
  } else if (auto* o = std::get_if<StemPoolOp>(&params)) {
    if (r % 2) o->g.Ho = 55; else o->conv.Ho = 111;
  } else if (auto* o = std::get_if<ConvProjOp>(&params)) {
    if (r % 2) o->Cin2 = 96; else o->conv.has_res = 1;
  }
}

// (memberwise: the valid plans' descs against a corrupted one)
bool same_desc(const ConvDesc& a, const ConvDesc& b) {
  return a.H == b.H && a.W == b.W && a.Cin == b.Cin && a.Ho == b.Ho && a.Wo == b.Wo &&
         a.Cout == b.Cout && a.KH == b.KH && a.KW == b.KW && a.stride == b.stride &&
         a.pad == b.pad && a.K == b.K && a.Kpad == b.Kpad && a.Npad == b.Npad &&
         a.has_res == b.has_res && a.out_f32 == b.out_f32 && a.stem == b.stem &&
         a.fp8 == b.fp8 && a.in_scale == b.in_scale;
}

void set_et(OpParams& params, int et) {
  if (auto* o = std::get_if<MaxPoolOp>(&params)) o->et = et;
  if (auto* o = std::get_if<AvgPoolOp>(&params)) o->et = et;
  if (auto* o = std::get_if<HeadOp>(&params)) o->et = et;
  if (auto* o = std::get_if<BnActOp>(&params)) o->et = et;
}

// The second derivation: can every op be launched as it stands? Written from the contract in
// forward_plan.h, kind by kind, not from validate_plan's code.
bool launchable(const PlanSpec& s) {
  const long long nb = (long long)s.buf_bytes_per_image.size();
  if (nb < 2 || s.max_batch < 1 || s.slots < 1) return false;
  if (s.chunk_ops < 0 || s.chunk_images < 0) return false;
  if (s.chunk_ops > (long long)s.ops.size()) return false;
  for (size_t i = 0; i < s.ops.size(); ++i) {
    const PlanOp& op = s.ops[i];
    if (op.in < 0 || op.in >= nb || op.out < 0 || op.out >= nb) return false;
    if (op.res < -1 || op.res >= nb) return false;
    const int ids[3] = {op.in, op.out, op.res};
    const bool chunked = s.chunk_images > 0 && (long long)i < s.chunk_ops;
    for (int k = 0; k < 3; ++k) {
      if (op.bpi[k] < 0) return false;
      if (ids[k] < 0) continue;
      if (op.bpi[k] > s.buf_bytes_per_image[ids[k]]) return false;
      if (chunked && op.bpi[k] == 0) return false;
    }
    bool have = true;
    int et = 0;
    switch (op.kind()) {
      case OP_CONV: {
        const ConvOp& o = std::get<ConvOp>(op.params);
        // (geometry: the valid plans' conv, or one break_geometry broke; 2^14 x 2^14 x 16
        // elements per image are 2^32, over the kernels' 32-bit offsets at any batch)
        have = o.w && o.bias && (!o.conv.fp8 || o.wscale) &&
               same_desc(o.conv, conv3x3(o.conv.fp8));
        break;
      }
      case OP_MAXPOOL: et = std::get<MaxPoolOp>(op.params).et; break;
      case OP_AVGPOOL: et = std::get<AvgPoolOp>(op.params).et; break;
      case OP_HEAD: {
        const HeadOp& o = std::get<HeadOp>(op.params);
        et = o.et;
        have = o.w && o.bias;
        break;
      }
      case OP_BN_ACT: {
        const BnActOp& o = std::get<BnActOp>(op.params);
        et = o.et;
        have = o.scale && o.shift;
        break;
      }
      case OP_RESNET20: {
        const ResNet20Params& p = std::get<ResNet20Params>(op.params);
        have = p.fc_w && p.fc_b && !p.batch_dev && !p.xs && !p.so.text;
        for (int j = 0; j < 19; ++j) have = have && p.w[j] && p.b[j] && (!p.fp8 || p.ws[j]);
        break;
      }
      case OP_LENET5: {
        const LeNet5Params& p = std::get<LeNet5Params>(op.params);
        have = p.w1 && p.b1 && p.w2 && p.b2 && p.w3 && p.b3 && p.w4 && p.b4 && p.w5 && p.b5 &&
               !p.batch_dev && !p.xs && !p.so.text;
        break;
      }
      case OP_BOTTLENECK: {
        const BottleneckParams& p = std::get<BottleneckParams>(op.params);
        have = p.w1 && p.b1 && p.w2 && p.b2 && p.w3 && p.b3 && (!p.down || (p.wd && p.bd)) &&
               p.cin == (p.down ? 64 : 256);
        break;
      }
      case OP_STEM_POOL: {
        const StemPoolOp& o = std::get<StemPoolOp>(op.params);
        have = o.w && o.bias && same_desc(o.conv, stem_desc()) && o.g.Ho == 56;
        break;
      }
      case OP_CONV_PROJ: {
        const ConvProjOp& o = std::get<ConvProjOp>(op.params);
        have = o.w && o.bias && o.wd && o.bd && op.res >= 0 && o.Cin2 == 64 &&
               same_desc(o.conv, conv3_desc());
        break;
      }
      default: break;  // softmax, stem_pack: dimensions only
    }
    if (!have || et < 0 || et > 2) return false;
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 4000;
  std::mt19937 rng(20240611);
  int accepted = 0, refused = 0, seen_kind[kOpKinds] = {0}, untouched_refused = 0;
  for (int kind = -2; kind < kOpKinds + 2; ++kind)
    CHECK(std::string(op_kind_name(kind)).size() > 0, "kind name %d", kind);
  for (int it = 0; it < iters; ++it) {
    PlanSpec s;
    const int nb = 2 + (int)(rng() % 7);
    for (int b = 0; b < nb; ++b) s.buf_bytes_per_image.push_back(1 + (long long)(rng() % 4096));
    s.max_batch = 1 + (int)(rng() % 256);
    s.slots = 1 + (int)(rng() % 3);
    // every kind once, in a random rotation, then a few more
    const int nops = kOpKinds + (int)(rng() % 6), first = (int)(rng() % kOpKinds);
    for (int i = 0; i < nops; ++i) {
      PlanOp op;
      const int kind = i < kOpKinds ? (first + i) % kOpKinds : (int)(rng() % kOpKinds);
      op.params = valid_params(kind, rng);
      CHECK(op.kind() == kind, "kind %d holds alternative %d", kind, op.kind());
      op.in = (int)(rng() % nb), op.out = (int)(rng() % nb);
      op.res = kind == OP_CONV_PROJ || rng() % 3 == 0 ? (int)(rng() % nb) : -1;
      const int ids[3] = {op.in, op.out, op.res};
      for (int k = 0; k < 3; ++k)
        if (ids[k] >= 0) op.bpi[k] = 1 + (long long)(rng() % s.buf_bytes_per_image[ids[k]]);
      op.layer = i;
      s.ops.push_back(op);
    }
    if (rng() % 2) s.chunk_ops = (int)(rng() % (nops + 1)), s.chunk_images = (int)(rng() % 5);
    const bool corrupt = rng() % 4 != 0;
    for (int m = corrupt ? 1 + (int)(rng() % 3) : 0; m > 0; --m) {
      PlanOp& op = s.ops[rng() % s.ops.size()];
      const int wild = (int)(rng() % (nb + 6)) - 3;  // -3 .. nb + 2
      switch (rng() % 10) {
        case 0: op.in = wild; break;
        case 1: op.out = wild; break;
        case 2: op.res = wild; break;
        case 3: null_a_pointer(op.params, rng); break;
        case 4: set_et(op.params, (int)(rng() % 8) - 2); break;
        case 5: op.bpi[rng() % 3] = (long long)(rng() % 8192) - 64; break;
        case 6:
          s.chunk_ops = (int)(rng() % (nops + 4)) - 2;
          s.chunk_images = (int)(rng() % 6) - 1;
          break;
        case 7: s.buf_bytes_per_image.resize(rng() % (nb + 1)); break;
        case 8: break_geometry(op.params, rng); break;
        default: (rng() % 2 ? s.max_batch : s.slots) = (int)(rng() % 3) - 1;
      }
    }
    const bool want = launchable(s);
    bool got = false;
    try {
      validate_plan(s);
      got = true;
    } catch (const std::invalid_argument& e) {
      CHECK(std::string(e.what()).size() > 0, "empty refusal");
    } catch (...) {
      CHECK(false, "iteration %d: refused by something other than invalid_argument", it);
    }
    CHECK(got == want, "iteration %d: validate_plan %s a plan that is %s", it,
          got ? "accepted" : "refused", want ? "launchable" : "not launchable");
    if (got) {
      ++accepted;
      const int n = (int)s.buf_bytes_per_image.size();
      for (const PlanOp& op : s.ops) {
        CHECK(op.in >= 0 && op.in < n && op.out >= 0 && op.out < n && op.res >= -1 && op.res < n,
              "iteration %d: an accepted plan indexes outside the buffer table", it);
        ++seen_kind[op.kind()];
      }
    } else {
      ++refused;
      untouched_refused += !corrupt;
    }
  }
  CHECK(untouched_refused == 0, "%d uncorrupted plans refused", untouched_refused);
  CHECK(accepted > iters / 8 && refused > iters / 8, "accepted %d, refused %d of %d", accepted,
        refused, iters);
  for (int k = 0; k < kOpKinds; ++k) CHECK(seen_kind[k] > 0, "no accepted %s op", op_kind_name(k));
  printf("%d plans: %d accepted, %d refused\n", iters, accepted, refused);
  if (failures) {
    fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  printf("all checks passed\n");
  return 0;
}
