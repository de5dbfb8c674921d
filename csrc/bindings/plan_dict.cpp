// Forward plan <-> Python dicts (see plan_dict.h).
#include "plan_dict.h"

#include <pybind11/stl.h>

#include <set>
#include <string>

namespace py = pybind11;

namespace gale {
namespace {

// Reads named fields out of a dict. Every key asked for is remembered, so done() can refuse the
// ones nobody asked for.
class Reader {
 public:
  static constexpr bool reading = true;
  Reader(const py::dict& d, std::string where) : d_(d), where_(std::move(where)) {}

  [[noreturn]] void fail(const std::string& what) const {
    throw py::value_error(where_ + ": " + what);
  }

  template <typename T>
  void num(const char* key, T& v) {
    if (!opt(key, v)) fail(std::string("missing key '") + key + "'");
  }
  template <typename T>
  bool opt(const char* key, T& v) {
    seen_.insert(key);
    if (!d_.contains(key)) return false;
    try {
      v = d_[key].cast<T>();
    } catch (const py::cast_error&) {
      fail(std::string("bad value for '") + key + "'");
    }
    return true;
  }
  template <typename P>
  void ptr(const char* key, const P*& p) {
    uintptr_t v = 0;
    num(key, v);
    p = reinterpret_cast<const P*>(v);
  }
  template <typename T, size_t N>
  void nums(const char* key, T (&out)[N]) {
    if (!opt_nums(key, out)) fail(std::string("missing key '") + key + "'");
  }
  template <typename T, size_t N>
  bool opt_nums(const char* key, T (&out)[N]) {
    std::vector<T> v;
    if (!opt(key, v)) return false;
    if (v.size() != N)
      fail(std::string("'") + key + "' takes " + std::to_string(N) + " entries, got " +
           std::to_string(v.size()));
    for (size_t i = 0; i < N; ++i) out[i] = v[i];
    return true;
  }
  template <typename P, size_t N>
  void ptr_list(const char* key, const P* (&out)[N]) {
    uintptr_t v[N];
    nums(key, v);
    for (size_t i = 0; i < N; ++i) out[i] = reinterpret_cast<const P*>(v[i]);
  }
  template <typename T>
  void nested(const char* key, T& v);  // a dict of v's fields, read as strictly

  void done() const {
    for (auto kv : d_) {
      const std::string k = py::str(kv.first);
      if (!seen_.count(k)) fail("unknown key '" + k + "'");
    }
  }

 private:
  const py::dict& d_;
  std::string where_;
  std::set<std::string> seen_;
};

// Writes the same fields into a dict.
class Writer {
 public:
  static constexpr bool reading = false;
  explicit Writer(py::dict& d) : d_(d) {}
  template <typename T>
  void num(const char* key, T& v) {
    d_[key] = v;
  }
  template <typename T>
  bool opt(const char* key, T& v) {
    num(key, v);
    return true;
  }
  template <typename P>
  void ptr(const char* key, const P*& p) {
    d_[key] = reinterpret_cast<uintptr_t>(p);
  }
  template <typename T, size_t N>
  void nums(const char* key, T (&v)[N]) {
    py::list l;
    for (size_t i = 0; i < N; ++i) l.append(v[i]);
    d_[key] = l;
  }
  template <typename T, size_t N>
  bool opt_nums(const char* key, T (&v)[N]) {
    nums(key, v);
    return true;
  }
  template <typename P, size_t N>
  void ptr_list(const char* key, const P* (&v)[N]) {
    py::list l;
    for (size_t i = 0; i < N; ++i) l.append(reinterpret_cast<uintptr_t>(v[i]));
    d_[key] = l;
  }
  template <typename T>
  void nested(const char* key, T& v);

 private:
  py::dict& d_;
};

// ---- the field lists: one per struct, serving both directions ---------------------------------

template <typename Ar>
void fields(Ar& a, ConvDesc& c) {
  a.num("H", c.H), a.num("W", c.W), a.num("Cin", c.Cin);
  a.num("Ho", c.Ho), a.num("Wo", c.Wo), a.num("Cout", c.Cout);
  a.num("KH", c.KH), a.num("KW", c.KW), a.num("stride", c.stride), a.num("pad", c.pad);
  a.num("K", c.K), a.num("Kpad", c.Kpad), a.num("Npad", c.Npad);
  if constexpr (Ar::reading) {  // what the optional fields default to
    c.res_H = c.Ho, c.res_W = c.Wo, c.res_C = c.Cout, c.res_stride = 1;
    c.in_scale = c.out_scale = c.res_scale = 1.0f;
  }
  a.opt("relu", c.relu), a.opt("has_res", c.has_res);
  a.opt("res_H", c.res_H), a.opt("res_W", c.res_W), a.opt("res_C", c.res_C);
  a.opt("res_stride", c.res_stride);
  a.opt("in_f32", c.in_f32), a.opt("out_f32", c.out_f32), a.opt("fp8", c.fp8);
  a.opt("in_scale", c.in_scale), a.opt("out_scale", c.out_scale);
  a.opt("res_scale", c.res_scale);
  a.opt("stem", c.stem), a.opt("f32", c.f32);
}
template <typename Ar>
void fields(Ar& a, PoolGeom& g) {
  a.num("H", g.H), a.num("W", g.W), a.num("C", g.C), a.num("k", g.k), a.num("s", g.s);
  a.num("pad", g.pad), a.num("Ho", g.Ho), a.num("Wo", g.Wo);
}
template <typename Ar>
void fields(Ar& a, ConvOp& o) {
  a.nested("conv", o.conv);
  a.ptr("w", o.w), a.ptr("bias", o.bias), a.ptr("wscale", o.wscale);
}
template <typename Ar>
void fields(Ar& a, MaxPoolOp& o) {
  fields(a, o.g);
  a.num("et", o.et);
}
template <typename Ar>
void fields(Ar& a, AvgPoolOp& o) {
  a.num("HW", o.HW), a.num("C", o.C), a.num("et", o.et);
}
template <typename Ar>
void fields(Ar& a, HeadOp& o) {
  a.num("HW", o.HW), a.num("C", o.C), a.num("N", o.N), a.num("et", o.et);
  a.num("in_scale", o.in_scale);
  a.ptr("w", o.w), a.ptr("bias", o.bias);
}
template <typename Ar>
void fields(Ar& a, SoftmaxOp& o) {
  a.num("N", o.N), a.num("ld", o.ld);
}
template <typename Ar>
void fields(Ar& a, StemPackOp& o) {
  a.num("H", o.H), a.num("W", o.W), a.num("C", o.C), a.num("Wp", o.Wp), a.num("lp", o.lp);
}
template <typename Ar>
void fields(Ar& a, BnActOp& o) {
  a.num("HW", o.HW), a.num("Wo", o.Wo), a.num("C", o.C), a.num("relu", o.relu);
  a.num("res_H", o.res_H), a.num("res_W", o.res_W), a.num("res_C", o.res_C);
  a.num("res_stride", o.res_stride), a.num("et", o.et);
  a.ptr("scale", o.scale), a.ptr("shift", o.shift);
}
template <typename Ar>
void fields(Ar& a, ResNet20Params& p) {  // (batch_dev, xs and so are per launch: never in a plan)
  a.num("fp8", p.fp8);
  a.ptr_list("w", p.w), a.ptr_list("b", p.b), a.ptr("fc_w", p.fc_w), a.ptr("fc_b", p.fc_b);
  a.ptr_list("ws", p.ws);
  a.nums("s_in", p.s_in), a.nums("s_out", p.s_out), a.nums("s_res", p.s_res);
}
template <typename Ar>
void fields(Ar& a, LeNet5Params& p) {
  a.ptr("w1", p.w1), a.ptr("b1", p.b1), a.ptr("w2", p.w2), a.ptr("b2", p.b2);
  a.ptr("w3", p.w3), a.ptr("b3", p.b3), a.ptr("w4", p.w4), a.ptr("b4", p.b4);
  a.ptr("w5", p.w5), a.ptr("b5", p.b5);
}
template <typename Ar>
void fields(Ar& a, BottleneckParams& p) {
  a.ptr("w1", p.w1), a.ptr("b1", p.b1), a.ptr("w2", p.w2), a.ptr("b2", p.b2);
  a.ptr("w3", p.w3), a.ptr("b3", p.b3), a.ptr("wd", p.wd), a.ptr("bd", p.bd);
  a.num("cin", p.cin), a.num("down", p.down);
}
template <typename Ar>
void fields(Ar& a, StemPoolOp& o) {
  a.nested("conv", o.conv);
  a.ptr("w", o.w), a.ptr("bias", o.bias);
  fields(a, o.g);
}
template <typename Ar>
void fields(Ar& a, ConvProjOp& o) {
  a.nested("conv", o.conv);
  a.ptr("w", o.w), a.ptr("bias", o.bias), a.ptr("wd", o.wd), a.ptr("bd", o.bd);
  a.num("H2", o.H2), a.num("W2", o.W2), a.num("Cin2", o.Cin2), a.num("stride2", o.stride2);
  a.num("Kpad2", o.Kpad2);
}
// what every op has; res, bpi and layer may be left out
template <typename Ar>
void common_fields(Ar& a, PlanOp& op) {
  a.num("in", op.in), a.num("out", op.out), a.opt("res", op.res);
  a.opt_nums("bpi", op.bpi), a.opt("layer", op.layer);
}

template <typename T>
void Reader::nested(const char* key, T& v) {
  py::dict d;
  num(key, d);
  Reader r(d, where_ + " " + key);
  fields(r, v);
  r.done();
}
template <typename T>
void Writer::nested(const char* key, T& v) {
  py::dict d;
  Writer w(d);
  fields(w, v);
  d_[key] = d;
}

// OpParams holding alternative `kind` (value-initialised)
template <size_t I = 0>
OpParams params_of_kind(int kind) {
  if constexpr (I < std::variant_size_v<OpParams>) {
    if (kind == (int)I) return OpParams(std::in_place_index<I>);
    return params_of_kind<I + 1>(kind);
  } else {
    return OpParams();
  }
}

PlanOp op_from_dict(const py::dict& d, size_t index) {
  const std::string at = "plan op " + std::to_string(index);
  int kind = -1;
  Reader(d, at).num("kind", kind);
  if (kind < 0 || kind >= kOpKinds)
    throw py::value_error(at + ": unknown kind " + std::to_string(kind));
  Reader r(d, at + " (" + op_kind_name(kind) + ")");
  r.num("kind", kind);
  PlanOp op;
  op.params = params_of_kind(kind);
  common_fields(r, op);
  std::visit([&r](auto& p) { fields(r, p); }, op.params);
  r.done();
  return op;
}

}  // namespace

ConvDesc desc_from_dict(const py::dict& d) {
  ConvDesc c{};
  Reader r(d, "conv desc");
  fields(r, c);
  return c;
}

PlanSpec plan_spec_from_py(const py::list& ops, std::vector<long long> buf_bytes, int max_batch,
                           int slots, std::vector<int> buckets, int chunk_ops, int chunk_images) {
  PlanSpec spec;
  size_t i = 0;
  for (auto o : ops) {
    if (!py::isinstance<py::dict>(o))
      throw py::value_error("plan op " + std::to_string(i) + ": not a dict");
    spec.ops.push_back(op_from_dict(py::reinterpret_borrow<py::dict>(o), i++));
  }
  spec.buf_bytes_per_image = std::move(buf_bytes);
  spec.max_batch = max_batch;
  spec.slots = slots;
  spec.buckets = std::move(buckets);
  spec.chunk_ops = chunk_ops;
  spec.chunk_images = chunk_images;
  return spec;
}

py::list plan_ops_to_py(const PlanSpec& spec) {
  py::list out;
  for (PlanOp op : spec.ops) {  // (a copy: the field lists take non-const members)
    py::dict d;
    Writer w(d);
    int kind = op.kind();
    w.num("kind", kind);
    common_fields(w, op);
    std::visit([&w](auto& p) { fields(w, p); }, op.params);
    out.append(d);
  }
  return out;
}

}  // namespace gale
