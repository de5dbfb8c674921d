// Python bindings of the gale native library (module gale._C).
//
// Kernels take raw device pointers (torch tensors' data_ptr()) and a hipStream_t handle
// (torch.cuda.current_stream().cuda_stream), so they interoperate with PyTorch-ROCm tensors
// without linking libtorch. Long-running calls release the GIL.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <optional>
#include <stdexcept>
#include <vector>

#include "../comm/rccl.h"
#include "gale/executor.h"
#include "gale/kernels.h"
#include "plan_dict.h"

namespace py = pybind11;

namespace gale {
void bind_host(py::module_& m);  // codec / kafka / engine bindings (host_bindings.cpp)
}

namespace {

using gale::ConvDesc;
using gale::desc_from_dict;

inline hipStream_t S(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }
inline void* P(uintptr_t p) { return reinterpret_cast<void*>(p); }

void chk(hipError_t e, const char* what) { gale::check_hip(e, what); }

// The InputPrep of a parse / decode binding `name`: a / b (four coefficients each) or nchw given
// means one is passed (identity ones too); none of them, no prep (nullopt).
std::optional<gale::InputPrep> prep_from(const char* name,
                                         const std::optional<std::vector<float>>& a,
                                         const std::optional<std::vector<float>>& b, bool nchw) {
  if ((a && a->size() != 4) || (b && b->size() != 4))
    throw std::invalid_argument(std::string(name) + ": a / b take four coefficients");
  if (!a && !b && !nchw) return std::nullopt;
  gale::InputPrep prep;
  for (int i = 0; i < 4; ++i) {
    if (a) prep.a[i] = (*a)[i];
    if (b) prep.b[i] = (*b)[i];
  }
  prep.nchw = nchw ? 1 : 0;
  return prep;
}

}  // namespace

namespace gale {
void install_crash_handler();  // runtime/crash.cpp
}

namespace {
// Host-mapped pinned memory (hipHostMallocMapped) for tests of the zero-copy kernel paths: the
// GPU ingest reads its plan and the packed text from, and writes its results to, such memory.
struct MappedBuffer {
  uint8_t* p = nullptr;
  size_t n = 0;
  explicit MappedBuffer(size_t bytes) : n(bytes) {
    gale::check_hip(hipHostMalloc(reinterpret_cast<void**>(&p), bytes ? bytes : 1,
                                  hipHostMallocMapped),
                    "hipHostMalloc(mapped)");
    void* dp = nullptr;
    gale::check_hip(hipHostGetDevicePointer(&dp, p, 0), "hipHostGetDevicePointer");
    if (dp != p) throw std::runtime_error("mapped buffer: device address differs from host");
  }
  ~MappedBuffer() {
    if (p) hipHostFree(p);
  }
};
}  // namespace

PYBIND11_MODULE(_C, m) {
  py::class_<MappedBuffer, std::shared_ptr<MappedBuffer>>(
      m, "MappedBuffer", "host-mapped pinned buffer (same address on the host and the GPU)")
      .def(py::init<size_t>())
      .def_property_readonly("ptr", [](const MappedBuffer& b) { return (uintptr_t)b.p; })
      .def_property_readonly("size", [](const MappedBuffer& b) { return b.n; })
      .def("numpy", [](std::shared_ptr<MappedBuffer> b) {
        // a uint8 view that keeps the buffer alive
        return py::array_t<uint8_t>({(py::ssize_t)b->n}, {1}, b->p,
                                    py::capsule(new std::shared_ptr<MappedBuffer>(b), [](void* c) {
                                      delete static_cast<std::shared_ptr<MappedBuffer>*>(c);
                                    }));
      });
  m.doc() = "gale native library: gfx950 kernels, plan executor, host runtime";
  gale::install_crash_handler();

  m.def("conv2d",
        [](py::dict desc, int batch, uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t wscale,
           uintptr_t res, uintptr_t y, uintptr_t stream) {
          ConvDesc d = desc_from_dict(desc);
          chk(gale::conv2d(d, batch, P(x), P(w), static_cast<const float*>(P(bias)),
                           static_cast<const float*>(P(wscale)), P(res), P(y), S(stream)),
              "conv2d");
        },
        py::arg("desc"), py::arg("batch"), py::arg("x"), py::arg("w"), py::arg("bias"),
        py::arg("wscale"), py::arg("res"), py::arg("y"), py::arg("stream"));
  m.def("bottleneck56",
        [](int batch, uintptr_t x, uintptr_t w1, uintptr_t b1, uintptr_t w2, uintptr_t b2,
           uintptr_t w3, uintptr_t b3, uintptr_t wd, uintptr_t bd, uintptr_t y, int cin,
           int down, uintptr_t stream) {
          gale::BottleneckParams bp;
          bp.w1 = P(w1); bp.w2 = P(w2); bp.w3 = P(w3); bp.wd = P(wd);
          bp.b1 = static_cast<const float*>(P(b1));
          bp.b2 = static_cast<const float*>(P(b2));
          bp.b3 = static_cast<const float*>(P(b3));
          bp.bd = static_cast<const float*>(P(bd));
          bp.cin = cin;
          bp.down = down;
          chk(gale::bottleneck56(bp, batch, P(x), P(y), S(stream)), "bottleneck56");
        },
        py::arg("batch"), py::arg("x"), py::arg("w1"), py::arg("b1"), py::arg("w2"),
        py::arg("b2"), py::arg("w3"), py::arg("b3"), py::arg("wd"), py::arg("bd"), py::arg("y"),
        py::arg("cin"), py::arg("down"), py::arg("stream"));
  m.def("bottleneck56_supported", &gale::bottleneck56_supported, py::arg("H"), py::arg("W"),
        py::arg("cin"), py::arg("cmid"), py::arg("cout"), py::arg("down"));
  m.def("stem_pool",
        [](int batch, uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t y, uintptr_t stream) {
          chk(gale::stem_pool(batch, P(x), P(w), static_cast<const float*>(P(bias)), P(y),
                              S(stream)),
              "stem_pool");
        },
        py::arg("batch"), py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("y"),
        py::arg("stream"));
  m.def("stem_pack",
        [](int batch, int H, int W, int C, int Wp, int lp, uintptr_t x, uintptr_t y,
           uintptr_t stream) {
          chk(gale::stem_pack(batch, H, W, C, Wp, lp, static_cast<const float*>(P(x)), P(y),
                              S(stream)),
              "stem_pack");
        });
  m.def("maxpool2d",
        [](int batch, int H, int W, int C, int k, int s, int p, int Ho, int Wo, uintptr_t x,
           uintptr_t y, uintptr_t stream, int fp8) {
          chk(gale::maxpool2d(batch, H, W, C, k, s, p, Ho, Wo, P(x), P(y), fp8, S(stream)),
              "maxpool2d");
        },
        py::arg("batch"), py::arg("H"), py::arg("W"), py::arg("C"), py::arg("k"), py::arg("s"),
        py::arg("p"), py::arg("Ho"), py::arg("Wo"), py::arg("x"), py::arg("y"), py::arg("stream"),
        py::arg("fp8") = 0);
  m.def("avgpool_global",
        [](int batch, int HW, int C, uintptr_t x, uintptr_t y, uintptr_t stream, int fp8) {
          chk(gale::avgpool_global(batch, HW, C, P(x), P(y), fp8, S(stream)), "avgpool_global");
        },
        py::arg("batch"), py::arg("HW"), py::arg("C"), py::arg("x"), py::arg("y"),
        py::arg("stream"), py::arg("fp8") = 0);
  m.def("head_pool_dense_softmax",
        [](int batch, int HW, int C, int N, uintptr_t x, uintptr_t w, uintptr_t b, uintptr_t out,
           uintptr_t stream, int fp8, float in_scale) {
          chk(gale::head_pool_dense_softmax(batch, HW, C, N, P(x), fp8, in_scale,
                                            static_cast<const float*>(P(w)),
                                            static_cast<const float*>(P(b)),
                                            static_cast<float*>(P(out)), S(stream)),
              "head_pool_dense_softmax");
        },
        py::arg("batch"), py::arg("HW"), py::arg("C"), py::arg("N"), py::arg("x"), py::arg("w"),
        py::arg("b"), py::arg("out"), py::arg("stream"), py::arg("fp8") = 0,
        py::arg("in_scale") = 1.0f);
  m.def("softmax_rows", [](int batch, int N, int ld, uintptr_t x, uintptr_t out, uintptr_t stream) {
    chk(gale::softmax_rows(batch, N, ld, static_cast<const float*>(P(x)),
                           static_cast<float*>(P(out)), S(stream)),
        "softmax_rows");
  });
  m.def("cast_f32_bf16",
        [](int64_t n, float scale, float shift, uintptr_t x, uintptr_t y, uintptr_t stream) {
          chk(gale::cast_f32_bf16(n, scale, shift, static_cast<const float*>(P(x)), P(y),
                                  S(stream)),
              "cast_f32_bf16");
        });
  m.def("bn_act",
        [](int batch, int HW, int Wo, int C, uintptr_t x, uintptr_t scale, uintptr_t shift,
           uintptr_t res, int res_H, int res_W, int res_C, int rs, int relu, uintptr_t y,
           uintptr_t stream) {
          chk(gale::bn_act(batch, HW, Wo, C, P(x), static_cast<const float*>(P(scale)),
                           static_cast<const float*>(P(shift)), P(res), res_H, res_W, res_C, rs,
                           relu, P(y), S(stream)),
              "bn_act");
        });
  // The serving forms (kernels.h) by keyword: d_ntiles non-zero: the tile count is read there on
  // the device (ntiles = the launch size); status non-zero: the verdicts go to status[record] and
  // recs / tile_rec are only read; tile_bad non-zero (count_pass false): one plain-stored verdict
  // per tile. recs[].images < 0 (with has_cnt): the image count comes from the record's group sums
  m.def("json_parse_instances",
        [](int nrec, int ntiles, uintptr_t recs, uintptr_t tile_rec, uintptr_t bytes, int H,
           int W, int C, uintptr_t tile_counts, uintptr_t out, uintptr_t stream,
           bool count_pass, std::optional<std::vector<float>> a,
           std::optional<std::vector<float>> b, bool nchw, uintptr_t d_ntiles, uintptr_t status,
           uintptr_t tile_bad) {
          // a / b (four coefficients each) or nchw: an InputPrep is passed (identity ones too)
          const auto prep = prep_from("json_parse_instances", a, b, nchw);
          chk(gale::json_parse_instances(nrec, ntiles, static_cast<gale::JsonRecord*>(P(recs)),
                                         static_cast<const int*>(P(tile_rec)),
                                         static_cast<const uint8_t*>(P(bytes)), H, W, C,
                                         static_cast<int*>(P(tile_counts)),
                                         static_cast<float*>(P(out)), S(stream), count_pass,
                                         static_cast<const int*>(P(d_ntiles)),
                                         static_cast<int*>(P(status)),
                                         static_cast<int*>(P(tile_bad)),
                                         prep ? &*prep : nullptr),
              "json_parse_instances");
        },
        py::arg("nrec"), py::arg("ntiles"), py::arg("recs"), py::arg("tile_rec"),
        py::arg("bytes"), py::arg("H"), py::arg("W"), py::arg("C"), py::arg("tile_counts"),
        py::arg("out"), py::arg("stream"), py::arg("count_pass") = true,
        py::arg("a") = py::none(), py::arg("b") = py::none(), py::arg("nchw") = false,
        py::arg("d_ntiles") = 0, py::arg("status") = 0, py::arg("tile_bad") = 0);
  m.def("json_tile_count", &gale::json_tile_count);
  m.def("b64_decode_instances",
        [](int images, uintptr_t imgs, uintptr_t bytes, int H, int W, int C, uintptr_t out,
           uintptr_t status, uintptr_t stream, uintptr_t d_images,
           std::optional<std::vector<float>> a, std::optional<std::vector<float>> b, bool nchw) {
          // imgs: B64_IMAGE_BYTES-byte descriptors (int64 off, int32 slot, int32 rec); d_images
          // non-zero: the image count is read there on the device (images = the launch size).
          // a / b (four coefficients each) or nchw: an InputPrep is passed (identity ones too)
          const auto prep = prep_from("b64_decode_instances", a, b, nchw);
          chk(gale::b64_decode_instances(images, static_cast<const gale::B64Image*>(P(imgs)),
                                         static_cast<const uint8_t*>(P(bytes)), H, W, C,
                                         static_cast<float*>(P(out)),
                                         static_cast<int*>(P(status)), S(stream),
                                         static_cast<const int*>(P(d_images)),
                                         prep ? &*prep : nullptr),
              "b64_decode_instances");
        },
        py::arg("images"), py::arg("imgs"), py::arg("bytes"), py::arg("H"), py::arg("W"),
        py::arg("C"), py::arg("out"), py::arg("status"), py::arg("stream"),
        py::arg("d_images") = 0, py::arg("a") = py::none(), py::arg("b") = py::none(),
        py::arg("nchw") = false);
  m.def("b64_yuv_instances",
        [](int images, uintptr_t imgs, uintptr_t bytes, int HS, int WS, int C, uintptr_t out,
           uintptr_t status, uintptr_t stream, uintptr_t d_images, const std::string& format,
           std::vector<int32_t> coeffs, std::optional<std::vector<float>> a,
           std::optional<std::vector<float>> b, bool nchw, int pairs) {
          // imgs / d_images / a / b / nchw: as b64_decode_instances. format: "i420" | "nv12"
          // (anything else reaches the launcher as an unknown format); coeffs: (cy, crv, cgu,
          // cgv, cbu, yo). Returns the launcher's hipError_t as an int (0 = launched): its
          // refusals are part of the contract, so they do not throw
          const auto prep = prep_from("b64_yuv_instances", a, b, nchw);
          if (coeffs.size() != 6)
            throw std::invalid_argument("b64_yuv_instances: coeffs takes (cy, crv, cgu, cgv, "
                                        "cbu, yo)");
          gale::YuvCoeffs k;
          k.cy = coeffs[0], k.crv = coeffs[1], k.cgu = coeffs[2], k.cgv = coeffs[3];
          k.cbu = coeffs[4], k.yo = coeffs[5];
          const int fmt = format == "i420"   ? (int)gale::YUV_I420
                          : format == "nv12" ? (int)gale::YUV_NV12
                                             : (int)gale::YUV_NONE;
          return (int)gale::b64_yuv_instances(
              images, static_cast<const gale::B64Image*>(P(imgs)),
              static_cast<const uint8_t*>(P(bytes)), HS, WS, C, static_cast<float*>(P(out)),
              static_cast<int*>(P(status)), S(stream), static_cast<const int*>(P(d_images)),
              prep ? &*prep : nullptr, fmt, k, pairs);
        },
        py::arg("images"), py::arg("imgs"), py::arg("bytes"), py::arg("HS"), py::arg("WS"),
        py::arg("C"), py::arg("out"), py::arg("status"), py::arg("stream"),
        py::arg("d_images") = 0, py::arg("format") = "i420",
        py::arg("coeffs") = std::vector<int32_t>{1220945, 1673555, -410793, -852458, 2115221, 16},
        py::arg("a") = py::none(), py::arg("b") = py::none(), py::arg("nchw") = false,
        py::arg("pairs") = 0);
  m.def("b64_packed_instances",
        [](int images, uintptr_t imgs, uintptr_t bytes, int HS, int WS, int C, uintptr_t out,
           uintptr_t status, uintptr_t stream, uintptr_t d_images, const std::string& format,
           std::optional<std::vector<float>> a, std::optional<std::vector<float>> b, bool nchw) {
          // imgs / d_images / a / b / nchw: as b64_decode_instances. format: "bgr24" | "rgba" |
          // "bgra" | "gray" (anything else reaches the launcher as an unknown format). Returns
          // the launcher's hipError_t as an int (0 = launched): its refusals are part of the
          // contract, so they do not throw
          const auto prep = prep_from("b64_packed_instances", a, b, nchw);
          return (int)gale::b64_packed_instances(
              images, static_cast<const gale::B64Image*>(P(imgs)),
              static_cast<const uint8_t*>(P(bytes)), HS, WS, C, static_cast<float*>(P(out)),
              static_cast<int*>(P(status)), S(stream), static_cast<const int*>(P(d_images)),
              prep ? &*prep : nullptr, gale::packed_format_of(format.c_str()));
        },
        py::arg("images"), py::arg("imgs"), py::arg("bytes"), py::arg("HS"), py::arg("WS"),
        py::arg("C"), py::arg("out"), py::arg("status"), py::arg("stream"),
        py::arg("d_images") = 0, py::arg("format") = "bgr24", py::arg("a") = py::none(),
        py::arg("b") = py::none(), py::arg("nchw") = false);
  m.def("b64_typed_instances",
        [](int images, uintptr_t imgs, uintptr_t bytes, int HS, int WS, int C, uintptr_t out,
           uintptr_t status, uintptr_t stream, uintptr_t d_images, const std::string& dtype,
           std::optional<std::vector<float>> a, std::optional<std::vector<float>> b, bool nchw) {
          // imgs / d_images / a / b / nchw: as b64_decode_instances. dtype: "u16" | "f16" |
          // "bf16" | "f32" (anything else, "u8" too, reaches the launcher as an unknown type).
          // Returns the launcher's hipError_t as an int (0 = launched): its refusals are part of
          // the contract, so they do not throw
          const auto prep = prep_from("b64_typed_instances", a, b, nchw);
          return (int)gale::b64_typed_instances(
              images, static_cast<const gale::B64Image*>(P(imgs)),
              static_cast<const uint8_t*>(P(bytes)), HS, WS, C, static_cast<float*>(P(out)),
              static_cast<int*>(P(status)), S(stream), static_cast<const int*>(P(d_images)),
              prep ? &*prep : nullptr, gale::elem_type_of(dtype.c_str()));
        },
        py::arg("images"), py::arg("imgs"), py::arg("bytes"), py::arg("HS"), py::arg("WS"),
        py::arg("C"), py::arg("out"), py::arg("status"), py::arg("stream"),
        py::arg("d_images") = 0, py::arg("dtype") = "f32", py::arg("a") = py::none(),
        py::arg("b") = py::none(), py::arg("nchw") = false);
  m.def("b64_yuv_pairs", &gale::b64_yuv_pairs);
  m.def("b64_yuv_lds_bytes", &gale::b64_yuv_lds_bytes);
  m.attr("YUV_LDS_BUDGET") = (int)gale::kYuvLdsBudget;
  m.attr("HIP_ERROR_INVALID_VALUE") = (int)hipErrorInvalidValue;
  m.attr("B64_IMAGE_BYTES") = (int)sizeof(gale::B64Image);
  py::module_ comm = m.def_submodule("comm", "in-process RCCL communicator (ncclCommInitAll)");
  py::class_<gale::CommGroup, std::shared_ptr<gale::CommGroup>>(comm, "CommGroup")
      .def(py::init([](std::vector<int> devices) {
             py::gil_scoped_release nogil;
             return std::make_shared<gale::CommGroup>(devices);
           }),
           py::arg("devices"))
      .def_property_readonly("size", &gale::CommGroup::size)
      .def_property_readonly("devices", &gale::CommGroup::devices)
      .def("broadcast",
           [](gale::CommGroup& g, uintptr_t send_root, std::vector<uintptr_t> recv, size_t bytes,
              int root) {
             std::vector<void*> r;
             for (uintptr_t p : recv) r.push_back(reinterpret_cast<void*>(p));
             py::gil_scoped_release nogil;
             g.broadcast(reinterpret_cast<const void*>(send_root), r, bytes, root);
           },
           py::arg("send_root"), py::arg("recv"), py::arg("bytes"), py::arg("root") = 0)
      .def("all_reduce_sum_f64",
           [](gale::CommGroup& g, std::vector<uintptr_t> bufs, size_t count) {
             std::vector<double*> b;
             for (uintptr_t p : bufs) b.push_back(reinterpret_cast<double*>(p));
             py::gil_scoped_release nogil;
             g.all_reduce_sum_f64(b, count);
           },
           py::arg("bufs"), py::arg("count"));
  m.def("crc32c_chunks",
        [](uintptr_t bytes, uintptr_t chunks, int n, uintptr_t tables, uintptr_t out,
           uintptr_t stream) {
          gale::check_hip(gale::crc32c_chunks(reinterpret_cast<const uint8_t*>(bytes),
                                              reinterpret_cast<const gale::CrcChunk*>(chunks), n,
                                              reinterpret_cast<const uint32_t*>(tables),
                                              reinterpret_cast<uint32_t*>(out),
                                              reinterpret_cast<hipStream_t>(stream)),
                          "crc32c_chunks");
        });
  m.def("ingest_crc_count",
        [](uintptr_t bytes, uintptr_t chunks, int nchunks, uintptr_t tables, uintptr_t crc_out,
           int nrec, int ngroups, uintptr_t recs, uintptr_t groups, uintptr_t counts,
           uintptr_t gsum, uintptr_t stream, uintptr_t gbad, uintptr_t packed, uintptr_t tab,
           uintptr_t text_out) {
          gale::check_hip(
              gale::ingest_crc_count(reinterpret_cast<const uint8_t*>(bytes),
                                     reinterpret_cast<const gale::CrcChunk*>(chunks), nchunks,
                                     reinterpret_cast<const uint32_t*>(tables),
                                     reinterpret_cast<uint32_t*>(crc_out), nrec, ngroups,
                                     reinterpret_cast<gale::JsonRecord*>(recs),
                                     reinterpret_cast<const int2*>(groups),
                                     reinterpret_cast<int*>(counts),
                                     reinterpret_cast<int*>(gsum),
                                     reinterpret_cast<int*>(gbad),
                                     reinterpret_cast<hipStream_t>(stream),
                                     reinterpret_cast<const uint8_t*>(packed),
                                     reinterpret_cast<const uint32_t*>(tab),
                                     reinterpret_cast<uint8_t*>(text_out)),
              "ingest_crc_count");
        },
        py::arg("bytes"), py::arg("chunks"), py::arg("nchunks"), py::arg("tables"),
        py::arg("crc_out"), py::arg("nrec"), py::arg("ngroups"), py::arg("recs"),
        py::arg("groups"), py::arg("counts"), py::arg("gsum"), py::arg("stream"),
        py::arg("gbad") = 0, py::arg("packed") = 0, py::arg("tab") = 0, py::arg("text_out") = 0,
        "groups: int32 (record, first tile) pairs, GROUP_TILES tiles each; counts: per record "
        "tile0 + grp0 -> [tile counts][group sums]; gsum: one int per group");
  m.attr("GROUP_TILES") = gale::kGroupTiles;
  m.def("ingest_crc_b64",
        [](uintptr_t bytes, uintptr_t chunks, int nchunks, uintptr_t tables, uintptr_t crc_out,
           int images, uintptr_t imgs, int H, int W, int C, uintptr_t arena, uintptr_t wg_bad,
           uintptr_t stream, std::optional<std::vector<float>> a,
           std::optional<std::vector<float>> b, bool nchw) {
          // imgs: B64_IMAGE_BYTES-byte descriptors; wg_bad: one int per decode workgroup
          // (images * ceil(L / B64_CHUNK_CHARS)). a / b / nchw: as b64_decode_instances
          const auto prep = prep_from("ingest_crc_b64", a, b, nchw);
          chk(gale::ingest_crc_b64(static_cast<const uint8_t*>(P(bytes)),
                                   static_cast<const gale::CrcChunk*>(P(chunks)), nchunks,
                                   static_cast<const uint32_t*>(P(tables)),
                                   static_cast<uint32_t*>(P(crc_out)), images,
                                   static_cast<const gale::B64Image*>(P(imgs)), H, W, C,
                                   static_cast<float*>(P(arena)), static_cast<int*>(P(wg_bad)),
                                   S(stream), prep ? &*prep : nullptr),
              "ingest_crc_b64");
        },
        py::arg("bytes"), py::arg("chunks"), py::arg("nchunks"), py::arg("tables"),
        py::arg("crc_out"), py::arg("images"), py::arg("imgs"), py::arg("H"), py::arg("W"),
        py::arg("C"), py::arg("arena"), py::arg("wg_bad"), py::arg("stream"),
        py::arg("a") = py::none(), py::arg("b") = py::none(), py::arg("nchw") = false);
  m.attr("B64_CHUNK_CHARS") = gale::kB64ChunkChars;
  m.def("text_unpack", [](uintptr_t packed, uintptr_t tab, int64_t n, uintptr_t out,
                          uintptr_t stream) {
    if (out % 16 || packed % 8) throw std::invalid_argument("text_unpack: misaligned buffers");
    gale::check_hip(gale::text_unpack(reinterpret_cast<const uint8_t*>(packed),
                                      reinterpret_cast<const uint32_t*>(tab), n,
                                      reinterpret_cast<uint8_t*>(out),
                                      reinterpret_cast<hipStream_t>(stream)),
                    "text_unpack");
  });
  m.def("format_floats_java", [](int n, uintptr_t x, uintptr_t out16, uintptr_t stream) {
    gale::check_hip(gale::format_floats_java(n, reinterpret_cast<const float*>(x),
                                             reinterpret_cast<void*>(out16),
                                             reinterpret_cast<hipStream_t>(stream)),
                    "format_floats_java");
  });
  // the step's forms of the formatter: the value count is (*d_count) * per on the device
  // (max_n = the launch size); _step also hands the parse verdicts over (kernels.h)
  m.def("format_floats_java_dev",
        [](int max_n, uintptr_t d_count, int per, uintptr_t x, uintptr_t out16,
           uintptr_t stream) {
          chk(gale::format_floats_java_dev(max_n, static_cast<const int*>(P(d_count)), per,
                                           static_cast<const float*>(P(x)), P(out16), S(stream)),
              "format_floats_java_dev");
        },
        py::arg("max_n"), py::arg("d_count"), py::arg("per"), py::arg("x"), py::arg("out16"),
        py::arg("stream"));
  m.def("format_floats_java_step",
        [](int max_n, uintptr_t d_count, int per, uintptr_t x, uintptr_t out16, uintptr_t d_nrec,
           uintptr_t status, uintptr_t status_out, uintptr_t stream) {
          chk(gale::format_floats_java_step(max_n, static_cast<const int*>(P(d_count)), per,
                                            static_cast<const float*>(P(x)), P(out16),
                                            static_cast<const int*>(P(d_nrec)),
                                            static_cast<int*>(P(status)),
                                            static_cast<int*>(P(status_out)), S(stream)),
              "format_floats_java_step");
        },
        py::arg("max_n"), py::arg("d_count"), py::arg("per"), py::arg("x"), py::arg("out16"),
        py::arg("d_nrec"), py::arg("status"), py::arg("status_out"), py::arg("stream"));
  // the top-k selection + text kernel (topk.hip) in its three forms, as the formatter's
  m.def("topk_java",
        [](int rows, int classes, int k, uintptr_t x, uintptr_t text16, uintptr_t idx,
           uintptr_t stream) {
          chk(gale::topk_java(rows, classes, k, static_cast<const float*>(P(x)), P(text16),
                              static_cast<int32_t*>(P(idx)), S(stream)),
              "topk_java");
        },
        py::arg("rows"), py::arg("classes"), py::arg("k"), py::arg("x"), py::arg("text16"),
        py::arg("idx"), py::arg("stream"));
  m.def("topk_java_dev",
        [](int max_rows, uintptr_t d_rows, int classes, int k, uintptr_t x, uintptr_t text16,
           uintptr_t idx, uintptr_t stream) {
          chk(gale::topk_java_dev(max_rows, static_cast<const int*>(P(d_rows)), classes, k,
                                  static_cast<const float*>(P(x)), P(text16),
                                  static_cast<int32_t*>(P(idx)), S(stream)),
              "topk_java_dev");
        },
        py::arg("max_rows"), py::arg("d_rows"), py::arg("classes"), py::arg("k"), py::arg("x"),
        py::arg("text16"), py::arg("idx"), py::arg("stream"));
  m.def("topk_java_step",
        [](int max_rows, uintptr_t d_rows, int classes, int k, uintptr_t x, uintptr_t text16,
           uintptr_t idx, uintptr_t d_nrec, uintptr_t status, uintptr_t status_out,
           uintptr_t stream) {
          chk(gale::topk_java_step(max_rows, static_cast<const int*>(P(d_rows)), classes, k,
                                   static_cast<const float*>(P(x)), P(text16),
                                   static_cast<int32_t*>(P(idx)),
                                   static_cast<const int*>(P(d_nrec)),
                                   static_cast<int*>(P(status)),
                                   static_cast<int*>(P(status_out)), S(stream)),
              "topk_java_step");
        },
        py::arg("max_rows"), py::arg("d_rows"), py::arg("classes"), py::arg("k"), py::arg("x"),
        py::arg("text16"), py::arg("idx"), py::arg("d_nrec"), py::arg("status"),
        py::arg("status_out"), py::arg("stream"));
  // the input resize kernel (resize_crop.hip) in its two forms; tables: the six device pointers
  // (y0, y1, wy, x0, x1, wx) of the plan
  auto resize_plan = [](int HS, int WS, int H, int W, int C, const std::vector<uintptr_t>& t) {
    if (t.size() != 6) throw std::invalid_argument("resize_crop: six table pointers");
    gale::ResizePlan p;
    p.HS = HS, p.WS = WS, p.H = H, p.W = W, p.C = C;
    p.y0 = static_cast<const int32_t*>(P(t[0]));
    p.y1 = static_cast<const int32_t*>(P(t[1]));
    p.wy = static_cast<const float*>(P(t[2]));
    p.x0 = static_cast<const int32_t*>(P(t[3]));
    p.x1 = static_cast<const int32_t*>(P(t[4]));
    p.wx = static_cast<const float*>(P(t[5]));
    return p;
  };
  m.def("resize_crop",
        [resize_plan](int images, int HS, int WS, int H, int W, int C,
                      std::vector<uintptr_t> tables, uintptr_t src, uintptr_t dst,
                      uintptr_t stream) {
          chk(gale::resize_crop(images, resize_plan(HS, WS, H, W, C, tables),
                                static_cast<const float*>(P(src)), static_cast<float*>(P(dst)),
                                S(stream)),
              "resize_crop");
        },
        py::arg("images"), py::arg("HS"), py::arg("WS"), py::arg("H"), py::arg("W"), py::arg("C"),
        py::arg("tables"), py::arg("src"), py::arg("dst"), py::arg("stream"));
  m.def("resize_crop_dev",
        [resize_plan](int max_images, uintptr_t d_images, int HS, int WS, int H, int W, int C,
                      std::vector<uintptr_t> tables, uintptr_t src, uintptr_t dst,
                      uintptr_t stream) {
          chk(gale::resize_crop_dev(max_images, static_cast<const int*>(P(d_images)),
                                    resize_plan(HS, WS, H, W, C, tables),
                                    static_cast<const float*>(P(src)), static_cast<float*>(P(dst)),
                                    S(stream)),
              "resize_crop_dev");
        },
        py::arg("max_images"), py::arg("d_images"), py::arg("HS"), py::arg("WS"), py::arg("H"),
        py::arg("W"), py::arg("C"), py::arg("tables"), py::arg("src"), py::arg("dst"),
        py::arg("stream"));
  // the antialiased resize kernel (resize_crop_aa.hip) in its two forms; dims: (HS, WS, HR, WR, H,
  // W, C); tables: the six device pointers (ys, yn, wy, xs, xn, wx) in the kernel's layout;
  // launch: (ty, tx, band, band_rows) (build_resize_aa_tables(..., device=True) gives all)
  auto resize_aa_plan = [](const std::vector<int>& dims, const std::vector<uintptr_t>& t,
                           const std::vector<int>& launch) {
    if (dims.size() != 7 || t.size() != 6 || launch.size() != 4)
      throw std::invalid_argument("resize_crop_aa: seven dims, six table pointers, four figures");
    gale::ResizeAaPlan p;
    p.HS = dims[0], p.WS = dims[1], p.HR = dims[2], p.WR = dims[3], p.H = dims[4], p.W = dims[5];
    p.C = dims[6];
    p.ty = launch[0], p.tx = launch[1], p.band = launch[2], p.band_rows = launch[3];
    p.ys = static_cast<const int32_t*>(P(t[0]));
    p.yn = static_cast<const int32_t*>(P(t[1]));
    p.wy = static_cast<const float*>(P(t[2]));
    p.xs = static_cast<const int32_t*>(P(t[3]));
    p.xn = static_cast<const int32_t*>(P(t[4]));
    p.wx = static_cast<const float*>(P(t[5]));
    return p;
  };
  m.def("resize_crop_aa",
        [resize_aa_plan](int images, std::vector<int> dims, std::vector<uintptr_t> tables,
                         std::vector<int> launch, uintptr_t src, uintptr_t dst, uintptr_t stream) {
          chk(gale::resize_crop_aa(images, resize_aa_plan(dims, tables, launch),
                                   static_cast<const float*>(P(src)), static_cast<float*>(P(dst)),
                                   S(stream)),
              "resize_crop_aa");
        },
        py::arg("images"), py::arg("dims"), py::arg("tables"), py::arg("launch"), py::arg("src"),
        py::arg("dst"), py::arg("stream"));
  m.def("resize_crop_aa_dev",
        [resize_aa_plan](int max_images, uintptr_t d_images, std::vector<int> dims,
                         std::vector<uintptr_t> tables, std::vector<int> launch, uintptr_t src,
                         uintptr_t dst, uintptr_t stream) {
          chk(gale::resize_crop_aa_dev(max_images, static_cast<const int*>(P(d_images)),
                                       resize_aa_plan(dims, tables, launch),
                                       static_cast<const float*>(P(src)),
                                       static_cast<float*>(P(dst)), S(stream)),
              "resize_crop_aa_dev");
        },
        py::arg("max_images"), py::arg("d_images"), py::arg("dims"), py::arg("tables"),
        py::arg("launch"), py::arg("src"), py::arg("dst"), py::arg("stream"));
  m.attr("FLOAT_TEXT_SLOT") = gale::kFloatTextSlot;
  m.attr("INPUT_TABLE_IMAGES") = gale::kInputTableImages;
  m.attr("INPUT_TABLE_BASES") = gale::kInputTableBases;
  m.def("set_conv_path", &gale::set_conv_path);
  m.def("set_conv_patch", &gale::set_conv_patch);
  m.def("conv_patch_supported", [](py::dict desc, int batch, bool has_res) {
    return gale::conv_patch_supported(desc_from_dict(desc), batch, has_res);
  });
  // the launch of the MFMA conv kernel for this layer and batch (host only, no HIP call)
  auto mfma_dict = [](const gale::ConvMfmaPlan& p) {
    static const char* const kModes[] = {"fast", "gather", "1x1"};
    py::dict r;
    r["ok"] = p.ok;
    r["mode"] = kModes[p.mode];
    r["nt"] = p.nt;
    r["pr"] = p.pr;
    r["n_blocks"] = p.n_blocks;
    r["bk"] = p.bk;
    r["nkc"] = p.nkc;
    r["m_tiles"] = p.m_tiles;
    r["grid_m"] = p.grid_m;
    r["lds_bytes"] = p.lds_bytes;
    return r;
  };
  m.def("conv_mfma_plan", [mfma_dict](py::dict desc, int batch, bool has_res) {
    return mfma_dict(gale::conv_mfma_plan(desc_from_dict(desc), batch, has_res));
  }, py::arg("desc"), py::arg("batch"), py::arg("has_res"));
  // the launch conv2d() makes for this layer and batch under the process policy: "kernel"
  // ("none" / "f32" / "gemm" / "patch" / "mfma"), "refusal" (None unless "none") and the chosen
  // kernel's plan fields (host only, no HIP call)
  m.def("conv_route", [mfma_dict](py::dict desc, int batch, bool has_res) {
    const gale::ConvRoute t = gale::conv_route(desc_from_dict(desc), batch, has_res);
    py::dict r;
    switch (t.kernel) {
      case gale::CONV_F32:
        r["M"] = t.f32.M, r["grid_m"] = t.f32.grid_m, r["grid_n"] = t.f32.grid_n;
        break;
      case gale::CONV_GEMM: {
        const gale::ConvGemmPlan& p = t.gemm;
        r["bn"] = p.bn, r["stages"] = p.stages, r["stem"] = p.stem, r["M"] = p.M;
        r["m_tiles"] = p.m_tiles, r["n_tiles"] = p.n_tiles, r["nwg"] = p.nwg;
        r["nkb"] = p.nkb, r["cin_blocks"] = p.cin_blocks;
        break;
      }
      case gale::CONV_PATCH: {
        const gale::ConvPatchPlan& p = t.patch;
        r["bn"] = p.bn, r["prr"] = p.prr, r["TR"] = p.TR, r["IMG"] = p.IMG, r["P"] = p.P;
        r["PW"] = p.PW, r["PR1"] = p.PR1, r["PR"] = p.PR, r["rblocks"] = p.rblocks;
        r["nsteps"] = p.nsteps, r["batch"] = p.batch, r["n_tiles"] = p.n_tiles;
        r["nwg"] = p.nwg;
        break;
      }
      case gale::CONV_MFMA:
        r = mfma_dict(t.mfma);
        r["M"] = t.mfma.M, r["cin_shift"] = t.mfma.cin_shift, r["kw_magic"] = t.mfma.kw_magic;
        break;
      default: break;
    }
    r["kernel"] = gale::conv_kernel_name(t.kernel);
    r["refusal"] = t.refusal ? py::object(py::str(t.refusal)) : py::object(py::none());
    return r;
  }, py::arg("desc"), py::arg("batch"), py::arg("has_res"));
  m.def("device_pci_bus_id", [](int device) {
    char buf[64] = {0};
    chk(hipDeviceGetPCIBusId(buf, (int)sizeof(buf), device), "hipDeviceGetPCIBusId");
    return std::string(buf);
  });
  m.def("conv_path", &gale::conv_path);
  m.attr("JSON_TILE_BYTES") = gale::kJsonTileBytes;
  m.attr("JSON_RECORD_BYTES") = (int)sizeof(gale::JsonRecord);
  m.def("memcpy_async",
        [](uintptr_t dst, uintptr_t src, size_t n, uintptr_t stream) {
          chk(hipMemcpyAsync(P(dst), P(src), n, hipMemcpyDefault, S(stream)), "memcpy_async");
        });
  m.def("stream_sync", [](uintptr_t stream) {
    py::gil_scoped_release nogil;
    chk(hipStreamSynchronize(S(stream)), "stream_sync");
  });

  py::class_<gale::Executor, std::shared_ptr<gale::Executor>>(m, "Executor")
      .def(py::init([](int device, py::list ops, std::vector<long long> buf_bytes, int max_batch,
                       int slots, std::vector<int> buckets, int chunk_ops, int chunk_images) {
             // a plan that does not parse or validate is a ValueError before any HIP call
             return std::make_shared<gale::Executor>(
                 device, gale::plan_spec_from_py(ops, std::move(buf_bytes), max_batch, slots,
                                                 std::move(buckets), chunk_ops, chunk_images));
           }),
           py::arg("device"), py::arg("ops"), py::arg("buf_bytes"), py::arg("max_batch"),
           py::arg("slots") = 2, py::arg("buckets") = std::vector<int>{}, py::arg("chunk_ops") = 0,
           py::arg("chunk_images") = 0)
      .def("run",
           [](gale::Executor& e, int slot, int batch, uintptr_t stream, bool use_graph) {
             py::gil_scoped_release nogil;
             e.run(slot, batch, S(stream), use_graph);
           },
           py::arg("slot"), py::arg("batch"), py::arg("stream"), py::arg("use_graph") = true)
      .def("run_on",
           [](gale::Executor& e, int batch, uintptr_t in, uintptr_t out, uintptr_t stream) {
             py::gil_scoped_release nogil;
             e.run_on(batch, P(in), P(out), S(stream));
           })
      .def("capture_all",
           [](gale::Executor& e, uintptr_t stream) {
             py::gil_scoped_release nogil;
             e.capture_all(S(stream));
           })
      // the serving forms of the whole-network plans (tests): raw addresses as everywhere else.
      // A StepOut is passed only when text or status_out is non-zero
      .def("launch_device_batch",
           [](gale::Executor& e, int slot, uintptr_t d_batch, uintptr_t stream, uintptr_t text,
              uintptr_t status, uintptr_t status_out, uintptr_t nrec, uintptr_t xs) {
             if (status_out && (!status || !nrec))
               throw py::value_error("launch_device_batch: status_out needs status and nrec");
             gale::StepOut so;
             so.text = P(text);
             so.status = static_cast<int*>(P(status));
             so.status_out = static_cast<int*>(P(status_out));
             so.nrec = static_cast<const int*>(P(nrec));
             py::gil_scoped_release nogil;
             e.launch_device_batch(slot, static_cast<const int*>(P(d_batch)), S(stream),
                                   text || status_out ? &so : nullptr,
                                   static_cast<const float* const*>(P(xs)));
           },
           py::arg("slot"), py::arg("d_batch"), py::arg("stream"), py::arg("text") = 0,
           py::arg("status") = 0, py::arg("status_out") = 0, py::arg("nrec") = 0,
           py::arg("xs") = 0)
      .def("launch_table",
           [](gale::Executor& e, int slot, int batch, std::vector<uintptr_t> bases,
              std::vector<uint32_t> codes, uintptr_t stream, uintptr_t text) {
             if (bases.size() > (size_t)gale::kInputTableBases ||
                 codes.size() > (size_t)gale::kInputTableImages)
               throw py::value_error("launch_table: too many bases / codes for an InputTable");
             gale::InputTable tab{};
             for (size_t i = 0; i < bases.size(); ++i)
               tab.base[i] = static_cast<const float*>(P(bases[i]));
             for (size_t i = 0; i < codes.size(); ++i) tab.code[i] = codes[i];
             gale::StepOut so;
             so.text = P(text);
             py::gil_scoped_release nogil;
             e.launch_table(slot, batch, tab, S(stream), text ? &so : nullptr);
           },
           py::arg("slot"), py::arg("batch"), py::arg("bases"), py::arg("codes"),
           py::arg("stream"), py::arg("text") = 0)
      .def("input_ptr", [](gale::Executor& e, int slot) { return (uintptr_t)e.input(slot); })
      .def("output_ptr", [](gale::Executor& e, int slot) { return (uintptr_t)e.output(slot); })
      .def("bucket_for", &gale::Executor::bucket_for)
      .def_property_readonly("buckets", &gale::Executor::buckets)
      .def_property_readonly("max_batch", &gale::Executor::max_batch)
      .def_property_readonly("slots", &gale::Executor::slots)
      .def_property_readonly("device", &gale::Executor::device)
      .def_property_readonly("graphs_captured", &gale::Executor::graphs_captured)
      .def_property_readonly("graph_pays", &gale::Executor::graph_pays)
      .def_property_readonly("step_out_ok", &gale::Executor::step_out_ok);

  gale::bind_host(m);
}
