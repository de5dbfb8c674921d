// Sanitizer run of PixelSource (csrc/codec/pixel_source.h), the one holder of what a b64 string
// carries, for all seven configuration names: the bytes of a string against H*W*C, yuv420_bytes
// and packed_bytes; every refusal of check() and of the names, by its text; the dimensions a
// string presents to the ingest's plan; and parse_host against the source's public parser
// (status, image count, floats) on valid records and a few hundred mutated and truncated ones per
// name - the mutation scheme of pixfmt_check.cpp, every input in a heap block of exactly its
// size. Host only, no HIP call.
//   build/asan/pixel_source_check [records per name]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../codec/pixel_source.h"

using namespace gale;

namespace {

int failures = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      ++failures;                             \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);           \
      fprintf(stderr, "\n");                  \
    }                                         \
  } while (0)

std::string b64(const std::vector<uint8_t>& v) {  // (any size: '=' padded)
  static const char kA[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  std::string s;
  for (size_t i = 0; i < v.size(); i += 3) {
    const size_t left = v.size() - i;
    const uint32_t x = ((uint32_t)v[i] << 16) | ((uint32_t)(left > 1 ? v[i + 1] : 0) << 8) |
                       (uint32_t)(left > 2 ? v[i + 2] : 0);
    s += kA[(x >> 18) & 63];
    s += kA[(x >> 12) & 63];
    s += left > 1 ? kA[(x >> 6) & 63] : '=';
    s += left > 2 ? kA[x & 63] : '=';
  }
  return s;
}

std::string record(const std::vector<std::vector<uint8_t>>& images, bool spaces) {
  const char* ws = spaces ? " \n" : "";
  std::string s = std::string(ws) + "{" + ws + "\"instances\"" + ws + ":" + ws + "[";
  for (size_t i = 0; i < images.size(); ++i) {
    if (i) s += std::string(ws) + ",";
    s += std::string(ws) + "{" + ws + "\"b64\"" + ws + ":" + ws + "\"" + b64(images[i]) + "\"" +
         ws + "}";
  }
  return s + ws + "]" + ws + "}" + ws;
}

struct Name {
  const char* name;
  PixelSource::Kind kind;
  int yuv, packed;
};
const Name kNames[] = {
    {"rgb", PixelSource::RGB, YUV_NONE, PACKED_NONE},
    {"i420", PixelSource::YUV, YUV_I420, PACKED_NONE},
    {"nv12", PixelSource::YUV, YUV_NV12, PACKED_NONE},
    {"bgr24", PixelSource::PACKED, YUV_NONE, PACKED_BGR24},
    {"rgba", PixelSource::PACKED, YUV_NONE, PACKED_RGBA},
    {"bgra", PixelSource::PACKED, YUV_NONE, PACKED_BGRA},
    {"gray", PixelSource::PACKED, YUV_NONE, PACKED_GRAY},
};
struct Size {
  int HS, WS;
};
const Size kSizes[] = {{1, 1}, {2, 2}, {5, 7}, {6, 10}, {32, 32}};

// what f() throws as std::invalid_argument ("" when it does not throw)
template <typename F>
std::string refusal(F f) {
  try {
    f();
  } catch (const std::invalid_argument& e) {
    return e.what();
  }
  return "";
}

// The source's public parser, called directly.
int parse_public(const Name& nm, const YuvCoeffs& k, const uint8_t* p, size_t n, int HS, int WS,
                 int C, float* out, int max_images, int* images) {
  return nm.kind == PixelSource::PACKED
             ? codec::parse_instances_packed_host(p, n, HS, WS, nm.packed, out, max_images, images)
         : nm.kind == PixelSource::YUV
             ? codec::parse_instances_yuv_host(p, n, HS, WS, nm.yuv, k, out, max_images, images)
             : codec::parse_instances_b64_host(p, n, HS, WS, C, out, max_images, images);
}

// parse_host and the public parser on an exact-size heap copy of `s`; returns the status.
int compare(const PixelSource& src, const Name& nm, const std::string& s, const Size& sz, int C,
            int max_images) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[s.size() ? s.size() : 1]);
  memcpy(buf.get(), s.data(), s.size());
  const size_t per = (size_t)sz.HS * sz.WS * (size_t)C;
  // (room for every image a record of this length could hold)
  const size_t cap = s.size() / 4 + 1;
  std::vector<float> a(cap * per, -1.f), b(cap * per, -1.f);
  int ia = -1, ib = -1;
  const int sa = src.parse_host(buf.get(), s.size(), sz.HS, sz.WS, C, a.data(), max_images, &ia);
  const int sb = parse_public(nm, src.yuv(), buf.get(), s.size(), sz.HS, sz.WS, C, b.data(),
                              max_images, &ib);
  CHECK(sa == sb && ia == ib, "%s: parse_host %d (%d images) != public parser %d (%d)", nm.name,
        sa, ia, sb, ib);
  CHECK(a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0,
        "%s: floats differ", nm.name);
  // validate-only (no output): the same verdict
  int iv = -1;
  const int sv = src.parse_host(buf.get(), s.size(), sz.HS, sz.WS, C, nullptr, max_images, &iv);
  CHECK(sv == sa && iv == ia, "%s: validate-only %d (%d) != %d (%d)", nm.name, sv, iv, sa, ia);
  return sa;
}

}  // namespace

int main(int argc, char** argv) {
  const int per_name = argc > 1 ? atoi(argv[1]) : 400;
  std::mt19937 rng(20261021u);
  const std::string bt709 = "bt709", full = "full", bt601 = "bt601", limited = "limited";
  int ok = 0, bad = 0;

  // ---- names -----------------------------------------------------------------------------------
  CHECK(PixelSource().kind() == PixelSource::RGB && PixelSource().wants_ingest_decode(),
        "default source is not rgb");
  for (const Name& nm : kNames) {
    const PixelSource s = PixelSource::from_names(nm.name, nullptr, nullptr);
    CHECK(s.kind() == nm.kind && s.yuv_format() == nm.yuv && s.packed_format() == nm.packed,
          "%s: kind / formats", nm.name);
    CHECK(s.wants_ingest_decode() == (nm.kind == PixelSource::RGB), "%s: ingest decode", nm.name);
    YuvCoeffs d;  // (bt601, limited)
    CHECK(memcmp(&s.yuv(), &d, sizeof(d)) == 0, "%s: default coefficients", nm.name);
  }
  {
    YuvCoeffs want;
    CHECK(yuv_coeffs(YUV_BT709, YUV_FULL, &want), "table");
    const PixelSource s = PixelSource::from_names("nv12", &bt709, &full);
    CHECK(memcmp(&s.yuv(), &want, sizeof(want)) == 0, "bt709 / full coefficients");
    const PixelSource t = PixelSource::from_names("i420", &bt601, &limited);
    YuvCoeffs d;
    CHECK(memcmp(&t.yuv(), &d, sizeof(d)) == 0, "bt601 / limited coefficients");
  }
  for (const char* t : {"", "RGB", "yuv", "argb", "i42", "nv21", "grey", "bgr"})
    CHECK(refusal([&] { PixelSource::from_names(t, nullptr, nullptr); }) ==
              "pixel_format: rgb, i420, nv12, bgr24, rgba, bgra or gray",
          "name %s", t);
  for (const char* t : {"bgr24", "rgba", "bgra", "gray"}) {
    const char* want = "yuv_matrix / yuv_range need pixel_format i420 or nv12";
    CHECK(refusal([&] { PixelSource::from_names(t, &bt601, nullptr); }) == want, "%s matrix", t);
    CHECK(refusal([&] { PixelSource::from_names(t, nullptr, &limited); }) == want, "%s range", t);
  }
  for (const char* t : {"rgb", "i420", "nv12"}) {
    const char* want = "yuv_matrix: bt601 or bt709; yuv_range: limited or full";
    const std::string junk = "bt2020", junk2 = "tv";
    CHECK(refusal([&] { PixelSource::from_names(t, &junk, nullptr); }) == want, "%s matrix", t);
    CHECK(refusal([&] { PixelSource::from_names(t, nullptr, &junk2); }) == want, "%s range", t);
    CHECK(refusal([&] { PixelSource::from_names(t, &bt709, &full); }).empty(), "%s named", t);
  }

  // ---- bytes, ingest dimensions, check ---------------------------------------------------------
  for (const Name& nm : kNames) {
    const PixelSource s = PixelSource::from_names(nm.name, nullptr, nullptr);
    for (const Size& sz : kSizes) {
      const bool odd = (sz.HS | sz.WS) & 1;
      if (nm.kind == PixelSource::YUV && odd) continue;
      for (int C : {1, 3, 4}) {
        const int64_t want = nm.kind == PixelSource::PACKED ? packed_bytes(sz.HS, sz.WS, nm.packed)
                             : nm.kind == PixelSource::YUV  ? yuv420_bytes(sz.HS, sz.WS)
                                                            : (int64_t)sz.HS * sz.WS * C;
        CHECK(s.bytes(sz.HS, sz.WS, C) == want, "%s %dx%dx%d: bytes", nm.name, sz.HS, sz.WS, C);
        const PixelSource::Dims d = s.ingest_dims(sz.HS, sz.WS, C);
        const PixelSource::Dims w = nm.kind == PixelSource::PACKED
                                        ? PixelSource::Dims{sz.HS, sz.WS, packed_bpp(nm.packed)}
                                    : nm.kind == PixelSource::YUV
                                        ? PixelSource::Dims{sz.HS / 2, sz.WS, 3}
                                        : PixelSource::Dims{sz.HS, sz.WS, C};
        CHECK(d.H == w.H && d.W == w.W && d.C == w.C, "%s %dx%dx%d: ingest dims", nm.name, sz.HS,
              sz.WS, C);
        // the plan's image of those dimensions is as long as the string
        CHECK((int64_t)d.H * d.W * d.C == want, "%s %dx%d: ingest dims' bytes", nm.name, sz.HS,
              sz.WS);
      }
    }
    // check(): rgb goes with everything; the others refuse in this order
    const std::string what = nm.kind == PixelSource::YUV
                                 ? "pixel_format i420 / nv12"
                                 : "pixel_format bgr24 / rgba / bgra / gray";
    if (nm.kind == PixelSource::RGB) {
      for (int C : {1, 3, 7})
        for (bool nchw : {false, true})
          for (bool b64 : {false, true})
            CHECK(refusal([&] { s.check(C, nchw, 5, 7, b64); }).empty(), "rgb refused");
      continue;
    }
    CHECK(refusal([&] { s.check(3, false, 6, 10, true); }).empty(), "%s: good topology", nm.name);
    CHECK(refusal([&] { s.check(1, true, 5, 7, false); }) == what + " needs input_format b64",
          "%s: json", nm.name);
    CHECK(refusal([&] { s.check(1, true, 5, 7, true); }) == what + ": no nchw layout",
          "%s: nchw", nm.name);
    for (int C : {1, 2, 4})
      CHECK(refusal([&] { s.check(C, false, 5, 7, true); }) == what + " needs a 3-channel model",
            "%s: C = %d", nm.name, C);
    for (const Size& sz : {Size{5, 8}, Size{6, 7}, Size{1, 1}}) {
      const std::string got = refusal([&] { s.check(3, false, sz.HS, sz.WS, true); });
      if (nm.kind == PixelSource::YUV)
        CHECK(got == what + " needs even record-side H, W", "%s: odd size", nm.name);
      else
        CHECK(got.empty(), "%s: odd size refused", nm.name);
    }
  }

  // ---- parse_host against the public parsers ---------------------------------------------------
  for (const Name& nm : kNames) {
    const PixelSource src = nm.kind == PixelSource::YUV
                                ? PixelSource::from_names(nm.name, &bt709, &full)
                                : PixelSource::from_names(nm.name, nullptr, nullptr);
    for (int it = 0; it < per_name; ++it) {
      Size sz = kSizes[rng() % 4];  // (32x32 is left to the byte counts: the records stay small)
      if (nm.kind == PixelSource::YUV && ((sz.HS | sz.WS) & 1))
        sz = it % 2 ? Size{2, 2} : Size{6, 10};
      const int C = nm.kind == PixelSource::RGB ? 1 + (int)(rng() % 4) : 3;
      const int images = 1 + (int)(rng() % 3);
      std::vector<std::vector<uint8_t>> strings;
      for (int i = 0; i < images; ++i) {
        std::vector<uint8_t> v((size_t)src.bytes(sz.HS, sz.WS, C));
        for (uint8_t& b : v) b = (uint8_t)rng();
        strings.push_back(v);
      }
      std::string s = record(strings, rng() % 2 != 0);
      if (it % 8 == 0) {
        CHECK(compare(src, nm, s, sz, C, -1) == codec::OK, "%s: valid record rejected", nm.name);
        if (images > 1)
          CHECK(compare(src, nm, s, sz, C, images - 1) == codec::TOO_LARGE, "%s: max_images",
                nm.name);
        // a refused shape reaches the parser's own pre-check
        compare(src, nm, s, Size{0, sz.WS}, C, -1);
        ++ok;
        continue;
      }
      const int muts = 1 + (int)(rng() % 3);
      for (int m = 0; m < muts && !s.empty(); ++m) {
        const size_t at = rng() % s.size();
        static const char kBytes[] = "{}[]\",:\\=-_ \nAb64/+nul\x80\xff\0";
        const char c = kBytes[rng() % (sizeof(kBytes) - 1)];
        switch (rng() % 5) {
          case 0: s[at] = c; break;
          case 1: s.erase(at, 1 + rng() % 3); break;
          case 2: s.insert(at, 1 + rng() % 3, c); break;
          case 3: s.resize(at); break;                         // truncated
          default: s[at] = (char)rng(); break;
        }
      }
      compare(src, nm, s, sz, C, -1) == codec::OK ? ++ok : ++bad;
    }
  }
  printf("pixel_source_check: %d records accepted, %d rejected, %d failures\n", ok, bad, failures);
  if (failures || ok == 0 || bad == 0) return 1;
  printf("pixel_source_check OK\n");
  return 0;
}
