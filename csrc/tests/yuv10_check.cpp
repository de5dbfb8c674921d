// Sanitizer run of the 10-bit YUV 4:2:0 host codec (csrc/codec/yuv.h: yuv420p10_to_rgb_host,
// yuv10_coeffs; csrc/codec/json_codec.h: parse_instances_raw_yuv420p10_host and the raw length
// scan / splitter under it; csrc/codec/pixel_source.h: the rules for p010le / yuv420p10le) on
// untrusted input. A fixed seed, valid raw records of several frame sizes in both formats and a
// few thousand mutated and truncated copies. Every input lives in a heap block of exactly its
// size, so AddressSanitizer sees any access past n. Checks that every status is one of the
// format's verdicts, that scan, splitter, parser and PixelSource::parse_host agree, that a valid
// record decodes to the conversion of its frames, that the six ignored bits of a word change
// nothing, and that the two layouts of the same samples give the same image. Host only, no HIP
// call.
//   build/asan/yuv10_check [iterations]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <random>
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

struct Size {
  int HS, WS;
};

template <class F>
std::string refusal(F f) {
  try {
    f();
  } catch (const std::invalid_argument& e) {
    return e.what();
  }
  return "";
}

// One frame of 10-bit samples y[hw], u[hw/4], v[hw/4] in `format`, `junk` in the ignored bits.
std::vector<uint8_t> pack(const std::vector<uint16_t>& y, const std::vector<uint16_t>& u,
                          const std::vector<uint16_t>& v, int format, uint16_t junk) {
  std::vector<uint16_t> w(y);
  if (format == YUV_P010LE) {
    for (size_t i = 0; i < u.size(); ++i) w.push_back(u[i]), w.push_back(v[i]);
  } else {
    w.insert(w.end(), u.begin(), u.end());
    w.insert(w.end(), v.begin(), v.end());
  }
  std::vector<uint8_t> f;
  for (uint16_t s : w) {
    const uint16_t x = format == YUV_P010LE ? (uint16_t)(s << 6 | (junk & 63))
                                            : (uint16_t)(s | (junk & 0xFC00));
    f.push_back((uint8_t)(x & 255)), f.push_back((uint8_t)(x >> 8));
  }
  return f;
}

// Runs scan, splitter, parser and PixelSource::parse_host on an exact-size heap copy of `s`;
// returns the parser's status.
int run(const std::string& s, const Size& sz, const PixelSource& src, std::vector<float>* decoded) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[s.size() ? s.size() : 1]);
  memcpy(buf.get(), s.data(), s.size());
  const uint8_t* p = buf.get();
  const size_t n = s.size();
  const int64_t B = yuv420p10_bytes(sz.HS, sz.WS);
  CHECK(src.bytes(sz.HS, sz.WS, 3) == B, "PixelSource::bytes");
  const codec::Scan sc = codec::scan_instances_raw(n, B);
  CHECK(sc.status == codec::OK || sc.status == codec::EMPTY || sc.status == codec::BAD_SHAPE,
        "scan status %d", sc.status);
  std::vector<float> out;
  const size_t per = (size_t)sz.HS * sz.WS * 3;
  if (sc.status == codec::OK) {
    CHECK(sc.images > 0 && (int64_t)n == sc.images * B, "scan accepted %d images", sc.images);
    out.assign((size_t)sc.images * per, -1.f);
    std::vector<std::pair<uint32_t, uint32_t>> spans;
    // fragments of at most 2 frames: whole frames, in order, covering the value
    CHECK(codec::split_instances_raw(n, B, 2, spans), "raw split");
    size_t at = 0;
    for (const auto& sp : spans) {
      CHECK(sp.first == at && sp.second > sp.first && (sp.second - sp.first) % B == 0 &&
                (sp.second - sp.first) <= 2 * B, "raw fragment");
      at = sp.second;
    }
    CHECK(at == n, "raw fragments do not cover the value");
  }
  int images = -1;
  const int st = codec::parse_instances_raw_yuv420p10_host(
      p, n, sz.HS, sz.WS, src.yuv_format(), src.yuv(), out.empty() ? nullptr : out.data(), -1,
      &images);
  CHECK(st == sc.status, "parser %d != scan %d", st, sc.status);
  if (st == codec::OK) {
    CHECK(images == sc.images, "image count");
    for (float v : out) CHECK(v >= 0.f && v <= 255.f && 4.f * v == (float)(int)(4.f * v), "value %g", v);
    std::vector<float> out2(out.size(), -2.f);
    int im = -1;
    CHECK(src.parse_host(p, n, sz.HS, sz.WS, 3, out2.data(), -1, &im) == codec::OK &&
              im == images && out2 == out, "PixelSource::parse_host");
    if (images > 1)
      CHECK(src.parse_host(p, n, sz.HS, sz.WS, 3, nullptr, images - 1, &im) == codec::TOO_LARGE,
            "max_images");
  } else {
    CHECK(images == 0, "images reported for a bad record");
  }
  if (decoded) *decoded = out;
  return st;
}

}  // namespace

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 4000;
  std::mt19937 rng(20261126u);
  const Size sizes[] = {{2, 2}, {2, 10}, {4, 8}, {6, 18}, {2, 34}, {8, 6}};
  const std::string bt709 = "bt709", full = "full";
  const char* const names[] = {"p010le", "yuv420p10le"};
  YuvCoeffs k0;
  CHECK(yuv10_coeffs(YUV_BT601, YUV_LIMITED, &k0) && k0.yo == 64 && k0.cy == 305236, "table");
  CHECK(!yuv10_coeffs(2, 0, &k0) && !yuv10_coeffs(0, -1, &k0), "table range");
  {  // refusals of the twin and the parser; the byte count
    uint8_t frame[24] = {0};
    uint16_t q[24];
    CHECK(yuv420p10_bytes(2, 4) == 24 && yuv420p10_bytes(6, 18) == 324, "bytes");
    CHECK(!codec::yuv420p10_to_rgb_host(frame, 1, 4, YUV_P010LE, k0, q, nullptr), "odd HS");
    CHECK(!codec::yuv420p10_to_rgb_host(frame, 2, 3, YUV_P010LE, k0, q, nullptr), "odd WS");
    CHECK(!codec::yuv420p10_to_rgb_host(frame, 0, 2, YUV_YUV420P10LE, k0, q, nullptr), "HS 0");
    CHECK(!codec::yuv420p10_to_rgb_host(frame, 2, 2, YUV_NV12, k0, q, nullptr), "format");
    CHECK(codec::yuv420p10_to_rgb_host(frame, 2, 4, YUV_YUV420P10LE, k0, q, nullptr), "2x4");
    int im = -1;
    const auto parse = codec::parse_instances_raw_yuv420p10_host;
    CHECK(parse(frame, 24, 2, 3, YUV_P010LE, k0, nullptr, -1, &im) == codec::BAD_SHAPE, "WS 3");
    CHECK(parse(frame, 24, 2, 4, YUV_I420, k0, nullptr, -1, &im) == codec::BAD_SHAPE, "fmt");
    CHECK(parse(frame, 24, -2, 4, YUV_P010LE, k0, nullptr, -1, &im) == codec::BAD_SHAPE, "HS");
    CHECK(parse(frame, 24, 2, 4, YUV_P010LE, k0, nullptr, -1, &im) == codec::OK && im == 1, "2x4");
    CHECK(parse(frame, 23, 2, 4, YUV_P010LE, k0, nullptr, -1, &im) == codec::BAD_SHAPE, "23 of 24");
    CHECK(parse(frame, 0, 2, 4, YUV_P010LE, k0, nullptr, -1, &im) == codec::EMPTY, "0 bytes");
  }
  for (const char* nm : names) {  // PixelSource's rules for the two names, by their text
    const PixelSource b64 = PixelSource::from_names(nm, nullptr, nullptr);
    const PixelSource raw = b64.as_raw();
    const std::string what = "pixel_format p010le / yuv420p10le";
    CHECK(raw.kind() == PixelSource::YUV && raw.hi420() && !raw.yuv422() && !raw.planar() &&
              !raw.wants_ingest_decode(), "%s: kind", nm);
    CHECK(memcmp(&raw.yuv(), &k0, sizeof(k0)) == 0, "%s: default table", nm);
    YuvCoeffs want;
    yuv10_coeffs(YUV_BT709, YUV_FULL, &want);
    CHECK(memcmp(&PixelSource::from_names(nm, &bt709, &full).yuv(), &want, sizeof(want)) == 0,
          "%s: named table", nm);
    CHECK(refusal([&] { raw.check(3, false, 32, 32, true); }).empty(), "%s: accepted", nm);
    CHECK(refusal([&] { b64.check(3, false, 32, 32, true); }) == what + " needs input_format raw",
          "%s: b64", nm);
    CHECK(refusal([&] { b64.check(3, false, 32, 32, false); }) == what + " needs input_format raw",
          "%s: json", nm);
    CHECK(refusal([&] { raw.check(3, true, 32, 32, true); }) == what + ": no nchw layout",
          "%s: nchw", nm);
    CHECK(refusal([&] { raw.check(1, false, 32, 32, true); }) == what + " needs a 3-channel model",
          "%s: C", nm);
    for (const Size& odd : {Size{33, 32}, Size{32, 33}})
      CHECK(refusal([&] { raw.check(3, false, odd.HS, odd.WS, true); }) ==
                what + " needs even record-side H, W", "%s: odd", nm);
    CHECK(refusal([&] { raw.with_elem("f16"); }) == "input_dtype f16 needs pixel_format rgb",
          "%s: dtype", nm);
    int im = -1;
    uint8_t frame[12] = {0};
    CHECK(b64.parse_host(frame, 12, 2, 2, 3, nullptr, -1, &im) == codec::BAD_SHAPE, "%s: b64 parse", nm);
  }
  int ok = 0, bad = 0;
  for (int it = 0; it < iters; ++it) {
    const int fi = (int)(rng() % 2), format = fi ? YUV_YUV420P10LE : YUV_P010LE;
    const Size& sz = sizes[rng() % 6];
    const size_t hw = (size_t)sz.HS * sz.WS;
    const std::string ym = rng() % 2 ? "bt709" : "bt601", yr = rng() % 2 ? "full" : "limited";
    const PixelSource src = PixelSource::from_names(names[fi], &ym, &yr).as_raw();
    const int images = 1 + (int)(rng() % 4);
    std::string s, other;  // other: the same samples in the other layout, no junk
    std::vector<float> want;
    for (int i = 0; i < images; ++i) {
      std::vector<uint16_t> y(hw), u(hw / 4), v(hw / 4);
      for (auto* pl : {&y, &u, &v})
        for (uint16_t& x : *pl) x = rng() % 4 ? (uint16_t)(rng() % 1024) : (rng() % 2 ? 1023 : 0);
      const std::vector<uint8_t> f = pack(y, u, v, format, (uint16_t)rng());
      const std::vector<uint8_t> g = pack(y, u, v, fi ? YUV_P010LE : YUV_YUV420P10LE, 0);
      s.append(reinterpret_cast<const char*>(f.data()), f.size());
      other.append(reinterpret_cast<const char*>(g.data()), g.size());
      std::vector<float> fl(hw * 3);
      std::vector<uint16_t> q(hw * 3);
      CHECK(codec::yuv420p10_to_rgb_host(f.data(), sz.HS, sz.WS, format, src.yuv(), q.data(),
                                         fl.data()), "conversion refused");
      for (size_t e = 0; e < fl.size(); ++e)
        CHECK(q[e] <= 1020 && fl[e] == (float)q[e] * 0.25f, "float != q / 4");
      want.insert(want.end(), fl.begin(), fl.end());
    }
    if (it % 8 == 0) {  // the valid record decodes to the conversion of its frames
      std::vector<float> got, got2;
      CHECK(run(s, sz, src, &got) == codec::OK, "valid record rejected");
      CHECK(got == want, "decoded frames differ from the conversion twin");
      const PixelSource src2 = PixelSource::from_names(names[1 - fi], &ym, &yr).as_raw();
      CHECK(run(other, sz, src2, &got2) == codec::OK && got2 == want,
            "the other layout of the same samples, ignored bits cleared, differs");
      ++ok;
      continue;
    }
    switch (rng() % 4) {  // (every byte pattern of a whole length is a frame: lengths matter)
      case 0: s.resize(rng() % (s.size() + 1)); break;           // truncated
      case 1: s.append(1 + rng() % 5, (char)rng()); break;       // extended
      case 2: s[rng() % s.size()] = (char)rng(); break;          // mutated, still whole
      default: s.erase(rng() % s.size(), 1 + rng() % 3); break;
    }
    run(s, sz, src, nullptr) == codec::OK ? ++ok : ++bad;
  }
  printf("yuv10_check: %d records accepted, %d rejected, %d failures\n", ok, bad, failures);
  if (failures || ok == 0 || bad == 0) return 1;
  printf("all checks passed\n");
  return 0;
}
