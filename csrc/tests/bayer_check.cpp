// Sanitizer run of the Bayer mosaic host codec (csrc/codec/bayer.h: bayer_to_rgb_host;
// csrc/codec/json_codec.h: parse_instances_raw_bayer_host and the raw length scan / splitter under
// it; csrc/codec/pixel_source.h: the rules for the four bayer_*8 names) on untrusted input. A
// fixed seed, valid raw records of several frame sizes in all four orders and a few thousand
// mutated and truncated copies. Every input lives in a heap block of exactly its size, so
// AddressSanitizer sees any access past n. Checks that every status is one of the format's
// verdicts, that scan, splitter, parser and PixelSource::parse_host agree, that a valid record
// decodes to the twin's image of its frames, and that a mosaic sampled from a flat colour
// demosaics to that colour. Host only, no HIP call.
//   build/asan/bayer_check [iterations]
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

// Runs scan, splitter, parser and PixelSource::parse_host on an exact-size heap copy of `s`;
// returns the parser's status.
int run(const std::string& s, const Size& sz, const PixelSource& src, std::vector<float>* decoded) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[s.size() ? s.size() : 1]);
  memcpy(buf.get(), s.data(), s.size());
  const uint8_t* p = buf.get();
  const size_t n = s.size();
  const int64_t B = bayer_bytes(sz.HS, sz.WS);
  CHECK(src.bytes(sz.HS, sz.WS, 3) == B, "PixelSource::bytes");
  const codec::Scan sc = codec::scan_instances_raw(n, B);
  CHECK(sc.status == codec::OK || sc.status == codec::EMPTY || sc.status == codec::BAD_SHAPE,
        "scan status %d", sc.status);
  std::vector<float> out;
  if (sc.status == codec::OK) {
    CHECK(sc.images > 0 && (int64_t)n == sc.images * B, "scan accepted %d images", sc.images);
    out.assign((size_t)sc.images * (size_t)B * 3, -1.f);
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
  const int st = codec::parse_instances_raw_bayer_host(
      p, n, sz.HS, sz.WS, src.bayer_order(), out.empty() ? nullptr : out.data(), -1, &images);
  CHECK(st == sc.status, "parser %d != scan %d", st, sc.status);
  if (st == codec::OK) {
    CHECK(images == sc.images, "image count");
    for (float v : out) CHECK(v >= 0.f && v <= 255.f && v == (float)(int)v, "value %g", v);
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
  const Size sizes[] = {{2, 2}, {2, 10}, {4, 6}, {6, 18}, {2, 34}, {8, 6}};
  const char* const names[] = {"bayer_rggb8", "bayer_bggr8", "bayer_grbg8", "bayer_gbrg8"};
  {  // refusals of the twin and the parser; the byte count; the names
    uint8_t frame[8] = {0}, rgb[24];
    CHECK(bayer_bytes(2, 4) == 8 && bayer_bytes(6, 18) == 108 && !bayer_bytes(3, 4) &&
              !bayer_bytes(2, 5) && !bayer_bytes(0, 2) && !bayer_bytes(2, -2), "bytes");
    CHECK(!bayer_order_of("bayer_rggb") && !bayer_order_of("bayer_rggb16") &&
              !bayer_order_of("gray") && !bayer_order_of(""), "names");
    CHECK(!codec::bayer_to_rgb_host(frame, 1, 4, BAYER_RGGB, rgb, nullptr), "odd HS");
    CHECK(!codec::bayer_to_rgb_host(frame, 2, 3, BAYER_RGGB, rgb, nullptr), "odd WS");
    CHECK(!codec::bayer_to_rgb_host(frame, 2, 4, BAYER_NONE, rgb, nullptr), "order 0");
    CHECK(!codec::bayer_to_rgb_host(frame, 2, 4, 5, rgb, nullptr), "order 5");
    CHECK(codec::bayer_to_rgb_host(frame, 2, 4, BAYER_GBRG, rgb, nullptr), "2x4");
    int im = -1;
    const auto parse = codec::parse_instances_raw_bayer_host;
    CHECK(parse(frame, 8, 2, 3, BAYER_RGGB, nullptr, -1, &im) == codec::BAD_SHAPE, "WS 3");
    CHECK(parse(frame, 8, 2, 4, BAYER_NONE, nullptr, -1, &im) == codec::BAD_SHAPE, "order");
    CHECK(parse(frame, 8, -2, 4, BAYER_RGGB, nullptr, -1, &im) == codec::BAD_SHAPE, "HS");
    CHECK(parse(frame, 8, 2, 4, BAYER_RGGB, nullptr, -1, &im) == codec::OK && im == 1, "2x4");
    CHECK(parse(frame, 7, 2, 4, BAYER_RGGB, nullptr, -1, &im) == codec::BAD_SHAPE, "7 of 8");
    CHECK(parse(frame, 0, 2, 4, BAYER_RGGB, nullptr, -1, &im) == codec::EMPTY, "0 bytes");
  }
  for (int oi = 0; oi < 4; ++oi) {  // PixelSource's rules for the four names, by their text
    const char* nm = names[oi];
    const PixelSource b64 = PixelSource::from_names(nm, nullptr, nullptr);
    const PixelSource raw = b64.as_raw();
    const std::string what = "pixel_format bayer_rggb8 / bayer_bggr8 / bayer_grbg8 / bayer_gbrg8";
    const std::string bt709 = "bt709", full = "full";
    CHECK(raw.kind() == PixelSource::BAYER && raw.bayer_order() == oi + 1 && !raw.hi420() &&
              raw.yuv_format() == YUV_NONE && raw.packed_format() == PACKED_NONE &&
              !raw.wants_ingest_decode(), "%s: kind", nm);
    const PixelSource::Dims dm = raw.ingest_dims(6, 18, 3);
    CHECK(dm.H == 6 && dm.W == 18 && dm.C == 1, "%s: ingest_dims", nm);
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
    CHECK(refusal([&] { PixelSource::from_names(nm, &bt709, nullptr); }) ==
              "yuv_matrix / yuv_range need pixel_format i420 or nv12", "%s: matrix", nm);
    CHECK(refusal([&] { PixelSource::from_names(nm, nullptr, &full); }) ==
              "yuv_matrix / yuv_range need pixel_format i420 or nv12", "%s: range", nm);
    CHECK(!refusal([&] { raw.with_chroma("linear").check(3, false, 32, 32, true); }).empty(),
          "%s: chroma", nm);
    int im = -1;
    uint8_t frame[4] = {0};
    CHECK(b64.parse_host(frame, 4, 2, 2, 3, nullptr, -1, &im) == codec::BAD_SHAPE, "%s: b64 parse", nm);
    // a mosaic of a flat colour is that colour at every pixel, edges and corners included
    const uint8_t flat[3] = {(uint8_t)rng(), (uint8_t)rng(), (uint8_t)rng()};
    const int gf = bayer_green_first(oi + 1), bf = bayer_blue_first(oi + 1);
    std::vector<uint8_t> mosaic(6 * 10), rgb(6 * 10 * 3);
    for (int y = 0; y < 6; ++y)
      for (int x = 0; x < 10; ++x)
        mosaic[y * 10 + x] = ((x + y) & 1) != gf ? flat[1] : flat[(y & 1) != bf ? 2 : 0];
    CHECK(codec::bayer_to_rgb_host(mosaic.data(), 6, 10, oi + 1, rgb.data(), nullptr), "flat");
    for (size_t e = 0; e < rgb.size(); ++e) CHECK(rgb[e] == flat[e % 3], "%s: flat colour", nm);
  }
  int ok = 0, bad = 0;
  for (int it = 0; it < iters; ++it) {
    const int order = 1 + (int)(rng() % 4);
    const Size& sz = sizes[rng() % 6];
    const size_t hw = (size_t)sz.HS * sz.WS;
    const PixelSource src = PixelSource::from_names(names[order - 1], nullptr, nullptr).as_raw();
    const int images = 1 + (int)(rng() % 4);
    std::string s;
    std::vector<float> want;
    for (int i = 0; i < images; ++i) {
      std::unique_ptr<uint8_t[]> f(new uint8_t[hw]);  // (exactly a frame: the twin's own reads)
      for (size_t e = 0; e < hw; ++e) f[e] = rng() % 4 ? (uint8_t)rng() : (rng() % 2 ? 255 : 0);
      s.append(reinterpret_cast<const char*>(f.get()), hw);
      std::vector<float> fl(hw * 3);
      std::vector<uint8_t> u8(hw * 3);
      CHECK(codec::bayer_to_rgb_host(f.get(), sz.HS, sz.WS, order, u8.data(), fl.data()),
            "demosaic refused");
      for (size_t e = 0; e < fl.size(); ++e) CHECK(fl[e] == (float)u8[e], "float != byte");
      // a site keeps its own sample
      for (size_t e = 0; e < hw; ++e) {
        const int y = (int)(e / sz.WS), x = (int)(e % sz.WS);
        const int c = ((x + y) & 1) != (int)bayer_green_first(order)
                          ? 1
                          : ((y & 1) != (int)bayer_blue_first(order) ? 2 : 0);
        CHECK(u8[3 * e + c] == f[e], "site (%d, %d) lost its sample", y, x);
      }
      want.insert(want.end(), fl.begin(), fl.end());
    }
    if (it % 8 == 0) {  // the valid record decodes to the twin's image of its frames
      std::vector<float> got;
      CHECK(run(s, sz, src, &got) == codec::OK, "valid record rejected");
      CHECK(got == want, "decoded frames differ from the twin");
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
  printf("bayer_check: %d records accepted, %d rejected, %d failures\n", ok, bad, failures);
  if (failures || ok == 0 || bad == 0) return 1;
  printf("all checks passed\n");
  return 0;
}
