// Sanitizer run of linear chroma for i420 / nv12 on the host (csrc/codec/yuv.h:
// yuv420_linear_to_rgb_host; csrc/codec/json_codec.h: parse_instances_yuv_host's linear form;
// csrc/codec/pixel_source.h: with_chroma, check, parse_host). A fixed seed, random frames of
// several sizes in both formats, each in a heap block of exactly its size so AddressSanitizer
// sees any access past it, and mutated and truncated records. Checks that the twin equals
// yuvp_to_rgb_host on (Y, U', V') with U', V' from a loop that follows libjpeg's
// h2v2_fancy_upsample (first, middle, last column), that constant chroma gives the nearest
// conversion, that PixelSource::parse_host and the parser agree on every record, and the
// refusals of yuv_chroma. Host only, no HIP call.
//   build/asan/yuv_chroma_check [iterations]
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

template <class F>
std::string refusal(F f) {
  try {
    f();
  } catch (const std::invalid_argument& e) {
    return e.what();
  }
  return "";
}

// libjpeg's loop on one plane c[ch][cw] -> out[2 ch][2 cw]
std::vector<uint8_t> fancy(const std::vector<uint8_t>& c, int ch, int cw) {
  std::vector<uint8_t> out((size_t)4 * ch * cw);
  for (int y = 0; y < 2 * ch; ++y) {
    const int r0 = y >> 1, r1 = (y & 1) ? (r0 + 1 < ch ? r0 + 1 : r0) : (r0 > 0 ? r0 - 1 : r0);
    std::vector<int> s(cw);
    for (int x = 0; x < cw; ++x) s[x] = 3 * c[(size_t)r0 * cw + x] + c[(size_t)r1 * cw + x];
    uint8_t* o = out.data() + (size_t)y * 2 * cw;
    if (cw == 1) {
      o[0] = (uint8_t)((4 * s[0] + 8) >> 4), o[1] = (uint8_t)((4 * s[0] + 7) >> 4);
      continue;
    }
    o[0] = (uint8_t)((4 * s[0] + 8) >> 4), o[1] = (uint8_t)((3 * s[0] + s[1] + 7) >> 4);
    for (int x = 1; x < cw - 1; ++x) {
      o[2 * x] = (uint8_t)((3 * s[x] + s[x - 1] + 8) >> 4);
      o[2 * x + 1] = (uint8_t)((3 * s[x] + s[x + 1] + 7) >> 4);
    }
    o[2 * cw - 2] = (uint8_t)((3 * s[cw - 1] + s[cw - 2] + 8) >> 4);
    o[2 * cw - 1] = (uint8_t)((4 * s[cw - 1] + 7) >> 4);
  }
  return out;
}

std::string b64(const uint8_t* p, size_t n) {
  static const char* A = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  std::string s;
  for (size_t i = 0; i < n; i += 3) {  // (n is a multiple of 3)
    const uint32_t v = (uint32_t)p[i] << 16 | (uint32_t)p[i + 1] << 8 | p[i + 2];
    s += A[v >> 18], s += A[(v >> 12) & 63], s += A[(v >> 6) & 63], s += A[v & 63];
  }
  return s;
}

}  // namespace

int main(int argc, char** argv) {
  const int iterations = argc > 1 ? atoi(argv[1]) : 2000;
  std::mt19937 rng(20261126);
  const int sizes[][2] = {{2, 2}, {2, 4}, {4, 2}, {4, 4}, {6, 18}, {12, 8}, {32, 32}};
  const std::string bt709 = "bt709", full = "full";
  int accepted = 0, rejected = 0;
  for (const auto& sz : sizes)
    for (const char* name : {"i420", "nv12"}) {
      const int HS = sz[0], WS = sz[1], ch = HS / 2, cw = WS / 2;
      const size_t hw = (size_t)HS * WS, B = hw * 3 / 2;
      const PixelSource near = PixelSource::from_names(name, &bt709, &full);
      const PixelSource lin = near.with_chroma("linear");
      CHECK(lin.chroma_linear() && !near.chroma_linear() && !near.with_chroma("nearest").chroma_linear(),
            "with_chroma");
      CHECK(lin.bytes(HS, WS, 3) == (int64_t)B && lin.kind() == PixelSource::YUV, "bytes / kind");
      lin.check(3, false, HS, WS, true);
      for (int constant = 0; constant < 2; ++constant) {
        std::vector<uint8_t> y(hw), u(hw / 4), v(hw / 4);
        for (auto& x : y) x = (uint8_t)rng();
        for (auto& x : u) x = constant ? 77 : (uint8_t)rng();
        for (auto& x : v) x = constant ? 201 : (uint8_t)rng();
        std::unique_ptr<uint8_t[]> frame(new uint8_t[B]);  // exactly B bytes
        memcpy(frame.get(), y.data(), hw);
        for (size_t i = 0; i < hw / 4; ++i)
          if (lin.yuv_format() == YUV_NV12)
            frame[hw + 2 * i] = u[i], frame[hw + 2 * i + 1] = v[i];
          else
            frame[hw + i] = u[i], frame[hw + hw / 4 + i] = v[i];
        std::vector<float> got(3 * hw), want(3 * hw);
        std::vector<uint8_t> rgb(3 * hw);
        CHECK(codec::yuv420_linear_to_rgb_host(frame.get(), HS, WS, lin.yuv_format(), lin.yuv(),
                                               rgb.data(), got.data()), "twin refused");
        std::vector<uint8_t> f444(y);
        const auto U = fancy(u, ch, cw), V = fancy(v, ch, cw);
        f444.insert(f444.end(), U.begin(), U.end());
        f444.insert(f444.end(), V.begin(), V.end());
        codec::yuvp_to_rgb_host(f444.data(), HS, WS, YUV_YUV444P, lin.yuv(), nullptr, want.data());
        CHECK(got == want, "%s %dx%d: twin != yuv444p of the loop upsampler", name, HS, WS);
        for (size_t i = 0; i < 3 * hw; ++i) CHECK(got[i] == (float)rgb[i], "rgb / f32");
        if (constant) {
          codec::yuv420_to_rgb_host(frame.get(), HS, WS, near.yuv_format(), near.yuv(), nullptr,
                                    want.data());
          CHECK(got == want, "%s %dx%d: constant chroma != nearest", name, HS, WS);
        }
        // records: the valid one, then mutated and truncated copies
        const std::string rec = "{\"instances\":[{\"b64\":\"" + b64(frame.get(), B) + "\"}]}";
        for (int it = 0; it < iterations / 14; ++it) {
          std::string s = rec;
          if (it > 0) {
            if (rng() & 1) s.resize(rng() % (s.size() + 1));
            for (int m = rng() % 3; m >= 0 && !s.empty(); --m) s[rng() % s.size()] = (char)rng();
          }
          std::unique_ptr<uint8_t[]> buf(new uint8_t[s.size() ? s.size() : 1]);
          memcpy(buf.get(), s.data(), s.size());
          std::vector<float> a(3 * hw, -1.f), b(3 * hw, -2.f);
          int na = 0, nb = 0;
          const int sa = codec::parse_instances_yuv_host(buf.get(), s.size(), HS, WS,
                                                         lin.yuv_format(), lin.yuv(), a.data(), 1,
                                                         &na, true);
          const int sb = lin.parse_host(buf.get(), s.size(), HS, WS, 3, b.data(), 1, &nb);
          CHECK(sa == sb && na == nb, "parser %d/%d != parse_host %d/%d", sa, na, sb, nb);
          if (sa == codec::OK) CHECK(a == b, "parser and parse_host floats");
          if (it == 0) CHECK(sa == codec::OK && na == 1 && a == got, "the valid record");
          sa == codec::OK ? ++accepted : ++rejected;
        }
      }
    }
  // the refusals: every source but b64 i420 / nv12, a raw encoding, a json topology, the width
  for (const char* pf : {"rgb", "yuyv422", "yuv422p", "yuv444p", "bgr24", "gray"}) {
    const PixelSource s = PixelSource::from_names(pf, nullptr, nullptr).with_chroma("linear");
    CHECK(refusal([&] { s.check(3, false, 32, 32, true); }).find("yuv_chroma") == 0, "%s", pf);
  }
  const PixelSource lin = PixelSource::from_names("i420", nullptr, nullptr).with_chroma("linear");
  CHECK(refusal([&] { lin.check(3, false, 32, 32, false); }).find("yuv_chroma") == 0, "json");
  CHECK(refusal([&] { lin.as_raw().check(3, false, 32, 32, true); }).find("yuv_chroma") == 0, "raw");
  CHECK(refusal([&] { lin.check(3, false, 2, kYuv420LinearMaxWS + 2, true); }).find("yuv_chroma") == 0,
        "width");
  lin.check(3, false, 2, kYuv420LinearMaxWS, true);
  CHECK(refusal([&] { lin.with_chroma("bilinear"); }).find("yuv_chroma") == 0, "name");
  CHECK(!refusal([&] { lin.check(1, false, 32, 32, true); }).empty(), "C = 1");
  CHECK(!refusal([&] { lin.check(3, false, 33, 32, true); }).empty(), "odd HS");
  const PixelSource p10 = PixelSource::from_names("p010le", nullptr, nullptr).as_raw();
  CHECK(refusal([&] { p10.with_chroma("linear").check(3, false, 32, 32, true); }).find("yuv_chroma") == 0,
        "p010le");
  p10.with_chroma("nearest").check(3, false, 32, 32, true);
  printf("yuv_chroma_check: %d failures (%d records accepted, %d rejected)\n", failures, accepted,
         rejected);
  return failures ? 1 : 0;
}
