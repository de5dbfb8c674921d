// Sanitizer run of the raw binary records' host side (json_codec.h: scan_instances_raw,
// split_instances_raw, parse_instances_raw_host; PixelSource's raw encoding): a few thousand
// values of random, whole and truncated lengths with random contents, every one in a heap block
// of exactly its size, for every element type and packed format. The parser is checked against
// the element and pixel functions applied to the value's own bytes, the scan and the splitter
// against the arithmetic, PixelSource::parse_host against the public parser, and the refusals by
// their text. Host only, no HIP call.
//   build/asan/raw_check [values per kind]
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

template <typename F>
std::string refusal(F f) {
  try {
    f();
  } catch (const std::invalid_argument& e) {
    return e.what();
  }
  return "";
}

struct Kind {
  const char* name;
  int elem, format;
};
const Kind kKinds[] = {{"u8", ELEM_U8, PACKED_NONE},     {"u16", ELEM_U16, PACKED_NONE},
                       {"f16", ELEM_F16, PACKED_NONE},   {"bf16", ELEM_BF16, PACKED_NONE},
                       {"f32", ELEM_F32, PACKED_NONE},   {"bgr24", ELEM_U8, PACKED_BGR24},
                       {"rgba", ELEM_U8, PACKED_RGBA},   {"bgra", ELEM_U8, PACKED_BGRA},
                       {"gray", ELEM_U8, PACKED_GRAY}};

PixelSource source_of(const Kind& k) {
  PixelSource s =
      PixelSource::from_names(k.format ? k.name : "rgb", nullptr, nullptr).with_elem(
          k.format ? "u8" : k.name);
  return s.as_raw();
}

}  // namespace

int main(int argc, char** argv) {
  const int per_kind = argc > 1 ? atoi(argv[1]) : 600;
  std::mt19937_64 rng(20260101);
  int accepted = 0, rejected = 0;

  // ---- the scan and the splitter against the arithmetic ---------------------------------------
  for (int it = 0; it < 4000; ++it) {
    const int64_t B = (int64_t)(rng() % 300) - 3;  // (-3 .. 296: non-positive ones too)
    const size_t n = rng() % 4 == 0 && B > 0 ? (size_t)B * (rng() % 40) : (size_t)(rng() % 9000);
    const codec::Scan s = codec::scan_instances_raw(n, B);
    const int want = n == 0 ? codec::EMPTY : B <= 0 || n % (size_t)B ? codec::BAD_SHAPE : codec::OK;
    CHECK(s.status == want, "scan(%zu, %lld) = %d, want %d", n, (long long)B, s.status, want);
    if (s.status == codec::OK)
      CHECK(s.arr_off == 0 && s.arr_len == (int64_t)n && s.images == (int)(n / (size_t)B),
            "scan(%zu, %lld) fields", n, (long long)B);
    else
      CHECK(s.images == 0, "scan(%zu, %lld): images on a refusal", n, (long long)B);
    const int mb = (int)(rng() % 6);
    std::vector<std::pair<uint32_t, uint32_t>> spans;
    const bool ok = codec::split_instances_raw(n, B, mb, spans);
    CHECK(ok == (want == codec::OK && mb >= 1), "split(%zu, %lld, %d)", n, (long long)B, mb);
    if (ok) {
      uint32_t at = 0;
      for (const auto& sp : spans) {
        CHECK(sp.first == at && sp.second > sp.first && (sp.second - sp.first) % B == 0 &&
                  (int64_t)(sp.second - sp.first) <= mb * B,
              "split(%zu, %lld, %d): span", n, (long long)B, mb);
        at = sp.second;
      }
      CHECK(at == n, "split(%zu, %lld, %d): cover", n, (long long)B, mb);
    } else {
      CHECK(spans.empty(), "split: spans on a refusal");
    }
  }
  CHECK(codec::scan_instances_raw(((size_t)1 << 30) + 1, 1).status == codec::TOO_LARGE, "2^30");

  // ---- the parser on random and truncated values ----------------------------------------------
  for (const Kind& k : kKinds) {
    const PixelSource src = source_of(k);
    CHECK(src.raw() && !src.wants_ingest_decode(), "%s: raw source", k.name);
    for (int it = 0; it < per_kind; ++it) {
      const int HS = 1 + (int)(rng() % 6), WS = 1 + (int)(rng() % 7);
      const int C = k.format ? 3 : 1 + (int)(rng() % 5);
      const int64_t B = src.bytes(HS, WS, C);
      const int N = 1 + (int)(rng() % 4);
      size_t n = (size_t)(B * N);
      const int mode = (int)(rng() % 4);  // whole, cut, grown, random length
      if (mode == 1) n -= 1 + rng() % (size_t)B;
      if (mode == 2) n += 1 + rng() % 3;
      if (mode == 3) n = rng() % (size_t)(B * 5);
      std::unique_ptr<uint8_t[]> buf(new uint8_t[n ? n : 1]);
      for (size_t i = 0; i < n; ++i) buf[i] = (uint8_t)rng();
      const size_t per = (size_t)HS * WS * C;
      std::vector<float> out((size_t)(n / (size_t)B + 1) * per, -7.f);
      const int max_images = (int)(rng() % 6) - 1;  // (-1: no limit)
      int images = -1;
      const int st = codec::parse_instances_raw_host(buf.get(), n, HS, WS, C, k.elem, k.format,
                                                     out.data(), max_images, &images);
      int iv = -1, ih = -1;
      const int sv = codec::parse_instances_raw_host(buf.get(), n, HS, WS, C, k.elem, k.format,
                                                     nullptr, max_images, &iv);
      const int sh = src.parse_host(buf.get(), n, HS, WS, C, nullptr, max_images, &ih);
      CHECK(sv == st && iv == images && sh == st && ih == images,
            "%s: validating %d (%d) / parse_host %d (%d) != decoding %d (%d)", k.name, sv, iv, sh,
            ih, st, images);
      // the verdict and the floats from the value's own bytes
      int want = n == 0 ? codec::EMPTY : n % (size_t)B ? codec::BAD_SHAPE : codec::OK;
      const int cnt = want == codec::OK ? (int)(n / (size_t)B) : 0;
      if (want == codec::OK && max_images >= 0 && cnt > max_images) want = codec::TOO_LARGE;
      std::vector<float> ref((size_t)cnt * per);
      if (want == codec::OK) {
        bool finite = true;
        for (int e = 0; e < cnt; ++e) {
          const uint8_t* img = buf.get() + (size_t)e * (size_t)B;
          if (k.format)
            codec::packed_to_rgb_host(img, HS, WS, k.format, nullptr, ref.data() + e * per);
          else
            finite &= codec::typed_to_float_host(img, per, k.elem, ref.data() + e * per);
        }
        if (!finite) want = codec::BAD_NUMBER;
      }
      CHECK(st == want, "%s %dx%dx%d n=%zu: status %d, want %d", k.name, HS, WS, C, n, st, want);
      CHECK(images == (want == codec::OK ? cnt : 0), "%s: images %d", k.name, images);
      if (st == codec::OK) {
        CHECK(memcmp(out.data(), ref.data(), ref.size() * sizeof(float)) == 0, "%s: floats",
              k.name);
        ++accepted;
      } else {
        ++rejected;
      }
    }
    // unknown kinds and sizes
    int im = -1;
    uint8_t one[16] = {0};
    CHECK(codec::parse_instances_raw_host(one, 16, 0, 4, 1, k.elem, k.format, nullptr, -1, &im) ==
              codec::BAD_SHAPE, "%s: H = 0", k.name);
    CHECK(codec::parse_instances_raw_host(one, 16, 2, 2, 1, 9, k.format, nullptr, -1, &im) ==
              codec::BAD_SHAPE, "%s: type 9", k.name);
    CHECK(codec::parse_instances_raw_host(one, 16, 2, 2, 3, k.elem, 7, nullptr, -1, &im) ==
              codec::BAD_SHAPE, "%s: format 7", k.name);
  }

  // ---- PixelSource: what a raw source refuses, by its text -------------------------------------
  {
    const PixelSource yuv = PixelSource::from_names("nv12", nullptr, nullptr).as_raw();
    CHECK(refusal([&] { yuv.check(3, false, 4, 4, true); }) ==
              "input_format raw: no pixel_format i420 / nv12", "raw yuv");
    int im = -1;
    uint8_t one[24] = {0};
    CHECK(yuv.parse_host(one, 24, 4, 4, 3, nullptr, -1, &im) == codec::BAD_SHAPE, "raw yuv parse");
    const PixelSource gray = PixelSource::from_names("gray", nullptr, nullptr).as_raw();
    gray.check(3, false, 5, 7, true);
    CHECK(refusal([&] { gray.check(1, false, 5, 7, true); }) ==
              "pixel_format bgr24 / rgba / bgra / gray needs a 3-channel model", "raw gray C = 1");
    CHECK(refusal([&] { gray.check(3, true, 5, 7, true); }) ==
              "pixel_format bgr24 / rgba / bgra / gray: no nchw layout", "raw gray nchw");
    const PixelSource u8 = PixelSource().as_raw();
    u8.check(5, true, 5, 7, true, true);
    CHECK(refusal([&] { u8.check(5, false, 5, 7, true, false); }) ==
              "input_format raw: per-channel input_a / input_b need C <= 4", "raw u8 C = 5");
    CHECK(PixelSource().wants_ingest_decode() && !PixelSource().raw(), "the default is b64 rgb");
  }

  printf("raw_check: %d values accepted, %d rejected, %d failures\n", accepted, rejected,
         failures);
  if (failures) return 1;
  printf("raw_check OK\n");
  return 0;
}
