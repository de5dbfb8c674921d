// Sanitizer run of the packed-pixel host codec (csrc/codec/pixfmt.h, csrc/codec/json_codec.h) on
// untrusted input: the unpack twin, the record decoder and the byte-count forms of the scan, the
// offsets helper and the splitter. A fixed seed, valid records of several image sizes (1x1 and
// odd sizes among them: the strings' padding takes all three lengths) in the four formats and a
// few thousand mutated and truncated copies. Every input lives in a heap block of exactly its
// size, so AddressSanitizer sees any access past n. Checks the twin against a scalar restatement,
// that every status is one of the format's verdicts, that the functions agree with each other,
// that a valid record decodes to the unpack of its images - and to what the RGB decoder gives for
// the RGB record of those - and the refusals. Host only, no HIP call.
//   build/asan/pixfmt_check [iterations]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../codec/json_codec.h"

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

struct Size {
  int HS, WS;
};

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

bool known_status(int st, bool decoder) {
  switch (st) {
    case codec::OK:
    case codec::BAD_ENVELOPE:
    case codec::UNKNOWN_KEY:
    case codec::BAD_SHAPE:
    case codec::EMPTY:
    case codec::NULL_INSTANCES:
    case codec::TOO_LARGE:
      return true;
    case codec::BAD_NUMBER:
      return decoder;
    default:
      return false;
  }
}

// the definition, restated per pixel with a table of its own
void scalar_unpack(const std::vector<uint8_t>& src, int HS, int WS, int format, uint8_t* rgb) {
  static const int kBpp[5] = {0, 3, 4, 4, 1};
  static const int kOff[5][3] = {{0, 0, 0}, {2, 1, 0}, {0, 1, 2}, {2, 1, 0}, {0, 0, 0}};
  for (int y = 0; y < HS; ++y)
    for (int x = 0; x < WS; ++x)
      for (int c = 0; c < 3; ++c)
        rgb[(y * WS + x) * 3 + c] = src[(size_t)(y * WS + x) * kBpp[format] + kOff[format][c]];
}

// Runs everything on an exact-size heap copy of `s`; returns the decoder's status.
int run(const std::string& s, const Size& sz, int format, std::vector<float>* decoded) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[s.size() ? s.size() : 1]);
  memcpy(buf.get(), s.data(), s.size());
  const uint8_t* p = buf.get();
  const size_t n = s.size();
  const int64_t B = packed_bytes(sz.HS, sz.WS, format);
  const size_t L = (size_t)codec::b64_chars_bytes(B);
  const codec::Scan sc = codec::scan_instances_b64_bytes(p, n, B);
  CHECK(known_status(sc.status, false), "scan status %d", sc.status);
  // the byte-count form and the (H, W, C) form of the same byte count agree
  const codec::Scan sc3 = codec::scan_instances_b64(p, n, sz.HS, sz.WS, packed_bpp(format));
  CHECK(sc3.status == sc.status && sc3.images == sc.images && sc3.arr_off == sc.arr_off &&
            sc3.arr_len == sc.arr_len,
        "scan forms disagree");
  std::vector<float> out;
  int images = -1;
  const size_t per = (size_t)sz.HS * sz.WS * 3;
  if (sc.status == codec::OK) {
    CHECK(sc.images > 0 && sc.arr_off > 0 && sc.arr_off + sc.arr_len <= (int64_t)n,
          "scan result out of range");
    out.assign((size_t)sc.images * per, -1.f);
    std::unique_ptr<uint8_t[]> arr(new uint8_t[(size_t)sc.arr_len]);
    memcpy(arr.get(), p + sc.arr_off, (size_t)sc.arr_len);
    std::vector<uint32_t> offs;
    std::vector<std::pair<uint32_t, uint32_t>> spans;
    const bool ok1 = codec::b64_image_offsets_bytes(arr.get(), (size_t)sc.arr_len, B, offs);
    const bool ok2 = codec::split_instances_b64_bytes(arr.get(), (size_t)sc.arr_len, B, spans);
    CHECK(ok1 && ok2 && (int)offs.size() == sc.images && (int)spans.size() == sc.images,
          "offsets / split disagree with the scan");
    for (size_t i = 0; ok1 && ok2 && i < offs.size(); ++i) {
      CHECK(offs[i] + L < (size_t)sc.arr_len && arr[offs[i] + L] == '"' &&
                arr[offs[i] - 1] == '"',
            "string offset %zu", i);
      CHECK(spans[i].first < offs[i] && spans[i].second > offs[i] + L &&
                arr[spans[i].first] == '{' && arr[spans[i].second - 1] == '}',
            "element span %zu", i);
    }
  }
  const int st = codec::parse_instances_packed_host(p, n, sz.HS, sz.WS, format,
                                                    out.empty() ? nullptr : out.data(), -1,
                                                    &images);
  CHECK(known_status(st, true), "decoder status %d", st);
  if (sc.status != codec::OK) CHECK(st == sc.status, "decoder %d != scan %d", st, sc.status);
  else CHECK(st == codec::OK || st == codec::BAD_NUMBER, "decoder %d after an OK scan", st);
  // the RGB decoder of the same byte count gives the same verdict: the characters and the
  // padding are judged alike
  {
    int im = -1;
    const int st3 = codec::parse_instances_b64_host(p, n, sz.HS, sz.WS, packed_bpp(format),
                                                    nullptr, -1, &im);
    CHECK(st3 == st && im == images, "rgb decoder %d (%d images) != packed %d (%d)", st3, im, st,
          images);
  }
  if (st == codec::OK) {
    CHECK(images == sc.images, "image count");
    for (float v : out) CHECK(v >= 0.f && v <= 255.f && v == (float)(int)v, "value %g", v);
  } else {
    CHECK(images == 0, "images reported for a bad record");
  }
  if (sc.status == codec::OK && sc.images > 1) {
    int im = -1;
    CHECK(codec::parse_instances_packed_host(p, n, sz.HS, sz.WS, format, nullptr, sc.images - 1,
                                             &im) == codec::TOO_LARGE,
          "max_images");
  }
  if (decoded) *decoded = out;
  return st;
}

}  // namespace

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 4000;
  std::mt19937 rng(20261020u);
  const Size sizes[] = {{1, 1}, {1, 2}, {3, 1}, {2, 2}, {5, 7}, {4, 4}, {6, 10}, {3, 11}, {1, 34}};
  const int formats[] = {PACKED_BGR24, PACKED_RGBA, PACKED_BGRA, PACKED_GRAY};
  int ok = 0, bad = 0;
  // the tables
  CHECK(packed_bpp(PACKED_NONE) == 0 && packed_bpp(5) == 0 && packed_bpp(-1) == 0, "bpp of none");
  CHECK(packed_bpp(PACKED_BGR24) == 3 && packed_bpp(PACKED_RGBA) == 4 &&
            packed_bpp(PACKED_BGRA) == 4 && packed_bpp(PACKED_GRAY) == 1, "bpp");
  CHECK(packed_format_of("bgr24") == PACKED_BGR24 && packed_format_of("rgba") == PACKED_RGBA &&
            packed_format_of("bgra") == PACKED_BGRA && packed_format_of("gray") == PACKED_GRAY,
        "names");
  for (const char* t : {"", "rgb", "bgr", "yuyv", "bgr2", "bgr240", "grey", "argb", "i420"})
    CHECK(packed_format_of(t) == PACKED_NONE, "name %s", t);
  CHECK(packed_bytes(5, 7, PACKED_RGBA) == 140 && packed_bytes(5, 7, PACKED_GRAY) == 35 &&
            packed_bytes(0, 7, PACKED_GRAY) == 0 && packed_bytes(5, -1, PACKED_BGR24) == 0 &&
            packed_bytes(5, 7, 0) == 0 && packed_bytes(32768, 32768, PACKED_BGRA) == (1ll << 32),
        "packed_bytes");
  // refusals of the twin and the decoder: non-positive sizes, unknown formats
  {
    uint8_t image[16] = {0}, rgb[12];
    CHECK(!codec::packed_to_rgb_host(image, 0, 2, PACKED_BGR24, rgb, nullptr), "HS 0");
    CHECK(!codec::packed_to_rgb_host(image, 2, -2, PACKED_BGR24, rgb, nullptr), "WS < 0");
    CHECK(!codec::packed_to_rgb_host(image, 2, 2, 0, rgb, nullptr), "format 0");
    CHECK(!codec::packed_to_rgb_host(image, 2, 2, 5, rgb, nullptr), "format 5");
    CHECK(codec::packed_to_rgb_host(image, 2, 2, PACKED_BGRA, rgb, nullptr), "2x2");
    int im = -1;
    const std::string t = "{\"instances\":[{\"b64\":\"AAAAAA==\"}]}";  // 4 bytes
    const uint8_t* tp = reinterpret_cast<const uint8_t*>(t.data());
    CHECK(codec::parse_instances_packed_host(tp, t.size(), 1, 1, PACKED_RGBA, nullptr, -1, &im) ==
              codec::OK && im == 1, "1x1 rgba record");
    CHECK(codec::parse_instances_packed_host(tp, t.size(), 2, 2, PACKED_GRAY, nullptr, -1, &im) ==
              codec::OK && im == 1, "2x2 gray record");
    CHECK(codec::parse_instances_packed_host(tp, t.size(), 1, 1, PACKED_BGR24, nullptr, -1,
                                             &im) == codec::BAD_SHAPE, "3-byte image");
    CHECK(codec::parse_instances_packed_host(tp, t.size(), 1, 1, 0, nullptr, -1, &im) ==
              codec::BAD_SHAPE, "format 0");
    CHECK(codec::parse_instances_packed_host(tp, t.size(), 1, 1, 9, nullptr, -1, &im) ==
              codec::BAD_SHAPE, "format 9");
    CHECK(codec::parse_instances_packed_host(tp, t.size(), 0, 1, PACKED_RGBA, nullptr, -1, &im) ==
              codec::BAD_SHAPE, "HS 0");
    CHECK(codec::parse_instances_packed_host(tp, t.size(), 1, -1, PACKED_RGBA, nullptr, -1,
                                             &im) == codec::BAD_SHAPE, "WS < 0");
    // padding: a data character where '=' belongs, '=' where data belongs
    std::string u = t;
    u[u.find("==")] = 'A';
    CHECK(codec::parse_instances_packed_host(reinterpret_cast<const uint8_t*>(u.data()), u.size(),
                                             1, 1, PACKED_RGBA, nullptr, -1, &im) ==
              codec::BAD_NUMBER, "data in the padding");
    u = t;
    u[u.find("AAAA")] = '=';
    CHECK(codec::parse_instances_packed_host(reinterpret_cast<const uint8_t*>(u.data()), u.size(),
                                             1, 1, PACKED_RGBA, nullptr, -1, &im) ==
              codec::BAD_NUMBER, "'=' in the data");
  }
  for (const char* t : {"", " ", "{", "{}", "[", "{\"instances\"", "{\"instances\":[",
                        "{\"instances\":[]}", "{\"instances\":null}", "{\"instances\":[{",
                        "{\"instances\":[{\"b64\":\"", "{\"instances\":[{\"b64\":\"AAAA\"}]}",
                        "{\"instances\":[{}]}", "{\"instances\":[[[[1,2,3]]]]}"})
    for (int format : formats) run(t, sizes[3], format, nullptr);
  run("{\"instances\":[{\"b64\":\"", Size{20000, 20000}, PACKED_BGRA, nullptr);  // L past the end
  for (int it = 0; it < iters; ++it) {
    const Size& sz = sizes[rng() % (sizeof(sizes) / sizeof(sizes[0]))];
    const int format = formats[rng() % 4];
    const int P = packed_bpp(format);
    const int images = 1 + (int)(rng() % 3);
    const size_t hw = (size_t)sz.HS * sz.WS;
    std::vector<std::vector<uint8_t>> packed, unpacked;
    std::vector<float> want;
    for (int i = 0; i < images; ++i) {
      std::vector<uint8_t> src(hw * P);
      for (uint8_t& b : src) b = (uint8_t)rng();
      std::vector<uint8_t> rgb(hw * 3), ref(hw * 3);
      std::vector<float> f(hw * 3), fp(hw * 3);
      CHECK(codec::packed_to_rgb_host(src.data(), sz.HS, sz.WS, format, rgb.data(), f.data()),
            "unpack refused");
      scalar_unpack(src, sz.HS, sz.WS, format, ref.data());
      CHECK(rgb == ref, "twin differs from the scalar restatement");
      for (size_t e = 0; e < f.size(); ++e) CHECK(f[e] == (float)rgb[e], "float != byte");
      // the prep's coefficients are indexed by model channel
      const float a[3] = {0.5f, 0.25f, 2.f}, b[3] = {1.f, -3.f, 0.125f};
      CHECK(codec::packed_to_rgb_host(src.data(), sz.HS, sz.WS, format, nullptr, fp.data(), a, b),
            "unpack with prep refused");
      for (size_t e = 0; e < fp.size(); ++e)
        CHECK(fp[e] == __builtin_fmaf((float)ref[e], a[e % 3], b[e % 3]), "prep");
      packed.push_back(src);
      unpacked.push_back(rgb);
      want.insert(want.end(), f.begin(), f.end());
    }
    std::string s = record(packed, rng() % 2 != 0);
    if (it % 8 == 0) {  // the valid record decodes to the unpack, and to the RGB record's floats
      std::vector<float> got;
      CHECK(run(s, sz, format, &got) == codec::OK, "valid record rejected");
      CHECK(got == want, "decoded images differ from the unpack twin");
      const std::string r3 = record(unpacked, false);
      std::vector<float> rgbf(want.size(), -1.f);
      int im = -1;
      CHECK(codec::parse_instances_b64_host(reinterpret_cast<const uint8_t*>(r3.data()), r3.size(),
                                            sz.HS, sz.WS, 3, rgbf.data(), -1, &im) == codec::OK &&
                im == images, "rgb record of the unpacked images rejected");
      CHECK(rgbf == want, "packed record differs from the rgb record of its unpacked images");
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
    const int st = run(s, sz, format, nullptr);
    st == codec::OK ? ++ok : ++bad;
  }
  printf("pixfmt_check: %d records accepted, %d rejected, %d failures\n", ok, bad, failures);
  if (failures || ok == 0 || bad == 0) return 1;
  printf("all checks passed\n");
  return 0;
}
