// Sanitizer run of the base64 record scanner, host decoder, offsets helper and splitter
// (csrc/codec/json_codec.h) on untrusted input: a fixed seed, valid records of several shapes and
// a few thousand mutated and truncated copies of them. Every input lives in a heap block of
// exactly its size, so AddressSanitizer sees any access past n. Checks that every status is one
// of the format's verdicts and that the four functions agree with each other.
//   build/asan/b64_scan_check [iterations]
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

std::string b64(const std::vector<uint8_t>& v) {
  static const char kA[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  std::string s;
  for (size_t i = 0; i < v.size(); i += 3) {
    const size_t m = std::min<size_t>(3, v.size() - i);
    uint32_t x = 0;
    for (size_t j = 0; j < 3; ++j) x = (x << 8) | (j < m ? v[i + j] : 0);
    s += kA[(x >> 18) & 63];
    s += kA[(x >> 12) & 63];
    s += m > 1 ? kA[(x >> 6) & 63] : '=';
    s += m > 2 ? kA[x & 63] : '=';
  }
  return s;
}

struct Shape {
  int H, W, C;
};

std::string record(std::mt19937& rng, const Shape& sh, int images, bool spaces,
                   std::vector<uint8_t>* pixels) {
  const char* ws = spaces ? " \n" : "";
  std::string s = std::string(ws) + "{" + ws + "\"instances\"" + ws + ":" + ws + "[";
  for (int i = 0; i < images; ++i) {
    std::vector<uint8_t> px((size_t)sh.H * sh.W * sh.C);
    for (uint8_t& b : px) b = (uint8_t)rng();
    if (pixels) pixels->insert(pixels->end(), px.begin(), px.end());
    if (i) s += std::string(ws) + ",";
    s += std::string(ws) + "{" + ws + "\"b64\"" + ws + ":" + ws + "\"" + b64(px) + "\"" + ws + "}";
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

// Runs everything on an exact-size heap copy of `s`; returns the decoder's status.
int run(const std::string& s, const Shape& sh, std::vector<float>* decoded) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[s.size() ? s.size() : 1]);
  memcpy(buf.get(), s.data(), s.size());
  const uint8_t* p = buf.get();
  const size_t n = s.size();
  const codec::Scan sc = codec::scan_instances_b64(p, n, sh.H, sh.W, sh.C);
  CHECK(known_status(sc.status, false), "scan status %d", sc.status);
  std::vector<float> out;
  int images = -1;
  const size_t per = (size_t)sh.H * sh.W * sh.C;
  if (sc.status == codec::OK) {
    CHECK(sc.images > 0 && sc.arr_off > 0 && sc.arr_off + sc.arr_len <= (int64_t)n,
          "scan result out of range");
    out.assign((size_t)sc.images * per, -1.f);
    // the array alone, again in a block of its own size
    std::unique_ptr<uint8_t[]> arr(new uint8_t[(size_t)sc.arr_len]);
    memcpy(arr.get(), p + sc.arr_off, (size_t)sc.arr_len);
    std::vector<uint32_t> offs;
    std::vector<std::pair<uint32_t, uint32_t>> spans;
    const bool ok1 = codec::b64_image_offsets(arr.get(), (size_t)sc.arr_len, sh.H, sh.W, sh.C, offs);
    const bool ok2 =
        codec::split_instances_b64(arr.get(), (size_t)sc.arr_len, sh.H, sh.W, sh.C, spans);
    CHECK(ok1 && ok2 && (int)offs.size() == sc.images && (int)spans.size() == sc.images,
          "offsets / split disagree with the scan");
    const size_t L = (size_t)codec::b64_chars(sh.H, sh.W, sh.C);
    for (size_t i = 0; ok1 && ok2 && i < offs.size(); ++i) {
      CHECK(offs[i] + L < (size_t)sc.arr_len && arr[offs[i] + L] == '"' &&
                arr[offs[i] - 1] == '"',
            "string offset %zu", i);
      CHECK(spans[i].first < offs[i] && spans[i].second > offs[i] + L &&
                arr[spans[i].first] == '{' && arr[spans[i].second - 1] == '}',
            "element span %zu", i);
    }
  }
  const int st = codec::parse_instances_b64_host(p, n, sh.H, sh.W, sh.C,
                                                 out.empty() ? nullptr : out.data(), -1, &images);
  CHECK(known_status(st, true), "decoder status %d", st);
  if (sc.status != codec::OK) CHECK(st == sc.status, "decoder %d != scan %d", st, sc.status);
  else CHECK(st == codec::OK || st == codec::BAD_NUMBER, "decoder %d after an OK scan", st);
  if (st == codec::OK) {
    CHECK(images == sc.images, "image count");
    for (float v : out) CHECK(v >= 0.f && v <= 255.f && v == (float)(int)v, "value %g", v);
  } else {
    CHECK(images == 0, "images reported for a bad record");
  }
  // a cap below the count is TOO_LARGE
  if (sc.status == codec::OK && sc.images > 1) {
    int im = -1;
    CHECK(codec::parse_instances_b64_host(p, n, sh.H, sh.W, sh.C, nullptr, sc.images - 1, &im) ==
              codec::TOO_LARGE,
          "max_images");
  }
  if (decoded) *decoded = out;
  return st;
}

}  // namespace

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 4000;
  std::mt19937 rng(20260117u);
  const Shape shapes[] = {{5, 4, 3}, {5, 4, 1}, {28, 28, 1}, {1, 1, 1}, {2, 1, 1}, {3, 3, 5}};
  int ok = 0, bad = 0;
  // fixed cases: the empty input, lone tokens, deep nesting, a huge length claim
  const Shape s0 = shapes[0];
  for (const char* t : {"", " ", "{", "{}", "[", "{\"instances\"", "{\"instances\":", "{\"instances\":[",
                        "{\"instances\":[]}", "{\"instances\":null}", "{\"instances\":[{",
                        "{\"instances\":[{\"b64\"", "{\"instances\":[{\"b64\":", "{\"instances\":[{\"b64\":\"",
                        "{\"instances\":[{\"b64\":\"AAAA\"}]}", "{\"instances\":[{}]}",
                        "{\"instances\":[[[[1,2,3]]]]}", "{\"instances\":{}}"})
    run(t, s0, nullptr);
  run("{\"instances\":" + std::string(100000, '[') + "}", s0, nullptr);
  run("{\"instances\":[" + std::string(100000, '{') + "]}", s0, nullptr);
  run("{\"instances\":[{\"b64\":\"", Shape{30000, 30000, 4}, nullptr);  // L far beyond the end
  for (int it = 0; it < iters; ++it) {
    const Shape& sh = shapes[rng() % (sizeof(shapes) / sizeof(shapes[0]))];
    const int images = 1 + (int)(rng() % 3);
    std::vector<uint8_t> px;
    std::string s = record(rng, sh, images, rng() % 2 != 0, &px);
    if (it % 8 == 0) {  // the valid record itself decodes to its pixels
      std::vector<float> got;
      CHECK(run(s, sh, &got) == codec::OK, "valid record rejected");
      CHECK(got.size() == px.size(), "decoded size");
      for (size_t i = 0; i < px.size() && i < got.size(); ++i)
        CHECK(got[i] == (float)px[i], "pixel %zu", i);
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
    const int st = run(s, sh, nullptr);
    st == codec::OK ? ++ok : ++bad;
  }
  printf("b64_scan_check: %d records accepted, %d rejected, %d failures\n", ok, bad, failures);
  if (failures || ok == 0 || bad == 0) return 1;
  printf("all checks passed\n");
  return 0;
}
