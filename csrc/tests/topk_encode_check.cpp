// Sanitizer run of the two top-k encoders (csrc/codec/json_codec.h) over generated rows: random
// bit patterns (NaNs, infinities, denormals, both zeros), rows of equal values and softmax-like
// rows, for several (classes, k). Every input lives in a heap block of exactly its size, so
// AddressSanitizer sees any access past it. Checks the order rule on each selected list
// independently, and that encode_predictions_topk_text reproduces encode_predictions_topk byte
// for byte from slots and indices parsed back out of its output.
//   build/asan/topk_encode_check [iterations]
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

float from_bits(uint32_t b) {
  float v;
  memcpy(&v, &b, 4);
  return v;
}

// the comma-separated items of the list that follows `key` in the record starting at *pos
std::vector<std::string> list_after(const std::string& doc, const char* key, size_t* pos) {
  std::vector<std::string> items;
  const size_t at = doc.find(key, *pos);
  if (at == std::string::npos) return items;
  size_t p = doc.find('[', at) + 1;
  const size_t end = doc.find(']', p);
  while (p < end) {
    size_t q = doc.find(',', p);
    if (q == std::string::npos || q > end) q = end;
    items.push_back(doc.substr(p, q - p));
    p = q + 1;
  }
  *pos = end;
  return items;
}

void check_case(std::mt19937& rng, int n, int classes, int k, int kind, bool java8) {
  const size_t total = (size_t)n * classes;
  std::unique_ptr<float[]> x(new float[total]);
  for (size_t i = 0; i < total; ++i) {
    switch (kind) {
      case 0: x[i] = from_bits((uint32_t)rng()); break;                  // any bit pattern
      case 1: x[i] = 0.125f; break;                                      // all equal
      case 2: x[i] = from_bits((uint32_t)rng() % 3 == 0 ? 0x80000000u : (uint32_t)rng() % 4);
              break;                                                     // zeros and denormals
      default: x[i] = (float)(rng() % 16) / 16.f; break;                 // many duplicates
    }
  }
  std::string doc;
  codec::encode_predictions_topk(x.get(), n, classes, k, false, doc, java8);
  CHECK(doc.compare(0, 16, "{\"predictions\":[") == 0 && doc.size() >= 18 &&
            doc.compare(doc.size() - 2, 2, "]}") == 0,
        "envelope: %s", doc.substr(0, 40).c_str());
  std::unique_ptr<uint8_t[]> slots(new uint8_t[(size_t)n * k * 16]);
  std::unique_ptr<int32_t[]> idx(new int32_t[(size_t)n * k]);
  memset(slots.get(), 0, (size_t)n * k * 16);
  size_t pos = 0;
  char buf[48];
  for (int i = 0; i < n; ++i) {
    const std::vector<std::string> cls = list_after(doc, "\"classes\"", &pos);
    const std::vector<std::string> sc = list_after(doc, "\"scores\"", &pos);
    CHECK((int)cls.size() == k && (int)sc.size() == k, "image %d: %zu classes, %zu scores", i,
          cls.size(), sc.size());
    if ((int)cls.size() != k || (int)sc.size() != k) return;
    const float* row = x.get() + (size_t)i * classes;
    std::vector<char> taken((size_t)classes, 0);
    for (int j = 0; j < k; ++j) {
      const int c = atoi(cls[(size_t)j].c_str());
      CHECK(c >= 0 && c < classes && !taken[(size_t)c], "image %d entry %d: class %d", i, j, c);
      if (c < 0 || c >= classes) return;
      taken[(size_t)c] = 1;
      const int len = java8 ? codec::format_float_java8(row[c], buf)
                            : codec::format_float_java(row[c], buf);
      CHECK(sc[(size_t)j] == std::string(buf, (size_t)len), "image %d entry %d: score text", i, j);
      idx[(size_t)i * k + j] = c;
      uint8_t* slot = slots.get() + ((size_t)i * k + j) * 16;
      CHECK(sc[(size_t)j].size() <= 15, "score text longer than a slot");
      memcpy(slot, sc[(size_t)j].data(), std::min<size_t>(15, sc[(size_t)j].size()));
      slot[15] = (uint8_t)std::min<size_t>(15, sc[(size_t)j].size());
      if (j) {  // descending by key, ties to the lower index
        const int p = idx[(size_t)i * k + j - 1];
        const uint32_t kp = codec::score_key(row[p]), kc = codec::score_key(row[c]);
        CHECK(kp > kc || (kp == kc && p < c), "image %d entry %d out of order", i, j);
      }
    }
    // nothing left out beats the last one taken
    const int last = idx[(size_t)i * k + k - 1];
    for (int c = 0; c < classes; ++c) {
      if (taken[(size_t)c]) continue;
      const uint32_t kl = codec::score_key(row[last]), kc = codec::score_key(row[c]);
      CHECK(kl > kc || (kl == kc && last < c), "image %d: class %d beats entry %d", i, c, last);
    }
  }
  for (int js = 0; js < 2; ++js) {
    std::string a, b;
    codec::encode_predictions_topk(x.get(), n, classes, k, js != 0, a, java8);
    codec::encode_predictions_topk_text(slots.get(), idx.get(), n, k, js != 0, b);
    CHECK(a == b, "text form differs (json_string %d, classes %d, k %d)", js, classes, k);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 200;
  std::mt19937 rng(20240607);
  const int shapes[][2] = {{1, 1}, {10, 1}, {10, 3}, {10, 10}, {63, 5}, {64, 64}, {65, 64},
                           {1000, 5}, {4096, 64}};
  int cases = 0;
  for (int it = 0; it < iters; ++it) {
    const auto& s = shapes[it % (int)(sizeof(shapes) / sizeof(shapes[0]))];
    const int n = 1 + (int)(rng() % 4);
    check_case(rng, n, s[0], s[1], (int)(rng() % 4), (rng() & 7) == 0);
    ++cases;
  }
  std::string empty;
  codec::encode_predictions_topk(nullptr, 0, 10, 3, false, empty);
  CHECK(empty == "{\"predictions\":[]}", "no images: %s", empty.c_str());
  codec::encode_predictions_topk_text(nullptr, nullptr, 0, 3, true, empty);
  CHECK(empty == "\"{\\\"predictions\\\":[]}\"", "no images, json_string: %s", empty.c_str());
  printf("topk_encode_check: %d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
