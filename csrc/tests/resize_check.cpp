// Sanitizer run of the input resize's table builder and host twin (csrc/codec/resize.h): every
// (source, resize, model) size of 1..24 with resize >= model, per axis, and the 4096 extremes.
// Every image lives in a heap block of exactly its size, so AddressSanitizer sees any access
// past it. Checked here: the table indices are inside the source, 0 <= w < 1, the first index is
// monotone, each entry is the stated integer formula, refused dimensions throw, tampered tables
// are refused before anything is written, and a crop (source == resize size) is a bit copy, also
// of NaNs and next to +-max values.
//   build/asan/resize_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <stdexcept>
#include <vector>

#include "../codec/resize.h"

using namespace gale;

namespace {

int failures = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      ++failures;                                          \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                        \
      fprintf(stderr, "\n");                               \
    }                                                      \
  } while (0)

float from_bits(uint32_t b) {
  float v;
  memcpy(&v, &b, 4);
  return v;
}

uint32_t bits_of(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  return b;
}

uint32_t rng_state = 0x9e3779b9u;
uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

// one axis of built tables against the definition
void check_axis(const std::vector<int32_t>& i0, const std::vector<int32_t>& i1,
                const std::vector<float>& w, int n_src, int n_rs, int n_out) {
  CHECK(i0.size() == (size_t)n_out && i1.size() == (size_t)n_out && w.size() == (size_t)n_out,
        "table sizes for (%d, %d, %d)", n_src, n_rs, n_out);
  if (i0.size() != (size_t)n_out || i1.size() != (size_t)n_out || w.size() != (size_t)n_out) return;
  const int64_t off = (n_rs - n_out) / 2, den = 2 * (int64_t)n_rs;
  for (int i = 0; i < n_out; ++i) {
    const size_t k = (size_t)i;
    CHECK(i0[k] >= 0 && i0[k] < n_src && i1[k] >= 0 && i1[k] < n_src,
          "index out of range at %d of (%d, %d, %d): %d %d", i, n_src, n_rs, n_out, i0[k], i1[k]);
    CHECK(w[k] >= 0.f && w[k] < 1.f, "weight %g at %d of (%d, %d, %d)", (double)w[k], i, n_src,
          n_rs, n_out);
    if (i > 0) CHECK(i0[k] >= i0[k - 1], "first index not monotone at %d of (%d, %d, %d)", i,
                     n_src, n_rs, n_out);
    const int64_t num = (2 * (i + off) + 1) * (int64_t)n_src - n_rs;
    int e0 = 0, e1 = 0;
    float ew = 0.f;
    if (num >= 0) {
      const int64_t q = num / den, rem = num % den;
      if (q >= n_src - 1) {
        e0 = e1 = n_src - 1;
      } else {
        e0 = (int)q, e1 = (int)q + 1;
        ew = (float)((double)rem / (double)den);  // (the correctly rounded quotient again)
      }
    }
    CHECK(i0[k] == e0 && i1[k] == e1 && bits_of(w[k]) == bits_of(ew),
          "entry %d of (%d, %d, %d): %d %d %a, expected %d %d %a", i, n_src, n_rs, n_out, i0[k],
          i1[k], (double)w[k], e0, e1, (double)ew);
  }
}

// A resize of n random images (a few NaN / +-max / +-inf values among them) in exact-size heap
// blocks; with crop, the output must be the source's window bit for bit
void run_resize(int HS, int WS, int HR, int WR, int H, int W, int C, int n) {
  codec::ResizeTables t;
  codec::build_resize_tables(HS, WS, HR, WR, H, W, t);
  CHECK(codec::resize_tables_ok(t), "built tables refused (%d %d %d %d %d %d)", HS, WS, HR, WR, H,
        W);
  const size_t sn = (size_t)n * HS * WS * C, dn = (size_t)n * H * W * C;
  std::unique_ptr<float[]> src(new float[sn]), dst(new float[dn]);
  static const uint32_t special[] = {0x7fc00000u, 0x7f7fffffu, 0xff7fffffu, 0x7f800000u,
                                     0xff800000u, 0x00000001u, 0x80000000u};
  for (size_t i = 0; i < sn; ++i) {
    const uint32_t r = rnd();
    src[i] = (r & 15) == 0 ? from_bits(special[(r >> 4) % 7])
                           : (float)((int)(r >> 8 & 0xffff) - 32768) / 64.f;
  }
  for (size_t i = 0; i < dn; ++i) dst[i] = from_bits(0x7fa5a5a5u);
  codec::resize_crop_host(src.get(), n, C, t, dst.get());
  if (HS == HR && WS == WR) {
    const int oy = (HR - H) / 2, ox = (WR - W) / 2;
    for (int i = 0; i < n; ++i)
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
          for (int c = 0; c < C; ++c) {
            const float a = dst[(((size_t)i * H + y) * W + x) * C + c];
            const float b = src[(((size_t)i * HS + y + oy) * WS + x + ox) * C + c];
            CHECK(bits_of(a) == bits_of(b), "crop is not a copy at (%d, %d, %d, %d) of %dx%d", i,
                  y, x, c, HS, WS);
          }
  }
}

template <typename F>
bool throws_invalid(F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

}  // namespace

int main() {
  // every (source, resize, model) of 1..24 with resize >= model, per axis; each triple also runs
  // a resize with another triple on the column axis (and every crop one is checked as a copy)
  long triples = 0;
  for (int HS = 1; HS <= 24; ++HS)
    for (int HR = 1; HR <= 24; ++HR)
      for (int H = 1; H <= HR; ++H) {
        codec::ResizeTables t;
        codec::build_resize_tables(HS, 1, HR, 1, H, 1, t);
        check_axis(t.y0, t.y1, t.wy, HS, HR, H);
        codec::build_resize_tables(1, HS, 1, HR, 1, H, t);
        check_axis(t.x0, t.x1, t.wx, HS, HR, H);
        // the column axis: a crop for every other crop triple, else another size mix
        const bool crop = HS == HR && ((H + HS) & 1);
        const int W = (int)(rnd() % 24) + 1;
        const int WR = W + (int)(rnd() % (25 - W));
        const int WS = crop ? WR : (int)(rnd() % 24) + 1;
        run_resize(HS, WS, HR, WR, H, W, 1 + (int)(triples % 3), 1 + (int)(triples % 2));
        ++triples;
      }
  // the 4096 extremes, per axis, and resizes that touch the last source pixel of a long axis
  const int ext[][3] = {{4096, 4096, 4096}, {1, 4096, 4096}, {4096, 4096, 1}, {4096, 1, 1},
                        {1, 1, 1},          {4095, 4096, 4096}, {4096, 4095, 4095}, {2, 4096, 4095}};
  for (const auto& e : ext) {
    codec::ResizeTables t;
    codec::build_resize_tables(e[0], 1, e[1], 1, e[2], 1, t);
    check_axis(t.y0, t.y1, t.wy, e[0], e[1], e[2]);
  }
  run_resize(4096, 1, 4096, 1, 4096, 1, 3, 1);
  run_resize(1, 4096, 1, 4096, 1, 4096, 1, 2);
  run_resize(4096, 2, 4096, 3, 4095, 2, 1, 1);
  run_resize(3, 4096, 5, 4096, 4, 4096, 2, 1);
  run_resize(1, 1, 4096, 4096, 64, 64, 1, 1);
  // refusals
  codec::ResizeTables t;
  CHECK(throws_invalid([&] { codec::build_resize_tables(0, 4, 4, 4, 4, 4, t); }), "HS 0");
  CHECK(throws_invalid([&] { codec::build_resize_tables(4, 4097, 4, 4, 4, 4, t); }), "WS 4097");
  CHECK(throws_invalid([&] { codec::build_resize_tables(4, 4, 3, 4, 4, 4, t); }), "HR < H");
  CHECK(throws_invalid([&] { codec::build_resize_tables(4, 4, 4, 3, 4, 4, t); }), "WR < W");
  CHECK(throws_invalid([&] { codec::build_resize_tables(4, 4, 4097, 4, 4, 4, t); }), "HR 4097");
  CHECK(throws_invalid([&] { codec::build_resize_tables(4, 4, 4, 4, 4, -1, t); }), "W -1");
  // tampered tables are refused and nothing is written
  {
    std::unique_ptr<float[]> src(new float[5 * 6 * 2]), dst(new float[4 * 4 * 2]);
    for (int i = 0; i < 60; ++i) src[i] = (float)i;
    for (int i = 0; i < 32; ++i) dst[i] = -7.f;
    for (int k = 0; k < 5; ++k) {
      codec::build_resize_tables(5, 6, 5, 5, 4, 4, t);
      switch (k) {
        case 0: t.y1[3] = 5; break;
        case 1: t.x0[0] = -1; break;
        case 2: t.wx[2] = 1.f; break;
        case 3: t.wy[1] = from_bits(0x7fc00000u); break;
        case 4: t.x1.pop_back(); break;
      }
      CHECK(throws_invalid([&] { codec::resize_crop_host(src.get(), 1, 2, t, dst.get()); }),
            "tampered table %d accepted", k);
    }
    for (int i = 0; i < 32; ++i) CHECK(dst[i] == -7.f, "refused call wrote at %d", i);
    codec::build_resize_tables(5, 6, 5, 5, 4, 4, t);
    CHECK(throws_invalid([&] { codec::resize_crop_host(src.get(), -1, 2, t, dst.get()); }), "n -1");
    CHECK(throws_invalid([&] { codec::resize_crop_host(src.get(), 1, 0, t, dst.get()); }), "C 0");
    CHECK(throws_invalid([&] { codec::resize_crop_host(nullptr, 1, 2, t, dst.get()); }), "null");
  }
  if (failures) {
    fprintf(stderr, "resize_check: %d failure(s)\n", failures);
    return 1;
  }
  printf("resize_check OK: %ld size triples per axis, 4096 extremes\n", triples);
  return 0;
}
