// Sanitizer run of the antialiased input resize's table builder and host twin
// (csrc/codec/resize.h): every (source, resize, model) size of 1..24 with resize >= model and
// source <= 8 resize, per axis, the 4096 extremes, and refusal of every triple over the limit.
// Every image lives in a heap block of exactly its size, so AddressSanitizer sees any access
// past it. Checked here: each entry is the stated integer formula (the run is exactly the k
// with u > 0, contiguous and non-empty, the weights are (float)((double)u / (double)U)), counts
// are 1..17, runs lie inside the source, starts and ends are monotone, the strided device layout
// and the band figures match the tables, tampered tables are refused before anything is
// written, and a crop (source == resize size) is a bit copy, also of NaNs and next to +-max.
//   build/asan/resize_aa_check
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

// one axis of built tables against the definition, by a scan over every source index
void check_axis(const std::vector<int32_t>& start, const std::vector<int32_t>& count,
                const std::vector<float>& w, int taps, int n_src, int n_rs, int n_out) {
  CHECK(start.size() == (size_t)n_out && count.size() == (size_t)n_out, "table sizes (%d, %d, %d)",
        n_src, n_rs, n_out);
  if (start.size() != (size_t)n_out || count.size() != (size_t)n_out) return;
  const int64_t off = (n_rs - n_out) / 2, S = n_src > n_rs ? n_src : n_rs;
  size_t o = 0;
  int most = 0;
  for (int i = 0; i < n_out; ++i) {
    const size_t e = (size_t)i;
    const int64_t c = (2 * (i + off) + 1) * (int64_t)n_src;
    int first = -1, n = 0;
    int64_t U = 0;
    bool contiguous = true;
    for (int k = 0; k < n_src; ++k) {
      const int64_t a = (2 * (int64_t)k + 1) * n_rs - c;
      const int64_t u = 2 * S - (a < 0 ? -a : a);
      if (u <= 0) continue;
      if (first < 0) first = k;
      else if (k != first + n) contiguous = false;
      ++n, U += u;
    }
    CHECK(n >= 1 && n <= codec::kResizeAaMaxTaps && contiguous && U <= ((int64_t)1 << 26),
          "run of %d at %d of (%d, %d, %d)", n, i, n_src, n_rs, n_out);
    CHECK(start[e] == first && count[e] == n, "entry %d of (%d, %d, %d): %d+%d, expected %d+%d", i,
          n_src, n_rs, n_out, start[e], count[e], first, n);
    if (start[e] != first || count[e] != n || o + (size_t)n > w.size()) return;
    if (i > 0)
      CHECK(start[e] >= start[e - 1] && start[e] + count[e] >= start[e - 1] + count[e - 1],
            "run not monotone at %d of (%d, %d, %d)", i, n_src, n_rs, n_out);
    for (int k = 0; k < n; ++k) {
      const int64_t a = (2 * (int64_t)(first + k) + 1) * n_rs - c;
      const float want = (float)((double)(2 * S - (a < 0 ? -a : a)) / (double)U);
      CHECK(bits_of(w[o + (size_t)k]) == bits_of(want) && want > 0.f && want <= 1.f,
            "weight %d of entry %d of (%d, %d, %d): %a, expected %a", k, i, n_src, n_rs, n_out,
            (double)w[o + (size_t)k], (double)want);
    }
    if (n == 1) CHECK(w[o] == 1.f, "single tap of weight %a", (double)w[o]);
    o += (size_t)n;
    if (n > most) most = n;
  }
  CHECK(o == w.size() && most == taps, "weights %zu of %zu, taps %d of %d", o, w.size(), most,
        taps);
}

// the device layout and the band figures of built tables
void check_layout(const codec::ResizeAaTables& t) {
  const std::vector<float> wy = codec::resize_aa_strided(t.yn, t.wy, t.ty);
  CHECK(wy.size() == (size_t)t.H * (size_t)t.ty, "strided size");
  size_t o = 0;
  for (int y = 0; y < t.H && wy.size() == (size_t)t.H * (size_t)t.ty; ++y)
    for (int k = 0; k < t.ty; ++k) {
      const float want = k < t.yn[(size_t)y] ? t.wy[o++] : 0.f;
      CHECK(bits_of(wy[(size_t)y * (size_t)t.ty + (size_t)k]) == bits_of(want), "strided %d %d", y,
            k);
    }
  const int band = codec::resize_aa_choose_band(t);
  const int rows = codec::resize_aa_band_rows(t, band);
  CHECK(band >= 1 && band <= 8 && rows >= 1 && rows + t.tx <= codec::kResizeAaLdsRows,
        "band %d rows %d tx %d", band, rows, t.tx);
  for (int y0 = 0; y0 < t.H; y0 += band) {
    const int y1 = (y0 + band < t.H ? y0 + band : t.H) - 1;
    CHECK(t.ys[(size_t)y1] + t.yn[(size_t)y1] - t.ys[(size_t)y0] <= rows, "band at %d over %d rows",
          y0, rows);
  }
}

// A resize of n random images (a few NaN / +-max / +-inf values among them) in exact-size heap
// blocks; with crop, the output must be the source's window bit for bit
void run_resize(int HS, int WS, int HR, int WR, int H, int W, int C, int n) {
  codec::ResizeAaTables t;
  codec::build_resize_aa_tables(HS, WS, HR, WR, H, W, t);
  CHECK(codec::resize_aa_tables_ok(t), "built tables refused (%d %d %d %d %d %d)", HS, WS, HR, WR,
        H, W);
  check_layout(t);
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
  codec::resize_crop_aa_host(src.get(), n, C, t, dst.get());
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
  // every (source, resize, model) of 1..24 with resize >= model, per axis: within the 8x limit
  // checked against the definition and run (with another triple on the column axis; every other
  // crop triple as a crop on both axes), over the limit refused
  long triples = 0, refused = 0;
  for (int HS = 1; HS <= 24; ++HS)
    for (int HR = 1; HR <= 24; ++HR)
      for (int H = 1; H <= HR; ++H) {
        codec::ResizeAaTables t;
        if (HS > 8 * HR) {
          CHECK(throws_invalid([&] { codec::build_resize_aa_tables(HS, 1, HR, 1, H, 1, t); }) &&
                    throws_invalid([&] { codec::build_resize_aa_tables(1, HS, 1, HR, 1, H, t); }),
                "(%d, %d, %d) over the limit accepted", HS, HR, H);
          ++refused;
          continue;
        }
        codec::build_resize_aa_tables(HS, 1, HR, 1, H, 1, t);
        check_axis(t.ys, t.yn, t.wy, t.ty, HS, HR, H);
        codec::build_resize_aa_tables(1, HS, 1, HR, 1, H, t);
        check_axis(t.xs, t.xn, t.wx, t.tx, HS, HR, H);
        const bool crop = HS == HR && ((H + HS) & 1);
        const int W = (int)(rnd() % 24) + 1;
        const int WR = W + (int)(rnd() % (25 - W));
        const int ws = (int)(rnd() % 24) + 1;
        const int WS = crop ? WR : ws > 8 * WR ? 8 * WR : ws;
        run_resize(HS, WS, HR, WR, H, W, 1 + (int)(triples % 3), 1 + (int)(triples % 2));
        ++triples;
      }
  CHECK(refused > 0, "no triple over the limit");
  // the 4096 extremes, per axis, within the limit
  const int ext[][3] = {{4096, 4096, 4096}, {1, 4096, 4096}, {4096, 4096, 1},    {4096, 512, 1},
                        {4096, 512, 512},   {1, 1, 1},       {4095, 4096, 4096}, {4096, 4095, 4095},
                        {2, 4096, 4095},    {4095, 512, 2},  {4096, 513, 511}};
  for (const auto& e : ext) {
    codec::ResizeAaTables t;
    codec::build_resize_aa_tables(e[0], 1, e[1], 1, e[2], 1, t);
    check_axis(t.ys, t.yn, t.wy, t.ty, e[0], e[1], e[2]);
    check_layout(t);
  }
  run_resize(4096, 1, 4096, 1, 4096, 1, 3, 1);
  run_resize(1, 4096, 1, 4096, 1, 4096, 1, 2);
  run_resize(4096, 2, 512, 3, 511, 2, 1, 1);
  run_resize(3, 4096, 5, 512, 4, 512, 2, 1);
  run_resize(4096, 4095, 512, 512, 1, 2, 1, 1);
  run_resize(1, 1, 4096, 4096, 64, 64, 1, 1);
  // refusals
  codec::ResizeAaTables t;
  CHECK(throws_invalid([&] { codec::build_resize_aa_tables(0, 4, 4, 4, 4, 4, t); }), "HS 0");
  CHECK(throws_invalid([&] { codec::build_resize_aa_tables(4, 4097, 4, 4, 4, 4, t); }), "WS 4097");
  CHECK(throws_invalid([&] { codec::build_resize_aa_tables(4, 4, 3, 4, 4, 4, t); }), "HR < H");
  CHECK(throws_invalid([&] { codec::build_resize_aa_tables(4, 4, 4, 3, 4, 4, t); }), "WR < W");
  CHECK(throws_invalid([&] { codec::build_resize_aa_tables(4, 4, 4097, 4, 4, 4, t); }), "HR 4097");
  CHECK(throws_invalid([&] { codec::build_resize_aa_tables(4, 4, 4, 4, 4, -1, t); }), "W -1");
  CHECK(throws_invalid([&] { codec::build_resize_aa_tables(4096, 4, 511, 4, 4, 4, t); }), "8x H");
  CHECK(throws_invalid([&] { codec::build_resize_aa_tables(4, 33, 4, 4, 4, 4, t); }), "8x W");
  // tampered tables are refused and nothing is written
  {
    std::unique_ptr<float[]> src(new float[9 * 6 * 2]), dst(new float[4 * 4 * 2]);
    for (int i = 0; i < 108; ++i) src[i] = (float)i;
    for (int i = 0; i < 32; ++i) dst[i] = -7.f;
    for (int k = 0; k < 9; ++k) {
      codec::build_resize_aa_tables(9, 6, 5, 5, 4, 4, t);
      switch (k) {
        case 0: t.ys[3] = 9 - t.yn[3] + 1; break;  // the run ends past the source
        case 1: t.xs[0] = -1; break;
        case 2: t.wx[2] = 1.5f; break;
        case 3: t.wy[1] = from_bits(0x7fc00000u); break;
        case 4: t.xn.pop_back(); break;
        case 5: t.yn[0] = 0; break;
        case 6: t.wx[0] = 0.f; break;
        case 7: t.wy.pop_back(); break;
        case 8: t.ty = 18, t.yn[1] = 18; break;
      }
      CHECK(!codec::resize_aa_tables_ok(t), "tampered table %d passes the check", k);
      CHECK(throws_invalid([&] { codec::resize_crop_aa_host(src.get(), 1, 2, t, dst.get()); }),
            "tampered table %d accepted", k);
    }
    for (int i = 0; i < 32; ++i) CHECK(dst[i] == -7.f, "refused call wrote at %d", i);
    codec::build_resize_aa_tables(9, 6, 5, 5, 4, 4, t);
    CHECK(throws_invalid([&] { codec::resize_crop_aa_host(src.get(), -1, 2, t, dst.get()); }),
          "n -1");
    CHECK(throws_invalid([&] { codec::resize_crop_aa_host(src.get(), 1, 0, t, dst.get()); }),
          "C 0");
    CHECK(throws_invalid([&] { codec::resize_crop_aa_host(nullptr, 1, 2, t, dst.get()); }), "null");
  }
  if (failures) {
    fprintf(stderr, "resize_aa_check: %d failure(s)\n", failures);
    return 1;
  }
  printf("resize_aa_check OK: %ld size triples per axis, %ld refused over the limit, 4096 "
         "extremes\n", triples, refused);
  return 0;
}
