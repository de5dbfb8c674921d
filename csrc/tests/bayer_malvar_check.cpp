// Sanitizer run of the gradient-corrected Bayer demosaic on the host: bayer_malvar_to_rgb_host
// (csrc/codec/bayer.h) against a loop form over the paper's four 5 x 5 kernels (times 2) on random
// frames in heap blocks of exactly their size, whole, truncated and extended records through
// PixelSource::parse_host, the parser's verdicts and PixelSource's rules for bayer_demosaic.
// Host only, no HIP call.      build/asan/bayer_malvar_check [iterations]
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
#define CHECK(cond, ...)                                                                    \
  do {                                                                                      \
    if (!(cond)) ++failures, fprintf(stderr, "FAIL line %d: ", __LINE__), fprintf(stderr, __VA_ARGS__), fputc('\n', stderr); \
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

// Malvar's kernels times 2, rows dy = -2 .. 2: G at R / B; R / B at a green site of its own row
// (transposed: of its own column); the opposite colour at R / B.
const int kCross[5][5] = {{0, 0, -2, 0, 0}, {0, 0, 4, 0, 0}, {-2, 4, 8, 4, -2}, {0, 0, 4, 0, 0}, {0, 0, -2, 0, 0}};
const int kRow[5][5] = {{0, 0, 1, 0, 0}, {0, -2, 0, -2, 0}, {-2, 8, 10, 8, -2}, {0, -2, 0, -2, 0}, {0, 0, 1, 0, 0}};
const int kDiag[5][5] = {{0, 0, -3, 0, 0}, {0, 4, 0, 4, 0}, {-3, 0, 12, 0, -3}, {0, 4, 0, 4, 0}, {0, 0, -3, 0, 0}};

int reflect(int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }

std::vector<uint8_t> loop_form(const uint8_t* s, int HS, int WS, int order) {
  std::vector<uint8_t> rgb((size_t)HS * WS * 3);
  const auto tap = [&](const int (*k)[5], bool transposed, int y, int x) {
    int n = 0;
    for (int dy = -2; dy <= 2; ++dy)
      for (int dx = -2; dx <= 2; ++dx)
        n += (transposed ? k[dx + 2][dy + 2] : k[dy + 2][dx + 2]) *
             s[(size_t)reflect(y + dy, HS) * WS + reflect(x + dx, WS)];
    n = (n + 8) >> 4;
    return (uint8_t)(n < 0 ? 0 : n > 255 ? 255 : n);
  };
  for (int y = 0; y < HS; ++y)
    for (int x = 0; x < WS; ++x) {
      const bool green = (((x + y) & 1) != 0) != bayer_green_first(order);
      const int row_colour = ((y & 1) != 0) != bayer_blue_first(order) ? 2 : 0;  // B or R
      uint8_t* px = &rgb[((size_t)y * WS + x) * 3];
      const uint8_t v = s[(size_t)y * WS + x];
      px[1] = green ? v : tap(kCross, false, y, x);
      px[row_colour] = green ? tap(kRow, false, y, x) : v;
      px[2 - row_colour] = green ? tap(kRow, true, y, x) : tap(kDiag, false, y, x);
    }
  return rgb;
}

}  // namespace

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 2000;
  std::mt19937 rng(20261127u);
  const char* const names[] = {"bayer_rggb8", "bayer_bggr8", "bayer_grbg8", "bayer_gbrg8"};
  {  // the twin's and the parser's verdicts
    uint8_t frame[16] = {0}, rgb[48];
    int im = -1;
    CHECK(!codec::bayer_malvar_to_rgb_host(frame, 2, 8, BAYER_RGGB, rgb, nullptr), "HS 2");
    CHECK(!codec::bayer_malvar_to_rgb_host(frame, 8, 2, BAYER_RGGB, rgb, nullptr), "WS 2");
    CHECK(!codec::bayer_malvar_to_rgb_host(frame, 4, 4, BAYER_NONE, rgb, nullptr), "order");
    const auto parse = codec::parse_instances_raw_bayer_demosaic_host;
    CHECK(parse(frame, 16, 2, 8, BAYER_RGGB, nullptr, -1, &im, false) == codec::OK, "bilinear 2x8");
    CHECK(parse(frame, 16, 2, 8, BAYER_RGGB, nullptr, -1, &im, true) == codec::BAD_SHAPE, "2x8");
    CHECK(parse(frame, 16, 4, 4, BAYER_RGGB, nullptr, -1, &im, true) == codec::OK && im == 1, "4x4");
    CHECK(parse(frame, 0, 4, 4, BAYER_RGGB, nullptr, -1, &im, true) == codec::EMPTY, "0 bytes");
  }
  {  // PixelSource's rules for bayer_demosaic, by their text
    const PixelSource raw = PixelSource::from_names("bayer_grbg8", nullptr, nullptr).as_raw();
    const PixelSource mv = raw.with_demosaic("malvar");
    CHECK(mv.bayer_malvar() && !raw.bayer_malvar() && !mv.with_demosaic("bilinear").bayer_malvar() &&
              mv.kind() == PixelSource::BAYER && mv.bytes(6, 10, 3) == 60, "with_demosaic");
    CHECK(refusal([&] { raw.with_demosaic("vng"); }) == "bayer_demosaic: bilinear or malvar", "name");
    CHECK(refusal([&] { mv.check(3, false, 4, 4, true); }).empty(), "accepted");
    CHECK(refusal([&] { raw.check(3, false, 2, 2, true); }).empty(), "bilinear 2x2");
    for (const int small : {0, 1})  // HS = 2, then WS = 2
      CHECK(refusal([&] { mv.check(3, false, small ? 32 : 2, small ? 2 : 32, true); })
                    .find("bayer_demosaic malvar") == 0, "size under 4");
    for (const char* pf : {"rgb", "gray", "yuyv422", "p010le"}) {
      const PixelSource s = PixelSource::from_names(pf, nullptr, nullptr).as_raw();
      CHECK(refusal([&] { s.with_demosaic("malvar").check(3, false, 32, 32, true); })
                    .find("bayer_demosaic malvar") == 0, "%s", pf);
      CHECK(refusal([&] { s.with_demosaic("bilinear").check(3, false, 32, 32, true); }).empty(),
            "%s: bilinear", pf);
    }
  }
  int ok = 0, bad = 0;
  for (int it = 0; it < iters; ++it) {
    const int order = 1 + (int)(rng() % 4), images = 1 + (int)(rng() % 3);
    const int HS = 4 + 2 * (int)(rng() % 5), WS = 4 + 2 * (int)(rng() % 9);
    const size_t hw = (size_t)HS * WS;
    const PixelSource src =
        PixelSource::from_names(names[order - 1], nullptr, nullptr).as_raw().with_demosaic("malvar");
    std::string s;
    std::vector<float> want;
    for (int i = 0; i < images; ++i) {
      std::unique_ptr<uint8_t[]> f(new uint8_t[hw]);  // (exactly a frame: the twin's own reads)
      for (size_t e = 0; e < hw; ++e) f[e] = rng() % 3 ? (uint8_t)rng() : (rng() % 2 ? 255 : 0);
      s.append(reinterpret_cast<const char*>(f.get()), hw);
      std::vector<uint8_t> u8(hw * 3);
      CHECK(codec::bayer_malvar_to_rgb_host(f.get(), HS, WS, order, u8.data(), nullptr), "refused");
      CHECK(u8 == loop_form(f.get(), HS, WS, order), "twin != loop form, %dx%d order %d", HS, WS,
            order);
      want.insert(want.end(), u8.begin(), u8.end());
    }
    const int cut = (int)(rng() % 3);  // whole, truncated, extended
    if (cut == 1) s.resize(rng() % s.size());
    if (cut == 2) s.append(1 + rng() % 5, (char)rng());
    std::unique_ptr<uint8_t[]> buf(new uint8_t[s.size() ? s.size() : 1]);
    memcpy(buf.get(), s.data(), s.size());
    std::vector<float> got(want.size(), -1.f);
    int im = -1;
    const int st = src.parse_host(buf.get(), s.size(), HS, WS, 3, got.data(), -1, &im);
    const bool whole = s.size() && s.size() % hw == 0;
    CHECK(st == (whole ? codec::OK : s.empty() ? codec::EMPTY : codec::BAD_SHAPE), "status %d", st);
    CHECK(im == (whole ? (int)(s.size() / hw) : 0), "image count %d", im);
    got.resize((size_t)im * hw * 3), want.resize(got.size());  // (a whole prefix of the frames)
    CHECK(got == want, "parsed frames differ from the twin");
    st == codec::OK ? ++ok : ++bad;
  }
  printf("bayer_malvar_check: %d records accepted, %d rejected, %d failures\n", ok, bad, failures);
  if (failures || ok == 0 || bad == 0) return 1;
  printf("all checks passed\n");
  return 0;
}
