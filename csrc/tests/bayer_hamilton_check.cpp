// Sanitizer run of the edge-directed Bayer demosaic on the host: bayer_hamilton_to_rgb_host
// (csrc/codec/bayer.h) against a loop form that builds the green plane on the frame reflected
// three deep and the colour-difference plane with its ring, on random, low-amplitude and striped
// frames in heap blocks of exactly their size; whole, truncated and extended records through
// PixelSource::parse_host, the parser's verdicts and PixelSource's rules for bayer_demosaic
// hamilton. Host only, no HIP call.      build/asan/bayer_hamilton_check [iterations]
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

int reflect(int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }
int clamp255(int n) { return n < 0 ? 0 : n > 255 ? 255 : n; }

// Planes, not lambdas: P = S reflected three deep, K = P - G^ on the frame and a ring of one
// (every position, as if it were an R / B site; only those are read).
std::vector<uint8_t> loop_form(const uint8_t* s, int HS, int WS, int order, int* taken) {
  const int PW = WS + 6, KW = WS + 2;
  std::vector<int> P((size_t)(HS + 6) * PW), K((size_t)(HS + 2) * KW);
  for (int y = 0; y < HS + 6; ++y)
    for (int x = 0; x < PW; ++x) P[(size_t)y * PW + x] = s[(size_t)reflect(y - 3, HS) * WS + reflect(x - 3, WS)];
  const bool gf = bayer_green_first(order);
  for (int y = -1; y <= HS; ++y)
    for (int x = -1; x <= WS; ++x) {
      const int* c = &P[(size_t)(y + 3) * PW + x + 3];
      const int hd = 2 * c[0] - c[-2] - c[2], vd = 2 * c[0] - c[-2 * PW] - c[2 * PW];
      const int dh = abs(c[-1] - c[1]) + abs(hd), dv = abs(c[-PW] - c[PW]) + abs(vd);
      const int which = dh < dv ? 0 : dv < dh ? 1 : 2;
      const int g = which == 0   ? (2 * (c[-1] + c[1]) + hd + 2) >> 2
                    : which == 1 ? (2 * (c[-PW] + c[PW]) + vd + 2) >> 2
                                 : (2 * (c[-1] + c[1] + c[-PW] + c[PW]) + hd + vd + 4) >> 3;
      K[(size_t)(y + 1) * KW + x + 1] = c[0] - clamp255(g);
      const bool site = (((x + y) & 1) != 0) == gf;  // an R / B site
      if (site && y >= 0 && y < HS && x >= 0 && x < WS) ++taken[which];
    }
  std::vector<uint8_t> rgb((size_t)HS * WS * 3);
  for (int y = 0; y < HS; ++y)
    for (int x = 0; x < WS; ++x) {
      const int* k = &K[(size_t)(y + 1) * KW + x + 1];
      const int v = s[(size_t)y * WS + x];
      const bool green = (((x + y) & 1) != 0) != gf;
      const int row_colour = ((y & 1) != 0) != bayer_blue_first(order) ? 2 : 0;  // B or R
      uint8_t* px = &rgb[((size_t)y * WS + x) * 3];
      const int g = green ? v : v - k[0];
      px[1] = (uint8_t)g;
      px[row_colour] = (uint8_t)(green ? clamp255(v + ((k[-1] + k[1] + 1) >> 1)) : v);
      px[2 - row_colour] = (uint8_t)(
          green ? clamp255(v + ((k[-KW] + k[KW] + 1) >> 1))
                : clamp255(g + ((k[-KW - 1] + k[-KW + 1] + k[KW - 1] + k[KW + 1] + 2) >> 2)));
    }
  return rgb;
}

}  // namespace

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 2000;
  std::mt19937 rng(20261128u);
  const char* const names[] = {"bayer_rggb8", "bayer_bggr8", "bayer_grbg8", "bayer_gbrg8"};
  {  // the twin's and the parser's verdicts
    uint8_t frame[16] = {0}, rgb[48];
    int im = -1;
    CHECK(!codec::bayer_hamilton_to_rgb_host(frame, 2, 8, BAYER_RGGB, rgb, nullptr), "HS 2");
    CHECK(!codec::bayer_hamilton_to_rgb_host(frame, 8, 2, BAYER_RGGB, rgb, nullptr), "WS 2");
    CHECK(!codec::bayer_hamilton_to_rgb_host(frame, 4, 4, BAYER_NONE, rgb, nullptr), "order");
    const auto parse = codec::parse_instances_raw_bayer_named_host;
    CHECK(parse(frame, 16, 2, 8, BAYER_RGGB, nullptr, -1, &im, BAYER_BILINEAR) == codec::OK, "2x8");
    CHECK(parse(frame, 16, 2, 8, BAYER_RGGB, nullptr, -1, &im, BAYER_HAMILTON) == codec::BAD_SHAPE, "2x8");
    CHECK(parse(frame, 16, 4, 4, BAYER_RGGB, nullptr, -1, &im, BAYER_HAMILTON) == codec::OK && im == 1, "4x4");
    CHECK(parse(frame, 16, 4, 4, BAYER_RGGB, nullptr, -1, &im, 3) == codec::BAD_SHAPE, "demosaic 3");
    CHECK(parse(frame, 0, 4, 4, BAYER_RGGB, nullptr, -1, &im, BAYER_HAMILTON) == codec::EMPTY, "0 bytes");
    CHECK(bayer_demosaic_of("hamilton") == BAYER_HAMILTON && bayer_demosaic_of("vng") < 0 &&
              bayer_demosaic_of("hamilto") < 0 && bayer_demosaic_of("malvar") == BAYER_MALVAR, "names");
  }
  {  // PixelSource's rules for bayer_demosaic hamilton, by their text
    const PixelSource raw = PixelSource::from_names("bayer_grbg8", nullptr, nullptr).as_raw();
    const PixelSource ha = raw.with_demosaic("hamilton");
    CHECK(ha.bayer_hamilton() && !ha.bayer_malvar() && !raw.bayer_hamilton() &&
              !ha.with_demosaic("malvar").bayer_hamilton() && ha.bayer_demosaic() == BAYER_HAMILTON &&
              ha.kind() == PixelSource::BAYER && ha.bytes(6, 10, 3) == 60, "with_demosaic");
    CHECK(!refusal([&] { ha.with_demosaic("vng"); }).empty(), "name");
    CHECK(refusal([&] { ha.check(3, false, 4, 4, true); }).empty(), "accepted");
    for (const int small : {0, 1})  // HS = 2, then WS = 2
      CHECK(refusal([&] { ha.check(3, false, small ? 32 : 2, small ? 2 : 32, true); })
                    .find("bayer_demosaic hamilton") == 0, "size under 4");
    for (const char* pf : {"rgb", "gray", "yuyv422", "p010le", "bayer_rggb10le", "bayer_gbrg12p"}) {
      const PixelSource s = PixelSource::from_names(pf, nullptr, nullptr).as_raw();
      CHECK(refusal([&] { s.with_demosaic("hamilton").check(3, false, 32, 32, true); })
                    .find("bayer_demosaic hamilton") == 0, "%s", pf);
    }
  }
  int ok = 0, bad = 0, taken[3] = {0, 0, 0};
  for (int it = 0; it < iters; ++it) {
    const int order = 1 + (int)(rng() % 4), images = 1 + (int)(rng() % 3);
    const int HS = 4 + 2 * (int)(rng() % 5), WS = 4 + 2 * (int)(rng() % 9);
    const size_t hw = (size_t)HS * WS;
    const PixelSource src =
        PixelSource::from_names(names[order - 1], nullptr, nullptr).as_raw().with_demosaic("hamilton");
    std::string s;
    std::vector<float> want;
    for (int i = 0; i < images; ++i) {
      std::unique_ptr<uint8_t[]> f(new uint8_t[hw]);  // (exactly a frame: the twin's own reads)
      const int kind = (int)(rng() % 4);  // noise with extremes, values 0..3, row or column stripes
      for (size_t e = 0; e < hw; ++e)
        f[e] = kind == 0   ? (rng() % 3 ? (uint8_t)rng() : (rng() % 2 ? 255 : 0))
               : kind == 1 ? (uint8_t)(rng() % 4)
               : ((kind == 2 ? e / WS : e % WS) & 1) ? 255 : 0;
      s.append(reinterpret_cast<const char*>(f.get()), hw);
      std::vector<uint8_t> u8(hw * 3);
      CHECK(codec::bayer_hamilton_to_rgb_host(f.get(), HS, WS, order, u8.data(), nullptr), "refused");
      CHECK(u8 == loop_form(f.get(), HS, WS, order, taken), "twin != loop form, %dx%d order %d kind %d",
            HS, WS, order, kind);
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
  printf("bayer_hamilton_check: %d records accepted, %d rejected, branches %d / %d / %d, %d failures\n",
         ok, bad, taken[0], taken[1], taken[2], failures);
  if (failures || ok == 0 || bad == 0 || !taken[0] || !taken[1] || !taken[2]) return 1;
  printf("all checks passed\n");
  return 0;
}
