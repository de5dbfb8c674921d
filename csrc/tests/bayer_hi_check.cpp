// Sanitizer run of the 10/12/16-bit Bayer host codec: bayer_hi_sample and bayer_hi_to_rgb_host
// (csrc/codec/bayer_hi.h) against a loop-form unpack, bit by bit from the layouts' definitions
// (the twin of a packed frame must equal the twin of its loop-form samples as words); frames in
// heap blocks of exactly their size, whole, truncated and extended records through
// PixelSource::parse_host, the names and PixelSource's rules. Host only, no HIP call.
//      build/asan/bayer_hi_check [iterations]
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

// Bit j of the frame, as a stream: byte j / 8, bit j mod 8.
int bit(const uint8_t* s, size_t j) { return (s[j >> 3] >> (j & 7)) & 1; }

// Sample i of a frame from the layouts' definitions, one bit at a time.
int loop_sample(const uint8_t* s, size_t i, int bits, int packing) {
  int v = 0;
  for (int k = 0; k < bits; ++k) {
    size_t j;  // where bit k of the sample sits
    if (packing == BAYER_PACK_LE16) {
      j = 16 * i + k;
    } else {
      const int n = bits == 10 ? 4 : 2, low = bits - 8;  // pixels a group, bits in its last byte
      const size_t g = i / n * (n + 1) * 8, p = i % n;
      j = k >= low ? g + 8 * p + (k - low) : g + 8 * n + low * p + k;
    }
    v |= bit(s, j) << k;
  }
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 2000;
  std::mt19937 rng(20261128u);
  const char* const orders[] = {"rggb", "bggr", "grbg", "gbrg"};
  const struct {
    const char* name;
    int bits, packing;
  } forms[] = {{"10le", 10, BAYER_PACK_LE16}, {"12le", 12, BAYER_PACK_LE16},
               {"16le", 16, BAYER_PACK_LE16}, {"10p", 10, BAYER_PACK_MIPI},
               {"12p", 12, BAYER_PACK_MIPI}};
  {  // names, byte counts and verdicts
    for (const char* bad : {"bayer_rggb8", "bayer_rggb16", "bayer_rggb16p", "bayer_rggb14le",
                            "bayer_rgbg10p", "bayer_rggb10pp", "rggb10p", "gray", ""})
      CHECK(!bayer_hi_format_of(bad).order, "%s", bad);
    const BayerHiFormat f = bayer_hi_format_of("bayer_gbrg12p");
    CHECK(f.order == BAYER_GBRG && f.bits == 12 && f.packing == BAYER_PACK_MIPI, "gbrg12p");
    CHECK(bayer_order_of("bayer_rggb16le") == BAYER_NONE, "the 8-bit parser knows no deep name");
    CHECK(bayer_hi_bytes(4, 8, 10, BAYER_PACK_MIPI) == 40 && bayer_hi_bytes(4, 6, 12, BAYER_PACK_MIPI) == 36 &&
              bayer_hi_bytes(4, 6, 12, BAYER_PACK_LE16) == 48, "bytes");
    CHECK(!bayer_hi_bytes(4, 6, 10, BAYER_PACK_MIPI) && !bayer_hi_bytes(3, 4, 16, BAYER_PACK_LE16) &&
              !bayer_hi_bytes(4, 4, 16, BAYER_PACK_MIPI) && !bayer_hi_bytes(4, 4, 14, BAYER_PACK_LE16) &&
              !bayer_hi_bytes(4, 4, 8, BAYER_PACK_NONE), "no frame");
    uint8_t frame[40] = {0};
    uint16_t rgb[96];
    int im = -1;
    CHECK(!codec::bayer_hi_to_rgb_host(frame, 2, 8, BAYER_RGGB, 10, BAYER_PACK_MIPI, true, rgb, nullptr), "malvar HS 2");
    CHECK(!codec::bayer_hi_to_rgb_host(frame, 4, 4, BAYER_NONE, 16, BAYER_PACK_LE16, false, rgb, nullptr), "order");
    const auto parse = codec::parse_instances_raw_bayer_hi_host;
    CHECK(parse(frame, 40, 4, 8, BAYER_RGGB, 10, BAYER_PACK_MIPI, nullptr, -1, &im, true) == codec::OK && im == 1, "4x8");
    CHECK(parse(frame, 20, 2, 8, BAYER_RGGB, 10, BAYER_PACK_MIPI, nullptr, -1, &im, true) == codec::BAD_SHAPE, "2x8");
    CHECK(parse(frame, 0, 4, 8, BAYER_RGGB, 10, BAYER_PACK_MIPI, nullptr, -1, &im, false) == codec::EMPTY, "0 bytes");
    CHECK(parse(frame, 39, 4, 8, BAYER_RGGB, 10, BAYER_PACK_MIPI, nullptr, -1, &im, false) == codec::BAD_SHAPE, "B - 1");
    CHECK(parse(frame, 30, 4, 6, BAYER_RGGB, 10, BAYER_PACK_MIPI, nullptr, -1, &im, false) == codec::BAD_SHAPE, "WS 6");
    CHECK(parse(frame, 40, 4, 8, BAYER_RGGB, 10, BAYER_PACK_MIPI, nullptr, 0, &im, false) == codec::TOO_LARGE, "max");
  }
  {  // PixelSource: kind BAYER with bits and packing, and the new refusal by its text
    const PixelSource p10 = PixelSource::from_names("bayer_grbg10p", nullptr, nullptr).as_raw();
    CHECK(p10.kind() == PixelSource::BAYER && p10.bayer_hi() && p10.bayer_bits() == 10 &&
              p10.bayer_order() == BAYER_GRBG && p10.bytes(6, 12, 3) == 90, "10p source");
    const PixelSource::Dims d = p10.ingest_dims(6, 12, 3);
    CHECK(d.H == 6 && d.W == 15 && d.C == 1, "ingest dims");
    CHECK(!PixelSource::from_names("bayer_grbg8", nullptr, nullptr).bayer_hi(), "8-bit");
    CHECK(refusal([&] { p10.with_demosaic("malvar").check(3, false, 4, 4, true); }).empty(), "ok");
    CHECK(refusal([&] { p10.check(3, false, 4, 6, true); }) ==
              "pixel_format bayer_*10p needs a record-side W that is a multiple of 4", "WS 6");
  }
  int ok = 0, bad = 0;
  for (int it = 0; it < iters; ++it) {
    const auto& form = forms[rng() % 5];
    const int order = 1 + (int)(rng() % 4), images = 1 + (int)(rng() % 3);
    const bool malvar = rng() & 1;
    const int HS = (malvar ? 4 : 2) + 2 * (int)(rng() % 5);
    int WS = (malvar ? 4 : 2) + 2 * (int)(rng() % 9);
    if (form.packing == BAYER_PACK_MIPI && form.bits == 10) WS = (WS + 3) & ~3;
    const size_t hw = (size_t)HS * WS, B = (size_t)bayer_hi_bytes(HS, WS, form.bits, form.packing);
    CHECK(B == hw * (form.packing == BAYER_PACK_LE16 ? 16 : form.bits) / 8, "bytes %zu", B);
    const std::string name = std::string("bayer_") + orders[order - 1] + form.name;
    const PixelSource src = PixelSource::from_names(name, nullptr, nullptr)
                                .as_raw()
                                .with_demosaic(malvar ? "malvar" : "bilinear");
    CHECK(src.bytes(HS, WS, 3) == (int64_t)B, "%s: source bytes", name.c_str());
    std::string s;
    std::vector<float> want;
    for (int i = 0; i < images; ++i) {
      std::unique_ptr<uint8_t[]> f(new uint8_t[B]);  // (exactly a frame: the twin's own reads)
      for (size_t e = 0; e < B; ++e) f[e] = rng() % 4 ? (uint8_t)rng() : (rng() % 2 ? 255 : 0);
      // the loop-form samples, as a frame of masked words: the twin must see the same mosaic
      std::unique_ptr<uint8_t[]> le(new uint8_t[2 * hw]);
      for (size_t e = 0; e < hw; ++e) {
        const int raw = loop_sample(f.get(), e, form.packing == BAYER_PACK_LE16 ? 16 : form.bits,
                                    form.packing);
        const int v = raw & ((1 << form.bits) - 1);
        CHECK(bayer_hi_sample(f.get(), e, form.bits, form.packing) == v, "%s sample %zu",
              name.c_str(), e);
        le[2 * e] = (uint8_t)v, le[2 * e + 1] = (uint8_t)(v >> 8);
      }
      s.append(reinterpret_cast<const char*>(f.get()), B);
      std::vector<uint16_t> u16(hw * 3), ref(hw * 3);
      std::vector<float> f32(hw * 3);
      CHECK(codec::bayer_hi_to_rgb_host(f.get(), HS, WS, order, form.bits, form.packing, malvar,
                                        u16.data(), f32.data()), "refused");
      CHECK(codec::bayer_hi_to_rgb_host(le.get(), HS, WS, order, form.bits, BAYER_PACK_LE16, malvar,
                                        ref.data(), nullptr) && u16 == ref,
            "%s: the twin differs from the twin of the loop-form samples", name.c_str());
      for (size_t e = 0; e < hw * 3; ++e) CHECK(f32[e] == (float)u16[e], "float of %d", u16[e]);
      want.insert(want.end(), f32.begin(), f32.end());
    }
    const int cut = (int)(rng() % 3);  // whole, truncated, extended
    if (cut == 1) s.resize(rng() % s.size());
    if (cut == 2) s.append(1 + rng() % 5, (char)rng());
    std::unique_ptr<uint8_t[]> buf(new uint8_t[s.size() ? s.size() : 1]);
    memcpy(buf.get(), s.data(), s.size());
    std::vector<float> got(want.size(), -1.f);
    int im = -1;
    const int st = src.parse_host(buf.get(), s.size(), HS, WS, 3, got.data(), -1, &im);
    const bool whole = s.size() && s.size() % B == 0;
    CHECK(st == (whole ? codec::OK : s.empty() ? codec::EMPTY : codec::BAD_SHAPE), "status %d", st);
    CHECK(im == (whole ? (int)(s.size() / B) : 0), "image count %d", im);
    got.resize((size_t)im * hw * 3), want.resize(got.size());  // (a whole prefix of the frames)
    CHECK(got == want, "parsed frames differ from the twin");
    st == codec::OK ? ++ok : ++bad;
  }
  printf("bayer_hi_check: %d records accepted, %d rejected, %d failures\n", ok, bad, failures);
  if (failures || ok == 0 || bad == 0) return 1;
  printf("all checks passed\n");
  return 0;
}
