// Sanitizer run of the input resize's host plan (csrc/runtime/resize_plan.h): InputResize, the
// device image of its tables (pack) and the kernel plan bound to an uploaded copy (bind), in
// both forms. Over every (source, resize, model) size of 1..12 per axis with resize >= model
// (antialiased: source <= 8 resize), each on the rows with a seeded sample of the same triples
// on the columns and the other way round, and the 4096 extremes of resize_check /
// resize_aa_check. Checked here: every section starts on a 16-byte boundary, the sections are in
// order, do not overlap and end inside the image; every byte outside their payloads is zero;
// each payload is its table bit for bit (antialiased weights: codec::resize_aa_strided of the
// axis, the launch figures those of the codec's functions); bind gives base + offset and the
// tables' integers; apply_host is the form's host twin bit for bit, NaN and -0 among the values;
// build refuses what the two builders refuse, with their messages.
//   build/asan/resize_plan_check
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../runtime/resize_plan.h"

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

uint32_t rng_state = 0x9e3779b9u;
uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

struct Triple {
  int src, rs, out;
};

// the layout, the payloads and the bound plan of one resize
void check_image(const InputResize& r, int C) {
  char what[96];
  snprintf(what, sizeof what, "%s (%d %d %d %d %d %d)", r.antialias() ? "aa" : "plain", r.HS(),
           r.WS(), r.HR(), r.WR(), r.H(), r.W());
  CHECK(r.ok(), "%s: built resize is not ok", what);
  const ResizeDeviceImage im = pack(r);
  // an arbitrary base that is not an allocation's start
  static const uint8_t arena[64] = {};
  const uint8_t* base = arena + 16 + 4 * (rnd() % 8);
  const BoundResize b = bind(im, r, C, base);
  CHECK(b.antialias == r.antialias(), "%s: bound form", what);
  // per section: the table it stands for, its 4-byte words, and the plan's pointer to it
  const void* tab[6];
  size_t words[6];
  const void* ptr[6];
  auto section = [&](int i, const void* p, size_t n, const void* bound) {
    tab[i] = p, words[i] = n, ptr[i] = bound;
  };
  std::vector<float> wy, wx;
  if (r.antialias()) {
    const codec::ResizeAaTables& t = r.aa_tables();
    const ResizeAaPlan& p = b.aa;
    wy = codec::resize_aa_strided(t.yn, t.wy, t.ty);
    wx = codec::resize_aa_strided(t.xn, t.wx, t.tx);
    CHECK(wy.size() == (size_t)t.H * (size_t)t.ty && wx.size() == (size_t)t.W * (size_t)t.tx,
          "%s: strided sizes", what);
    section(0, t.ys.data(), t.ys.size(), p.ys), section(1, t.yn.data(), t.yn.size(), p.yn);
    section(2, wy.data(), wy.size(), p.wy);
    section(3, t.xs.data(), t.xs.size(), p.xs), section(4, t.xn.data(), t.xn.size(), p.xn);
    section(5, wx.data(), wx.size(), p.wx);
    const int band = codec::resize_aa_choose_band(t);
    CHECK(im.ty == t.ty && im.tx == t.tx && im.band == band &&
              im.band_rows == codec::resize_aa_band_rows(t, band),
          "%s: launch figures %d %d %d %d", what, im.ty, im.tx, im.band, im.band_rows);
    CHECK(p.HS == t.HS && p.WS == t.WS && p.HR == t.HR && p.WR == t.WR && p.H == t.H &&
              p.W == t.W && p.C == C && p.ty == im.ty && p.tx == im.tx && p.band == im.band &&
              p.band_rows == im.band_rows,
          "%s: bound integers", what);
  } else {
    const codec::ResizeTables& t = r.tables();
    const ResizePlan& p = b.plain;
    section(0, t.y0.data(), t.y0.size(), p.y0), section(1, t.y1.data(), t.y1.size(), p.y1);
    section(2, t.wy.data(), t.wy.size(), p.wy);
    section(3, t.x0.data(), t.x0.size(), p.x0), section(4, t.x1.data(), t.x1.size(), p.x1);
    section(5, t.wx.data(), t.wx.size(), p.wx);
    CHECK(im.ty == 0 && im.tx == 0 && im.band == 0 && im.band_rows == 0, "%s: launch figures",
          what);
    CHECK(p.HS == t.HS && p.WS == t.WS && p.H == t.H && p.W == t.W && p.C == C,
          "%s: bound integers", what);
  }
  CHECK(words[0] == (size_t)r.H() && words[1] == (size_t)r.H() && words[3] == (size_t)r.W() &&
            words[4] == (size_t)r.W(),
        "%s: table sizes", what);
  size_t end = 0;
  std::vector<uint8_t> payload(im.bytes.size(), 0);
  for (int i = 0; i < 6; ++i) {
    const size_t len = words[i] * 4;
    CHECK(im.off[i] % 16 == 0, "%s: section %d at %zu", what, i, im.off[i]);
    CHECK(im.off[i] >= end && im.off[i] + len <= im.bytes.size(),
          "%s: section %d [%zu, +%zu) after %zu in %zu bytes", what, i, im.off[i], len, end,
          im.bytes.size());
    if (im.off[i] < end || im.off[i] + len > im.bytes.size()) return;
    end = im.off[i] + len;
    memset(payload.data() + im.off[i], 1, len);
    CHECK(memcmp(im.bytes.data() + im.off[i], tab[i], len) == 0, "%s: section %d is not its table",
          what, i);
    CHECK(ptr[i] == base + im.off[i], "%s: bound pointer %d", what, i);
  }
  CHECK(im.off[0] == 0 && im.bytes.size() == ((end + 15) & ~(size_t)15), "%s: %zu bytes for %zu",
        what, im.bytes.size(), end);
  for (size_t k = 0; k < im.bytes.size(); ++k)
    if (!payload[k]) CHECK(im.bytes[k] == 0, "%s: padding byte %zu is %d", what, k, im.bytes[k]);
}

// apply_host against the form's host twin on n random images in exact-size heap blocks, NaN,
// -0, +-max and +-inf among the values
void check_apply(const InputResize& r, int C, int n) {
  const size_t sn = (size_t)n * r.HS() * r.WS() * C, dn = (size_t)n * r.H() * r.W() * C;
  std::unique_ptr<float[]> src(new float[sn]), got(new float[dn]), want(new float[dn]);
  static const uint32_t special[] = {0x7fc00000u, 0x80000000u, 0x7f7fffffu, 0xff7fffffu,
                                     0x7f800000u, 0xff800000u, 0x7fa12345u};
  for (size_t i = 0; i < sn; ++i) {
    const uint32_t v = rnd();
    src[i] = (v & 7) == 0 ? from_bits(special[(v >> 4) % 7])
                          : (float)((int)(v >> 8 & 0xffff) - 32768) / 64.f;
  }
  if (sn > 1) src[0] = from_bits(0x7fc00000u), src[1] = from_bits(0x80000000u);
  for (size_t i = 0; i < dn; ++i) got[i] = from_bits(0x7fa5a5a5u), want[i] = from_bits(0x7fb5b5b5u);
  r.apply_host(src.get(), n, C, got.get());
  if (r.antialias()) codec::resize_crop_aa_host(src.get(), n, C, r.aa_tables(), want.get());
  else codec::resize_crop_host(src.get(), n, C, r.tables(), want.get());
  CHECK(memcmp(got.get(), want.get(), dn * 4) == 0,
        "apply_host differs from the host twin (%d %d %d %d %d %d, aa %d)", r.HS(), r.WS(), r.HR(),
        r.WR(), r.H(), r.W(), (int)r.antialias());
}

void run(const Triple& y, const Triple& x, bool aa, int C, int n) {
  const InputResize r = InputResize::build(y.src, x.src, y.rs, x.rs, y.out, x.out, aa);
  CHECK(r.antialias() == aa && r.HS() == y.src && r.WS() == x.src && r.HR() == y.rs &&
            r.WR() == x.rs && r.H() == y.out && r.W() == x.out,
        "accessors of (%d %d %d %d %d %d)", y.src, x.src, y.rs, x.rs, y.out, x.out);
  check_image(r, C);
  check_apply(r, C, n);
}

// what() of the std::invalid_argument f throws, "" when it throws nothing or something else
template <typename F>
std::string refusal(F f) {
  try {
    f();
  } catch (const std::invalid_argument& e) {
    return e.what()[0] ? e.what() : "?";
  } catch (...) {
  }
  return "";
}

}  // namespace

int main() {
  long cases = 0;
  for (int aa = 0; aa < 2; ++aa) {
    std::vector<Triple> all;
    for (int s = 1; s <= 12; ++s)
      for (int rs = 1; rs <= 12; ++rs)
        for (int o = 1; o <= rs; ++o)
          if (!aa || s <= codec::kResizeAaMaxScale * rs) all.push_back({s, rs, o});
    rng_state = 0x9e3779b9u;  // the same sample on every run
    for (size_t i = 0; i < all.size(); ++i) {
      const int C = 1 + (int)(i % 3), n = 1 + (int)(i % 2);
      run(all[i], all[rnd() % all.size()], aa != 0, C, n);
      run(all[rnd() % all.size()], all[i], aa != 0, C, n);
      cases += 2;
    }
    // the 4096 extremes of resize_check / resize_aa_check, per axis and combined
    const Triple one = {1, 1, 1};
    const Triple ext[] = {{4096, 4096, 4096}, {1, 4096, 4096},    {4096, 4096, 1},
                          {4096, 1, 1},       {4096, 512, 1},     {4096, 512, 512},
                          {1, 1, 1},          {4095, 4096, 4096}, {4096, 4095, 4095},
                          {2, 4096, 4095},    {4095, 512, 2},     {4096, 513, 511}};
    for (const Triple& e : ext) {
      if (aa && e.src > codec::kResizeAaMaxScale * e.rs) continue;
      run(e, one, aa != 0, 3, 1);
      run(one, e, aa != 0, 1, 2);
      cases += 2;
    }
    const Triple both[][2] = {{{4096, 4096, 4095}, {2, 3, 2}},   {{3, 5, 4}, {4096, 4096, 4096}},
                              {{4096, 512, 511}, {2, 3, 2}},     {{3, 5, 4}, {4096, 512, 512}},
                              {{4096, 512, 1}, {4095, 512, 2}},  {{1, 4096, 64}, {1, 4096, 64}}};
    for (const auto& b : both) {
      run(b[0], b[1], aa != 0, 2, 1);
      ++cases;
    }
  }
  // refusals: what the builders refuse, with their messages; the antialias limit only there
  const int bad[][6] = {{0, 4, 4, 4, 4, 4},    {4, 0, 4, 4, 4, 4},    {4, 4, 0, 4, 0, 4},
                        {4, 4, 4, 0, 4, 0},    {4, 4, 4, 4, 0, 4},    {4, 4, 4, 4, 4, -1},
                        {4097, 4, 4, 4, 4, 4}, {4, 4097, 4, 4, 4, 4}, {4, 4, 4097, 4, 4, 4},
                        {4, 4, 4, 4097, 4, 4}, {4, 4, 4097, 4, 4097, 4}, {4, 4, 4, 4097, 4, 4097},
                        {4, 4, 3, 4, 4, 4},    {4, 4, 4, 3, 4, 4}};
  const int over[][6] = {{33, 4, 4, 4, 4, 4}, {4, 33, 4, 4, 4, 4}, {4096, 4, 511, 4, 4, 4},
                         {4, 4096, 4, 511, 4, 4}};
  for (const auto& d : bad) {
    codec::ResizeTables t;
    codec::ResizeAaTables ta;
    const std::string plain =
        refusal([&] { codec::build_resize_tables(d[0], d[1], d[2], d[3], d[4], d[5], t); });
    const std::string anti =
        refusal([&] { codec::build_resize_aa_tables(d[0], d[1], d[2], d[3], d[4], d[5], ta); });
    CHECK(!plain.empty() && !anti.empty(), "the builders accept (%d %d %d %d %d %d)", d[0], d[1],
          d[2], d[3], d[4], d[5]);
    CHECK(refusal([&] { InputResize::build(d[0], d[1], d[2], d[3], d[4], d[5], false); }) == plain,
          "build (%d %d %d %d %d %d)", d[0], d[1], d[2], d[3], d[4], d[5]);
    CHECK(refusal([&] { InputResize::build(d[0], d[1], d[2], d[3], d[4], d[5], true); }) == anti,
          "antialiased build (%d %d %d %d %d %d)", d[0], d[1], d[2], d[3], d[4], d[5]);
  }
  for (const auto& d : over) {
    codec::ResizeAaTables ta;
    const std::string anti =
        refusal([&] { codec::build_resize_aa_tables(d[0], d[1], d[2], d[3], d[4], d[5], ta); });
    CHECK(!anti.empty(), "the antialiased builder accepts (%d %d ...)", d[0], d[1]);
    CHECK(refusal([&] { InputResize::build(d[0], d[1], d[2], d[3], d[4], d[5], true); }) == anti,
          "antialiased build over the limit (%d %d ...)", d[0], d[1]);
    CHECK(InputResize::build(d[0], d[1], d[2], d[3], d[4], d[5], false).ok(),
          "plain build within its limits (%d %d ...)", d[0], d[1]);
  }
  CHECK(InputResize::build(32, 32, 4, 4, 4, 4, true).ok(), "exactly 8x");
  if (failures) {
    fprintf(stderr, "resize_plan_check: %d failure(s)\n", failures);
    return 1;
  }
  printf("resize_plan_check OK: %ld resizes in both forms, 4096 extremes\n", cases);
  return 0;
}
