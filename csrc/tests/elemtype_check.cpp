// Sanitizer run of the typed tensor records' host side (csrc/codec/elemtype.h, the typed parser of
// json_codec.h and PixelSource's fourth arm): the names and byte counts; float32(x) of all 65 536
// patterns of the 16-bit types against an independent conversion (ldexp on the fields) and of
// f32 patterns against the bits themselves, with the non-finite verdict; PixelSource::with_elem
// (kind, bytes, ingest dimensions, every refusal by its text, the ingest rule); and
// parse_instances_typed_host against a plain decode of the record's own bytes, through
// PixelSource::parse_host too, on valid records and a few thousand mutated and truncated ones -
// the mutation scheme of pixel_source_check.cpp, every input in a heap block of exactly its size.
// Host only, no HIP call.
//   build/asan/elemtype_check [records per type]
#include <math.h>
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

template <typename F>
std::string refusal(F f) {
  try {
    f();
  } catch (const std::invalid_argument& e) {
    return e.what();
  }
  return "";
}

uint32_t bits_of(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}

// binary16 -> binary32 from the fields, in double (exact), independent of elemtype.h
float half_by_fields(uint32_t h, bool* finite) {
  const int e = (h >> 10) & 31, m = h & 0x3FF;
  *finite = e != 31;
  double v = e == 0 ? ldexp((double)m, -24) : ldexp((double)(m + 1024), e - 25);
  if (e == 31) v = m ? NAN : INFINITY;
  return (float)((h & 0x8000) ? -v : v);
}

const int kTyped[] = {ELEM_U16, ELEM_F16, ELEM_BF16, ELEM_F32};
struct Shape {
  int HS, WS, C;
};
const Shape kShapes[] = {{1, 1, 1}, {1, 2, 1}, {5, 7, 1}, {5, 7, 3}, {2, 3, 5}};

// The record's floats and verdict by a plain decode of its own bytes.
bool expect(const std::vector<std::vector<uint8_t>>& strings, int t, std::vector<float>& want) {
  bool finite = true;
  want.clear();
  for (const auto& v : strings) {
    const int E = elem_bytes(t);
    for (size_t i = 0; i + E <= v.size(); i += E) {
      uint32_t raw = 0;
      for (int j = 0; j < E; ++j) raw |= (uint32_t)v[i + j] << (8 * j);
      float f;
      bool fin = true;
      if (t == ELEM_U16) {
        f = (float)raw;
      } else if (t == ELEM_F16) {
        f = half_by_fields(raw, &fin);
      } else {
        const uint32_t b = t == ELEM_BF16 ? raw << 16 : raw;
        memcpy(&f, &b, 4);
        fin = ((b >> 23) & 0xFF) != 0xFF;
      }
      finite &= fin;
      want.push_back(f);
    }
  }
  return finite;
}

// The typed parser, directly and through PixelSource, decoding and validating only, on an
// exact-size heap copy of `s`; returns the status.
int parse_all(const PixelSource& src, int t, const std::string& s, const Shape& sh,
              int max_images, std::vector<float>* got, int* images) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[s.size() ? s.size() : 1]);
  memcpy(buf.get(), s.data(), s.size());
  const size_t per = (size_t)(sh.HS > 0 ? sh.HS : 0) * sh.WS * (size_t)sh.C;
  const size_t cap = s.size() / 4 + 1;  // (room for every image a record this long could hold)
  std::vector<float> a(cap * per, -1.f), b(cap * per, -1.f);
  int ia = -1, ib = -1, iv = -1;
  const int sa = codec::parse_instances_typed_host(buf.get(), s.size(), sh.HS, sh.WS, sh.C, t,
                                                   a.data(), max_images, &ia);
  const int sb = src.parse_host(buf.get(), s.size(), sh.HS, sh.WS, sh.C, b.data(), max_images,
                                &ib);
  const int sv = codec::parse_instances_typed_host(buf.get(), s.size(), sh.HS, sh.WS, sh.C, t,
                                                   nullptr, max_images, &iv);
  CHECK(sa == sb && ia == ib, "%s: parser %d (%d images) != parse_host %d (%d)",
        elem_type_name(t), sa, ia, sb, ib);
  CHECK(sv == sa && iv == ia, "%s: validate-only %d (%d) != %d (%d)", elem_type_name(t), sv, iv,
        sa, ia);
  if (sa == codec::OK)
    CHECK(memcmp(a.data(), b.data(), (size_t)ia * per * sizeof(float)) == 0, "%s: floats differ",
          elem_type_name(t));
  else
    CHECK(ia == 0, "%s: %d images with status %d", elem_type_name(t), ia, sa);
  if (got) got->assign(a.begin(), a.begin() + (sa == codec::OK ? (size_t)ia * per : 0));
  if (images) *images = ia;
  return sa;
}

}  // namespace

int main(int argc, char** argv) {
  const int per_type = argc > 1 ? atoi(argv[1]) : 800;
  std::mt19937 rng(20261021u);
  int ok = 0, bad = 0;

  // ---- names and sizes -------------------------------------------------------------------------
  static const char* const kNames[] = {"u8", "u16", "f16", "bf16", "f32"};
  static const int kBytes[] = {1, 2, 2, 2, 4};
  for (int t = 0; t < kElemTypes; ++t) {
    CHECK(elem_type_of(kNames[t]) == t && !strcmp(elem_type_name(t), kNames[t]), "name %d", t);
    CHECK(elem_bytes(t) == kBytes[t], "bytes of %s", kNames[t]);
    CHECK(typed_bytes(5, 7, 3, t) == 105 * kBytes[t] && typed_bytes(0, 7, 3, t) == 0 &&
              typed_bytes(5, -1, 3, t) == 0 && typed_bytes(5, 7, 0, t) == 0,
          "typed_bytes of %s", kNames[t]);
  }
  for (const char* n : {"", "U16", "fp16", "f64", "i16", "u8 ", "float"})
    CHECK(elem_type_of(n) == -1, "name %s accepted", n);
  CHECK(elem_bytes(-1) == 0 && elem_bytes(5) == 0 && typed_bytes(5, 7, 3, 9) == 0, "unknown type");

  // ---- float32(x), every 16-bit pattern; f32 patterns ------------------------------------------
  for (uint32_t h = 0; h < 65536; ++h) {
    const uint8_t le[2] = {(uint8_t)h, (uint8_t)(h >> 8)};
    float f = -1.f;
    CHECK(codec::typed_to_float_host(le, 1, ELEM_U16, &f) && f == (float)h, "u16 %u", h);
    bool fin = true;
    const float want = half_by_fields(h, &fin);
    CHECK(codec::typed_to_float_host(le, 1, ELEM_F16, &f) == fin, "f16 %04x: verdict", h);
    if (fin)
      CHECK(bits_of(f) == bits_of(want), "f16 %04x: %08x != %08x", h, bits_of(f), bits_of(want));
    else
      CHECK(((bits_of(f) >> 23) & 0xFF) == 0xFF && (bits_of(f) & 0x7FFFFF) == (h & 0x3FF) << 13 &&
                bits_of(f) >> 31 == h >> 15,
            "f16 %04x: non-finite bits %08x", h, bits_of(f));
    const bool bfin = ((h >> 7) & 0xFF) != 0xFF;
    CHECK(codec::typed_to_float_host(le, 1, ELEM_BF16, &f) == bfin && bits_of(f) == h << 16,
          "bf16 %04x", h);
  }
  {
    std::vector<uint32_t> pats = {0u, 0x80000000u, 1u, 0x80000001u, 0x007FFFFFu, 0x00800000u,
                                  0x7F7FFFFFu, 0xFF7FFFFFu, 0x7F800000u, 0xFF800000u, 0x7FC00000u,
                                  0x7F800001u, 0xFFFFFFFFu, 0x3F800000u};
    for (int i = 0; i < 100000; ++i) pats.push_back((uint32_t)rng());
    for (uint32_t b : pats) {
      const uint8_t le[4] = {(uint8_t)b, (uint8_t)(b >> 8), (uint8_t)(b >> 16), (uint8_t)(b >> 24)};
      float f = -1.f;
      const bool fin = ((b >> 23) & 0xFF) != 0xFF;
      CHECK(codec::typed_to_float_host(le, 1, ELEM_F32, &f) == fin && bits_of(f) == b,
            "f32 %08x", b);
    }
    float f = -1.f;
    const uint8_t z[4] = {0, 0, 0, 0};
    CHECK(!codec::typed_to_float_host(z, 1, 7, &f) && f == -1.f, "unknown type wrote");
    // an unaligned source, n = 0
    std::unique_ptr<uint8_t[]> buf(new uint8_t[9]);
    for (int i = 0; i < 9; ++i) buf[i] = (uint8_t)(0x3C + i);
    float two[2];
    CHECK(codec::typed_to_float_host(buf.get() + 1, 2, ELEM_F32, two), "unaligned");
    CHECK(codec::typed_to_float_host(buf.get() + 9, 0, ELEM_F32, two), "n = 0");
  }

  // ---- PixelSource's fourth arm ----------------------------------------------------------------
  {
    const PixelSource rgb = PixelSource::from_names("rgb", nullptr, nullptr);
    CHECK(rgb.with_elem("u8").kind() == PixelSource::RGB && rgb.with_elem("u8").elem() == ELEM_U8 &&
              rgb.with_elem("u8").wants_ingest_decode(),
          "u8 is not the rgb source");
    CHECK(PixelSource().elem() == ELEM_U8, "default element type");
    for (int t : kTyped) {
      const PixelSource s = rgb.with_elem(elem_type_name(t));
      CHECK(s.kind() == PixelSource::TYPED && s.elem() == t && !s.wants_ingest_decode() &&
                s.yuv_format() == YUV_NONE && s.packed_format() == PACKED_NONE,
            "%s: kind", elem_type_name(t));
      for (const Shape& sh : kShapes) {
        const int64_t want = (int64_t)sh.HS * sh.WS * sh.C * elem_bytes(t);
        CHECK(s.bytes(sh.HS, sh.WS, sh.C) == want, "%s: bytes", elem_type_name(t));
        const PixelSource::Dims d = s.ingest_dims(sh.HS, sh.WS, sh.C);
        CHECK(d.H == sh.HS && d.W == sh.WS * elem_bytes(t) && d.C == sh.C &&
                  (int64_t)d.H * d.W * d.C == want,
              "%s: ingest dims", elem_type_name(t));
      }
      for (int C : {1, 3, 7})
        for (bool nchw : {false, true}) {
          CHECK(refusal([&] { s.check(C, nchw, 5, 7, true); }).empty(), "%s refused",
                elem_type_name(t));
          CHECK(refusal([&] { s.check(C, nchw, 5, 7, false); }) ==
                    std::string("input_dtype ") + elem_type_name(t) + " needs input_format b64",
                "%s: json", elem_type_name(t));
        }
      // per-channel coefficients: refused past four channels only
      CHECK(refusal([&] { s.check(4, false, 5, 7, true, false); }).empty(), "%s: C = 4",
            elem_type_name(t));
      CHECK(refusal([&] { s.check(5, false, 5, 7, true, false); }) ==
                std::string("input_dtype ") + elem_type_name(t) +
                    ": per-channel input_a / input_b need C <= 4",
            "%s: C = 5, per-channel", elem_type_name(t));
      for (const char* pf : {"i420", "nv12", "bgr24", "rgba", "bgra", "gray"}) {
        const PixelSource other = PixelSource::from_names(pf, nullptr, nullptr);
        CHECK(refusal([&] { other.with_elem(elem_type_name(t)); }) ==
                  std::string("input_dtype ") + elem_type_name(t) + " needs pixel_format rgb",
              "%s with %s", elem_type_name(t), pf);
        CHECK(other.with_elem("u8").kind() == other.kind(), "u8 with %s", pf);
      }
    }
    for (const char* n : {"", "F16", "f64", "half"})
      CHECK(refusal([&] { rgb.with_elem(n); }) == "input_dtype: u8, u16, f16, bf16 or f32",
            "name %s", n);
  }

  // ---- the parser on valid, planted, mutated and truncated records -----------------------------
  for (int t : kTyped) {
    const PixelSource src = PixelSource().with_elem(elem_type_name(t));
    const int E = elem_bytes(t);
    for (int it = 0; it < per_type; ++it) {
      const Shape sh = kShapes[rng() % 5];
      const int images = 1 + (int)(rng() % 3);
      const size_t per = (size_t)sh.HS * sh.WS * sh.C;
      std::vector<std::vector<uint8_t>> strings;
      for (int i = 0; i < images; ++i) {
        std::vector<uint8_t> v(per * E);
        for (uint8_t& b : v) b = (uint8_t)rng();
        // keep the random elements finite: clear one exponent bit
        if (t != ELEM_U16)
          for (size_t e = 0; e < per; ++e) v[e * E + E - 1] &= 0xBF;  // (bit 14 / bit 30)
        strings.push_back(v);
      }
      std::vector<float> want, got;
      int n = 0;
      if (it % 8 == 0) {  // valid
        CHECK(expect(strings, t, want), "%s: the generator made a non-finite", elem_type_name(t));
        std::string s = record(strings, rng() % 2 != 0);
        CHECK(parse_all(src, t, s, sh, -1, &got, &n) == codec::OK && n == images,
              "%s: valid record rejected", elem_type_name(t));
        CHECK(got.size() == want.size() &&
                  memcmp(got.data(), want.data(), want.size() * sizeof(float)) == 0,
              "%s %dx%dx%d: floats", elem_type_name(t), sh.HS, sh.WS, sh.C);
        if (images > 1)
          CHECK(parse_all(src, t, s, sh, images - 1, nullptr, nullptr) == codec::TOO_LARGE,
                "%s: max_images", elem_type_name(t));
        CHECK(parse_all(src, t, s, Shape{0, sh.WS, sh.C}, -1, nullptr, nullptr) ==
                  codec::BAD_SHAPE,
              "%s: a zero size", elem_type_name(t));
        ++ok;
        continue;
      }
      if (it % 8 == 1 && t != ELEM_U16) {  // a non-finite element, first or last of an image
        auto& v = strings[rng() % images];
        const size_t e = rng() % 2 ? 0 : per - 1;
        const int cls = (int)(rng() % 4);  // +Inf, -Inf, quiet NaN, NaN with mantissa bit 0 only
        uint32_t raw = t == ELEM_F16 ? 0x7C00u : t == ELEM_BF16 ? 0x7F80u : 0x7F800000u;
        if (cls == 1) raw |= t == ELEM_F32 ? 0x80000000u : 0x8000u;
        if (cls == 2) raw |= t == ELEM_F16 ? 0x0200u : t == ELEM_BF16 ? 0x0040u : 0x00400000u;
        if (cls == 3) raw |= 1u;
        for (int j = 0; j < E; ++j) v[e * E + j] = (uint8_t)(raw >> (8 * j));
        CHECK(!expect(strings, t, want), "plant");
        CHECK(parse_all(src, t, record(strings, false), sh, -1, nullptr, nullptr) ==
                  codec::BAD_NUMBER,
              "%s: non-finite class %d accepted", elem_type_name(t), cls);
        ++bad;
        continue;
      }
      if (it % 8 == 2) {  // a bad character, and a non-'=' in the padding
        std::string s = record(strings, false);
        const size_t q = s.find("\"b64\":\"") + 7;
        const size_t L = (size_t)codec::b64_chars_bytes((int64_t)per * E);
        const size_t pad = (3 - per * E % 3) % 3;
        std::string s1 = s;
        s1[q + rng() % (L - pad)] = '-';
        CHECK(parse_all(src, t, s1, sh, -1, nullptr, nullptr) == codec::BAD_NUMBER,
              "%s: bad character accepted", elem_type_name(t));
        if (pad) {
          s1 = s;
          s1[q + L - 1] = 'A';
          CHECK(parse_all(src, t, s1, sh, -1, nullptr, nullptr) == codec::BAD_NUMBER,
                "%s: bad padding accepted", elem_type_name(t));
        }
        ++bad;
        continue;
      }
      std::string s = record(strings, rng() % 2 != 0);
      const int muts = 1 + (int)(rng() % 3);
      for (int m = 0; m < muts && !s.empty(); ++m) {
        const size_t at = rng() % s.size();
        static const char kBytes2[] = "{}[]\",:\\=-_ \nAb64/+nul\x80\xff\0";
        const char c = kBytes2[rng() % (sizeof(kBytes2) - 1)];
        switch (rng() % 5) {
          case 0: s[at] = c; break;
          case 1: s.erase(at, 1 + rng() % 3); break;
          case 2: s.insert(at, 1 + rng() % 3, c); break;
          case 3: s.resize(at); break;                         // truncated
          default: s[at] = (char)rng(); break;
        }
      }
      parse_all(src, t, s, sh, -1, nullptr, nullptr) == codec::OK ? ++ok : ++bad;
    }
  }
  printf("elemtype_check: %d records accepted, %d rejected, %d failures\n", ok, bad, failures);
  if (failures || ok == 0 || bad == 0) return 1;
  printf("elemtype_check OK\n");
  return 0;
}
