// Sanitizer run of the YUV 4:2:0 host codec (csrc/codec/yuv.h, csrc/codec/json_codec.h) on
// untrusted input: the conversion twin, the frame-record decoder and the byte-count forms of the
// scan, the offsets helper and the splitter. A fixed seed, valid records of several frame sizes
// in both formats and a few thousand mutated and truncated copies. Every input lives in a heap
// block of exactly its size, so AddressSanitizer sees any access past n. Checks that every status
// is one of the format's verdicts, that the functions agree with each other, that a valid record
// decodes to the conversion of its frames and that I420 and NV12 records of the same planes give
// the same image. Host only, no HIP call.
//   build/asan/yuv_check [iterations]
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

std::string b64(const std::vector<uint8_t>& v) {  // (v.size() is a multiple of 3)
  static const char kA[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  std::string s;
  for (size_t i = 0; i + 2 < v.size(); i += 3) {
    const uint32_t x = ((uint32_t)v[i] << 16) | ((uint32_t)v[i + 1] << 8) | v[i + 2];
    s += kA[(x >> 18) & 63];
    s += kA[(x >> 12) & 63];
    s += kA[(x >> 6) & 63];
    s += kA[x & 63];
  }
  return s;
}

struct Size {
  int HS, WS;
};

// planes Y [HS][WS], U, V [HS/2][WS/2] -> the frame in `format`
std::vector<uint8_t> pack(const std::vector<uint8_t>& Y, const std::vector<uint8_t>& U,
                          const std::vector<uint8_t>& V, int format) {
  std::vector<uint8_t> f(Y);
  if (format == YUV_I420) {
    f.insert(f.end(), U.begin(), U.end());
    f.insert(f.end(), V.begin(), V.end());
  } else {
    for (size_t i = 0; i < U.size(); ++i) {
      f.push_back(U[i]);
      f.push_back(V[i]);
    }
  }
  return f;
}

std::string record(const std::vector<std::vector<uint8_t>>& frames, bool spaces) {
  const char* ws = spaces ? " \n" : "";
  std::string s = std::string(ws) + "{" + ws + "\"instances\"" + ws + ":" + ws + "[";
  for (size_t i = 0; i < frames.size(); ++i) {
    if (i) s += std::string(ws) + ",";
    s += std::string(ws) + "{" + ws + "\"b64\"" + ws + ":" + ws + "\"" + b64(frames[i]) + "\"" +
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

// Runs everything on an exact-size heap copy of `s`; returns the decoder's status.
int run(const std::string& s, const Size& sz, int format, const YuvCoeffs& k,
        std::vector<float>* decoded) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[s.size() ? s.size() : 1]);
  memcpy(buf.get(), s.data(), s.size());
  const uint8_t* p = buf.get();
  const size_t n = s.size();
  const int64_t B = yuv420_bytes(sz.HS, sz.WS);
  const size_t L = (size_t)codec::b64_chars_bytes(B);
  const codec::Scan sc = codec::scan_instances_b64_bytes(p, n, B);
  CHECK(known_status(sc.status, false), "scan status %d", sc.status);
  // the byte-count form and the (H, W, C) form of the same byte count agree
  const codec::Scan sc3 = codec::scan_instances_b64(p, n, sz.HS / 2, sz.WS, 3);
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
  const int st = codec::parse_instances_yuv_host(p, n, sz.HS, sz.WS, format, k,
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
  if (sc.status == codec::OK && sc.images > 1) {
    int im = -1;
    CHECK(codec::parse_instances_yuv_host(p, n, sz.HS, sz.WS, format, k, nullptr, sc.images - 1,
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
  const Size sizes[] = {{2, 2}, {2, 4}, {4, 6}, {6, 10}, {8, 8}, {2, 34}};
  int ok = 0, bad = 0;
  YuvCoeffs k0;
  // the coefficient lookup refuses what is outside its enums and leaves the table alone
  for (int m = -1; m <= 2; ++m)
    for (int r = -1; r <= 2; ++r) {
      YuvCoeffs k;
      const bool want = m >= 0 && m <= 1 && r >= 0 && r <= 1;
      CHECK(yuv_coeffs(m, r, &k) == want, "yuv_coeffs(%d, %d)", m, r);
      if (want) CHECK(k.yo == (r == YUV_LIMITED ? 16 : 0) && k.cy > 0 && k.cgu < 0, "table");
    }
  // refusals of the twin and the decoder: odd and non-positive sizes, unknown formats
  {
    uint8_t frame[6] = {0}, rgb[12];
    CHECK(!codec::yuv420_to_rgb_host(frame, 3, 2, YUV_I420, k0, rgb, nullptr), "odd HS");
    CHECK(!codec::yuv420_to_rgb_host(frame, 2, 0, YUV_I420, k0, rgb, nullptr), "WS 0");
    CHECK(!codec::yuv420_to_rgb_host(frame, 2, 2, 7, k0, rgb, nullptr), "format");
    CHECK(codec::yuv420_to_rgb_host(frame, 2, 2, YUV_NV12, k0, rgb, nullptr), "2x2");
    int im = -1;
    const std::string t = "{\"instances\":[{\"b64\":\"AAAAAAAA\"}]}";
    const uint8_t* tp = reinterpret_cast<const uint8_t*>(t.data());
    CHECK(codec::parse_instances_yuv_host(tp, t.size(), 2, 2, YUV_I420, k0, nullptr, -1, &im) ==
              codec::OK && im == 1, "2x2 record");
    CHECK(codec::parse_instances_yuv_host(tp, t.size(), 2, 3, YUV_I420, k0, nullptr, -1, &im) ==
              codec::BAD_SHAPE, "odd WS");
    CHECK(codec::parse_instances_yuv_host(tp, t.size(), 2, 2, 0, k0, nullptr, -1, &im) ==
              codec::BAD_SHAPE, "format 0");
    CHECK(codec::scan_instances_b64_bytes(tp, t.size(), 0).status == codec::BAD_SHAPE, "0 bytes");
    CHECK(codec::scan_instances_b64_bytes(tp, t.size(), -6).status == codec::BAD_SHAPE, "< 0");
  }
  for (const char* t : {"", " ", "{", "{}", "[", "{\"instances\"", "{\"instances\":[",
                        "{\"instances\":[]}", "{\"instances\":null}", "{\"instances\":[{",
                        "{\"instances\":[{\"b64\":\"", "{\"instances\":[{\"b64\":\"AAAA\"}]}",
                        "{\"instances\":[{}]}", "{\"instances\":[[[[1,2,3]]]]}"})
    run(t, sizes[0], YUV_I420, k0, nullptr);
  run("{\"instances\":[{\"b64\":\"", Size{30000, 30000}, YUV_NV12, k0, nullptr);  // L past the end
  for (int it = 0; it < iters; ++it) {
    const Size& sz = sizes[rng() % (sizeof(sizes) / sizeof(sizes[0]))];
    const int format = rng() % 2 ? YUV_I420 : YUV_NV12;
    YuvCoeffs k;
    yuv_coeffs((int)(rng() % 2), (int)(rng() % 2), &k);
    const int images = 1 + (int)(rng() % 3);
    std::vector<std::vector<uint8_t>> frames, twins;
    std::vector<float> want;
    for (int i = 0; i < images; ++i) {
      std::vector<uint8_t> Y((size_t)sz.HS * sz.WS), U(Y.size() / 4), V(Y.size() / 4);
      for (auto* pl : {&Y, &U, &V})
        for (uint8_t& b : *pl) b = (uint8_t)rng();
      frames.push_back(pack(Y, U, V, format));
      twins.push_back(pack(Y, U, V, format == YUV_I420 ? YUV_NV12 : YUV_I420));
      std::vector<float> f(Y.size() * 3);
      std::vector<uint8_t> rgb(Y.size() * 3);
      CHECK(codec::yuv420_to_rgb_host(frames.back().data(), sz.HS, sz.WS, format, k, rgb.data(),
                                      f.data()),
            "conversion refused");
      for (size_t e = 0; e < f.size(); ++e) CHECK(f[e] == (float)rgb[e], "float != byte");
      want.insert(want.end(), f.begin(), f.end());
    }
    std::string s = record(frames, rng() % 2 != 0);
    if (it % 8 == 0) {  // the valid record decodes to the conversion; so does its other format
      std::vector<float> got, got2;
      CHECK(run(s, sz, format, k, &got) == codec::OK, "valid record rejected");
      CHECK(got == want, "decoded frames differ from the conversion twin");
      CHECK(run(record(twins, false), sz, format == YUV_I420 ? YUV_NV12 : YUV_I420, k, &got2) ==
                codec::OK, "valid twin record rejected");
      CHECK(got2 == want, "I420 and NV12 records of the same planes differ");
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
    const int st = run(s, sz, format, k, nullptr);
    st == codec::OK ? ++ok : ++bad;
  }
  printf("yuv_check: %d records accepted, %d rejected, %d failures\n", ok, bad, failures);
  if (failures || ok == 0 || bad == 0) return 1;
  printf("all checks passed\n");
  return 0;
}
