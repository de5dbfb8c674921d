// Sanitizer run of the planar YUV 4:2:2 / 4:4:4 host codec (csrc/codec/yuv.h: yuvp_to_rgb_host;
// csrc/codec/json_codec.h: parse_instances_yuvp_host, parse_instances_raw_yuvp_host and the
// byte-count scan / splitter under them) on untrusted input. A fixed seed, valid records of
// several frame sizes in both formats and encodings - strings with no, one and two '=' - and a
// few thousand mutated and truncated copies. Every input lives in a heap block of exactly its
// size, so AddressSanitizer sees any access past n. Checks that every status is one of the
// format's verdicts, that scan, splitter and parser agree, that a valid record decodes to the
// conversion of its frames, and that a yuv444p frame with pairwise equal chroma columns gives the
// yuv422p image. Host only, no HIP call.
//   build/asan/yuvp_check [iterations]
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

std::string b64(const std::vector<uint8_t>& v) {  // standard alphabet, '=' padded
  static const char kA[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  std::string s;
  for (size_t i = 0; i < v.size(); i += 3) {
    const size_t m = v.size() - i < 3 ? v.size() - i : 3;
    const uint32_t x = ((uint32_t)v[i] << 16) | (m > 1 ? (uint32_t)v[i + 1] << 8 : 0u) |
                       (m > 2 ? v[i + 2] : 0u);
    s += kA[(x >> 18) & 63];
    s += kA[(x >> 12) & 63];
    s += m > 1 ? kA[(x >> 6) & 63] : '=';
    s += m > 2 ? kA[x & 63] : '=';
  }
  return s;
}

struct Size {
  int HS, WS;
};

// The record of `frames` in either encoding.
std::string record(const std::vector<std::vector<uint8_t>>& frames, bool raw) {
  std::string s = raw ? "" : "{\"instances\":[";
  for (size_t i = 0; i < frames.size(); ++i) {
    if (raw) s.append(reinterpret_cast<const char*>(frames[i].data()), frames[i].size());
    else s += std::string(i ? "," : "") + "{\"b64\":\"" + b64(frames[i]) + "\"}";
  }
  return raw ? s : s + "]}";
}

bool known_status(int st) {
  switch (st) {
    case codec::OK: case codec::BAD_ENVELOPE: case codec::UNKNOWN_KEY: case codec::BAD_SHAPE:
    case codec::EMPTY: case codec::NULL_INSTANCES: case codec::TOO_LARGE: case codec::BAD_NUMBER:
      return true;
    default:
      return false;
  }
}

// Runs scan, splitter and parser on an exact-size heap copy of `s`; returns the parser's status.
int run(const std::string& s, const Size& sz, int format, bool raw, const YuvCoeffs& k,
        std::vector<float>* decoded) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[s.size() ? s.size() : 1]);
  memcpy(buf.get(), s.data(), s.size());
  const uint8_t* p = buf.get();
  const size_t n = s.size();
  const int64_t B = yuvp_bytes(sz.HS, sz.WS, format);
  const codec::Scan sc = raw ? codec::scan_instances_raw(n, B)
                             : codec::scan_instances_b64_bytes(p, n, B);
  CHECK(known_status(sc.status) && sc.status != codec::BAD_NUMBER, "scan status %d", sc.status);
  std::vector<float> out;
  const size_t per = (size_t)sz.HS * sz.WS * 3;
  if (sc.status == codec::OK) {
    CHECK(sc.images > 0, "scan accepted no image");
    out.assign((size_t)sc.images * per, -1.f);
    std::vector<std::pair<uint32_t, uint32_t>> spans;
    if (raw) {  // fragments of at most 2 frames: whole frames, in order, covering the value
      CHECK(codec::split_instances_raw(n, B, 2, spans), "raw split");
      size_t at = 0;
      for (const auto& sp : spans) {
        CHECK(sp.first == at && sp.second > sp.first && (sp.second - sp.first) % B == 0 &&
                  (sp.second - sp.first) <= 2 * B, "raw fragment");
        at = sp.second;
      }
      CHECK(at == n, "raw fragments do not cover the value");
    } else {
      CHECK(sc.arr_off > 0 && sc.arr_off + sc.arr_len <= (int64_t)n, "scan result out of range");
      std::unique_ptr<uint8_t[]> arr(new uint8_t[(size_t)sc.arr_len]);
      memcpy(arr.get(), p + sc.arr_off, (size_t)sc.arr_len);
      CHECK(codec::split_instances_b64_bytes(arr.get(), (size_t)sc.arr_len, B, spans) &&
                (int)spans.size() == sc.images, "split disagrees with the scan");
      for (const auto& sp : spans)
        CHECK(sp.second <= (size_t)sc.arr_len && arr[sp.first] == '{' && arr[sp.second - 1] == '}',
              "element span");
    }
  }
  const auto parse = raw ? codec::parse_instances_raw_yuvp_host : codec::parse_instances_yuvp_host;
  int images = -1;
  const int st = parse(p, n, sz.HS, sz.WS, format, k, out.empty() ? nullptr : out.data(), -1,
                       &images);
  CHECK(known_status(st) && (!raw || st != codec::BAD_NUMBER), "parser status %d", st);
  if (sc.status != codec::OK) CHECK(st == sc.status, "parser %d != scan %d", st, sc.status);
  else CHECK(st == codec::OK || st == codec::BAD_NUMBER, "parser %d after an OK scan", st);
  if (st == codec::OK) {
    CHECK(images == sc.images, "image count");
    for (float v : out) CHECK(v >= 0.f && v <= 255.f && v == (float)(int)v, "value %g", v);
    int im = -1;
    if (images > 1)
      CHECK(parse(p, n, sz.HS, sz.WS, format, k, nullptr, images - 1, &im) == codec::TOO_LARGE,
            "max_images");
  } else {
    CHECK(images == 0, "images reported for a bad record");
  }
  if (decoded) *decoded = out;
  return st;
}

}  // namespace

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 4000;
  std::mt19937 rng(20261126u);
  // yuv422p strings with '==' (1x2), '=' (1x4, 5x2) and none (3x2); yuv444p never has any
  const Size sizes[] = {{1, 2}, {1, 4}, {3, 2}, {5, 2}, {3, 6}, {7, 10}, {2, 34}};
  const Size odd[] = {{1, 1}, {3, 3}, {5, 7}};  // yuv444p only
  YuvCoeffs k0;
  {  // refusals of the twin and both parsers; the byte counts
    uint8_t frame[12] = {0}, rgb[12];
    CHECK(yuvp_bytes(3, 2, YUV_YUV422P) == 12 && yuvp_bytes(3, 3, YUV_YUV444P) == 27, "bytes");
    CHECK(!codec::yuvp_to_rgb_host(frame, 1, 3, YUV_YUV422P, k0, rgb, nullptr), "odd WS");
    CHECK(!codec::yuvp_to_rgb_host(frame, 0, 2, YUV_YUV444P, k0, rgb, nullptr), "HS 0");
    CHECK(!codec::yuvp_to_rgb_host(frame, 2, 2, YUV_I420, k0, rgb, nullptr), "format");
    CHECK(codec::yuvp_to_rgb_host(frame, 1, 3, YUV_YUV444P, k0, rgb, nullptr), "1x3 4:4:4");
    int im = -1;
    for (const bool raw : {false, true}) {
      const auto parse = raw ? codec::parse_instances_raw_yuvp_host
                             : codec::parse_instances_yuvp_host;
      CHECK(parse(frame, 12, 2, 3, YUV_YUV422P, k0, nullptr, -1, &im) == codec::BAD_SHAPE, "WS 3");
      CHECK(parse(frame, 12, 2, 2, YUV_YUYV422, k0, nullptr, -1, &im) == codec::BAD_SHAPE, "fmt");
      CHECK(parse(frame, 12, -1, 2, YUV_YUV444P, k0, nullptr, -1, &im) == codec::BAD_SHAPE, "HS");
    }
    CHECK(codec::parse_instances_raw_yuvp_host(frame, 12, 3, 2, YUV_YUV422P, k0, nullptr, -1,
                                               &im) == codec::OK && im == 1, "3x2 raw");
    CHECK(codec::parse_instances_raw_yuvp_host(frame, 11, 3, 2, YUV_YUV422P, k0, nullptr, -1,
                                               &im) == codec::BAD_SHAPE, "11 of 12 bytes");
  }
  for (const char* t : {"", " ", "{", "{}", "{\"instances\":[", "{\"instances\":[]}",
                        "{\"instances\":null}", "{\"instances\":[{\"b64\":\"",
                        "{\"instances\":[{\"b64\":\"AAAA\"}]}", "{\"instances\":[[[[1,2,3]]]]}"})
    for (const bool raw : {false, true}) run(t, sizes[0], YUV_YUV422P, raw, k0, nullptr);
  run("{\"instances\":[{\"b64\":\"", Size{30000, 30000}, YUV_YUV444P, false, k0, nullptr);
  int ok = 0, bad = 0;
  for (int it = 0; it < iters; ++it) {
    const int format = rng() % 2 ? YUV_YUV422P : YUV_YUV444P;
    const Size& sz = format == YUV_YUV444P && rng() % 3 == 0 ? odd[rng() % 3] : sizes[rng() % 7];
    const bool raw = rng() % 2 != 0;
    const size_t hw = (size_t)sz.HS * sz.WS, hc = hw >> yuvp_shift(format);
    YuvCoeffs k;
    yuv_coeffs((int)(rng() % 2), (int)(rng() % 2), &k);
    const int images = 1 + (int)(rng() % 4);
    std::vector<std::vector<uint8_t>> frames, wide;  // wide: the 4:4:4 frame of a 4:2:2 one
    std::vector<float> want;
    for (int i = 0; i < images; ++i) {
      std::vector<uint8_t> f(hw + 2 * hc);
      for (uint8_t& b : f) b = (uint8_t)rng();
      frames.push_back(f);
      std::vector<uint8_t> w(f.begin(), f.begin() + hw);
      for (size_t q = 0; q < 2 * hw; ++q) w.push_back(f[hw + (q / hw) * hc + (q % hw >> 1)]);
      wide.push_back(w);
      std::vector<float> v(hw * 3);
      std::vector<uint8_t> rgb(hw * 3);
      CHECK(codec::yuvp_to_rgb_host(f.data(), sz.HS, sz.WS, format, k, rgb.data(), v.data()),
            "conversion refused");
      for (size_t e = 0; e < v.size(); ++e) CHECK(v[e] == (float)rgb[e], "float != byte");
      want.insert(want.end(), v.begin(), v.end());
    }
    std::string s = record(frames, raw);
    if (it % 8 == 0) {  // the valid record decodes to the conversion of its frames
      std::vector<float> got, got2;
      CHECK(run(s, sz, format, raw, k, &got) == codec::OK, "valid record rejected");
      CHECK(got == want, "decoded frames differ from the conversion twin");
      if (format == YUV_YUV422P) {
        CHECK(run(record(wide, raw), sz, YUV_YUV444P, raw, k, &got2) == codec::OK, "4:4:4 twin");
        CHECK(got2 == want, "4:4:4 with doubled chroma columns differs from 4:2:2");
      }
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
    run(s, sz, format, raw, k, nullptr) == codec::OK ? ++ok : ++bad;
  }
  printf("yuvp_check: %d records accepted, %d rejected, %d failures\n", ok, bad, failures);
  if (failures || ok == 0 || bad == 0) return 1;
  printf("all checks passed\n");
  return 0;
}
