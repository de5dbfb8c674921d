// Sanitizer run of the base64 ingest's host plan (csrc/runtime/ingest_plan.h) behind the real
// scanner: a fixed seed, fetch-like buffers of valid records of several shapes, then mutated and
// truncated copies of their text AND of the scan results handed to the plan (counts, offsets,
// extents). Every buffer is a heap block of exactly its size. The plan either throws
// std::invalid_argument or returns descriptors whose strings lie wholly inside their record, dense
// slots inside the arena, windows inside their batch and 16-byte-aligned sections.
//   build/asan/b64_plan_check [iterations]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../codec/json_codec.h"
#include "../runtime/ingest_plan.h"

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

struct Shape {
  int H, W, C;
};

std::string record(std::mt19937& rng, const Shape& sh, int images) {
  static const char kA[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  const int64_t per = (int64_t)sh.H * sh.W * sh.C;
  const int64_t L = codec::b64_chars(sh.H, sh.W, sh.C);
  const int pad = (int)((3 - per % 3) % 3);
  std::string s = "{\"instances\":[";
  for (int i = 0; i < images; ++i) {
    if (i) s += ",";
    s += "{\"b64\":\"";
    for (int64_t k = 0; k < L - pad; ++k) s += kA[rng() & 63];
    s.append((size_t)pad, '=');
    s += "\"}";
  }
  return s + "]}";
}

constexpr int64_t kAttr = 21;  // (kafka::kBatchAttrOffset; any value below a batch's length)

// One fetch: `nrec` record values behind a fake batch header each, scanned, planned, checked.
// mutate: 0 none, 1 the text, 2 the scan results. Returns 1 planned, 0 rejected.
int run(std::mt19937& rng, const Shape& sh, int nrec, int mutate, size_t arena_bytes) {
  std::string body;
  std::vector<std::pair<int64_t, int64_t>> batches;
  std::vector<std::pair<size_t, size_t>> values;  // (offset, length)
  for (int i = 0; i < nrec; ++i) {
    const size_t b0 = body.size();
    body.append(61 + rng() % 7, '\x01');  // batch + record framing
    std::string v = record(rng, sh, 1 + (int)(rng() % 3));
    if (mutate == 1 && rng() % 2) {
      const size_t at = rng() % v.size();
      switch (rng() % 4) {
        case 0: v[at] = (char)rng(); break;
        case 1: v.erase(at, 1 + rng() % 3); break;
        case 2: v.insert(at, 1 + rng() % 3, '"'); break;
        default: v.resize(at); break;
      }
    }
    values.emplace_back(body.size(), v.size());
    body += v;
    body.append(rng() % 3, '\x00');
    batches.emplace_back((int64_t)b0, (int64_t)(body.size() - b0));
  }
  std::unique_ptr<uint8_t[]> buf(new uint8_t[body.size() ? body.size() : 1]);
  memcpy(buf.get(), body.data(), body.size());
  std::vector<B64PlanRecord> recs((size_t)nrec);
  std::vector<uint32_t> offs, one;
  for (int i = 0; i < nrec; ++i) {
    const uint8_t* v = buf.get() + values[(size_t)i].first;
    const size_t n = values[(size_t)i].second;
    codec::Scan sc = codec::scan_instances_b64(v, n, sh.H, sh.W, sh.C);
    if (sc.status == codec::OK &&
        (!codec::b64_image_offsets(v + sc.arr_off, (size_t)sc.arr_len, sh.H, sh.W, sh.C, one) ||
         (int)one.size() != sc.images))
      sc.status = codec::BAD_SHAPE;
    B64PlanRecord& r = recs[(size_t)i];
    r.status = sc.status;
    r.images = sc.status == codec::OK ? sc.images : 0;
    r.value_off = (int64_t)values[(size_t)i].first;
    r.value_len = (int64_t)n;
    r.arr_off = sc.arr_off;
    if (sc.status == codec::OK) offs.insert(offs.end(), one.begin(), one.end());
  }
  if (mutate == 2) {  // a scan result that contradicts the buffer
    B64PlanRecord& r = recs[rng() % recs.size()];
    switch (rng() % 7) {
      case 0: r.images += 1 + (int)(rng() % 1000); break;
      case 1: r.images = -(int)(rng() % 5); r.status = 0; break;
      case 2: r.value_off = (int64_t)body.size() - (int64_t)(rng() % 8); break;
      case 3: r.arr_off = r.value_len - (int64_t)(rng() % 40); break;
      case 4: if (!offs.empty()) offs[rng() % offs.size()] += 1u << (rng() % 32); break;
      case 5: if (!offs.empty()) offs.resize(rng() % offs.size()); break;
      default: r.value_len = -1 - (int64_t)(rng() % 3); r.status = 0; break;
    }
  }
  B64IngestPlan p;
  const bool crcs = rng() % 4 != 0;
  try {
    plan_b64_ingest(batches, kAttr, crcs, recs, offs, sh.H, sh.W, sh.C, arena_bytes, body.size(),
                    p);
  } catch (const std::invalid_argument&) {
    CHECK(mutate == 2, "a consistent scan was refused");
    return 0;
  }
  const int64_t per = (int64_t)sh.H * sh.W * sh.C;
  const int64_t L = codec::b64_chars(sh.H, sh.W, sh.C);
  CHECK(p.slot0.size() == recs.size() && p.img0.size() == recs.size(), "per-record sizes");
  CHECK(p.chunks_per_image == (int)((L + kB64ChunkChars - 1) / kB64ChunkChars), "chunks");
  int64_t slot = 0;
  size_t img = 0;
  bool cut = false;
  for (size_t i = 0; i < recs.size(); ++i) {
    if (recs[i].status != 0) {
      CHECK(p.slot0[i] == -1 && p.img0[i] == -1, "slots for a bad record");
      continue;
    }
    if (p.slot0[i] < 0) {
      cut = true;
      CHECK(p.img0[i] == -1, "descriptors without slots");
      continue;
    }
    CHECK(!cut, "slots after the arena cut");
    CHECK(p.slot0[i] == slot && p.img0[i] == (int)img, "dense slots in record order");
    for (int k = 0; k < recs[i].images && img < p.imgs.size(); ++k, ++img, ++slot) {
      const B64Image& d = p.imgs[img];
      CHECK(d.slot == slot && d.rec == (int)i, "descriptor %zu", img);
      CHECK(d.off >= recs[i].value_off && d.off + L <= recs[i].value_off + recs[i].value_len,
            "string outside its record");
      CHECK((uint64_t)(d.slot + 1) * (uint64_t)per * 4 <= arena_bytes, "slot past the arena");
      if (mutate != 2) {
        CHECK(buf[(size_t)d.off - 1] == '"' && buf[(size_t)(d.off + L)] == '"',
              "descriptor not at a string");
      }
    }
  }
  CHECK(img == p.imgs.size(), "descriptor count");
  if (mutate != 2) {
    for (size_t i = 0; i < recs.size(); ++i)
      if (recs[i].status == 0)
        CHECK(p.lo <= (size_t)recs[i].value_off &&
                  p.hi >= (size_t)(recs[i].value_off + recs[i].value_len),
              "span misses a record");
  }
  CHECK(p.hi <= body.size() && p.lo <= p.hi, "span");
  CHECK(p.batch_chunks.size() == (crcs ? batches.size() : 0), "batch windows");
  for (size_t b = 0; b < p.batch_chunks.size(); ++b) {
    const int64_t rs = batches[b].first + kAttr, re = batches[b].first + batches[b].second;
    int64_t pos = rs;
    for (size_t k = 0; k < p.batch_chunks[b].second; ++k) {
      const CrcChunk& c = p.chunks[p.batch_chunks[b].first + k];
      CHECK(c.len >= 1 && c.len <= kCrcChunkBytes && c.end - c.len == pos, "window %zu", k);
      CHECK(k == 0 || c.len == kCrcChunkBytes, "only the first window is short");
      pos = c.end;
    }
    CHECK(pos == re, "windows do not cover the batch");
  }
  for (size_t o : {p.o_chunks, p.o_imgs, p.plan_bytes, p.o_crc, p.o_bad, p.result_bytes})
    CHECK(o % 16 == 0, "section offset %zu", o);
  CHECK(p.o_imgs >= p.o_chunks + p.chunks.size() * sizeof(CrcChunk) &&
            p.plan_bytes >= p.o_imgs + p.imgs.size() * sizeof(B64Image) &&
            p.o_bad >= p.o_crc + p.chunks.size() * 4 &&
            p.result_bytes >= p.o_bad + p.imgs.size() * (size_t)p.chunks_per_image * 4,
        "sections overlap");
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 3000;
  std::mt19937 rng(20260214u);
  const Shape shapes[] = {{2, 2, 1}, {5, 4, 3}, {28, 28, 1}, {1, 1, 1}, {33, 33, 3}, {3, 3, 5}};
  int planned = 0, refused = 0;
  for (int it = 0; it < iters; ++it) {
    const Shape& sh = shapes[rng() % (sizeof(shapes) / sizeof(shapes[0]))];
    const size_t per4 = (size_t)sh.H * sh.W * sh.C * 4;
    const size_t arena = it % 5 == 0 ? 0 : it % 5 == 1 ? per4 * (1 + rng() % 4) : per4 * 64;
    run(rng, sh, 1 + (int)(rng() % 5), it % 3, arena) ? ++planned : ++refused;
  }
  // empty inputs and a shape no plan takes
  {
    B64IngestPlan p;
    plan_b64_ingest({}, kAttr, true, {}, {}, 2, 2, 1, 0, 0, p);
    CHECK(p.chunks.empty() && p.imgs.empty() && p.plan_bytes == 0 && p.result_bytes == 0,
          "empty fetch");
    bool threw = false;
    try {
      plan_b64_ingest({}, kAttr, true, {}, {}, 0, 2, 1, 0, 0, p);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    CHECK(threw, "H = 0 accepted");
  }
  printf("b64_plan_check: %d plans, %d refused, %d failures\n", planned, refused, failures);
  if (failures || planned == 0 || refused == 0) return 1;
  printf("all checks passed\n");
  return 0;
}
