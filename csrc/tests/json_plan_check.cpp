// Sanitizer run of the JSON ingest's host plan (csrc/runtime/ingest_plan.h) behind the real
// envelope scanner: a fixed seed, fetch-like buffers of numeric records of several shapes behind
// fake batch framing, then mutated copies of their text AND of the scan results handed to the
// plan (extents, offsets, batches). Every buffer is a heap block of exactly its size, and the plan
// is filled into a heap block of exactly its DMA'd prefix. The plan either throws
// std::invalid_argument or every offset it hands the ingest kernels holds the checks below.
//   build/asan/json_plan_check [iterations]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../codec/json_codec.h"
#include "../codec/text_pack.h"
#include "../runtime/ingest_plan.h"

using namespace gale;

namespace {

int failures = 0;
// plans seen per branch of the layout (each must occur, or the inputs do not reach it)
int cov_packed = 0, cov_packed_in_chunk = 0, cov_in_chunk = 0, cov_lane_plan = 0,
    cov_no_counts = 0, cov_parsed = 0, cov_arena_skip = 0, cov_groups = 0;
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

// {"instances":[[[[n,...],...],...],...]} with numbers of 1 to ~12 characters
std::string record(std::mt19937& rng, const Shape& sh, int images) {
  std::string s = "{\"instances\":[";
  char num[32];
  for (int i = 0; i < images; ++i) {
    s += i ? ",[" : "[";
    for (int h = 0; h < sh.H; ++h) {
      s += h ? ",[" : "[";
      for (int w = 0; w < sh.W; ++w) {
        s += w ? ",[" : "[";
        for (int c = 0; c < sh.C; ++c) {
          if (c) s += ",";
          switch (rng() % 3) {
            case 0: snprintf(num, sizeof num, "%u", (unsigned)(rng() % 10)); break;
            case 1: snprintf(num, sizeof num, "0.%u", (unsigned)(rng() % 100000)); break;
            default: snprintf(num, sizeof num, "-%u.%uE-%u", (unsigned)(rng() % 10),
                              (unsigned)(rng() % 10000000), (unsigned)(rng() % 30)); break;
          }
          s += num;
        }
        s += "]";
      }
      s += "]";
    }
    s += "]";
  }
  return s + "]}";
}

constexpr int64_t kAttr = 21;  // (kafka::kBatchAttrOffset; any value below a batch's length)

// One fetch: `nrec` record values behind a fake batch header each, scanned, planned, filled,
// checked. mutate: 0 none, 1 the text, 2 the scan results. Returns 1 planned, 0 rejected.
int run(std::mt19937& rng, const Shape& sh, int nrec, int mutate, int arena_mode) {
  std::string body;
  std::vector<std::pair<int64_t, int64_t>> batches;
  std::vector<std::pair<size_t, size_t>> values;  // (offset, length)
  for (int i = 0; i < nrec; ++i) {
    const size_t b0 = body.size();
    body.append(61 + rng() % 7, '\x01');  // batch + record framing
    // mostly a few images; now and then enough text for several tile groups
    std::string v = record(rng, sh, rng() % 6 == 0 ? 20 + (int)(rng() % 60) : 1 + (int)(rng() % 3));
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
  if (rng() % 4 == 0) body.append(1 + rng() % 300, '\x02');  // a cut-off batch behind the last
  const size_t n = body.size();
  std::unique_ptr<uint8_t[]> buf(new uint8_t[n ? n : 1]);
  memcpy(buf.get(), body.data(), n);
  std::vector<JsonPlanRecord> recs((size_t)nrec);
  for (int i = 0; i < nrec; ++i) {
    const codec::Scan sc =
        codec::scan_envelope(buf.get() + values[(size_t)i].first, values[(size_t)i].second);
    JsonPlanRecord& r = recs[(size_t)i];
    r.status = sc.status;
    r.value_off = (int64_t)values[(size_t)i].first;
    r.value_len = (int64_t)values[(size_t)i].second;
    r.arr_off = sc.arr_off;
    r.arr_len = sc.arr_len;
  }
  if (mutate == 2) {  // a scan result that contradicts the buffer
    JsonPlanRecord& r = recs[rng() % recs.size()];
    auto& b = batches[rng() % batches.size()];
    switch (rng() % 9) {
      case 0: r.value_off = (int64_t)n - (int64_t)(rng() % 8); r.status = 0; break;
      case 1: r.arr_off = r.value_len - (int64_t)(rng() % 40); break;
      case 2: r.arr_len += 1 + (int64_t)(rng() % 1000); break;
      case 3: r.value_len = -1 - (int64_t)(rng() % 3); r.status = 0; break;
      case 4: r.arr_len = -1 - (int64_t)(rng() % 5); r.status = 0; break;
      case 5: r.arr_off = -1 - (int64_t)(rng() % 5); r.status = 0; break;
      case 6: b.second += 1 + (int64_t)(rng() % 100000); break;
      case 7: b.first = -1 - (int64_t)(rng() % 5); break;
      default: r.arr_len = ((int64_t)1 << 31) + (int64_t)(rng() % 5); break;
    }
  }
  const int64_t per = (int64_t)sh.H * sh.W * sh.C, S = 2 * per;
  // no arena, one that ends somewhere among the records' slots, one with room for all
  const size_t all = n / (size_t)S + 2;
  const size_t arena_bytes = (size_t)(per * 4) * (arena_mode == 0   ? 0
                                                  : arena_mode == 1 ? 1 + rng() % all
                                                                    : all);
  // raw, or a packed body with a stream of some length up to the text's
  const int64_t tap = rng() % 3 == 0 ? (int64_t)(rng() % (n + 1)) : -1;
  const size_t need = tap >= 0 ? codec::pack_offset(n) + (size_t)tap : n;
  static const size_t kRoom[] = {0, 70, 300, 700, 5000, (size_t)1 << 20};
  const size_t dev_cap = need + kRoom[rng() % 6];
  const bool crcs = rng() % 4 != 0, separate = rng() % 5 == 0;
  JsonIngestPlan p;
  try {
    plan_json_ingest(batches, kAttr, crcs, recs, sh.H, sh.W, sh.C, arena_bytes, n, dev_cap, tap,
                     separate, p);
  } catch (const std::invalid_argument&) {
    CHECK(mutate == 2, "a consistent scan was refused");
    return 0;
  }
  const size_t nc = p.nc(), nr = p.nr(), np = p.np();
  size_t ok = 0;
  for (const JsonPlanRecord& r : recs) ok += r.status == 0;
  CHECK(nr == ok, "counted records %zu, OK records %zu", nr, ok);
  if (p.empty()) {
    CHECK(p.io_bytes == 0 && p.o_gsum == 0 && p.cnt_base == -1 && !p.plan_in_chunk, "empty plan");
    return 1;
  }
  // ---- sections: 16-byte aligned, in order, disjoint
  const size_t ngroups = (size_t)p.ngroups, ntiles = (size_t)p.ntiles, ptiles = (size_t)p.ptiles;
  for (size_t o : {p.o_chunks, p.o_groups, p.o_recs, p.o_precs, p.o_ptr, p.o_gsum, p.o_crc,
                   p.o_gbad, p.o_pbad, p.io_bytes})
    CHECK(o % 16 == 0, "section offset %zu", o);
  CHECK(p.o_chunks >= p.ng * 8 && p.o_groups >= p.o_chunks + nc * sizeof(CrcChunk) &&
            p.o_recs >= p.o_groups + ngroups * 8 && p.o_precs >= p.o_recs + nr * 48 &&
            p.o_ptr >= p.o_precs + np * 48 && p.o_gsum >= p.o_ptr + ptiles * 4 &&
            p.o_crc >= p.o_gsum + ngroups * 4 && p.o_gbad >= p.o_crc + nc * 4 &&
            p.o_pbad >= p.o_gbad + ngroups * 4 && p.io_bytes >= p.o_pbad + ptiles * 4,
        "sections overlap");
  // ---- fill: into exactly the prefix (a write outside it is the sanitizer's to report); the
  // pack table in front of the sections is not fill's
  const size_t prefix = p.o_gsum;
  std::unique_ptr<uint8_t[]> blk(new uint8_t[prefix]);
  memset(blk.get(), 0xA5, prefix);
  fill_json_ingest(p, recs, blk.get());
  for (size_t k = 0; k < p.ng * 8; ++k) CHECK(blk[k] == 0xA5, "fill wrote the pack table");
  const CrcChunk* hc = reinterpret_cast<const CrcChunk*>(blk.get() + p.o_chunks);
  const int2* hg = reinterpret_cast<const int2*>(blk.get() + p.o_groups);
  const JsonRecord* hr = reinterpret_cast<const JsonRecord*>(blk.get() + p.o_recs);
  const JsonRecord* hp = reinterpret_cast<const JsonRecord*>(blk.get() + p.o_precs);
  const int* hpt = reinterpret_cast<const int*>(blk.get() + p.o_ptr);
  // ---- windows: inside their batch, only the first one short
  CHECK(p.batch_chunks.size() == (crcs ? batches.size() : 0), "batch windows");
  for (size_t b = 0; b < p.batch_chunks.size(); ++b) {
    const int64_t rs = batches[b].first + kAttr, re = batches[b].first + batches[b].second;
    int64_t pos = rs;
    for (size_t k = 0; k < p.batch_chunks[b].second; ++k) {
      const CrcChunk& c = hc[p.batch_chunks[b].first + k];
      CHECK(c.len >= 1 && c.len <= kCrcChunkBytes && c.end - c.len == pos, "window %zu", k);
      CHECK(k == 0 || c.len == kCrcChunkBytes, "only the first window is short");
      CHECK(c.end <= re && c.end <= (int64_t)n, "window past its batch");
      pos = c.end;
    }
    CHECK(pos == re, "windows do not cover the batch");
  }
  // ---- count records: consecutive tiles, groups covering each record's tiles exactly once
  int tile = 0, grp = 0;
  for (size_t j = 0; j < nr; ++j) {
    const JsonPlanRecord& r = recs[(size_t)p.rec_of[j]];
    const JsonRecord& jr = hr[j];
    CHECK(r.status == 0 && (j == 0 || p.rec_of[j] > p.rec_of[j - 1]), "rec_of");
    CHECK(jr.off == r.value_off + r.arr_off && jr.len == r.arr_len, "record %zu extent", j);
    CHECK(jr.off >= 0 && jr.off + jr.len <= (int64_t)n, "record text outside the fetch");
    CHECK(jr.off >= (int64_t)p.lo && jr.off + jr.len <= (int64_t)(p.lo + p.span), "span");
    CHECK(jr.tile0 == tile && jr.grp0 == grp, "record %zu tile0 / grp0", j);
    CHECK(jr.slot == 0 && jr.images == 0 && jr.status == 0 && jr.has_cnt == 0 && jr.cnt_off == 0,
          "count record fields");
    const int nt = json_tile_count(jr.off, jr.len);
    CHECK((int64_t)nt * kJsonTileBytes >= (jr.off & 15) + jr.len, "tiles cover the text");
    for (int t0 = 0; t0 < nt; t0 += kGroupTiles, ++grp) {
      CHECK((size_t)grp < ngroups, "more groups than planned");
      if ((size_t)grp < ngroups) CHECK(hg[grp].x == (int)j && hg[grp].y == t0, "group %d", grp);
    }
    tile += nt;
  }
  CHECK((size_t)tile == ntiles && (size_t)grp == ngroups, "tile / group totals");
  // ---- the count block behind the device's bytes, inside the mirror
  CHECK(p.c_lo + p.c_len == p.used && p.used <= dev_cap, "copy range");
  CHECK(p.packed == (tap >= 0) && p.link == (p.packed ? (size_t)tap : p.span), "link");
  if (p.packed)
    CHECK(p.lo == 0 && p.span == n && p.ng == codec::pack_groups(n) &&
              p.c_lo == codec::pack_offset(n) && p.tab_off == codec::tab_offset(n),
          "packed copy");
  else
    CHECK(p.c_lo == p.lo && p.lo % 16 == 0 && p.lo + p.span <= n, "raw copy");
  if (p.cnt_base >= 0) {
    CHECK(p.cnt_base % 256 == 0, "count block alignment");
    CHECK((size_t)p.cnt_base + (ntiles + ngroups) * 4 <= dev_cap, "count block past the mirror");
    CHECK((size_t)p.cnt_base >= p.used + 64, "count block on the text");
  } else {
    CHECK(np == 0, "parse records without a count block");
  }
  // ---- an in-chunk plan: behind the fetch, before the counts
  CHECK(!(separate && p.plan_in_chunk), "plan_separate ignored");
  if (p.plan_in_chunk) {
    CHECK(p.plan_off >= n && p.plan_off >= p.used && p.plan_off % 256 == 0, "plan on the fetch");
    CHECK(p.plan_off + prefix <= (p.cnt_base >= 0 ? (size_t)p.cnt_base : dev_cap),
          "plan on the counts / past the chunk");
    if (p.packed)
      CHECK(p.plan_off + prefix <= p.tab_off || p.tab_off + p.ng * 8 <= p.plan_off,
            "plan on the pack table it is built from");
  }
  // ---- parse records: their counts, the tile map, arena slots
  bool values_disjoint = true;  // (mutated scan results may overlap records; real ones never do)
  for (size_t a = 0; a + 1 < nr; ++a)
    values_disjoint &= hr[a].off + hr[a].len <= hr[a + 1].off;
  int pt = 0;
  std::vector<std::pair<int64_t, int64_t>> slots;
  for (size_t k = 0; k < np; ++k) {
    CHECK(p.pjs[k] >= 0 && (size_t)p.pjs[k] < nr && (k == 0 || p.pjs[k] > p.pjs[k - 1]), "pjs");
    const JsonRecord& jr = hr[p.pjs[k]];
    const JsonRecord& pr = hp[k];
    CHECK(pr.off == jr.off && pr.len == jr.len && pr.tile0 == pt && pr.images == -1 &&
              pr.status == 0 && pr.has_cnt == 1 && pr.grp0 == 0,
          "parse record %zu", k);
    CHECK(pr.cnt_off == p.cnt_base + (int64_t)(jr.tile0 + jr.grp0) * 4, "parse record cnt_off");
    const int nt = json_tile_count(pr.off, pr.len);
    const int ng = (nt + kGroupTiles - 1) / kGroupTiles;
    CHECK(pr.cnt_off + (int64_t)(nt + ng) * 4 <= p.cnt_base + (int64_t)(ntiles + ngroups) * 4,
          "count block of record %zu past the block", k);
    for (int t = 0; t < nt && (size_t)(pt + t) < ptiles; ++t)
      CHECK(hpt[pt + t] == (int)k, "tile map at %d", pt + t);
    pt += nt;
    const int64_t cap = pr.len / S;
    CHECK(cap > 0 && pr.slot == (pr.off + S - 1) / S, "slot of parse record %zu", k);
    CHECK((uint64_t)(pr.slot + cap) * (uint64_t)per * 4 <= arena_bytes, "slots past the arena");
    slots.emplace_back(pr.slot, pr.slot + cap);
  }
  CHECK((size_t)pt == ptiles, "parse tile total");
  if (values_disjoint)
    for (size_t a = 0; a + 1 < slots.size(); ++a)
      CHECK(slots[a].second <= slots[a + 1].first, "arena slots overlap");
  // every counted record that fits the arena is parsed, whatever the ones before it did
  if (arena_bytes > 0 && p.cnt_base >= 0) {
    size_t fit = 0;
    for (size_t j = 0; j < nr; ++j) {
      const int64_t slot = (hr[j].off + S - 1) / S, cap = hr[j].len / S;
      fit += cap > 0 && (uint64_t)(slot + cap) * (uint64_t)per * 4 <= arena_bytes;
    }
    CHECK(fit == np, "%zu records fit the arena, %zu parsed", fit, np);
  }
  cov_packed += p.packed;
  cov_in_chunk += p.plan_in_chunk;
  cov_packed_in_chunk += p.packed && p.plan_in_chunk;
  cov_lane_plan += !p.plan_in_chunk && !separate;
  cov_no_counts += ntiles > 0 && p.cnt_base < 0;
  cov_parsed += np > 0;
  cov_arena_skip += np > 0 && np < nr;
  cov_groups += ngroups > nr;  // a record of more than one tile group
  return 1;
}

bool refused(const std::vector<std::pair<int64_t, int64_t>>& batches,
             const std::vector<JsonPlanRecord>& recs, int H, size_t fetch, size_t dev_cap,
             int64_t tap = -1) {
  JsonIngestPlan p;
  try {
    plan_json_ingest(batches, kAttr, true, recs, H, 2, 1, 1 << 10, fetch, dev_cap, tap, false, p);
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

}  // namespace

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 3000;
  std::mt19937 rng(20260318u);
  const Shape shapes[] = {{2, 2, 1}, {4, 4, 3}, {1, 1, 1}, {8, 8, 3}, {3, 5, 2}};
  int planned = 0, refusals = 0;
  for (int it = 0; it < iters; ++it) {
    const Shape& sh = shapes[rng() % (sizeof(shapes) / sizeof(shapes[0]))];
    run(rng, sh, 1 + (int)(rng() % 6), it % 3, (it / 3) % 3) ? ++planned : ++refusals;
  }
  // the empty fetch, and each contradiction by itself
  {
    JsonIngestPlan p;
    plan_json_ingest({}, kAttr, true, {}, 2, 2, 1, 0, 0, 0, -1, false, p);
    CHECK(p.empty() && p.io_bytes == 0 && p.cnt_base == -1, "empty fetch");
    JsonPlanRecord r;
    r.value_off = 64;
    r.value_len = 100;
    r.arr_off = 13;
    r.arr_len = 86;
    const std::vector<std::pair<int64_t, int64_t>> b = {{0, 170}};
    CHECK(!refused(b, {r}, 2, 170, 4096), "a consistent record refused");
    CHECK(refused(b, {r}, 0, 170, 4096), "H = 0 accepted");
    CHECK(refused({{0, 171}}, {r}, 2, 170, 4096), "batch past the fetch accepted");
    CHECK(refused(b, {r}, 2, 163, 4096), "value past the fetch accepted");
    CHECK(refused(b, {r}, 2, 170, 169), "copy past the mirror accepted");
    CHECK(refused(b, {r}, 2, 170, 192 + 99, 100), "packed stream past the mirror accepted");
    JsonPlanRecord q = r;
    q.arr_len = 88;
    CHECK(refused(b, {q}, 2, 170, 4096), "array past its value accepted");
    q = r;
    q.arr_off = -1;
    CHECK(refused(b, {q}, 2, 170, 4096), "negative arr_off accepted");
    q.status = 3;  // (a record the scan refused is not looked at)
    CHECK(!refused(b, {q}, 2, 170, 4096), "a skipped record's extents were judged");
  }
  printf("json_plan_check: %d plans, %d refused, %d failures\n", planned, refusals, failures);
  printf("  packed %d (plan in chunk %d), plan in chunk %d, plan in the lane buffer %d, "
         "no count block %d, parsed %d, a record left out of the arena %d, several groups %d\n",
         cov_packed, cov_packed_in_chunk, cov_in_chunk, cov_lane_plan, cov_no_counts, cov_parsed,
         cov_arena_skip, cov_groups);
  if (failures || planned == 0 || refusals == 0) return 1;
  if (!cov_packed || !cov_packed_in_chunk || !cov_in_chunk || !cov_lane_plan || !cov_no_counts ||
      !cov_parsed || !cov_arena_skip || !cov_groups) {
    printf("a layout branch was never reached\n");
    return 1;
  }
  printf("all checks passed\n");
  return 0;
}
