// Sanitizer run of the GPU replica's host batch plan (csrc/runtime/batch_plan.h): a fixed seed,
// random batches of pinned, pageable, resident and preparsed records in every step form, JSON and
// b64, then mutated inputs (too many images, a b64 record that does not match its scan). The
// metadata is filled into a heap block that ends exactly where the bytes the step copies end, so
// a byte written past them is caught; what lies in front of them is checked to stay untouched.
// The plan either throws std::logic_error or holds the checks below.
//   build/asan/batch_plan_check [iterations]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <random>
#include <stdexcept>
#include <vector>

#include "../runtime/batch_plan.h"

using namespace gale;

namespace {

int failures = 0;
// plans seen per branch (each must occur, or the inputs do not reach it)
int cov_spans = 0, cov_staged = 0, cov_resident = 0, cov_preparsed = 0, cov_b64 = 0,
    cov_no_count_pass = 0, cov_no_tiles = 0, cov_too_many = 0, cov_bad_scan = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      ++failures;                                          \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                        \
      fprintf(stderr, "\n");                               \
    }                                                      \
  } while (0)

constexpr uint64_t kDevBytes = 0x7f0000100000ull;  // 256-byte aligned, as the slot's buffer is
constexpr uint64_t kInput = 0x7f0000a00000ull;
constexpr uint64_t kMirror = 0x7e0000000000ull;
constexpr uint64_t kArena = 0x7d0000000000ull;

struct Case {
  std::vector<BatchPlanRecord> recs;
  std::vector<uint32_t> offs;
  int max_batch = 0;
  int64_t per = 0;
  StepForm form = StepForm::OpByOp;
  bool ptr_input = false, b64 = false;
};

Case make_case(std::mt19937& rng) {
  Case c;
  c.max_batch = 1 + (int)(rng() % 24);
  c.per = 1 + (int64_t)(rng() % 64);
  c.form = (StepForm)(rng() % 3);
  c.ptr_input = c.form == StepForm::Kernels && rng() % 2;
  c.b64 = rng() % 3 == 0;
  const int n = 1 + (int)(rng() % 10);
  int64_t next_off[4] = {0, 0, 0, 0};  // records of one buffer do not overlap
  int room = c.max_batch;
  for (int i = 0; i < n && room > 0; ++i) {
    BatchPlanRecord r;
    r.images = 1 + (int)(rng() % std::min(room, 4));
    room -= r.images;
    const int lens[] = {0, 1, 15, 16, 17, 2033, 2034, 2048, 2049, 5000};
    r.arr_len = c.b64 ? 40 * r.images : lens[rng() % 10];
    const int kind = (int)(rng() % 4);
    if (kind >= 2) {  // resident, maybe with counts, maybe preparsed
      r.resident = true;
      r.dev_text = kMirror + rng() % 100000;
      r.dev_counts = rng() % 2 ? kMirror + 0x100000 + 4 * (rng() % 1000) : 0;
      r.preparsed = c.ptr_input && kind == 3;
      r.dev_image = r.preparsed ? kArena + 4 * (uint64_t)c.per * (rng() % 1000) : 0;
    } else {
      const int b = (int)(rng() % 4);
      r.buf = 100 + (uint64_t)b;
      r.pinned = kind == 1;
      r.arr_off = next_off[b] + (int64_t)(rng() % 100);
      next_off[b] = r.arr_off + r.arr_len;
    }
    if (c.b64 && !r.preparsed) {
      r.b64_first = (int32_t)c.offs.size();
      r.b64_n = r.images;
      for (int k = 0; k < r.images; ++k) c.offs.push_back((uint32_t)(40 * k + 9));
    }
    c.recs.push_back(r);
  }
  return c;
}

// true: planned and filled
bool run(const Case& c, BatchPlan& p) {
  try {
    plan_batch(c.recs, c.max_batch, c.per, c.form, c.ptr_input, c.b64, p);
  } catch (const std::logic_error&) {
    return false;
  }
  const MetaLayout L(c.max_batch, std::max(1, p.ntiles));
  const MetaRange used = L.used(p);
  CHECK(used.end() <= L.total, "used %zu past the allocation %zu", used.end(), L.total);
  // the block ends where the copied bytes end; in front of them nothing may change
  std::unique_ptr<uint8_t[]> meta(new uint8_t[used.end()]);
  memset(meta.get(), 0xab, used.end());
  fill_batch(p, c.recs, c.offs, L, kDevBytes, kInput, meta.get());
  for (size_t i = 0; i < used.off; ++i)
    if (meta[i] != 0xab) {
      CHECK(false, "byte %zu in front of the copied range written", i);
      break;
    }
  // the staged copies: the source's phase kept, in order, disjoint, inside the staged bytes
  size_t end = 0;
  for (const BatchPlan::Staged& g : p.staged) {
    const BatchPlanRecord& r = c.recs[(size_t)g.rec];
    CHECK(!r.resident && !r.pinned && g.len == (size_t)r.arr_len, "staged record %d", g.rec);
    CHECK(g.host % 16 == (size_t)r.arr_off % 16 && g.host >= end, "staged record %d placed", g.rec);
    end = g.host + g.len;
  }
  CHECK(end <= p.staged_bytes && p.staged_bytes % 16 == 0, "staged bytes %zu", p.staged_bytes);
  size_t dev = 0;
  for (const BatchPlan::Span& x : p.spans) {
    CHECK(x.lo % 16 == 0 && x.dev == dev, "span of buffer %llu", (unsigned long long)x.buf);
    dev = x.dev + ((x.len + 15) & ~(size_t)15);
  }
  CHECK(p.staged_dev == dev && p.dev_total == 16 + dev + p.staged_bytes, "device layout");
  // the records: each text inside the bytes copied for it, tiles numbered consecutively
  int nrec = 0, img = 0, ntiles = 0, b64n = 0;
  const JsonRecord* jr = reinterpret_cast<const JsonRecord*>(meta.get() + L.recs);
  const B64Image* tab = reinterpret_cast<const B64Image*>(meta.get() + L.b64_table);
  for (size_t i = 0; i < c.recs.size(); ++i) {
    const BatchPlanRecord& r = c.recs[i];
    if (r.preparsed) {
      CHECK(p.parse_idx[i] == -1, "preparsed record %zu", i);
      img += r.images;
      continue;
    }
    CHECK(p.parse_idx[i] == nrec, "parse index of record %zu", i);
    const int64_t off = c.b64 ? tab[b64n].off - c.offs[(size_t)r.b64_first] : jr[nrec].off;
    if (r.resident)
      CHECK((uint64_t)off + kDevBytes == r.dev_text, "resident record %zu", i);
    else
      CHECK(off >= 0 && (size_t)off % 16 == (size_t)r.arr_off % 16 &&
                (size_t)(off + r.arr_len) <= p.dev_total - 16,
            "record %zu at %lld", i, (long long)off);
    if (c.b64) {
      for (int k = 0; k < r.images; ++k)
        CHECK(tab[b64n + k].slot == img + k && tab[b64n + k].rec == nrec, "descriptor %d", b64n + k);
      b64n += r.images;
    } else {
      const JsonRecord& j = jr[nrec];
      CHECK(j.len == r.arr_len && j.slot == img && j.images == r.images && j.status == 0 &&
                j.tile0 == ntiles && j.has_cnt == (r.resident && r.dev_counts ? 1 : 0),
            "record %zu's table entry", i);
      const int nt = json_tile_count(j.off, j.len);
      const int32_t* map = reinterpret_cast<const int32_t*>(meta.get() + L.tiles);
      for (int t = 0; t < nt; ++t) CHECK(map[ntiles + t] == nrec, "tile %d", ntiles + t);
      ntiles += nt;
    }
    ++nrec;
    img += r.images;
  }
  CHECK(nrec == p.nrec && img == p.img && ntiles == p.ntiles && b64n == p.b64n, "counts");
  cov_spans += !p.spans.empty();
  cov_staged += !p.staged.empty();
  cov_resident += p.resident > 0;
  cov_preparsed += p.npre > 0;
  cov_b64 += c.b64;
  cov_no_count_pass += !c.b64 && p.nrec > 0 && !p.count_pass;
  cov_no_tiles += p.ntiles == 0;
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 1000;
  std::mt19937 rng(20250117);
  BatchPlan reused;  // one plan object over every batch, as a slot keeps it
  int planned = 0, refused = 0;
  for (int it = 0; it < iters; ++it) {
    Case c = make_case(rng);
    if (run(c, reused)) {
      ++planned;
      BatchPlan fresh;  // the reused plan carries nothing over
      plan_batch(c.recs, c.max_batch, c.per, c.form, c.ptr_input, c.b64, fresh);
      CHECK(fresh.parse_idx == reused.parse_idx && fresh.off == reused.off &&
                fresh.spans.size() == reused.spans.size() &&
                fresh.staged.size() == reused.staged.size() && fresh.ntiles == reused.ntiles &&
                fresh.dev_total == reused.dev_total,
            "a reused plan differs from a fresh one");
    } else {
      CHECK(false, "a well-formed batch was refused");
    }
    // mutations: one image too many; a b64 record short of a string
    Case big = c;
    int img = 0;
    for (const BatchPlanRecord& r : big.recs) img += r.images;
    big.recs.back().images += big.max_batch - img + 1;
    if (!run(big, reused)) {
      ++refused;
      ++cov_too_many;
    } else {
      CHECK(false, "a batch over max_batch was planned");
    }
    if (c.b64) {
      Case bad = c;
      for (BatchPlanRecord& r : bad.recs)
        if (!r.preparsed) {
          r.b64_n = rng() % 2 ? r.b64_n - 1 : -1;
          break;
        }
      bool any = false;
      for (const BatchPlanRecord& r : bad.recs) any |= !r.preparsed;
      if (any) {
        if (!run(bad, reused)) {
          ++refused;
          ++cov_bad_scan;
        } else {
          CHECK(false, "a b64 record that does not match its scan was planned");
        }
      }
    }
  }
  const int* cov[] = {&cov_spans, &cov_staged, &cov_resident, &cov_preparsed, &cov_b64,
                      &cov_no_count_pass, &cov_no_tiles, &cov_too_many, &cov_bad_scan};
  for (size_t i = 0; i < sizeof cov / sizeof *cov; ++i)
    CHECK(*cov[i] > 0 || iters < 200, "branch %zu never reached", i);
  printf("batch_plan_check: %d plans, %d refused, %d failures\n", planned, refused, failures);
  if (failures == 0) printf("all checks passed\n");
  return failures ? 1 : 0;
}
