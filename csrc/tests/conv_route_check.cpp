// Sanitizer run of the conv route (gale/conv_route.h): a fixed seed, layer-like descs of every
// kernel's family with a few fields then pushed to extremes (fields up to 2^20, negative and
// zero ones, batches up to 2^30), and wholly random descs, under each policy. Whenever a kernel
// is chosen, every count its launcher passes on as a 32-bit value is recomputed here in 128 bits
// from the desc and must fit, and the grid must be one HIP takes. No HIP header, no HIP call.
//   build/asan/conv_route_check [iterations]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>

#include "gale/conv_route.h"

using namespace gale;

namespace {

typedef __int128 wide;
const wide kLim = (wide)1 << 31;
const wide kGridX = ((wide)1 << 32) / 256 - 1;  // 256-thread workgroups: < 2^32 threads
const wide kGridY = 65535;

int failures = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (++failures < 50) {                               \
        fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
        fprintf(stderr, __VA_ARGS__);                      \
        fprintf(stderr, "\n");                             \
      }                                                    \
    }                                                      \
  } while (0)

int pick(std::mt19937& rng, std::initializer_list<int> v) { return v.begin()[rng() % v.size()]; }

int extreme(std::mt19937& rng) {
  switch (rng() % 6) {
    case 0: return 0;
    case 1: return -(int)(rng() % 5) - 1;
    case 2: return 1 << 20;
    case 3: return (1 << 20) - (int)(rng() % 64);
    case 4: return 1 + (int)(rng() % 1024);
    default: return (int)(rng() % ((1 << 20) + 1));
  }
}

int round_up(int v, int m) { return (v + m - 1) / m * m; }

// a desc as the model builder writes them, for the family `fam`: 0 fp32, 1 packed stem,
// 2 3x3 stride 1 (patch), 3 wide bf16 (GEMM), 4 anything (MFMA)
ConvDesc layer(std::mt19937& rng, int fam) {
  ConvDesc d{};
  d.in_scale = d.out_scale = d.res_scale = 1.f;
  d.res_stride = 1;
  if (fam == 1) {
    d.Ho = d.Wo = 1 + (int)(rng() % 128);
    d.H = 2 * d.Ho, d.W = 2 * d.Wo + 6, d.Cin = 4, d.KH = d.KW = 8, d.stride = 2, d.pad = 3;
    d.K = d.Kpad = 256, d.Cout = d.Npad = pick(rng, {64, 128, 192}), d.relu = 1, d.stem = 1;
    return d;
  }
  int k = pick(rng, {1, 1, 3, 3, 5, 7}), stride = pick(rng, {1, 1, 2}), pad = k / 2;
  if (fam == 2) k = 3, stride = 1, pad = 1;
  d.H = fam == 2 ? pick(rng, {7, 14, 28, 56, 12, 30, 128, 130}) : 1 + (int)(rng() % 64);
  d.W = fam == 2 && rng() % 4 ? d.H : 1 + (int)(rng() % 64);
  d.Cin = fam == 2 || fam == 3 ? 64 * (1 + (int)(rng() % 8))
                               : pick(rng, {1, 3, 8, 16, 24, 32, 40, 64, 128});
  d.Cout = fam == 4 ? 4 * (1 + (int)(rng() % 64)) : 8 * (1 + (int)(rng() % 64));
  d.KH = d.KW = k, d.stride = stride, d.pad = pad;
  d.Ho = (d.H + 2 * pad - k) / stride + 1, d.Wo = (d.W + 2 * pad - k) / stride + 1;
  if (d.Ho < 1 || d.Wo < 1) d.Ho = d.Wo = 1;
  d.K = k * k * d.Cin;
  d.Kpad = round_up(d.K, fam == 0 ? 16 : 32);
  d.Npad = round_up(d.Cout, d.Cout <= 16 ? 16 : d.Cout <= 32 ? 32 : d.Cout <= 64 ? 64 : 128);
  d.relu = rng() % 2;
  d.f32 = fam == 0;
  if (fam == 4) d.fp8 = rng() % 2, d.in_f32 = rng() % 4 == 0, d.out_f32 = k == 1 && rng() % 4 == 0;
  if (rng() % 3 == 0) {
    d.has_res = 1, d.res_H = d.Ho, d.res_W = d.Wo, d.res_C = d.Cout;
    if (fam == 4 && rng() % 2) d.res_H = d.H, d.res_W = d.W, d.res_C = d.Cin, d.res_stride = stride;
  }
  return d;
}

void mutate(std::mt19937& rng, ConvDesc& d) {
  int* const f[] = {&d.H, &d.W, &d.Cin, &d.Ho, &d.Wo, &d.Cout, &d.KH, &d.KW, &d.stride, &d.pad,
                    &d.K, &d.Kpad, &d.Npad, &d.res_H, &d.res_W, &d.res_C, &d.res_stride};
  const int n = (int)(sizeof(f) / sizeof(f[0]));
  switch (rng() % 8) {
    case 0: d.fp8 ^= 1; break;
    case 1: d.in_scale = rng() % 2 ? 0.f : -1.f; break;
    case 2: d.out_f32 ^= 1; break;
    case 3: d.stem ^= 1; break;
    case 4: d.f32 ^= 1; break;
    default: *f[rng() % n] = extreme(rng);
  }
}

wide cdiv(wide a, wide b) { return (a + b - 1) / b; }

// every 32-bit quantity of the chosen kernel's launch, from the desc alone
void check_route(const ConvDesc& d, int batch, bool has_res, const ConvRoute& r) {
  const wide B = batch, M = B * d.Ho * d.Wo, in = B * d.H * d.W * d.Cin;
  CHECK(batch >= 1 && d.H >= 1 && d.W >= 1 && d.Cin >= 1 && d.Ho >= 1 && d.Wo >= 1 &&
            d.Cout >= 1 && d.KW >= 1 && d.KH >= 1 && d.Kpad >= 1,
        "a routed launch with a dimension below 1");
  CHECK(M >= 1 && M < kLim, "M outside an int");
  switch (r.kernel) {
    case CONV_F32: {
      const ConvF32Plan& p = r.f32;
      CHECK(p.M == M && p.grid_m == cdiv(M, 64) && p.grid_n == cdiv(d.Cout, 64), "f32 grid");
      CHECK(p.grid_m >= 1 && p.grid_m <= kGridX && p.grid_n >= 1 && p.grid_n <= kGridY,
            "f32 grid outside HIP's limits");
      CHECK(B * d.H < kLim && (!has_res || B * d.res_H < kLim), "f32 row index");
      CHECK(d.Kpad % 16 == 0 && d.K <= d.Kpad && d.Npad >= d.Cout && d.Cout % 4 == 0, "f32 desc");
      break;
    }
    case CONV_GEMM: {
      const ConvGemmPlan& p = r.gemm;
      CHECK(p.M == M && in < kLim, "gemm offsets");
      CHECK((p.bn == 64 || p.bn == 128) && (p.stages == 1 || p.stages == 2), "gemm form");
      CHECK(p.stem == (d.stem ? 1 : 0) && (!p.stem || p.stages == 2), "gemm stem form");
      CHECK(p.m_tiles == cdiv(M, 128) && (wide)p.n_tiles * p.bn == d.Npad && p.n_tiles >= 1,
            "gemm tiles");
      CHECK(p.nwg == (wide)p.m_tiles * p.n_tiles && p.nwg >= 1 && p.nwg <= kGridX, "gemm grid");
      CHECK(p.nkb >= 1 && p.nkb * 64 == d.K && (p.stages == 1) == (p.nkb == 1 && !p.stem),
            "gemm k-steps");
      CHECK(p.cin_blocks == (d.stem ? 1 : d.Cin / 64) && p.cin_blocks >= 1, "gemm cin blocks");
      CHECK(!d.fp8 && !d.in_f32 && !d.f32 && d.Kpad == d.K, "gemm desc");
      break;
    }
    case CONV_PATCH: {
      const ConvPatchPlan& p = r.patch;
      CHECK(in < kLim && B * d.H * d.W * d.Cout < kLim, "patch offsets");
      CHECK(p.batch == batch && p.TR >= 1 && p.IMG >= 1 && p.TR * p.rblocks == d.H, "patch rows");
      CHECK(p.IMG == 1 || p.TR == d.H, "several images per tile of partial images");
      CHECK(p.P == p.IMG * p.TR * d.W && p.P <= 128 && p.P >= 92, "patch tile pixels");
      CHECK(p.PW == d.W + 2 && p.PR1 == (p.TR + 2) * p.PW && p.PR == p.IMG * p.PR1, "patch geom");
      CHECK((p.prr == 152 || p.prr == 184 || p.prr == 240) && p.PR + 1 <= p.prr, "patch rows/LDS");
      CHECK((p.bn == 64 || p.bn == 128) && (p.bn == 64 || p.prr <= 184), "patch form");
      CHECK((wide)p.n_tiles * p.bn == d.Npad && p.nsteps == 9 * (d.Cin / 64) && p.nsteps >= 9,
            "patch tiles / steps");
      CHECK(p.nwg == cdiv(B, p.IMG) * p.rblocks * p.n_tiles && p.nwg >= 1 && p.nwg <= kGridX,
            "patch grid");
      CHECK(!d.fp8 && !d.f32 && !d.stem && d.KH == 3 && d.KW == 3 && d.Cin % 64 == 0, "patch desc");
      break;
    }
    case CONV_MFMA: {
      const ConvMfmaPlan& p = r.mfma;
      const ConvMfmaPlan q = conv_mfma_plan(d, batch, has_res);
      CHECK(p.ok && q.ok && p.mode == q.mode && p.nt == q.nt && p.pr == q.pr &&
                p.n_blocks == q.n_blocks && p.bk == q.bk && p.nkc == q.nkc &&
                p.m_tiles == q.m_tiles && p.grid_m == q.grid_m && p.lds_bytes == q.lds_bytes &&
                p.M == q.M && p.cin_shift == q.cin_shift && p.kw_magic == q.kw_magic,
            "the route's MFMA plan is not conv_mfma_plan's");
      const int BM = 64 * p.pr;
      CHECK(p.M == M && in < kLim && (!has_res || B * d.res_H * d.res_W * d.res_C < kLim),
            "mfma offsets");
      CHECK((p.pr == 1 || p.pr == 2 || p.pr == 4) && p.m_tiles == cdiv(M, BM) &&
                (wide)p.m_tiles * BM < kLim,
            "mfma pixel tiles");
      CHECK(p.grid_m >= 1 && p.grid_m <= p.m_tiles && p.grid_m <= kGridX && p.n_blocks >= 1 &&
                p.n_blocks <= kGridY && (wide)p.n_blocks * p.nt * 16 >= d.Cout,
            "mfma grid");
      CHECK(p.bk >= 32 && p.bk % 32 == 0 && (wide)p.bk * p.nkc >= d.Kpad &&
                p.lds_bytes <= (size_t)kConvMfmaLdsBudget,
            "mfma K chunks");
      CHECK(p.kw_magic == (65536 + d.KW - 1) / d.KW, "mfma kw_magic");
      CHECK(p.mode != CONV_MFMA_FAST || (1 << p.cin_shift) == d.Cin, "mfma cin_shift");
      CHECK(!d.fp8 || (d.in_scale > 0.f && d.out_scale > 0.f), "fp8 scales");
      break;
    }
    default: CHECK(false, "kernel %d", r.kernel);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 300000;
  std::mt19937 rng(20241021);
  const ConvPolicy policies[5] = {{0, 1}, {1, 1}, {2, 1}, {0, 0}, {0, 2}};
  long chosen[5] = {0, 0, 0, 0, 0}, proj_ok = 0;
  for (int k = -1; k < 7; ++k) CHECK(strlen(conv_kernel_name(k)) > 0, "kernel name %d", k);
  for (int it = 0; it < iters; ++it) {
    ConvDesc d{};
    if (it % 8 == 7) {  // wholly random
      int* const f[] = {&d.H, &d.W, &d.Cin, &d.Ho, &d.Wo, &d.Cout, &d.KH, &d.KW, &d.stride,
                        &d.pad, &d.K, &d.Kpad, &d.Npad, &d.res_H, &d.res_W, &d.res_C,
                        &d.res_stride};
      for (int* p : f) *p = extreme(rng);
      d.has_res = rng() % 2, d.fp8 = rng() % 2, d.f32 = rng() % 4 == 0, d.stem = rng() % 4 == 0;
      d.in_scale = d.out_scale = 1.f;
    } else {
      d = layer(rng, (int)(rng() % 5));
      for (int m = (int)(rng() % 4) - 1; m > 0; --m) mutate(rng, d);
    }
    int batch;
    switch (rng() % 6) {
      case 0: batch = (int)(rng() % 3) - 1; break;
      case 1: batch = 1 << 30; break;
      case 2: batch = 1 + (int)(rng() % (1 << 30)); break;
      case 3: batch = 1 + (int)(rng() % 65536); break;
      default: batch = 1 + (int)(rng() % 512);
    }
    const bool has_res = d.has_res && rng() % 4 != 0;
    for (const ConvPolicy& pol : policies) {
      const ConvRoute r = conv_route(d, batch, has_res, pol);
      CHECK(r.kernel >= CONV_NONE && r.kernel <= CONV_MFMA, "kernel %d", r.kernel);
      CHECK((r.kernel == CONV_NONE) == (r.refusal != nullptr), "refusal / kernel mismatch");
      CHECK(!r.refusal || strlen(r.refusal) > 0, "empty refusal");
      ++chosen[r.kernel];
      if (r.kernel == CONV_NONE) continue;
      check_route(d, batch, has_res, r);
      CHECK(pol.path != 1 || d.stem || (r.kernel != CONV_GEMM && r.kernel != CONV_PATCH),
            "path 1 chose a GEMM kernel");
      CHECK(pol.patch != 0 || r.kernel != CONV_PATCH, "patch 0 chose conv_patch");
      CHECK(r.kernel != CONV_PATCH || r.patch.bn == 128 || pol.patch >= 2,
            "64-channel patch tiles below patch mode 2");
      CHECK((r.kernel == CONV_F32) == (d.f32 != 0), "f32 desc / kernel mismatch");
    }
    // the process policy and the predicate built on it
    set_conv_path(policies[it % 5].path);
    set_conv_patch(policies[it % 5].patch);
    const ConvRoute a = conv_route(d, batch, has_res), b = conv_route(d, batch, has_res, policies[it % 5]);
    CHECK(a.kernel == b.kernel && a.refusal == b.refusal, "process policy route differs");
    CHECK(conv_patch_supported(d, batch, has_res) == (a.kernel == CONV_PATCH), "patch predicate");

    // the fused projection: any accepted plan's chunk keeps every offset and its grid in range
    const int H2 = extreme(rng) % 256, Cin2 = 64 * (int)(rng() % 20), s2 = (int)(rng() % 4);
    ConvDesc c = layer(rng, 3);
    c.KH = c.KW = c.stride = 1, c.pad = 0, c.K = c.Kpad = c.Cin, c.Ho = c.H, c.Wo = c.W;
    c.has_res = 0, c.Npad = round_up(c.Cout, 128);
    const int h2 = rng() % 2 ? H2 : c.H * (s2 ? s2 : 1), w2 = rng() % 2 ? H2 : c.W * (s2 ? s2 : 1);
    const int kpad2 = rng() % 8 ? Cin2 : 32;
    const ConvProjPlan pp = conv_gemm_proj_plan(c, batch, h2, w2, Cin2, s2, kpad2);
    CHECK(pp.ok == conv_gemm_proj_supported(c, batch, h2, w2, Cin2, s2, kpad2), "proj predicate");
    if (pp.ok) {
      ++proj_ok;
      const wide n = pp.chunk_images;
      CHECK(n >= 1 && n * c.Ho * c.Wo * c.Cout < kLim && n * c.H * c.W * c.Cin < kLim &&
                n * h2 * w2 * Cin2 < kLim, "proj chunk offsets");
      CHECK(cdiv(n * c.Ho * c.Wo, 128) * pp.n_tiles <= kGridX && pp.n_tiles >= 1, "proj grid");
      CHECK(pp.nkb1 == c.Cin / 64 && pp.nkb == pp.nkb1 + Cin2 / 64 && Cin2 >= 64, "proj k-steps");
    }
    (void)bottleneck56_supported(extreme(rng), extreme(rng), extreme(rng), 64, 256, rng() % 2);
    (void)stem_pool_supported(d, extreme(rng), 112, 64, 3, 2, 1, 56, 56);
  }
  set_conv_path(0);
  set_conv_patch(1);
  CHECK(bottleneck56_supported(56, 56, 256, 64, 256, 0) && bottleneck56_supported(56, 56, 64, 64, 256, 1) &&
            !bottleneck56_supported(56, 56, 128, 64, 256, 0) && !bottleneck56_supported(56, 56, 64, 64, 256, 0),
        "bottleneck56_supported");
  for (int k = CONV_NONE; k <= CONV_MFMA; ++k)
    CHECK(chosen[k] > iters / 100, "%s chosen only %ld times", conv_kernel_name(k), chosen[k]);
  CHECK(proj_ok > iters / 100, "fused projection accepted only %ld times", proj_ok);
  printf("%d descs x 5 policies: none %ld, f32 %ld, gemm %ld, patch %ld, mfma %ld; proj %ld\n",
         iters, chosen[0], chosen[1], chosen[2], chosen[3], chosen[4], proj_ok);
  if (failures) {
    fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  printf("all checks passed\n");
  return 0;
}
