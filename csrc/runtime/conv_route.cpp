// Conv kernel selection and launch plans (see gale/conv_route.h). Host only.
#include "gale/conv_route.h"

#include <algorithm>
#include <atomic>

namespace gale {
namespace {

typedef long long i64;
constexpr i64 kLim31 = 1ll << 31;  // the kernels' element offsets and pixel indices are ints
constexpr i64 kSat = 1ll << 62;

// a * b, saturated: the operands are non-negative once dims_refusal() has passed
i64 mul(i64 a, i64 b) {
  i64 r;
  if (a < 0 || b < 0 || __builtin_mul_overflow(a, b, &r) || r > kSat) return kSat;
  return r;
}
i64 mul(i64 a, i64 b, i64 c) { return mul(mul(a, b), c); }
i64 mul(i64 a, i64 b, i64 c, i64 d) { return mul(mul(a, b), mul(c, d)); }

// a 1-D grid of 256-thread workgroups: the count is an int in the kernel's arguments and HIP
// takes fewer than 2^32 threads per grid dimension
constexpr i64 kMaxGrid256 = (1ll << 32) / 256 - 1;
constexpr i64 kMaxGridY = 65535;

int ilog2_exact(int v) {
  int s = 0;
  while (s < 30 && (1 << s) < v) ++s;
  return ((1 << s) == v) ? s : -1;
}

const char* dims_refusal(const ConvDesc& d, bool has_res) {
  if (d.H < 1 || d.W < 1 || d.Cin < 1 || d.Ho < 1 || d.Wo < 1 || d.Cout < 1 || d.KH < 1 ||
      d.KW < 1 || d.stride < 1 || d.pad < 0 || d.K < 1 || d.Kpad < 1 || d.Npad < 1)
    return "a dimension below 1 (pad below 0)";
  if (has_res && (d.res_H < 1 || d.res_W < 1 || d.res_C < 1)) return "a residual dimension below 1";
  return nullptr;
}

int conv_n_tiles(int Cout) {
  // channel tiles per workgroup n-block: whole Cout for the small-channel CNNs, 128 otherwise
  if (Cout <= 16) return 1;
  if (Cout <= 32) return 2;
  if (Cout <= 64) return 4;
  return 8;
}

// conv_mfma_plan, and why not
ConvMfmaPlan mfma_plan(const ConvDesc& d, int batch, bool has_res, const char** why) {
  ConvMfmaPlan p;
  auto no = [&](const char* w) {
    *why = w;
    return p;
  };
  if (batch <= 0) return no("batch <= 0");
  if (const char* w = dims_refusal(d, has_res)) return no(w);
  if (d.KH == 1 && d.KW == 1 && d.pad == 0 && d.Cin % 8 == 0) p.mode = CONV_MFMA_1X1;
  else if (d.Cin % 8 == 0 && ilog2_exact(d.Cin) >= 0) p.mode = CONV_MFMA_FAST;
  else p.mode = CONV_MFMA_GATHER;
  if (d.out_f32 && p.mode != CONV_MFMA_1X1) return no("out_f32 outside a 1x1 conv");
  if (d.Cout % 4 != 0) return no("Cout % 4");
  if (d.Kpad % 32 != 0) return no("Kpad % 32");

  // the kernel's pixel index, input offsets and residual offsets are 32-bit
  const i64 M = mul(batch, d.Ho, d.Wo);
  if (M >= kLim31) return no("batch*Ho*Wo >= 2^31");
  if (mul(batch, d.H, d.W, d.Cin) >= kLim31) return no("batch*H*W*Cin >= 2^31");
  if (has_res && mul(batch, d.res_H, d.res_W, d.res_C) >= kLim31)
    return no("batch*res_H*res_W*res_C >= 2^31");

  p.nt = conv_n_tiles(d.Cout);
  const int BN = p.nt * 16;
  if (d.Npad % BN != 0) return no("Npad % (16 nt)");
  p.n_blocks = (d.Cout + BN - 1) / BN;
  // pixel tiles per wave: the largest of {4 (2 for 8 channel tiles), 2, 1} that still gives the
  // chip >= 4 workgroups per CU; small layers (late stages, small batches) trade B-fragment reuse
  // for occupancy, which is what bounds them
  p.pr = (p.nt >= 8) ? 2 : 4;
  while (p.pr > 1 && (M + 64 * p.pr - 1) / (64 * p.pr) * p.n_blocks < 1024) p.pr >>= 1;
  const int BM = 4 * p.pr * 16;
  // (pixels past M in the last tile are indexed too, then masked)
  if ((M + BM - 1) / BM * BM >= kLim31) return no("batch*Ho*Wo >= 2^31");
  p.m_tiles = (int)((M + BM - 1) / BM);

  // K chunk: whole K if it fits the LDS budget (weight-stationary), else the largest multiple of
  // 32 that does.
  const int eb = d.fp8 ? 1 : 2;
  p.bk = d.Kpad;
  if ((size_t)BN * (p.bk + 16) * eb > (size_t)kConvMfmaLdsBudget) {
    p.bk = (kConvMfmaLdsBudget / (BN * eb) - 16) & ~31;
    if (p.bk < 32) return no("K chunk below 32");
  }
  p.nkc = (d.Kpad + p.bk - 1) / p.bk;
  p.lds_bytes = (size_t)BN * (p.bk + 16) * eb;

  p.grid_m = p.m_tiles;
  if (p.nkc == 1) {
    // weight-stationary: enough workgroups to fill 256 CUs x 8, each walks several tiles
    const int cap = 2048 / p.n_blocks > 0 ? 2048 / p.n_blocks : 1;
    p.grid_m = p.m_tiles < cap ? p.m_tiles : cap;
  }
  p.M = (int)M;
  const int cs = ilog2_exact(d.Cin);
  p.cin_shift = cs < 0 ? 0 : cs;
  p.kw_magic = (65536 + d.KW - 1) / d.KW;
  p.ok = true;
  return p;
}

const char* f32_route(const ConvDesc& d, int batch, bool has_res, ConvF32Plan& p) {
  if (d.Kpad % 16) return "f32: Kpad % 16";
  if (d.Cout % 4) return "Cout % 4";
  if (d.K > d.Kpad) return "f32: K > Kpad";
  if (d.Npad < d.Cout) return "Npad < Cout";
  if (d.fp8 || d.stem) return "f32 with fp8 or stem";
  if (has_res && (d.res_stride < 1 || d.res_C > d.Cout || d.res_C % 4))
    return "f32: residual needs res_stride >= 1, res_C <= Cout, res_C % 4 == 0";
  const i64 M = mul(batch, d.Ho, d.Wo);
  if (M >= kLim31) return "batch*Ho*Wo >= 2^31";
  // (element offsets are 64-bit in this kernel; its row indices n*H + h are ints)
  if (mul(batch, d.H) >= kLim31 || (has_res && mul(batch, d.res_H) >= kLim31))
    return "batch*H >= 2^31";
  const i64 gm = (M + kConvF32Tile - 1) / kConvF32Tile;
  const i64 gn = ((i64)d.Cout + kConvF32Tile - 1) / kConvF32Tile;
  if (gm > kMaxGrid256 || gn > kMaxGridY) return "grid exceeds the HIP limits";
  p.M = (int)M, p.grid_m = (int)gm, p.grid_n = (int)gn;
  return nullptr;
}

// the tile grid of conv_gemm for a desc its conditions (stem or not) have passed
const char* gemm_grid(const ConvDesc& d, int batch, ConvGemmPlan& p) {
  const i64 M = mul(batch, d.Ho, d.Wo);
  if (M >= kLim31) return "batch*Ho*Wo >= 2^31";
  if (mul(batch, d.H, d.W, d.Cin) >= kLim31) return "batch*H*W*Cin >= 2^31";
  p.stem = d.stem ? 1 : 0;
  p.nkb = d.K / 64;
  p.cin_blocks = d.stem ? 1 : d.Cin / 64;
  // 64-channel tiles for the single-k-step (K = 64) 1x1 convs: these are bound by their
  // epilogue traffic, and half-width tiles (24 KB of LDS, 91 VGPRs) put 5 workgroups on a CU
  // instead of 4 (ResNet-50 batch 256: 4.87 -> 4.81 ms; at K = 128 / 256 / 512 the same change
  // costs 0.6 / 1.6 / 2.6 %, profiles/r4_resnet50_layers.txt)
  // (the single-stage form for the K = 128 1x1 convs, with 64- or 128-channel tiles, measured
  // 0.4 / 2.2 % slower in round 4; for the 64-channel K = 256 ones, within noise)
  p.bn = (d.Npad % 128 == 0 && !(d.K == 64 && d.KH == 1 && !d.stem)) ? 128 : 64;
  // per-shape choice: the packed stem; K = 64 (one k-step: 1x1 convs on 64 channels) in the
  // single-stage form; everything else double-buffered
  p.stages = (!d.stem && p.nkb == 1) ? 1 : 2;
  const i64 mt = (M + 127) / 128;
  p.n_tiles = d.Npad / p.bn;
  const i64 nwg = mul(mt, p.n_tiles);
  if (nwg > kMaxGrid256) return "grid exceeds the HIP limits";
  p.M = (int)M, p.m_tiles = (int)mt, p.nwg = (int)nwg;
  return nullptr;
}

const char* stem_route(const ConvDesc& d, int batch, bool has_res, ConvGemmPlan& p) {
  if (d.fp8 || d.in_f32 || d.out_f32) return "stem: bf16 in and out only";
  if (d.Cin != 4 || d.KH != 8 || d.KW != 8 || d.K != 256 || d.Kpad != 256)
    return "stem: not the packed 8x8x4 kernel (Cin 4, K = Kpad = 256)";
  if (d.stride != 2) return "stem: stride != 2";
  if (d.pad != 3) return "stem: pad != 3";
  if (d.W != 2 * d.Wo + 6) return "stem: W != 2 Wo + 6";
  if (d.Cout % 64 != 0 || d.Npad % 64 != 0) return "stem: Cout % 64 or Npad % 64";
  if (has_res) return "stem: takes no residual";
  return gemm_grid(d, batch, p);
}

const char* gemm_route(const ConvDesc& d, int batch, bool has_res, ConvGemmPlan& p) {
  if (d.fp8 || d.in_f32 || d.f32) return "gemm: bf16 only";
  if (d.Cin % 64 != 0 || d.Cout % 8 != 0) return "gemm: Cin % 64 or Cout % 8";
  if (d.K != mul(d.KH, d.KW, d.Cin) || d.Kpad != d.K) return "gemm: K != KH*KW*Cin or Kpad != K";
  // channel tiles cover Npad (zero weight rows past Cout; the epilogue stores c < Cout only)
  const int bn = (d.Npad % 128 == 0) ? 128 : 64;
  if (d.Npad % bn != 0 || d.Npad < d.Cout) return "gemm: Npad % 64 or Npad < Cout";
  if (has_res && (d.res_C != d.Cout || d.res_stride != 1 || d.res_H != d.Ho || d.res_W != d.Wo))
    return "gemm: identity residual only";
  // 32-bit element offsets inside the kernel. (No minimum size: measured faster than conv_mfma
  // from ResNet-50 batch 64 up, including the 98-tile stage-4 layers,
  // profiles/archive/r1_resnet50_*.)
  return gemm_grid(d, batch, p);
}

// the patch-row capacities compiled (2 workgroups per CU at BN = 128 up to 184 rows)
constexpr int kPrr[3] = {152, 184, 240};

const char* patch_route(const ConvDesc& d, int batch, bool has_res, int mode, ConvPatchPlan& p) {
  if (d.stem || d.fp8 || d.f32 || d.in_f32 || d.out_f32) return "patch: bf16 only";
  if (d.KH != 3 || d.KW != 3 || d.stride != 1 || d.pad != 1) return "patch: 3x3 stride 1 pad 1 only";
  if (d.Cin % 64 != 0 || d.K != mul(9, d.Cin) || d.Kpad != d.K) return "patch: Cin % 64 or K";
  if (d.Ho != d.H || d.Wo != d.W || d.W > 128 || d.Cout % 8 != 0) return "patch: size";
  p.bn = (d.Npad % 128 == 0) ? 128 : 64;
  if (d.Npad % p.bn != 0 || d.Npad < d.Cout) return "patch: Npad";
  if (p.bn == 64 && mode < 2) return "patch: 64-channel tiles are off";
  if (has_res && (d.res_C != d.Cout || d.res_stride != 1 || d.res_H != d.H || d.res_W != d.W))
    return "patch: identity residual only";
  // tile rows: the largest divisor of H whose rows hold <= 128 pixels
  p.TR = 0;
  for (int tr = 128 / d.W; tr >= 1 && !p.TR; --tr)
    if (d.H % tr == 0) p.TR = tr;
  if (p.TR < 1) return "patch: no tile";
  // whole images per tile: several when one image's rows fill less than half the tile (7x7:
  // 2 x 49 of 128 MFMA rows)
  p.IMG = p.TR != d.H ? 1 : std::max(1, 128 / (d.H * d.W));
  p.P = p.IMG * p.TR * d.W;
  // (a tile below 3/4 of its MFMA rows wastes too much)
  if (p.P * 4 < 128 * 3 - 16) return "patch: tile too empty";
  p.PW = d.W + 2;
  p.PR1 = (p.TR + 2) * p.PW;
  p.PR = p.IMG * p.PR1;
  p.prr = 0;
  for (int c : kPrr)
    if (!p.prr && p.PR + 1 <= c) p.prr = c;
  if (p.prr == 0 || (p.bn == 128 && p.prr > 184)) return "patch: patch rows exceed the LDS";
  if (mul(batch, d.H, d.W, d.Cin) >= kLim31) return "batch*H*W*Cin >= 2^31";
  if (mul(batch, d.H, d.W, d.Cout) >= kLim31) return "batch*Ho*Wo*Cout >= 2^31";
  p.rblocks = d.H / p.TR;
  p.nsteps = 9 * (d.Cin / 64);  // k-steps: one tap of 64 input channels each
  p.n_tiles = d.Npad / p.bn;
  const i64 nwg = mul(((i64)batch + p.IMG - 1) / p.IMG, p.rblocks, p.n_tiles);
  if (nwg > kMaxGrid256) return "grid exceeds the HIP limits";
  p.batch = batch, p.nwg = (int)nwg;
  return nullptr;
}

std::atomic<int> g_path{0}, g_patch{1};

}  // namespace

const char* conv_kernel_name(int kernel) {
  static const char* const kNames[] = {"none", "f32", "gemm", "patch", "mfma"};
  return kernel >= CONV_NONE && kernel <= CONV_MFMA ? kNames[kernel] : "?";
}

void set_conv_path(int mode) { g_path = mode; }
int conv_path() { return g_path; }
void set_conv_patch(int mode) { g_patch = mode; }
ConvPolicy conv_policy() {
  return {g_path.load(std::memory_order_relaxed), g_patch.load(std::memory_order_relaxed)};
}

ConvMfmaPlan conv_mfma_plan(const ConvDesc& d, int batch, bool has_res) {
  const char* why = nullptr;
  return mfma_plan(d, batch, has_res, &why);
}

ConvRoute conv_route(const ConvDesc& d, int batch, bool has_res, ConvPolicy policy) {
  ConvRoute r;
  auto only = [&](int kernel, const char* refusal) {  // a desc with one kernel to go to
    r.refusal = refusal;
    r.kernel = refusal ? CONV_NONE : kernel;
    return r;
  };
  if (batch <= 0) return only(CONV_NONE, "batch <= 0");
  if (const char* w = dims_refusal(d, has_res)) return only(CONV_NONE, w);
  if (d.f32) return only(CONV_F32, f32_route(d, batch, has_res, r.f32));
  if (d.stem) return only(CONV_GEMM, stem_route(d, batch, has_res, r.gemm));
  if (policy.path != 1) {
    if (policy.patch && !patch_route(d, batch, has_res, policy.patch, r.patch))
      return only(CONV_PATCH, nullptr);
    r.patch = ConvPatchPlan();
    if (!gemm_route(d, batch, has_res, r.gemm)) return only(CONV_GEMM, nullptr);
    r.gemm = ConvGemmPlan();
  }
  if (d.fp8 && (!(d.in_scale > 0.f) || !(d.out_scale > 0.f)))
    return only(CONV_NONE, "fp8 in_scale / out_scale must be > 0");
  const char* why = nullptr;
  r.mfma = mfma_plan(d, batch, has_res, &why);
  if (!why && ((i64)r.mfma.grid_m > kMaxGrid256 || r.mfma.n_blocks > kMaxGridY))
    why = "grid exceeds the HIP limits";
  if (why) r.mfma = ConvMfmaPlan();
  return only(CONV_MFMA, why);
}

ConvRoute conv_route(const ConvDesc& d, int batch, bool has_res) {
  return conv_route(d, batch, has_res, conv_policy());
}

bool conv_patch_supported(const ConvDesc& d, int batch, bool has_res) {
  return conv_route(d, batch, has_res).kernel == CONV_PATCH;
}

// ---- the fused ops -----------------------------------------------------------------------

ConvProjPlan conv_gemm_proj_plan(const ConvDesc& d, int batch, int H2, int W2, int Cin2,
                                 int stride2, int Kpad2) {
  // (no conv_path switch: like the fused block kernels this op has no other implementation)
  ConvProjPlan p;
  if (batch < 0 || dims_refusal(d, false) || H2 < 1 || W2 < 1 || Cin2 < 1) return p;
  if (d.fp8 || d.in_f32 || d.f32 || d.out_f32 || d.stem || d.has_res) return p;
  if (d.KH != 1 || d.KW != 1 || d.stride != 1 || d.pad != 0) return p;
  if (d.Cin % 64 != 0 || d.K != d.Cin || d.Kpad != d.K || d.Ho != d.H || d.Wo != d.W) return p;
  if (Cin2 % 64 != 0 || Kpad2 != Cin2 || stride2 < 1) return p;
  if ((H2 - 1) / stride2 + 1 != d.Ho || (W2 - 1) / stride2 + 1 != d.Wo) return p;
  if (d.Npad % 128 != 0 || d.Npad < d.Cout || d.Cout % 8 != 0) return p;
  // images per launch: every element offset of the launch's x, x2 and y (and its pixel count)
  // must stay below 2^31 (max_batch >= ~2675 overflowed the stage-2 projection's input)
  i64 per = mul(d.Ho, d.Wo, d.Cout);
  per = std::max(per, mul(d.H, d.W, d.Cin));
  per = std::max(per, mul(H2, W2, Cin2));
  p.chunk_images = (int)std::min<i64>((kLim31 - 1) / per, 1 << 20);
  p.n_tiles = d.Npad / 128;
  p.nkb1 = d.Cin / 64;
  p.nkb = p.nkb1 + Cin2 / 64;
  // (a chunk's grid: at most 2^31 / 128 pixel tiles times n_tiles)
  p.ok = p.chunk_images > 0 &&
         mul((mul(p.chunk_images, d.Ho, d.Wo) + 127) / 128, p.n_tiles) <= kMaxGrid256;
  return p;
}

bool conv_gemm_proj_supported(const ConvDesc& d, int batch, int H2, int W2, int Cin2,
                              int stride2, int Kpad2) {
  return conv_gemm_proj_plan(d, batch, H2, W2, Cin2, stride2, Kpad2).ok;
}

bool bottleneck56_supported(int H, int W, int cin, int cmid, int cout, int down) {
  return H == kBneckH && W == kBneckW && cmid == kBneckMid && cout == kBneckOut &&
         ((down && cin == kBneckDownIn) || (!down && cin == kBneckOut));
}

bool stem_pool_supported(const ConvDesc& d, int H, int W, int C, int k, int s, int p, int Ho,
                         int Wo) {
  return d.stem && !d.fp8 && !d.f32 && !d.out_f32 && d.relu && !d.has_res && d.H == kStemInH &&
         d.W == kStemInW && d.Ho == kStemOut && d.Wo == kStemOut && d.Cout == kStemC &&
         d.Npad == kStemC && d.K == kStemK && d.Kpad == kStemK && H == kStemOut &&
         W == kStemOut && C == kStemC && k == 3 && s == 2 && p == 1 && Ho == kStemPooled &&
         Wo == kStemPooled;
}

}  // namespace gale
