// Which kernel serves a convolution launch, and in which form: decided here, on the host, for
// every conv kernel (conv_f32, conv_gemm incl. the packed stem, conv_patch, conv_mfma) and for
// the fused ops' geometry checks. No HIP call here or in conv_route.cpp, so the decision is
// testable (and sanitizer-checked) without a GPU. conv2d() launches from a ConvRoute and from
// nothing else; validate_plan (gale/forward_plan.h) routes every conv op of a plan before the
// executor makes its first HIP call.
#pragma once
#include <stddef.h>

namespace gale {

// Geometry of one convolution (or fully connected layer expressed as a 1x1 convolution over a
// 1x1 image). Independent of the batch size, which is a launch argument so one descriptor serves
// every hipGraph batch bucket.
struct ConvDesc {
  int H, W, Cin;        // input spatial size and channel count (channel stride of the input)
  int Ho, Wo, Cout;     // output spatial size; Cout = stored output channels (channel stride of y)
  int KH, KW, stride, pad;
  int K;                // true reduction length KH*KW*Cin
  int Kpad;             // K rounded up to 32 (row stride of the packed weights)
  int Npad;             // rows of the packed weight matrix (multiple of the n-block)
  int relu;             // apply ReLU in the epilogue
  // residual added before the ReLU (ResNet shortcut). res_C < Cout zero-pads the extra channels
  // and res_stride > 1 subsamples: together they are the parameter-free "option A" shortcut.
  int has_res, res_H, res_W, res_C, res_stride;
  int in_f32;           // input tensor is fp32 (network input; converted to bf16 while staging)
  int out_f32;          // output tensor is fp32 (classifier logits)
  int fp8;              // OCP e4m3 operands (fp8 MFMA path): weights per-channel (wscale),
                        // activations per tensor (value = code * scale)
  float in_scale;       // fp8: input scale (in_f32: the input is quantised with this step)
  float out_scale;      // fp8: output scale (ignored for out_f32)
  float res_scale;      // fp8: residual scale
  // 1 = packed-stem layout (ResNet-50 7x7/2 stem, bf16): x is the stem_pack() image
  // [B][H][W][4] bf16 with W = 2*Wo + 6 (3 zero columns left, the rest right), the packed weights
  // are [Npad][256] with k = kh*32 + kw*4 + c over an 8x8x4 zero-padded kernel (KH = KW = 8,
  // K = Kpad = 256), so each kernel row of one output pixel is ONE 64-byte run of x.
  int stem;
  // 1 = reference-precision plan (--dtype fp32): x, w, residual and y are all fp32 and the conv
  // runs on the fp32 matrix core (conv_f32.hip, v_mfma_f32_16x16x4_f32); Kpad % 16 == 0
  int f32;
};

// ---- one launch plan per kernel: what its launcher needs beyond the desc and the pointers ------
// Every count below was computed in 64 bits and fits the kernel's 32-bit use of it.

// conv_mfma.hip: the template instantiation (mode, nt, pr) and the grid depend on the batch, not
// only on the layer. has_res: the launch reads a residual (d.has_res and a non-null pointer).
// ok == false: Cout % 4, Kpad % 32, Npad % (16 nt), out_f32 outside 1x1 mode, a K chunk below 32,
// or a launch the kernel's 32-bit offsets cannot index: batch*Ho*Wo (rounded up to whole pixel
// tiles), batch*H*W*Cin or, with a residual, batch*res_H*res_W*res_C at 2^31 or more.
enum ConvMfmaMode : int { CONV_MFMA_FAST = 0, CONV_MFMA_GATHER = 1, CONV_MFMA_1X1 = 2 };
struct ConvMfmaPlan {
  bool ok = false;
  int mode = CONV_MFMA_FAST;  // ConvMfmaMode
  int nt = 0;                 // channel tiles (16 channels each) per workgroup n-block
  int pr = 0;                 // pixel tiles (16 pixels each) per wave: the tile is 64 pr pixels
  int n_blocks = 0;           // grid.y
  int bk = 0;                 // K chunk staged in LDS
  int nkc = 0;                // K chunks; 1 = the weights stay resident and tiles are walked
  int m_tiles = 0;            // pixel tiles of the launch
  int grid_m = 0;             // grid.x; < m_tiles: workgroups walk the tiles grid-stride
  size_t lds_bytes = 0;
  int M = 0;                  // batch * Ho * Wo
  int cin_shift = 0;          // log2(Cin) in fast mode
  int kw_magic = 0;           // ceil(65536 / KW)
};
ConvMfmaPlan conv_mfma_plan(const ConvDesc& d, int batch, bool has_res);

// conv_gemm.hip (128-pixel tiles): bn channels per tile, one LDS stage (the single-k-step form)
// or two, or the packed-stem form; the grid is nwg = m_tiles * n_tiles workgroups.
struct ConvGemmPlan {
  int bn = 0, stages = 0, stem = 0;
  int M = 0, m_tiles = 0, n_tiles = 0, nwg = 0;
  int nkb = 0;         // 64-deep k-steps
  int cin_blocks = 0;  // Cin / 64 (1 for the stem)
};

// conv_patch.hip: TR whole output rows of IMG images per tile (P pixels), the halo patch of PR
// rows (PR1 per image, PW wide) in a buffer of prr rows (152 / 184 / 240), rblocks row blocks
// per image, nsteps k-steps (nine taps per 64 input channels).
struct ConvPatchPlan {
  int bn = 0, prr = 0;
  int TR = 0, IMG = 0, P = 0, PW = 0, PR1 = 0, PR = 0, rblocks = 0, nsteps = 0;
  int batch = 0, n_tiles = 0, nwg = 0;
};

// conv_f32.hip: kConvF32Tile pixels x kConvF32Tile channels per workgroup.
constexpr int kConvF32Tile = 64;
struct ConvF32Plan {
  int M = 0, grid_m = 0, grid_n = 0;
};

enum ConvKernel : int { CONV_NONE = 0, CONV_F32, CONV_GEMM, CONV_PATCH, CONV_MFMA };
const char* conv_kernel_name(int kernel);  // "none", "f32", "gemm", "patch", "mfma"

// conv selection (tests / A-B benches). path: 0 auto, 1 never the GEMM paths (conv_gemm and
// conv_patch), 2 as 0. patch: 0 conv_patch off, 1 (default) its 128-channel tiles only (ResNet-50
// 28x28 and 14x14 conv2: 90 -> 77 us and 86 -> 76 us per layer at batch 256), 2 also the
// 64-channel tiles (the 56x56 conv2 measured 104-110 -> 125-127 us there: one input block per
// tile leaves the patch load exposed, so those stay on conv_gemm;
// profiles/archive/r2_conv_patch.txt).
struct ConvPolicy {
  int path = 0;
  int patch = 1;
};
void set_conv_path(int mode);
int conv_path();
void set_conv_patch(int mode);
ConvPolicy conv_policy();  // the process-wide policy the three above set

// The launch conv2d() makes for (d, batch, has_res) under a policy: the kernel and its plan (the
// other three stay default). The order is fp32 -> packed stem -> patch -> GEMM -> MFMA; a desc a
// kernel's own conditions turn down falls through to the next, except the fp32 and stem descs,
// which have one kernel. kernel == CONV_NONE: no kernel takes the launch (conv2d() returns
// hipErrorInvalidValue) and refusal names the condition that failed, e.g. "Cout % 4" or
// "batch*H*W*Cin >= 2^31"; otherwise refusal is null. batch <= 0 is refused ("batch <= 0":
// conv2d() returns before it routes).
struct ConvRoute {
  int kernel = CONV_NONE;  // ConvKernel
  const char* refusal = nullptr;
  ConvF32Plan f32;
  ConvGemmPlan gemm;
  ConvPatchPlan patch;
  ConvMfmaPlan mfma;
};
ConvRoute conv_route(const ConvDesc& d, int batch, bool has_res, ConvPolicy policy);
ConvRoute conv_route(const ConvDesc& d, int batch, bool has_res);  // the process policy
// conv_route(...).kernel == CONV_PATCH under the process policy
bool conv_patch_supported(const ConvDesc& d, int batch, bool has_res);

// ---- the fused ops' geometry ---------------------------------------------------------------
// The sizes the fused kernels are compiled for: bottleneck_fused.hip and stem_pool.hip
// static_assert that their own constants equal these. kConvMfmaLdsBudget bounds the dynamic LDS
// conv_mfma_plan() gives a launch.
constexpr int kBneckH = 56, kBneckW = 56, kBneckMid = 64, kBneckOut = 256;
constexpr int kBneckDownIn = 64;  // input channels of the block with the projection shortcut
constexpr int kStemInH = 224, kStemInW = 230;  // packed input image
constexpr int kStemOut = 112, kStemPooled = 56, kStemC = 64, kStemK = 256;
constexpr int kConvMfmaLdsBudget = 80 * 1024;  // 2 workgroups per CU by LDS

// conv3 of a ResNet bottleneck with its projection shortcut as ONE GEMM (conv2d_gemm_proj). d:
// the 1x1 stride-1 conv on x (no residual); x2 [B][H2][W2][Cin2] bf16 sampled at stride2 onto
// d's output grid, w2 [Npad][Kpad2]. Any batch >= 0: the launcher splits it into chunks of
// chunk_images, whose 32-bit element offsets (x, x2, y) and pixel count hold.
struct ConvProjPlan {
  bool ok = false;
  int chunk_images = 0;
  int n_tiles = 0, nkb1 = 0, nkb = 0;  // 128-channel tiles; k-steps of x, and of x and x2
};
ConvProjPlan conv_gemm_proj_plan(const ConvDesc& d, int batch, int H2, int W2, int Cin2,
                                 int stride2, int Kpad2);
bool conv_gemm_proj_supported(const ConvDesc& d, int batch, int H2, int W2, int Cin2,
                              int stride2, int Kpad2);
// One whole ResNet-50 56x56 bottleneck per launch (bottleneck_fused.hip), bf16 NHWC:
// y = relu(conv3(relu(conv2(relu(conv1(x))))) + shortcut), shortcut = x (cin 256) or, with
// down = 1 (block 0, cin 64), the 1x1 projection bf16(wd . x + bd). Packed weights as conv2d's:
// w1 [64][cin], w2 [64][576], w3 / wd [256][64]; biases fp32 with BatchNorm folded in.
struct BottleneckParams {
  const void* w1 = nullptr;
  const void* w2 = nullptr;
  const void* w3 = nullptr;
  const void* wd = nullptr;
  const float* b1 = nullptr;
  const float* b2 = nullptr;
  const float* b3 = nullptr;
  const float* bd = nullptr;
  int cin = 256;
  int down = 0;
};
bool bottleneck56_supported(int H, int W, int cin, int cmid, int cout, int down);
// the stem's conv desc + the maxpool op's geometry
bool stem_pool_supported(const ConvDesc& d, int H, int W, int C, int k, int s, int p, int Ho,
                         int Wo);

}  // namespace gale
