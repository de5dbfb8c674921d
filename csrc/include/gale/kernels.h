// Host-visible declarations of the gale CDNA4 (gfx950) kernels.
//
// Every tensor is NHWC. Activations are bf16, the network input is fp32 (as parsed from the
// InstObj JSON contract, /root/reference/src/main/java/dke/model/data/InstObj.java:8) and the
// network output is the fp32 softmax (the reference fetches "output/Softmax:0",
// /root/reference/src/main/java/dke/model/InferenceBolt.java:83).
//
// These launchers never allocate or synchronise, so they can be captured into a hipGraph.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../codec/elemtype.h"  // InputElem (no HIP: shared with the host codec)
#include "../../codec/pixfmt.h"  // PackedFormat (no HIP: shared with the host codec)
#include "../../codec/yuv.h"  // YuvFormat, YuvCoeffs (no HIP: shared with the host codec)
#include "gale/conv_route.h"  // ConvDesc, the conv launch plans, BottleneckParams (no HIP)

namespace gale {

// y[B,Ho,Wo,Cout] = act(conv(x, w) + bias (+ residual)), by the kernel conv_route() picks for
// the launch (gale/conv_route.h; hipErrorInvalidValue where it picks none).
// w: [Npad][Kpad] (bf16 or e4m3), k = (kh*KW + kw)*Cin + ci, zero padded.
// bias: [Npad] fp32 (BatchNorm already folded in). wscale: [Npad] fp32 per-output-channel weight
// dequant scale (fp8 path only; nullptr otherwise). In the fp8 path x / res / y are e4m3 tensors
// (x fp32 when in_f32, y fp32 when out_f32).
hipError_t conv2d(const ConvDesc& d, int batch, const void* x, const void* w, const float* bias,
                  const float* wscale, const void* res, void* y, hipStream_t stream);

// Activation element types of the pooling / head kernels (their `et` argument; 1 was the old
// fp8 flag, so fp8 callers are unchanged)
enum ElemType : int { ET_BF16 = 0, ET_FP8 = 1, ET_F32 = 2 };

// conv3 of a ResNet bottleneck with its projection shortcut as ONE GEMM over the concatenated
// reduction (conv_gemm.hip): y = act(conv1x1(x, w) + bias + conv1x1_stride2(x2, w2) + bias2),
// launched from conv_gemm_proj_plan() (gale/conv_route.h). The projection's output tensor never
// exists.
hipError_t conv2d_gemm_proj(const ConvDesc& d, int batch, const void* x, const void* w,
                            const float* bias, const void* x2, int H2, int W2, int Cin2,
                            int stride2, int Kpad2, const void* w2, const float* bias2, void* y,
                            hipStream_t stream);

// One whole ResNet-50 56x56 bottleneck per launch (BottleneckParams, gale/conv_route.h).
hipError_t bottleneck56(const BottleneckParams& p, int batch, const void* x, void* y,
                        hipStream_t stream);

// ResNet-50 ImageNet stem conv (packed-stem ConvDesc, ReLU) + 3x3/2 max-pool in one launch
// (stem_pool.hip; stem_pool_supported, gale/conv_route.h): x = stem_pack() image bf16
// [B][224][230][4], w [64][256], y bf16 [B][56][56][64].
hipError_t stem_pool(int batch, const void* x, const void* w, const float* bias, void* y,
                     hipStream_t stream);

// fp32 NHWC [B][H][W][C<=4] -> bf16 [B][H][Wp][4] with `lp` zero columns on the left (and zeros
// up to Wp on the right, channels >= C zero): the input of a packed-stem conv (ConvDesc::stem).
hipError_t stem_pack(int batch, int H, int W, int C, int Wp, int lp, const float* x, void* y,
                     hipStream_t stream);

// Max pooling, NHWC bf16 / e4m3 (the scale passes through) / fp32 by `et` (ElemType), window k,
// stride s, -inf padding p.
hipError_t maxpool2d(int batch, int H, int W, int C, int k, int s, int p, int Ho, int Wo,
                     const void* x, void* y, int et, hipStream_t stream);

// Global average pooling, NHWC [B,H,W,C] -> same type [B,C] (same scale), `et` = ElemType.
hipError_t avgpool_global(int batch, int HW, int C, const void* x, void* y, int et,
                          hipStream_t stream);

// Fused classifier head: optional global average pool over HW, dense layer with fp32 weights
// w[N][C] + bias[N], then row softmax. x: bf16, e4m3 (scale in_scale) or fp32 [B,HW,C] by `et`
// (ElemType); out: fp32 [B,N]. One workgroup per image.
hipError_t head_pool_dense_softmax(int batch, int HW, int C, int N, const void* x, int et,
                                   float in_scale, const float* w, const float* bias, float* out,
                                   hipStream_t stream);

// Whole-network CIFAR-10 ResNet-20 (csrc/kernels/resnet20_fused.hip): x fp32 [B,32,32,3] ->
// The step graph's outputs written by a whole-network forward itself (all null: none): each
// softmax value also as a Java Float.toString slot (kFloatTextSlot bytes, as format_floats_java)
// in text, and, by workgroup 0 before anything else, the batch's parse verdicts handed over:
// status_out[i] = status[i], status[i] = 0 for i < *nrec (status: the parse's device array;
// text and status_out: host-mapped). The replica's step is then parse -> forward, two nodes.
// The inputs of a batch whose images the GPU ingest already parsed into fetch arenas, passed BY
// VALUE in the forward's kernel arguments, so a batch step needs no metadata copy at all: image
// i is at base[code[i] >> 24] + (code[i] & 0xffffff) * (H * W * C) floats. base[0] == null:
// no table (the forward reads x or xs).
constexpr int kInputTableImages = 512, kInputTableBases = 16;
struct InputTable {
  const float* base[kInputTableBases];
  uint32_t code[kInputTableImages];
};

struct StepOut {
  void* text = nullptr;
  int* status = nullptr;
  int* status_out = nullptr;
  const int* nrec = nullptr;
};

// softmax fp32 [B,10], one workgroup per image with every activation in LDS. w/b: the 19 convs
// in network order (packed [Npad][Kpad] + folded-BN fp32 bias), fc_w fp32 [10][64].
// fp8: w are e4m3 codes with per-channel scales ws; s_in / s_out / s_res are the per-tensor
// activation scales of each conv's input / output / residual (s_in[0] quantises the input).
struct ResNet20Params {
  const void* w[19];  // bf16 or e4m3
  const float* b[19];
  const float* fc_w;
  const float* fc_b;
  int fp8;
  const float* ws[19];
  float s_in[19], s_out[19], s_res[19];
  // non-null: the image count is read from device memory at run time (images <= the `batch`
  // the launch is sized for) - a captured step graph replays one launch for every batch size
  const int* batch_dev;
  StepOut so;  // (prediction text + verdict hand-off in the epilogue)
  // non-null: image i's fp32 [32][32][3] input is at xs[i] (images the GPU ingest already parsed
  // into its fetch arenas; device memory) instead of x + i * 3072
  const float* const* xs;
};
hipError_t resnet20_fused_forward(const ResNet20Params& p, int batch, const float* x, float* out,
                                  hipStream_t stream, const InputTable* tab = nullptr);

// Whole-network MNIST LeNet-5 (csrc/kernels/lenet5_fused.hip): x fp32 [B,28,28,1] -> softmax
// fp32 [B,10], one image per 256-thread workgroup (grid = batch) with every activation in LDS. Weights are the serving
// plan's packed bf16 matrices: conv1 [16][32], conv2 [16][224], fc1 [128][416], fc2 [128][128]
// (fp32 biases of Npad entries), fc3 fp32 [10][88] + [10].
struct LeNet5Params {
  const void* w1;
  const float* b1;
  const void* w2;
  const float* b2;
  const void* w3;
  const float* b3;
  const void* w4;
  const float* b4;
  const float* w5;
  const float* b5;
  const int* batch_dev;  // as ResNet20Params::batch_dev
  StepOut so;            // as ResNet20Params::so
  const float* const* xs;  // as ResNet20Params::xs ([28][28][1] images)
};
hipError_t lenet5_fused_forward(const LeNet5Params& p, int batch, const float* x, float* out,
                                hipStream_t stream, const InputTable* tab = nullptr);

// Row softmax, fp32 [B, ld] -> fp32 [B, N] (first N columns of each row).
hipError_t softmax_rows(int batch, int N, int ld, const float* x, float* out, hipStream_t stream);

// fp32 -> bf16 cast with optional affine normalisation y = x*scale + shift (n elements).
// Inference BatchNorm (per-channel scale/shift; nullptr = identity) + optional residual + ReLU
// over NHWC bf16 (et = ET_BF16) or fp32 (ET_F32: the fp32 unfolded-BN plan), [batch,
// HW = Ho*Wo, C stored]. The residual is [batch, res_H, res_W, res_C], read at (ho*rs, wo*rs),
// zero for channels >= res_C. In-place (x == y) is allowed.
hipError_t bn_act(int batch, int HW, int Wo, int C, const void* x, const float* scale,
                  const float* shift, const void* res, int res_H, int res_W, int res_C, int rs,
                  int relu, void* y, hipStream_t stream, int et = 0);

hipError_t cast_f32_bf16(int64_t n, float scale, float shift, const float* x, void* y,
                         hipStream_t stream);


// GPU decoder for the InstObj JSON contract: parses every number of each record's instances
// array into the fp32 NHWC batch tensor and validates the rectangular [N][H][W][C] structure.
// Work is split into kJsonTileBytes tiles of record text (one workgroup each); record i owns the
// global tiles [tile0, tile0 + json_tile_count(off, len)), numbered consecutively over the batch.
// The kernel raises each record's status (host zeroes it): 0 ok, 1 number-count mismatch,
// 2 malformed number / element, 3 bad structure (ragged / wrong rank).
constexpr int kJsonTileBytes = 2048;
constexpr int kGroupTiles = 4;  // tiles per ingest counting workgroup (one per wave) / group sum
struct JsonRecord {
  int64_t off;      // byte offset of the instances array inside the staged byte buffer
  int32_t len;      // array length in bytes
  int32_t slot;     // first image slot of this record inside the batch
  int32_t images;   // images in this record (from the host '[' count)
  int32_t status;   // raised by the kernel
  int32_t tile0;    // first global tile of this record
  // 1: the record's count block is already on the device at bytes + cnt_off (the GPU ingest pass
  // counted it and left it in the fetch buffer's device mirror): its nt tile token counts, then
  // one sum per group of kGroupTiles tiles. The parse skips its counting pass over this record.
  int32_t has_cnt;
  int64_t cnt_off;
  // ingest_crc_count only: groups in the records before this one, so the record's count block
  // starts at counts + tile0 + grp0
  int64_t grp0;
};
static_assert(sizeof(JsonRecord) == 48, "JsonRecord layout (host <-> device tables)");
// tiles of the record text [off, off + len): counted from its 16-byte-aligned start
inline int json_tile_count(int64_t off, int32_t len) {
  if (len <= 0) return 0;
  const int64_t abeg = off & ~(int64_t)15;
  return (int)((off + len - abeg + kJsonTileBytes - 1) / kJsonTileBytes);
}
// Input preprocessing applied at the parse's store: the model input for the record value x at
// channel c is fmaf(x, a[c], b[c]) (binary32, one rounding; a = scale / std, b = -mean / std,
// gale/models/preprocess.py). The coefficients travel by value in the kernel arguments (C <= 4
// per-channel; a scalar is broadcast into all four). nchw: the record's instances array is
// nested [N][C][H][W]; the stored tensor stays NHWC.
struct InputPrep {
  int nchw = 0;
  float a[4] = {1.f, 1.f, 1.f, 1.f};
  float b[4] = {0.f, 0.f, 0.f, 0.f};
  bool identity() const {
    for (int i = 0; i < 4; ++i)
      if (a[i] != 1.f || b[i] != 0.f) return false;
    return !nchw;
  }
};
// tile_rec[t]: index of the record owning global tile t. tile_counts: device scratch of
// >= ntiles ints.
// count_pass = false: every record has_cnt (the counting kernel is not launched at all).
// d_ntiles non-null: the kernels read the tile count from device memory (ntiles = the most the
// launch is sized for; waves past the device count exit) - the captured step graph's form.
// status non-null: the verdicts are raised in status[record] (device memory) instead of
// recs[record].status, and recs / tile_rec / d_ntiles are only read - they may then be
// host-mapped pinned memory (the step graph reads the batch's metadata where the host wrote it,
// with no copy node).
// images < 0 (with has_cnt): the record's image count is taken from the group sums of its count
// block on the device (the GPU ingest parses a fetch right behind its counting launch, before
// the host has read the counts); a total that is not whole images expects nothing (status 1).
// tile_bad non-null (count_pass false): each tile's verdict (0 / 1 / 2 / 3) goes to
// tile_bad[tile] by a plain store instead of raising a record status, so it may be host-mapped
// memory; a record's verdict is the max over its tiles.
// prep null or identity: the values are stored as parsed (the kernel instantiation without the
// preprocessing code). Otherwise each value is stored as fmaf(x, a[c], b[c]), and with nchw the
// structure is checked against [N][C][H][W] nesting and the store transposed to NHWC; needs
// H * W * C < 2^20, and C <= 4 unless a / b are uniform.
hipError_t json_parse_instances(int nrec, int ntiles, JsonRecord* recs, const int* tile_rec,
                                const uint8_t* bytes, int H, int W, int C, int* tile_counts,
                                float* out, hipStream_t stream, bool count_pass = true,
                                const int* d_ntiles = nullptr, int* status = nullptr,
                                int* tile_bad = nullptr, const InputPrep* prep = nullptr);

// GPU decoder of base64 uint8 image records (input format "b64", csrc/codec/json_codec.h): every
// image's string - L = 4 * ceil(H*W*C / 3) characters of standard base64, the last
// (3 - H*W*C % 3) % 3 of them '=' - becomes H*W*C floats (float)byte in the fp32 NHWC batch
// tensor. A lane decodes 16 characters into 12 values, a 256-thread workgroup 4096 characters;
// the grid is (chunks per image) x (images).
constexpr int kB64ChunkChars = 4096;
struct B64Image {
  int64_t off;   // byte offset of the string's first character inside the staged byte buffer
  int32_t slot;  // the image's slot in the batch
  int32_t rec;   // index of the owning record in `status`
};
static_assert(sizeof(B64Image) == 16, "B64Image layout (host <-> device tables)");
// status[rec] is set to 2 (host zeroes it) when a character outside the alphabet stands in the
// data part of one of the record's strings or a non-'=' in its padding; the image is written
// anyway (within its own slot). Any 16-byte phase of `off` is fine: the kernel loads the aligned
// 16-byte words around a lane's window, so it reads at most 15 bytes before a string and fewer
// than 16 bytes past it.
// d_images non-null: the image count is read from device memory (images = the most the launch
// is sized for; workgroups past the device count exit) - the captured step graph's form; imgs
// and d_images may be host-mapped pinned memory.
// prep null or identity: the instantiation without the preprocessing code. Otherwise the value v
// of channel c is stored as fmaf(v, a[c], b[c]), and with nchw the string's bytes are ordered
// [C][H][W] and the store transposes to NHWC; C <= 4 unless a / b are uniform.
hipError_t b64_decode_instances(int images, const B64Image* imgs, const uint8_t* bytes, int H,
                                int W, int C, float* out, int* status, hipStream_t stream,
                                const int* d_images = nullptr, const InputPrep* prep = nullptr);

// GPU decoder of base64 YUV 4:2:0 video-frame records (input pixel formats "i420" / "nv12",
// b64_yuv.hip): every frame's string - L = 4 B / 3 characters of standard base64, B = HS*WS*3/2,
// never a '=' - becomes the HS*WS*3 floats of its RGB image in the fp32 NHWC batch tensor, by the
// integer conversion that csrc/codec/yuv.h defines (format: YUV_I420 or YUV_NV12; coeffs: its
// table, by value in the kernel arguments like prep): the bits b64_decode_instances gives for
// the converted image sent as an RGB record with the same prep. imgs, status (2 for a character
// outside the alphabet anywhere in one of the record's strings; the frame is written anyway,
// within its own slot), d_images and the read bounds around a string are b64_decode_instances'.
// A workgroup decodes `pairs` whole row pairs of one frame into LDS and converts them; pairs = 0:
// b64_yuv_pairs(HS, WS), about 4096 pixels a workgroup. 16-byte stores when the image's base is
// 16-byte aligned, one float per lane otherwise; both contiguous over a wave.
// hipErrorInvalidValue, before any launch: odd or non-positive HS / WS, C != 3, a null pointer,
// an unknown format, an nchw prep, more than 65535 images, a frame of more than 2^30 floats,
// pairs outside 0 .. HS / 2, or a block of b64_yuv_lds_bytes(WS, pairs) > kYuvLdsBudget (a
// single row pair of WS > 21 836). images == 0 launches nothing.
constexpr size_t kYuvLdsBudget = 64 * 1024;
int b64_yuv_pairs(int HS, int WS);
size_t b64_yuv_lds_bytes(int WS, int pairs);
hipError_t b64_yuv_instances(int images, const B64Image* imgs, const uint8_t* bytes, int HS,
                             int WS, int C, float* out, int* status, hipStream_t stream,
                             const int* d_images, const InputPrep* prep, int format,
                             const YuvCoeffs& coeffs, int pairs = 0);

// GPU decoder of base64 packed-pixel records (input pixel formats "bgr24" / "rgba" / "bgra" /
// "gray", b64_packed.hip): every image's string - L = 4 ceil(B / 3) characters of standard
// base64, B = HS*WS*P bytes (csrc/codec/pixfmt.h), padded like an RGB string - becomes the
// HS*WS*3 floats of its RGB image in the fp32 NHWC batch tensor: the bits b64_decode_instances
// gives for the unpacked image sent as an RGB record with the same prep (whose coefficients are
// indexed by model channel, R, G, B). Alpha is dropped. imgs, status (2 for a character outside
// the alphabet in the data part or a non-'=' in the padding of one of the record's strings; the
// image is written anyway, within its own slot), d_images, the grid and the read bounds around a
// string are b64_decode_instances'. 16-byte stores when the image's base is 16-byte aligned, one
// float per lane otherwise; both contiguous over a wave.
// hipErrorInvalidValue, before any launch: non-positive HS / WS, C != 3, a null pointer, an
// unknown format, an nchw prep, more than 65535 images, an image of more than 2^30 floats.
// images == 0 launches nothing.
hipError_t b64_packed_instances(int images, const B64Image* imgs, const uint8_t* bytes, int HS,
                                int WS, int C, float* out, int* status, hipStream_t stream,
                                const int* d_images, const InputPrep* prep, int format);

// GPU decoder of base64 typed tensor records (input dtypes "u16" / "f16" / "bf16" / "f32",
// b64_typed.hip): every image's string - L = 4 ceil(B / 3) characters of standard base64,
// B = HS*WS*C*E bytes of little-endian elements (csrc/codec/elemtype.h), padded like an RGB
// string - becomes the HS*WS*C floats fmaf(float32(x), a[c], b[c]) of the fp32 NHWC batch tensor.
// float32(x) is exact (f16 subnormals too, whatever the denormal mode); without a prep the
// element's float32 bits are stored untouched (f32: -0 and subnormals as sent). imgs, status,
// d_images, the grid, the read bounds around a string, prep and its nchw are
// b64_decode_instances'. status[rec] is also set to 2 when an f16 / bf16 / f32 element of one of
// the record's strings has an all-ones exponent (Inf, NaN), judged on the element as sent; the
// image is written anyway, within its own slot. The 16-bit types store 16-byte vectors when the
// image's base is 16-byte aligned and one float per lane otherwise; f32 stores 12 bytes per lane;
// all contiguous over a wave.
// hipErrorInvalidValue, before any launch: non-positive HS / WS / C, a null pointer, a type
// other than ELEM_U16 / ELEM_F16 / ELEM_BF16 / ELEM_F32 (u8 strings are b64_decode_instances'),
// more than 65535 images, an image of more than 2^30 floats, C > 4 with non-uniform
// coefficients. images == 0 launches nothing.
hipError_t b64_typed_instances(int images, const B64Image* imgs, const uint8_t* bytes, int HS,
                               int WS, int C, float* out, int* status, hipStream_t stream,
                               const int* d_images, const InputPrep* prep, int type);

// ---- input resize (resize_crop.hip) ---------------------------------------------------------
// Bilinear resize (half-pixel centres, no antialiasing) + centre crop of fp32 NHWC images:
// src [n][HS][WS][C] -> dst [n][H][W][C]. The six tables (device memory; per output row y0 / y1
// / wy of H entries, per output column x0 / x1 / wx of W entries) are built on the host by
// codec::build_resize_tables (csrc/codec/resize.h, where the numerics are defined) and uploaded
// once (pack / bind, csrc/runtime/resize_plan.h: one device image, the plan's pointers into
// it); the plan travels by value in the kernel arguments. Bit-identical to
// codec::resize_crop_host. src and dst must not overlap.
struct ResizePlan {
  int HS = 0, WS = 0, H = 0, W = 0, C = 0;
  const int32_t* y0 = nullptr;
  const int32_t* y1 = nullptr;
  const float* wy = nullptr;
  const int32_t* x0 = nullptr;
  const int32_t* x1 = nullptr;
  const float* wx = nullptr;
};
// hipErrorInvalidValue, before any launch, for a null pointer, HS / WS / H / W outside 1..4096,
// C < 1, an image of 2^31 floats or more, images < 0 or images > 65535. images == 0 launches
// nothing. 16-byte stores when H * W * C is a multiple of 4 floats and dst is 16-byte aligned,
// one store per float otherwise.
hipError_t resize_crop(int images, const ResizePlan& plan, const float* src, float* dst,
                       hipStream_t stream);
// images = min(*d_images, max_images) read on the device (max_images: the launch size);
// workgroups of later images exit before touching memory: the step graph's form
hipError_t resize_crop_dev(int max_images, const int* d_images, const ResizePlan& plan,
                           const float* src, float* dst, hipStream_t stream);

// ---- antialiased input resize (resize_crop_aa.hip) -------------------------------------------
// The support-scaled triangle filter (PIL / torch antialias=True) + centre crop of fp32 NHWC
// images, src [n][HS][WS][C] -> dst [n][H][W][C], in the tap form that csrc/codec/resize.h
// defines: per output row a run of source rows ys[y] .. ys[y] + yn[y] - 1 with weights
// wy[y * ty + k], per output column xs / xn / wx[x * tx + k] (device memory; built by
// codec::build_resize_aa_tables, the weights laid out with a fixed stride per axis by
// codec::resize_aa_strided). Columns first, then rows, in one launch with no intermediate in
// global memory: a workgroup stages the column sums of the source rows that a band of `band`
// output rows touches in LDS. band (codec::resize_aa_choose_band) and band_rows
// (codec::resize_aa_band_rows: the most source rows a band touches) are computed on the host
// from the tables (with the device image, pack in csrc/runtime/resize_plan.h); the launcher
// sizes the LDS from them. Bit-identical to
// codec::resize_crop_aa_host. src and dst must not overlap.
struct ResizeAaPlan {
  int HS = 0, WS = 0, HR = 0, WR = 0, H = 0, W = 0, C = 0;
  int ty = 0, tx = 0;            // the largest tap count of a row / column = the weights' stride
  int band = 0, band_rows = 0;   // output rows per workgroup; source rows its LDS tile holds
  const int32_t* ys = nullptr;   // [H]
  const int32_t* yn = nullptr;   // [H]
  const float* wy = nullptr;     // [H][ty]
  const int32_t* xs = nullptr;   // [W]
  const int32_t* xn = nullptr;   // [W]
  const float* wx = nullptr;     // [W][tx]
};
// hipErrorInvalidValue, before any launch, for what resize_crop refuses (HR / WR included) and
// for HR < H, WR < W, HS > 8 HR or WS > 8 WR (the antialias limit), ty / tx outside 1..17, band
// outside 1..8, band_rows < 1 or band_rows + tx > 64 (the LDS tile). images == 0 launches
// nothing. 16-byte stores when W * C is a multiple of 4 floats and dst is 16-byte aligned, one
// store per float otherwise.
hipError_t resize_crop_aa(int images, const ResizeAaPlan& plan, const float* src, float* dst,
                          hipStream_t stream);
// images = min(*d_images, max_images) read on the device; workgroups of later images exit as a
// whole before any barrier or memory access: the step graph's form
hipError_t resize_crop_aa_dev(int max_images, const int* d_images, const ResizeAaPlan& plan,
                              const float* src, float* dst, hipStream_t stream);

// Raw (zero initial state, no final inversion) CRC32C of byte windows [end - len, end) of a
// device buffer, one wave per window (len <= kCrcChunkBytes): each lane folds 64 bytes with
// slicing-by-4 tables in LDS, shifts its register over the bytes after its piece (one GF(2)
// multiply by a per-lane constant) and the wave XOR-reduces. The host joins the windows of a
// Kafka record batch with crc = shift(crc, 4096) ^ window_crc and converts to the standard CRC
// (kafka::CrcShift). tables: kafka::crc32c_device_tables() (1088 words) in device memory.
constexpr int kCrcChunkBytes = 4096;
struct CrcChunk {
  int64_t end;  // one past the window's last byte (offset into `bytes`)
  int32_t len;  // window length, 1..kCrcChunkBytes
  int32_t pad_;
};
hipError_t crc32c_chunks(const uint8_t* bytes, const CrcChunk* chunks, int n,
                         const uint32_t* tables, uint32_t* out, hipStream_t stream);

// The GPU ingest pass of one fetch buffer in ONE launch: workgroups [0, crc blocks) fold the CRC
// windows (crc32c_chunks), the rest count the records' number tokens so the host learns each
// record's image count without reading its text: one workgroup per tile group, groups[g] =
// (record, record-relative first tile), kGroupTiles tiles each (a record's last group may be
// shorter). Record i's count block at counts + tile0 + grp0 gets its tile counts and group sums
// (see JsonRecord::has_cnt); gsum[g] = the tokens of group g (the host adds a record's groups);
// invalid bytes raise recs[i].status to 2, or, with gbad non-null, set gbad[g] = 2 (else 0) by a
// plain store and leave recs untouched - chunks, recs, groups, crc_out, gsum and gbad may then
// be host-mapped pinned memory (read and written over the link, no copies); bytes, tables and
// counts are device memory.
// packed non-null: the fetch body is the nibble-packed stream `packed` with its group table
// `tab` (both device memory; csrc/codec/text_pack.h) instead of text at `bytes`: the CRC
// windows and counting waves expand it in registers and the counting waves store every record's
// text (its 16-byte-aligned extent) into text_out - text_unpack folded into this launch.
hipError_t ingest_crc_count(const uint8_t* bytes, const CrcChunk* chunks, int nchunks,
                            const uint32_t* tables, uint32_t* crc_out, int nrec, int ngroups,
                            JsonRecord* recs, const int2* groups, int* counts, int* gsum,
                            int* gbad, hipStream_t stream, const uint8_t* packed = nullptr,
                            const uint32_t* tab = nullptr, uint8_t* text_out = nullptr);

// The GPU ingest pass of one fetch buffer of base64 image records (input format "b64") in ONE
// launch (b64_ingest.hip): workgroups [0, crc blocks) fold the CRC windows (crc32c_chunks), and
// workgroup crc blocks + g decodes chunk g % cpi of image g / cpi, cpi = ceil(L /
// kB64ChunkChars), from the device mirror `bytes` into arena + imgs[i].slot * H*W*C exactly as
// b64_decode_instances does (same read bounds, verdict rules, store paths and prep forms).
// wg_bad[g] = 2 when a lane of that workgroup saw a bad character or bad padding, else 0: every
// decode workgroup stores its word (plain store; the host never zeroes the array) and a
// record's verdict is the max over its images' words - B64Image::rec is not read. chunks, imgs,
// crc_out and wg_bad may be host-mapped pinned memory; bytes, tables and arena are device
// memory. nchunks == 0 or images == 0 leaves that half out; both zero launches nothing.
// hipErrorInvalidValue: more workgroups than a 1-D grid holds, or prep with C > 4 and
// non-uniform coefficients.
hipError_t ingest_crc_b64(const uint8_t* bytes, const CrcChunk* chunks, int nchunks,
                          const uint32_t* tables, uint32_t* crc_out, int images,
                          const B64Image* imgs, int H, int W, int C, float* arena, int* wg_bad,
                          hipStream_t stream, const InputPrep* prep = nullptr);

// Expands a nibble-packed span (csrc/codec/text_pack.h: 64-byte blocks, per-2-KiB-group
// {base offset, packed-block mask} pairs in tab) into out[0, n). out must be 16-byte aligned,
// packed 8-byte aligned. packed and tab may be host-mapped pinned memory (the GPU ingest reads the
// small group table from the source's pinned chunk; the packed stream itself is DMA'd first:
// kernel loads over the link expand it ~15x slower than the SDMA copy plus a device pass).
hipError_t text_unpack(const uint8_t* packed, const uint32_t* tab, int64_t n, uint8_t* out,
                       hipStream_t stream);

// ---- prediction text (format.hip) -----------------------------------------------------------
// n binary32 values -> Java Float.toString text (JDK 19+ shortest-digit rules, the same text as
// codec::format_float_java), one 16-byte slot per value: characters from byte 0, length in
// byte 15 (at most 14 characters).
constexpr int kFloatTextSlot = 16;
hipError_t format_floats_java(int n, const float* x, void* out16, hipStream_t stream);
// n = (*d_count) * per values (n <= max_n, the launch size): the step graph's form
hipError_t format_floats_java_dev(int max_n, const int* d_count, int per, const float* x,
                                  void* out16, hipStream_t stream);
// The step graph's last node: format_floats_java_dev, and the batch's parse verdicts handed
// back - status_out[i] = status[i], status[i] = 0 for i < *d_nrec (status: the parse's device
// array, cleared for the slot's next batch; status_out: host-mapped), so the step needs no
// status copy node. max_n must cover max_nrec values (the launch's threads do both).
hipError_t format_floats_java_step(int max_n, const int* d_count, int per, const float* x,
                                   void* out16, const int* d_nrec, int* status, int* status_out,
                                   hipStream_t stream);

// ---- top-k prediction output (topk.hip) -----------------------------------------------------
// Of each row of x (fp32 [rows][classes], device memory) the k best classes in score order
// (codec/json_codec.h "Score order": descending by the order-preserving key of the bits, ties to
// the lower class): entry (r, j) goes to slot r * k + j of text16 (kFloatTextSlot bytes, the
// value's text as format_floats_java writes it) and of idx (the 0-based class). text16 and idx
// may be host-mapped pinned memory. hipErrorInvalidValue, before any launch, for k < 1, k > 64,
// k > classes or classes > 4096. One wave per row, so the launch has 64 threads per row.
hipError_t topk_java(int rows, int classes, int k, const float* x, void* text16, int32_t* idx,
                     hipStream_t stream);
// rows = min(*d_rows, max_rows) read on the device (max_rows: the launch size); waves of later
// rows exit before touching memory: the step graph's form
hipError_t topk_java_dev(int max_rows, const int* d_rows, int classes, int k, const float* x,
                         void* text16, int32_t* idx, hipStream_t stream);
// topk_java_dev with format_floats_java_step's verdict hand-off by the launch's first threads
// (status_out[i] = status[i], status[i] = 0 for i < *d_nrec); *d_nrec <= 64 * max_rows
hipError_t topk_java_step(int max_rows, const int* d_rows, int classes, int k, const float* x,
                          void* text16, int32_t* idx, const int* d_nrec, int* status,
                          int* status_out, hipStream_t stream);

}  // namespace gale
