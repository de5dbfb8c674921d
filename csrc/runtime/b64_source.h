// The one decode launch of a b64 batch, chosen by what the strings carry. Host only: it keeps
// PixelSource (and the host codec's API behind it) out of the kernels' translation units.
#pragma once
#include "../codec/pixel_source.h"
#include "gale/kernels.h"

namespace gale {

// The decode launch of b64 strings that carry `src` (csrc/codec/pixel_source.h): exactly one of
// the b64 launchers of gale/kernels.h, or raw_instances for a raw source (a packed 4:2:2 frame:
// b64_yuv422_instances or raw_yuv422_instances; a planar 4:2:2 / 4:4:4 frame: b64_yuvp_instances
// or raw_yuvp_instances; a raw 10-bit 4:2:0 frame: raw_yuv420p10_instances; a raw Bayer mosaic:
// raw_bayer_instances, or raw_bayer_malvar_instances with bayer_demosaic malvar, or
// raw_bayer_hamilton_instances with bayer_demosaic hamilton; a raw 10/12/16-bit
// Bayer mosaic: raw_bayer_hi_instances with either demosaic; a b64 4:2:0 frame with
// linear chroma: b64_yuv_linear_instances), with these arguments. *which (optional): that
// launcher's name.
inline hipError_t b64_source_instances(int images, const B64Image* imgs, const uint8_t* bytes,
                                       int HS, int WS, int C, float* out, int* status,
                                       hipStream_t stream, const int* d_images,
                                       const InputPrep* prep, const PixelSource& src,
                                       const char** which = nullptr) {
  const PixelSource::Kind k = src.kind();
  if (src.yuv422()) {
    if (which) *which = src.raw() ? "raw_yuv422_instances" : "b64_yuv422_instances";
    return (src.raw() ? raw_yuv422_instances : b64_yuv422_instances)(
        images, imgs, bytes, HS, WS, C, out, status, stream, d_images, prep, src.yuv_format(),
        src.yuv());
  }
  if (src.planar()) {
    if (which) *which = src.raw() ? "raw_yuvp_instances" : "b64_yuvp_instances";
    return (src.raw() ? raw_yuvp_instances : b64_yuvp_instances)(
        images, imgs, bytes, HS, WS, C, out, status, stream, d_images, prep, src.yuv_format(),
        src.yuv());
  }
  if (src.hi420()) {
    if (which) *which = "raw_yuv420p10_instances";
    if (!src.raw()) return hipErrorInvalidValue;  // (PixelSource::check refuses it)
    return raw_yuv420p10_instances(images, imgs, bytes, HS, WS, C, out, status, stream, d_images,
                                   prep, src.yuv_format(), src.yuv());
  }
  if (src.bayer_hi()) {  // (a raw 10/12/16-bit Bayer mosaic, words or MIPI groups: bayer_hi.hip)
    if (which) *which = "raw_bayer_hi_instances";
    if (!src.raw()) return hipErrorInvalidValue;  // (PixelSource::check refuses it)
    return raw_bayer_hi_instances(images, imgs, bytes, HS, WS, C, out, status, stream, d_images,
                                  prep, src.bayer_order(), src.bayer_bits(), src.bayer_packing(),
                                  src.bayer_malvar());
  }
  if (k == PixelSource::BAYER && src.bayer_hamilton()) {  // (edge-directed: bayer_hamilton.hip)
    if (which) *which = "raw_bayer_hamilton_instances";
    if (!src.raw()) return hipErrorInvalidValue;  // (PixelSource::check refuses it)
    return raw_bayer_hamilton_instances(images, imgs, bytes, HS, WS, C, out, status, stream,
                                        d_images, prep, src.bayer_order());
  }
  if (k == PixelSource::BAYER) {  // (a raw 8-bit Bayer mosaic: bayer.hip / bayer_malvar.hip)
    if (which) *which = src.bayer_malvar() ? "raw_bayer_malvar_instances" : "raw_bayer_instances";
    if (!src.raw()) return hipErrorInvalidValue;  // (PixelSource::check refuses it)
    return (src.bayer_malvar() ? raw_bayer_malvar_instances : raw_bayer_instances)(
        images, imgs, bytes, HS, WS, C, out, status, stream, d_images, prep, src.bayer_order());
  }
  if (src.raw()) {
    if (which) *which = "raw_instances";
    if (k == PixelSource::YUV) return hipErrorInvalidValue;  // (PixelSource::check refuses it)
    return raw_instances(images, imgs, bytes, HS, WS, C, out, status, stream, d_images, prep,
                         src.elem(), src.packed_format());
  }
  if (src.chroma_linear()) {  // (b64 i420 / nv12: PixelSource::check refuses anything else)
    if (which) *which = "b64_yuv_linear_instances";
    return b64_yuv_linear_instances(images, imgs, bytes, HS, WS, C, out, status, stream, d_images,
                                    prep, src.yuv_format(), src.yuv());
  }
  if (which)
    *which = k == PixelSource::PACKED  ? "b64_packed_instances"
             : k == PixelSource::YUV   ? "b64_yuv_instances"
             : k == PixelSource::TYPED ? "b64_typed_instances"
                                       : "b64_decode_instances";
  if (k == PixelSource::TYPED)
    return b64_typed_instances(images, imgs, bytes, HS, WS, C, out, status, stream, d_images,
                               prep, src.elem());
  return k == PixelSource::PACKED
             ? b64_packed_instances(images, imgs, bytes, HS, WS, C, out, status, stream, d_images,
                                    prep, src.packed_format())
         : k == PixelSource::YUV
             ? b64_yuv_instances(images, imgs, bytes, HS, WS, C, out, status, stream, d_images,
                                 prep, src.yuv_format(), src.yuv())
             : b64_decode_instances(images, imgs, bytes, HS, WS, C, out, status, stream, d_images,
                                    prep);
}

}  // namespace gale
