// The one decode launch of a b64 batch, chosen by what the strings carry. Host only: it keeps
// PixelSource (and the host codec's API behind it) out of the kernels' translation units.
#pragma once
#include "../codec/pixel_source.h"
#include "gale/kernels.h"

namespace gale {

// The decode launch of b64 strings that carry `src` (csrc/codec/pixel_source.h): exactly one of
// the four launchers of gale/kernels.h, with these arguments. *which (optional): that
// launcher's name.
inline hipError_t b64_source_instances(int images, const B64Image* imgs, const uint8_t* bytes,
                                       int HS, int WS, int C, float* out, int* status,
                                       hipStream_t stream, const int* d_images,
                                       const InputPrep* prep, const PixelSource& src,
                                       const char** which = nullptr) {
  const PixelSource::Kind k = src.kind();
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
