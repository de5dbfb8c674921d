// What the b64 strings of a topology carry (engine keys pixel_format and input_dtype):
// interleaved RGB bytes, a YUV 4:2:0 frame (yuv.h), packed pixels (pixfmt.h) or a typed tensor
// (elemtype.h: the rgb layout with 16-bit or float elements). PixelSource is the one holder of
// {yuv format, YuvCoeffs, packed format, element type} and of the rules about them: the configuration names,
// the bytes of a string, what a topology may combine them with, what the ingest sees and which
// host parser and which GPU launcher (csrc/runtime/b64_source.h) decode them. The
// engine configuration and both replicas hold one; a new pixel format is added here.
// No HIP in this header: the sanitizer programs of the host codec include it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <stdexcept>
#include <string>

#include "elemtype.h"
#include "json_codec.h"
#include "pixfmt.h"
#include "yuv.h"

namespace gale {

class PixelSource {
 public:
  enum Kind { RGB, YUV, PACKED, TYPED };
  // the dimensions of an image whose string is as long as this source's (ingest_dims)
  struct Dims {
    int H, W, C;
  };

  PixelSource() = default;  // rgb

  // From the configuration names: pixel_format rgb | i420 | nv12 | bgr24 | rgba | bgra | gray;
  // yuv_matrix bt601 | bt709 and yuv_range limited | full, null where the configuration does not
  // name one (bt601, limited; naming one with a packed format is refused).
  static PixelSource from_names(const std::string& pixel_format, const std::string* yuv_matrix,
                                const std::string* yuv_range) {
    PixelSource s;
    s.packed_format_ = packed_format_of(pixel_format.c_str());
    if (pixel_format == "i420" || pixel_format == "nv12")
      s.yuv_format_ = pixel_format == "i420" ? (int)YUV_I420 : (int)YUV_NV12;
    else if (pixel_format != "rgb" && !s.packed_format_)
      throw std::invalid_argument("pixel_format: rgb, i420, nv12, bgr24, rgba, bgra or gray");
    if (s.packed_format_ && (yuv_matrix || yuv_range))
      throw std::invalid_argument("yuv_matrix / yuv_range need pixel_format i420 or nv12");
    const std::string ym = yuv_matrix ? *yuv_matrix : "bt601";
    const std::string yr = yuv_range ? *yuv_range : "limited";
    if (!yuv_coeffs(ym == "bt601" ? 0 : ym == "bt709" ? 1 : -1,
                    yr == "limited" ? 0 : yr == "full" ? 1 : -1, &s.yuv_))
      throw std::invalid_argument("yuv_matrix: bt601 or bt709; yuv_range: limited or full");
    return s;
  }

  // The same source with the element type of the configuration name input_dtype: u8 | u16 | f16
  // | bf16 | f32. Anything but u8 makes an rgb source a typed one and is refused on any other.
  PixelSource with_elem(const std::string& input_dtype) const {
    PixelSource s = *this;
    s.elem_ = elem_type_of(input_dtype.c_str());
    if (s.elem_ < 0) throw std::invalid_argument("input_dtype: u8, u16, f16, bf16 or f32");
    if (s.elem_ != ELEM_U8 && (packed_format_ || yuv_format_))
      throw std::invalid_argument("input_dtype " + input_dtype + " needs pixel_format rgb");
    return s;
  }

  Kind kind() const {
    return packed_format_ ? PACKED : yuv_format_ ? YUV : elem_ != ELEM_U8 ? TYPED : RGB;
  }
  int yuv_format() const { return yuv_format_; }        // YuvFormat (YUV_NONE unless YUV)
  const YuvCoeffs& yuv() const { return yuv_; }
  int packed_format() const { return packed_format_; }  // PackedFormat (PACKED_NONE unless PACKED)
  int elem() const { return elem_; }                    // InputElem (ELEM_U8 unless TYPED)

  // Bytes one string carries for record-side images of HS x WS (x C for rgb, x C x E typed).
  int64_t bytes(int HS, int WS, int C) const {
    return kind() == PACKED ? packed_bytes(HS, WS, packed_format_)
           : kind() == YUV  ? yuv420_bytes(HS, WS)
                            : (int64_t)HS * WS * C * elem_bytes(elem_);
  }

  // What a topology must look like to carry this source: model channels C, the prep's nchw,
  // record-side HS x WS, input_format b64. std::invalid_argument otherwise; rgb goes with all,
  // a typed tensor with everything rgb b64 records go with.
  // uniform_prep: whether the prep's four coefficient pairs are equal (a typed tensor may have
  // C > 4, which the decoders serve with uniform coefficients only: b64::prep_fits; the Python
  // configuration refuses the same by --input-mean / --input-std).
  void check(int C, bool nchw, int HS, int WS, bool input_b64, bool uniform_prep = true) const {
    if (kind() == RGB) return;
    if (kind() == TYPED) {  // (any C, either layout, any size: the rgb rules)
      if (!input_b64)
        throw std::invalid_argument(std::string("input_dtype ") + elem_type_name(elem_) +
                                    " needs input_format b64");
      if (C > 4 && !uniform_prep)
        throw std::invalid_argument(std::string("input_dtype ") + elem_type_name(elem_) +
                                    ": per-channel input_a / input_b need C <= 4");
      return;
    }
    const std::string what =
        kind() == YUV ? "pixel_format i420 / nv12" : "pixel_format bgr24 / rgba / bgra / gray";
    if (!input_b64) throw std::invalid_argument(what + " needs input_format b64");
    if (nchw) throw std::invalid_argument(what + ": no nchw layout");
    if (C != 3) throw std::invalid_argument(what + " needs a 3-channel model");
    if (kind() == YUV && ((HS | WS) & 1))
      throw std::invalid_argument(what + " needs even record-side H, W");
  }

  // The ingest's b64 decode and its image arena hold RGB strings' images: for every other
  // source a GPU ingest runs CRC-only (ingest_parse off) and the step decodes from the mirror.
  bool wants_ingest_decode() const { return kind() == RGB; }

  // What a string looks like to the ingest's plan (plan_b64_ingest), which checks it against
  // its record: a YUV frame's string is that of an (HS / 2) x WS x 3 byte image, a packed-pixel
  // string that of an HS x WS x P one, a typed tensor's string that of an HS x (WS E) x C one -
  // the element size widens a row, not the channel count, because the ingest's launcher applies
  // the C > 4 coefficient rule to the C it is given even when it decodes nothing.
  // (There is no arena for any of them, so nothing is decoded.)
  Dims ingest_dims(int HS, int WS, int C) const {
    return kind() == PACKED ? Dims{HS, WS, packed_bpp(packed_format_)}
           : kind() == YUV  ? Dims{HS / 2, WS, 3}
                            : Dims{HS, WS * elem_bytes(elem_), C};
  }

  // The host decode of one b64 record into out[N][HS][WS][C]: the source's public parser
  // (json_codec.h), with its status, image count and floats.
  int parse_host(const uint8_t* p, size_t n, int HS, int WS, int C, float* out, int max_images,
                 int* images) const {
    if (kind() == TYPED)
      return codec::parse_instances_typed_host(p, n, HS, WS, C, elem_, out, max_images, images);
    return kind() == PACKED
               ? codec::parse_instances_packed_host(p, n, HS, WS, packed_format_, out,
                                                    max_images, images)
           : kind() == YUV
               ? codec::parse_instances_yuv_host(p, n, HS, WS, yuv_format_, yuv_, out,
                                                 max_images, images)
               : codec::parse_instances_b64_host(p, n, HS, WS, C, out, max_images, images);
  }

 private:
  int yuv_format_ = YUV_NONE;
  YuvCoeffs yuv_;
  int packed_format_ = PACKED_NONE;
  int elem_ = ELEM_U8;
};

}  // namespace gale
