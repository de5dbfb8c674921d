// What the b64 strings of a topology carry (engine keys pixel_format and input_dtype):
// interleaved RGB bytes, a YUV 4:2:0, packed 4:2:2, planar 4:2:2 / 4:4:4 or 10-bit 4:2:0 (raw
// only) frame (yuv.h), packed pixels (pixfmt.h), an 8-bit Bayer mosaic (bayer.h, raw only), a
// 10/12/16-bit one in words or MIPI-packed groups (bayer_hi.h, raw only) or a typed tensor
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

#include "bayer.h"
#include "bayer_hi.h"
#include "elemtype.h"
#include "json_codec.h"
#include "pixfmt.h"
#include "yuv.h"

namespace gale {

class PixelSource {
 public:
  enum Kind { RGB, YUV, PACKED, TYPED, BAYER };
  // the dimensions of an image whose string is as long as this source's (ingest_dims)
  struct Dims {
    int H, W, C;
  };

  PixelSource() = default;  // rgb

  // From the configuration names: pixel_format rgb | i420 | nv12 | yuyv422 | uyvy422 | yuv422p |
  // yuv444p | p010le | yuv420p10le | bgr24 | rgba | bgra | gray | bayer_rggb8 | bayer_bggr8 |
  // bayer_grbg8 | bayer_gbrg8 | bayer_<order>{10le,12le,16le,10p,12p};
  // yuv_matrix bt601 | bt709 and yuv_range limited | full, null where the configuration does not
  // name one (bt601, limited; naming one with a packed format is refused).
  static PixelSource from_names(const std::string& pixel_format, const std::string* yuv_matrix,
                                const std::string* yuv_range) {
    PixelSource s;
    s.packed_format_ = packed_format_of(pixel_format.c_str());
    s.bayer_order_ = bayer_order_of(pixel_format.c_str());
    if (!s.bayer_order_) {  // (the deeper mosaics: kind BAYER with bits and packing of their own)
      const BayerHiFormat hi = bayer_hi_format_of(pixel_format.c_str());
      if (hi.order) s.bayer_order_ = hi.order, s.bayer_bits_ = hi.bits, s.bayer_packing_ = hi.packing;
    }
    if (pixel_format == "i420" || pixel_format == "nv12")
      s.yuv_format_ = pixel_format == "i420" ? (int)YUV_I420 : (int)YUV_NV12;
    else if (pixel_format == "yuyv422" || pixel_format == "uyvy422")
      s.yuv_format_ = pixel_format == "yuyv422" ? (int)YUV_YUYV422 : (int)YUV_UYVY422;
    else if (pixel_format == "yuv422p" || pixel_format == "yuv444p")
      s.yuv_format_ = pixel_format == "yuv422p" ? (int)YUV_YUV422P : (int)YUV_YUV444P;
    else if (pixel_format == "p010le" || pixel_format == "yuv420p10le")
      s.yuv_format_ = pixel_format == "p010le" ? (int)YUV_P010LE : (int)YUV_YUV420P10LE;
    else if (pixel_format != "rgb" && !s.packed_format_ && !s.bayer_order_)
      throw std::invalid_argument("pixel_format: rgb, i420, nv12, bgr24, rgba, bgra or gray");
    if ((s.packed_format_ || s.bayer_order_) && (yuv_matrix || yuv_range))
      throw std::invalid_argument("yuv_matrix / yuv_range need pixel_format i420 or nv12");
    const std::string ym = yuv_matrix ? *yuv_matrix : "bt601";
    const std::string yr = yuv_range ? *yuv_range : "limited";
    // (the 10-bit formats have tables of their own: the scale 2^18, yo = 64)
    if (!(yuv_is_420_hi(s.yuv_format_) ? yuv10_coeffs : yuv_coeffs)(
            ym == "bt601" ? 0 : ym == "bt709" ? 1 : -1,
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
    if (s.elem_ != ELEM_U8 && (packed_format_ || yuv_format_ || bayer_order_))
      throw std::invalid_argument("input_dtype " + input_dtype + " needs pixel_format rgb");
    return s;
  }

  // The same source with the chroma upsampling of the configuration name yuv_chroma: nearest |
  // linear (yuv.h: the triangle filter). check() refuses linear on anything but b64 i420 / nv12.
  PixelSource with_chroma(const std::string& yuv_chroma) const {
    PixelSource s = *this;
    if (yuv_chroma != "nearest" && yuv_chroma != "linear")
      throw std::invalid_argument("yuv_chroma: nearest or linear");
    s.chroma_linear_ = yuv_chroma == "linear";
    return s;
  }
  bool chroma_linear() const { return chroma_linear_; }

  // The same source with the demosaic of the configuration name bayer_demosaic: bilinear | malvar
  // (bayer.h: the 5 x 5 gradient-corrected filter) | hamilton (bayer.h: the edge-directed one).
  // check() refuses malvar on anything but a Bayer mosaic of at least 4 x 4, and hamilton on
  // anything but an 8-bit one of that size. (The refusal's text is what it was before hamilton:
  // a check program compares it whole.)
  PixelSource with_demosaic(const std::string& bayer_demosaic) const {
    PixelSource s = *this;
    s.bayer_demosaic_ = bayer_demosaic_of(bayer_demosaic.c_str());
    if (s.bayer_demosaic_ < 0) throw std::invalid_argument("bayer_demosaic: bilinear or malvar");
    return s;
  }
  int bayer_demosaic() const { return bayer_demosaic_; }  // BayerDemosaic
  bool bayer_malvar() const { return bayer_demosaic_ == BAYER_MALVAR; }
  bool bayer_hamilton() const { return bayer_demosaic_ == BAYER_HAMILTON; }

  // The same source for raw binary records (input_format raw): the value is the images' bytes
  // themselves, with no base64 and no envelope around them.
  PixelSource as_raw() const {
    PixelSource s = *this;
    s.raw_ = true;
    return s;
  }
  bool raw() const { return raw_; }  // the encoding: raw bytes, else b64 strings

  Kind kind() const {
    return bayer_order_    ? BAYER
           : packed_format_ ? PACKED
           : yuv_format_    ? YUV
           : elem_ != ELEM_U8 ? TYPED
                              : RGB;
  }
  int yuv_format() const { return yuv_format_; }        // YuvFormat (YUV_NONE unless YUV)
  bool yuv422() const { return yuv_is_422(yuv_format_); }  // a packed 4:2:2 frame (kind YUV)
  bool planar() const { return yuv_is_planar(yuv_format_); }  // a planar 4:2:2 / 4:4:4 frame (YUV)
  bool hi420() const { return yuv_is_420_hi(yuv_format_); }   // a 10-bit 4:2:0 frame (YUV)
  const YuvCoeffs& yuv() const { return yuv_; }
  int packed_format() const { return packed_format_; }  // PackedFormat (PACKED_NONE unless PACKED)
  int elem() const { return elem_; }                    // InputElem (ELEM_U8 unless TYPED)
  int bayer_order() const { return bayer_order_; }      // BayerOrder (BAYER_NONE unless BAYER)
  int bayer_bits() const { return bayer_bits_; }        // 8, or 10 / 12 / 16 (bayer_hi.h)
  int bayer_packing() const { return bayer_packing_; }  // BayerPacking (BAYER_PACK_NONE: 8-bit)
  bool bayer_hi() const { return bayer_packing_ != BAYER_PACK_NONE; }
  // bytes of one row of a deep mosaic: 2 WS, 5 WS / 4 or 3 WS / 2
  int bayer_hi_row_bytes(int WS) const {
    return bayer_packing_ == BAYER_PACK_LE16 ? 2 * WS : bayer_bits_ == 10 ? WS / 4 * 5 : WS / 2 * 3;
  }

  // Bytes one string carries for record-side images of HS x WS (x C for rgb, x C x E typed).
  int64_t bytes(int HS, int WS, int C) const {
    return bayer_hi()       ? bayer_hi_bytes(HS, WS, bayer_bits_, bayer_packing_)
           : kind() == BAYER ? bayer_bytes(HS, WS)
           : kind() == PACKED ? packed_bytes(HS, WS, packed_format_)
           : yuv422()       ? yuv422_bytes(HS, WS)
           : planar()       ? yuvp_bytes(HS, WS, yuv_format_)
           : hi420()        ? yuv420p10_bytes(HS, WS)
           : kind() == YUV  ? yuv420_bytes(HS, WS)
                            : (int64_t)HS * WS * C * elem_bytes(elem_);
  }

  // What a topology must look like to carry this source: model channels C, the prep's nchw,
  // record-side HS x WS, input_format b64 or raw (input_b64: one of the two). A raw source
  // carries no YUV 4:2:0 frame; a packed 4:2:2 frame goes with either encoding, any HS and an
  // even WS, and so does a planar frame (yuv444p: any WS); a 10-bit 4:2:0 frame goes with raw
  // only and even HS, WS, and so does a Bayer mosaic. std::invalid_argument otherwise; rgb goes with all, a typed tensor with everything
  // rgb b64 records go with.
  // uniform_prep: whether the prep's four coefficient pairs are equal (a typed tensor may have
  // C > 4, which the decoders serve with uniform coefficients only: b64::prep_fits; the Python
  // configuration refuses the same by --input-mean / --input-std).
  void check(int C, bool nchw, int HS, int WS, bool input_b64, bool uniform_prep = true) const {
    if (chroma_linear_) {
      if (raw_ || !input_b64 || (yuv_format_ != YUV_I420 && yuv_format_ != YUV_NV12))
        throw std::invalid_argument(
            "yuv_chroma linear needs input_format b64 and pixel_format i420 or nv12");
      if (WS > kYuv420LinearMaxWS)
        throw std::invalid_argument("yuv_chroma linear needs a record-side W of at most " +
                                    std::to_string(kYuv420LinearMaxWS));
    }
    if (bayer_hamilton()) {  // (8-bit mosaics only: bayer_hi.h has no edge-directed form)
      if (kind() != BAYER || bayer_hi())
        throw std::invalid_argument(
            "bayer_demosaic hamilton needs pixel_format bayer_rggb8 / bayer_bggr8 / bayer_grbg8 / "
            "bayer_gbrg8");
      if (HS < 4 || WS < 4)
        throw std::invalid_argument(
            "bayer_demosaic hamilton needs a record-side H, W of at least 4");
    }
    if (bayer_malvar()) {
      if (kind() != BAYER)
        throw std::invalid_argument(
            "bayer_demosaic malvar needs pixel_format bayer_rggb8 / bayer_bggr8 / bayer_grbg8 / "
            "bayer_gbrg8");  // (or a deeper mosaic, bayer_hi.h)
      if (HS < 4 || WS < 4)
        throw std::invalid_argument("bayer_demosaic malvar needs a record-side H, W of at least 4");
    }
    if (raw_ && kind() == YUV && !yuv422() && !planar() && !hi420())
      throw std::invalid_argument("input_format raw: no pixel_format i420 / nv12");
    if (raw_ && kind() == RGB && C > 4 && !uniform_prep)
      throw std::invalid_argument("input_format raw: per-channel input_a / input_b need C <= 4");
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
    if (kind() == BAYER) {
      const std::string what =
          bayer_hi() ? "pixel_format bayer_*10le / 12le / 16le / 10p / 12p"
                     : "pixel_format bayer_rggb8 / bayer_bggr8 / bayer_grbg8 / bayer_gbrg8";
      if (!input_b64 || !raw_) throw std::invalid_argument(what + " needs input_format raw");
      if (nchw) throw std::invalid_argument(what + ": no nchw layout");
      if (C != 3) throw std::invalid_argument(what + " needs a 3-channel model");
      if (HS <= 0 || WS <= 0 || ((HS | WS) & 1))
        throw std::invalid_argument(what + " needs even record-side H, W");
      if (bayer_hi() && bayer_packing_ == BAYER_PACK_MIPI && bayer_bits_ == 10 && (WS & 3))
        throw std::invalid_argument(
            "pixel_format bayer_*10p needs a record-side W that is a multiple of 4");
      return;
    }
    const std::string what = yuv422()        ? "pixel_format yuyv422 / uyvy422"
                             : planar()      ? "pixel_format yuv422p / yuv444p"
                             : hi420()       ? "pixel_format p010le / yuv420p10le"
                             : kind() == YUV ? "pixel_format i420 / nv12"
                                             : "pixel_format bgr24 / rgba / bgra / gray";
    if (hi420() && (!input_b64 || !raw_))
      throw std::invalid_argument(what + " needs input_format raw");
    if (!input_b64) throw std::invalid_argument(what + " needs input_format b64");
    if (nchw) throw std::invalid_argument(what + ": no nchw layout");
    if (C != 3) throw std::invalid_argument(what + " needs a 3-channel model");
    if (yuv422() && (WS & 1)) throw std::invalid_argument(what + " needs an even record-side W");
    if (yuv_format_ == YUV_YUV422P && (WS & 1))
      throw std::invalid_argument("pixel_format yuv422p needs an even record-side W");
    if (kind() == YUV && !yuv422() && !planar() && ((HS | WS) & 1))
      throw std::invalid_argument(what + " needs even record-side H, W");
  }

  // The ingest's b64 decode and its image arena hold RGB strings' images: for every other
  // source a GPU ingest runs CRC-only (ingest_parse off) and the step decodes from the mirror.
  bool wants_ingest_decode() const { return kind() == RGB && !raw_; }

  // What a string looks like to the ingest's plan (plan_b64_ingest), which checks it against
  // its record: a YUV 4:2:0 frame's string is that of an (HS / 2) x WS x 3 byte image, a packed
  // 4:2:2 frame's that of an HS x WS x 2 one, a planar frame's that of an HS x WS x 2 (yuv422p)
  // or x 3 (yuv444p) one, a packed-pixel
  // string that of an HS x WS x P one, a typed tensor's string that of an HS x (WS E) x C one -
  // a Bayer mosaic's that of an HS x WS x 1 one (a deep one: HS x its row bytes x 1);
  // the element size widens a row, not the channel count, because the ingest's launcher applies
  // the C > 4 coefficient rule to the C it is given even when it decodes nothing.
  // (There is no arena for any of them, so nothing is decoded.)
  Dims ingest_dims(int HS, int WS, int C) const {
    return bayer_hi()       ? Dims{HS, bayer_hi_row_bytes(WS), 1}
           : kind() == BAYER ? Dims{HS, WS, 1}
           : kind() == PACKED ? Dims{HS, WS, packed_bpp(packed_format_)}
           : yuv422()       ? Dims{HS, WS, 2}
           : planar()       ? Dims{HS, WS, 3 - yuvp_shift(yuv_format_)}
           : hi420()        ? Dims{HS, WS, 3}
           : kind() == YUV  ? Dims{HS / 2, WS, 3}
                            : Dims{HS, WS * elem_bytes(elem_), C};
  }

  // The host decode of one record (b64 or raw, by the encoding) into out[N][HS][WS][C]: the source's public parser
  // (json_codec.h), with its status, image count and floats.
  int parse_host(const uint8_t* p, size_t n, int HS, int WS, int C, float* out, int max_images,
                 int* images) const {
    if (bayer_hi())  // (raw only: check() refuses the b64 form)
      return raw_ ? codec::parse_instances_raw_bayer_hi_host(p, n, HS, WS, bayer_order_,
                                                             bayer_bits_, bayer_packing_, out,
                                                             max_images, images, bayer_malvar())
                  : (int)codec::BAD_SHAPE;
    if (kind() == BAYER)  // (raw only: check() refuses the b64 form)
      return raw_ ? codec::parse_instances_raw_bayer_named_host(p, n, HS, WS, bayer_order_, out,
                                                                max_images, images,
                                                                bayer_demosaic_)
                  : (int)codec::BAD_SHAPE;
    if (yuv422())
      return raw_ ? codec::parse_instances_raw_yuv422_host(p, n, HS, WS, yuv_format_, yuv_, out,
                                                           max_images, images)
                  : codec::parse_instances_yuv422_host(p, n, HS, WS, yuv_format_, yuv_, out,
                                                       max_images, images);
    if (planar())
      return raw_ ? codec::parse_instances_raw_yuvp_host(p, n, HS, WS, yuv_format_, yuv_, out,
                                                         max_images, images)
                  : codec::parse_instances_yuvp_host(p, n, HS, WS, yuv_format_, yuv_, out,
                                                     max_images, images);
    if (hi420())  // (raw only: check() refuses the b64 form)
      return raw_ ? codec::parse_instances_raw_yuv420p10_host(p, n, HS, WS, yuv_format_, yuv_,
                                                              out, max_images, images)
                  : (int)codec::BAD_SHAPE;
    if (raw_)
      return kind() == YUV ? (int)codec::BAD_SHAPE
                           : codec::parse_instances_raw_host(p, n, HS, WS, C, elem_,
                                                             packed_format_, out, max_images,
                                                             images);
    if (kind() == TYPED)
      return codec::parse_instances_typed_host(p, n, HS, WS, C, elem_, out, max_images, images);
    return kind() == PACKED
               ? codec::parse_instances_packed_host(p, n, HS, WS, packed_format_, out,
                                                    max_images, images)
           : kind() == YUV
               ? codec::parse_instances_yuv_host(p, n, HS, WS, yuv_format_, yuv_, out,
                                                 max_images, images, chroma_linear_)
               : codec::parse_instances_b64_host(p, n, HS, WS, C, out, max_images, images);
  }

 private:
  int yuv_format_ = YUV_NONE;
  YuvCoeffs yuv_;
  int packed_format_ = PACKED_NONE;
  int bayer_order_ = BAYER_NONE;
  int bayer_bits_ = 8;
  int bayer_packing_ = BAYER_PACK_NONE;
  int elem_ = ELEM_U8;
  bool raw_ = false;
  bool chroma_linear_ = false;
  int bayer_demosaic_ = BAYER_BILINEAR;
};

}  // namespace gale
