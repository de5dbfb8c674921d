// Host side of the InstObj / PredObj JSON contract.
//
// Input  (InstObj, /root/reference/src/main/java/dke/model/data/InstObj.java:8):
//     {"instances": float[N][H][W][C]}
// Output (PredObj, /root/reference/src/main/java/dke/model/data/PredObj.java:9):
//     {"predictions": float[N][classes]}
//
// The reference decodes with Jackson on the bolt thread (InferenceBolt.java:76) and re-encodes
// with a fresh ObjectMapper per tuple (:90-91). gale splits decoding in two:
//   * scan_instances() — a cheap AVX2 pass on the consumer thread: validates the envelope
//     (exactly one key, "instances", like Jackson's FAIL_ON_UNKNOWN_PROPERTIES) and derives N
//     from the '[' count of a rank-4 rectangular array (1 + N + N*H + N*H*W opening brackets);
//   * the float parsing and the full per-token structural check run on the GPU
//     (csrc/kernels/json_parse.hip), reading the staged bytes straight from pinned memory.
// parse_instances_host() is the complete host decoder (CPU stub replica, tests, diagnostics).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cstdint>

#include <string>
#include <utility>
#include <vector>

#include "elemtype.h"
#include "pixfmt.h"
#include "yuv.h"

namespace gale {
namespace codec {

enum Status : int {
  OK = 0,
  BAD_ENVELOPE = 1,   // not {"instances": [...]} (syntax error, not an object, no array)
  UNKNOWN_KEY = 2,    // a top-level key other than "instances" (Jackson FAIL_ON_UNKNOWN_PROPERTIES)
  BAD_SHAPE = 3,      // not rank 4, ragged, or per-image shape != model H x W x C
  EMPTY = 4,          // zero images
  BAD_NUMBER = 5,     // malformed JSON number / non-number element
  NULL_INSTANCES = 6, // "instances": null
  TOO_LARGE = 7,      // more images than the caller allows
  CORRUPT = 8,        // the Kafka batch holding the record could not be decoded (unknown codec,
                      // corrupt compressed data, CRC mismatch; kafka/compress.h poison records)
};
constexpr int kStatusCount = 9;

const char* status_name(int s);

struct Scan {
  int status = OK;
  int64_t arr_off = 0;  // byte offset of the outer '[' of the instances array
  int64_t arr_len = 0;  // bytes up to and including the matching ']'
  int images = 0;       // N
};

// Bounded envelope check: the {"instances": ... } prefix and the "] }" suffix only (reads a
// few bytes at each end; the array's interior, its image count and any key hidden inside it are
// left to the device ingest / parser). images stays 0.
// head_limit / tail_limit: only the first / last that many bytes of the value are read (a sparse
// host copy holds nothing else, kafka/fetch_framing.h); an envelope reaching beyond them is
// rejected as BAD_ENVELOPE (documented limit: <= ~200 bytes of whitespace around it).
Scan scan_envelope(const uint8_t* p, size_t n, size_t head_limit = SIZE_MAX,
                   size_t tail_limit = SIZE_MAX);

// Envelope validation + image count (the per-number work is left to the GPU parser).
Scan scan_instances(const uint8_t* p, size_t n, int H, int W, int C);

// Byte spans [begin, end) of the top-level elements (the images) of the instances array
// `arr[0..len)` (its outer '[' ... ']'), for splitting a record with more images than one
// micro-batch holds. false when the bracket structure is broken.
bool split_instances(const uint8_t* arr, size_t len,
                     std::vector<std::pair<uint32_t, uint32_t>>& spans);

// Full host decoder: validates structure and parses every number into out[N*H*W*C].
// Returns the status; *images receives N. out may be null to validate only.
int parse_instances_host(const uint8_t* p, size_t n, int H, int W, int C, float* out,
                         int max_images, int* images);

// The GPU parse's input preprocessing (InputPrep, gale/kernels.h) on a host-parsed block of
// `images` images, in place: y = fmaf(x, a[c], b[c]) in binary32 with one rounding (a, b: four
// coefficients, channels >= 3 take the last), bit-identical to the device. nchw: x holds each
// image as parsed from a [C][H][W] nesting (parse_instances_host with the dims permuted to
// (C, H, W)) and is transposed to [H][W][C].
void apply_input_prep(float* x, int images, int H, int W, int C, bool nchw, const float* a,
                      const float* b);

// ---- base64 uint8 image records (input format "b64") -------------------------------------------
//     {"instances":[{"b64":"<base64 of image 0>"},{"b64":"..."}]}
// One object per image with exactly one key, "b64"; its string is standard base64 (RFC 4648 §4)
// of exactly H*W*C bytes, one uint8 value each, so its length is L = 4 * ceil(H*W*C / 3) with
// the last (3 - H*W*C % 3) % 3 characters '='. The string body is never unescaped.

// Characters of one image's string.
inline int64_t b64_chars(int H, int W, int C) { return 4 * (((int64_t)H * W * C + 2) / 3); }
// The same from the string's byte count: the scan, b64_image_offsets and split_instances_b64
// below have a *_bytes form that takes the bytes one string carries (an H x W x C image: H*W*C;
// a YUV 4:2:0 frame: yuv420_bytes, yuv.h); the (H, W, C) forms forward to it. nbytes <= 0 is
// what a non-positive dimension is there.
inline int64_t b64_chars_bytes(int64_t nbytes) { return 4 * ((nbytes + 2) / 3); }

// Envelope and element-list check + image count. Walks the elements and never reads a string's
// body: after the opening quote it checks the closing quote L characters on. O(images), every
// access bounded by n. Verdicts: BAD_ENVELOPE (not an object, no instances array, syntax around
// the elements, a cut-off value), UNKNOWN_KEY (another top-level key; a key other than "b64" or
// a second key in an element), NULL_INSTANCES, EMPTY, BAD_SHAPE (an element that is not an
// object, a value that is not a string, a closing quote not at L characters), TOO_LARGE
// (more than 2^30 images). The characters themselves are judged by the decoder (BAD_NUMBER).
Scan scan_instances_b64(const uint8_t* p, size_t n, int H, int W, int C);
Scan scan_instances_b64_bytes(const uint8_t* p, size_t n, int64_t nbytes);

// Of a scanned record's instances array `arr[0..len)`: the offset (from arr) of the first
// character of every image's string. false when the element list is not what the scan accepted.
bool b64_image_offsets(const uint8_t* arr, size_t len, int H, int W, int C,
                       std::vector<uint32_t>& offs);
bool b64_image_offsets_bytes(const uint8_t* arr, size_t len, int64_t nbytes,
                             std::vector<uint32_t>& offs);

// split_instances for b64 records: the byte spans [begin, end) of the elements (each image's
// {"b64":"..."} object).
bool split_instances_b64(const uint8_t* arr, size_t len, int H, int W, int C,
                         std::vector<std::pair<uint32_t, uint32_t>>& spans);
bool split_instances_b64_bytes(const uint8_t* arr, size_t len, int64_t nbytes,
                               std::vector<std::pair<uint32_t, uint32_t>>& spans);

// Full host decoder: the scan's verdicts, then every string decoded into out[N*H*W*C] as
// (float)byte in string order (what parse_instances_host gives for the same pixels written as
// numbers). A character outside the alphabet in the data part, or a non-'=' in the padding, is
// BAD_NUMBER; unused low bits of the last data character are ignored. out may be null.
int parse_instances_b64_host(const uint8_t* p, size_t n, int H, int W, int C, float* out,
                             int max_images, int* images);

// Full host decoder of YUV 4:2:0 frame records (yuv.h): the same envelope, element list and
// verdicts with strings of yuv420_bytes(HS, WS) bytes (L = 4 B / 3 characters, never a '='; a
// character outside the alphabet anywhere is BAD_NUMBER), every frame converted by
// yuv420_to_rgb_host into out[N][HS][WS][3] as (float)RGB - what parse_instances_b64_host gives
// for the converted image sent as an RGB record. Odd or non-positive sizes and unknown formats
// are BAD_SHAPE. out may be null.
int parse_instances_yuv_host(const uint8_t* p, size_t n, int HS, int WS, int format,
                             const YuvCoeffs& k, float* out, int max_images, int* images);

// Full host decoder of packed-pixel records (pixfmt.h: bgr24 / rgba / bgra / gray): the same
// envelope, element list and verdicts with strings of packed_bytes(HS, WS, format) bytes
// (L = 4 ceil(B / 3) characters, the last (3 - B mod 3) mod 3 of them '='; a character outside
// the alphabet in the data part or a non-'=' in the padding is BAD_NUMBER), every image unpacked
// by packed_to_rgb_host into out[N][HS][WS][3] as (float)RGB - what parse_instances_b64_host
// gives for the unpacked image sent as an RGB record. An unknown format or a non-positive size
// is BAD_SHAPE. out may be null.
int parse_instances_packed_host(const uint8_t* p, size_t n, int HS, int WS, int format,
                                float* out, int max_images, int* images);

// Full host decoder of typed tensor records (elemtype.h: u16 / f16 / bf16 / f32; u8 decodes as
// parse_instances_b64_host): the same envelope, element list and verdicts with strings of
// typed_bytes(HS, WS, C, type) bytes (L = 4 ceil(B / 3) characters, the last (3 - B mod 3) mod 3
// of them '='; a character outside the alphabet in the data part or a non-'=' in the padding is
// BAD_NUMBER), every string's little-endian elements converted by typed_to_float_host into
// out[N][HS*WS*C] in string order, then the non-finite verdict: an f16 / bf16 / f32 element with
// an all-ones exponent is BAD_NUMBER. An unknown type or a non-positive size is BAD_SHAPE. out
// may be null (the elements are judged all the same).
int parse_instances_typed_host(const uint8_t* p, size_t n, int HS, int WS, int C, int type,
                               float* out, int max_images, int* images);

// Java Float.toString formatting (what Jackson emits for float[]): shortest digits
// that round-trip, decimal for 1e-3 <= |v| < 1e7 ("0.125", "3.0"), else "1.0E-5". Returns length.
int format_float_java(float v, char* out);
// Java 8 Float.toString (FloatingDecimal's free-format digit loop, csrc/codec/java8_float.cpp):
// the reference's runtime; it sometimes prints more digits than the shortest form. Parity with
// a real Java 8 is unpinned (no JVM here).
int format_float_java8(float v, char* out);

// {"predictions":[[p00,p01,...],[p10,...]]} (Jackson compact). json_string=true wraps the
// document in a JSON string literal, which is what spring-kafka's JsonSerializer does to the
// already-serialized String value (MainTopology.java:115).
// java8: Java 8 Float.toString digits (format_float_java8) instead of the JDK 19 rule
void encode_predictions(const float* probs, int n, int classes, bool json_string,
                        std::string& out, bool java8 = false);
// Same output from pre-formatted values: text16 holds n * classes 16-byte slots (characters,
// length in byte 15; format_floats_java in csrc/kernels/format.hip).
void encode_predictions_text(const uint8_t* text16, int n, int classes, bool json_string,
                             std::string& out);

// ---- top-k output (--top-k K) -------------------------------------------------------------------
//     {"predictions":[{"classes":[3,5,1],"scores":[0.9123,0.05,0.0101]},{...}]}
// One element per image, in image order: the K best classes (0-based) and their scores (the same
// Float.toString text as the full rows), in score order.
//
// Score order. It is defined on the bits, so host and device cannot differ:
//     key(v) = bits(v) ^ (bits(v) >> 31 ? 0xffffffff : 0x80000000), compared as unsigned;
// entry j of an image is its j-th largest (key, -index): descending by score, ties to the lower
// class index. So -0 sorts below +0 and a positive NaN above +Infinity. The device selection
// (csrc/kernels/topk.hip) implements this rule and refers here.
inline uint32_t score_key(float v) {
  uint32_t b;
  __builtin_memcpy(&b, &v, 4);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
// Selects on the host (std::partial_sort on (key, index)) and formats; 1 <= k <= classes.
void encode_predictions_topk(const float* probs, int n, int classes, int k, bool json_string,
                             std::string& out, bool java8 = false);
// Same output from a device selection: text16 holds n * k score slots (format as
// encode_predictions_text's), idx the n * k class indices, entry (i, j) at i * k + j.
void encode_predictions_topk_text(const uint8_t* text16, const int32_t* idx, int n, int k,
                                  bool json_string, std::string& out);

// {"instances":[[[[x,...]]]]} with Java Float.toString numbers: the load generator's encoder
// (the reference's producers are external; this is the shape README.md:22-27 documents).
void encode_instances(const float* x, int n, int H, int W, int C, std::string& out);

// {"error":"<status>","detail":"..."} record used by --on-error error-json.
void encode_error(int status, const char* detail, bool json_string, std::string& out);

}  // namespace codec
}  // namespace gale
