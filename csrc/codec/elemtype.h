// The element types of a typed tensor record (engine key input_dtype): a b64 string of pixel
// format rgb carries HS*WS*C little-endian elements of E bytes each instead of one uint8 a value.
//
//   u8    E = 1   the plain b64 record (b64_decode_instances); not a "typed" record
//   u16   E = 2   unsigned
//   f16   E = 2   IEEE binary16
//   bf16  E = 2   the top 16 bits of binary32
//   f32   E = 4   binary32
//
// float32(x) is exact for all of them and is defined here on the bits, once for the host codec
// and the kernel (b64_typed.hip): integer operations and one multiply by a power of two whose
// operands and result are normal binary32 numbers, so the result does not depend on a denormal
// mode. An f16 / bf16 / f32 element whose exponent field is all ones (Inf, NaN) is "non-finite":
// its record is refused (BAD_NUMBER; device status 2), judged on the element as sent.
// No HIP in this header: the sanitizer programs of the host codec include it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>

#if defined(__HIPCC__)
#define GALE_ELEM_HD __host__ __device__ __forceinline__
#else
#define GALE_ELEM_HD inline
#endif

namespace gale {

enum InputElem : int { ELEM_U8 = 0, ELEM_U16 = 1, ELEM_F16 = 2, ELEM_BF16 = 3, ELEM_F32 = 4 };
constexpr int kElemTypes = 5;

// The configuration names; -1 for anything else.
inline int elem_type_of(const char* name) {
  static const char* const kNames[kElemTypes] = {"u8", "u16", "f16", "bf16", "f32"};
  for (int t = 0; t < kElemTypes; ++t)
    if (strcmp(name, kNames[t]) == 0) return t;
  return -1;
}
inline const char* elem_type_name(int t) {
  static const char* const kNames[kElemTypes] = {"u8", "u16", "f16", "bf16", "f32"};
  return t >= 0 && t < kElemTypes ? kNames[t] : "?";
}
// Bytes of one element; 0 for an unknown type.
constexpr int elem_bytes(int t) {
  return t == ELEM_U8 ? 1 : t == ELEM_U16 || t == ELEM_F16 || t == ELEM_BF16 ? 2
         : t == ELEM_F32 ? 4 : 0;
}
// Bytes of an HS x WS x C tensor of type t; 0 for a non-positive size or an unknown type.
inline int64_t typed_bytes(int HS, int WS, int C, int t) {
  return HS <= 0 || WS <= 0 || C <= 0 ? 0 : (int64_t)HS * WS * C * elem_bytes(t);
}

GALE_ELEM_HD uint32_t elem_float_bits(float f) {
  uint32_t b;
  __builtin_memcpy(&b, &f, 4);
  return b;
}

// The binary32 bits of binary16 h (low 16 bits of h). Normal: rebias the exponent (+112);
// subnormal and zero: m * 2^-24 with m < 2^10 converted exactly - (float)m is a normal number or
// 0 and so is the product; Inf / NaN: exponent all ones, the mantissa kept.
GALE_ELEM_HD uint32_t f16_to_f32_bits(uint32_t h) {
  const uint32_t sign = (h & 0x8000u) << 16, em = h & 0x7FFFu;
  const uint32_t nrm = (em << 13) + 0x38000000u;
  const uint32_t sub = elem_float_bits((float)em * 5.9604644775390625e-08f);  // 2^-24
  return sign | (em < 0x0400u ? sub : em >= 0x7C00u ? nrm + 0x38000000u : nrm);
}

// The binary32 bits of element `raw` (its E bytes, little-endian, in the low bits) of type T.
template <int T>
GALE_ELEM_HD uint32_t typed_to_float_bits(uint32_t raw) {
  return T == ELEM_F32    ? raw
         : T == ELEM_BF16 ? raw << 16
         : T == ELEM_F16  ? f16_to_f32_bits(raw)
                          : elem_float_bits((float)(raw & (T == ELEM_U8 ? 0xFFu : 0xFFFFu)));
}
// Whether the element is Inf or NaN (never for the integer types).
template <int T>
GALE_ELEM_HD bool typed_nonfinite(uint32_t raw) {
  return T == ELEM_F32    ? (raw & 0x7F800000u) == 0x7F800000u
         : T == ELEM_BF16 ? (raw & 0x7F80u) == 0x7F80u
         : T == ELEM_F16  ? (raw & 0x7C00u) == 0x7C00u
                          : false;
}

namespace codec {

// n elements of type t at src (little-endian, any alignment) into dst as float32(x): the bits
// the kernel stores without a prep. Returns false if one of them is non-finite (dst is written
// all the same); an unknown type writes nothing and returns false.
inline bool typed_to_float_host(const uint8_t* src, size_t n, int t, float* dst) {
  bool finite = true;
  auto run = [&](auto tag) {
    constexpr int T = decltype(tag)::value;
    constexpr int E = elem_bytes(T);
    for (size_t i = 0; i < n; ++i) {
      uint32_t raw = 0;
      for (int j = 0; j < E; ++j) raw |= (uint32_t)src[i * E + j] << (8 * j);
      finite &= !typed_nonfinite<T>(raw);
      const uint32_t bits = typed_to_float_bits<T>(raw);
      __builtin_memcpy(dst + i, &bits, 4);
    }
  };
  switch (t) {
    case ELEM_U8: run(std::integral_constant<int, ELEM_U8>()); break;
    case ELEM_U16: run(std::integral_constant<int, ELEM_U16>()); break;
    case ELEM_F16: run(std::integral_constant<int, ELEM_F16>()); break;
    case ELEM_BF16: run(std::integral_constant<int, ELEM_BF16>()); break;
    case ELEM_F32: run(std::integral_constant<int, ELEM_F32>()); break;
    default: return false;
  }
  return finite;
}

}  // namespace codec
}  // namespace gale
