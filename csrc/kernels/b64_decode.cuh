// The decode of one base64 image string, shared by the batch step's decoder (b64_decode.hip) and
// the fetch ingest (b64_ingest.hip). See b64_decode.hip for the work split, the alignment scheme
// and the verdict rules; the callers differ only in how a workgroup finds its (image, chunk) and
// in where the verdict goes.
//
// It stands on the lane's window (load_window, window_bad): the one place that reads a string's
// characters, aligns them, turns them into 24-bit groups and judges them for b64_decode_body and
// the YUV decoder (b64_yuv.hip); each keeps only how a lane finds its window and what it does
// with the 12 bytes. (The packed-pixel decoder, b64_packed.hip, has a copy: see its header.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gale/kernels.h"

namespace gale {
namespace b64 {

constexpr int kLanesPerChunk = kB64ChunkChars / 16;  // 256: the workgroup size
constexpr int kStageWaves = kLanesPerChunk / 64;
// LDS staging of a workgroup: 3 float4 per lane, 3 KB per wave
typedef float4 Stage[3 * 64];

// ---- 4 characters per op ------------------------------------------------------------------------
// Nibble lookups with v_perm_b32, as the JSON parser classifies its bytes (classify4).
// Validity: a character c is outside the alphabet iff HI[c >> 4] & LO[c & 15] != 0 (or c >= 0x80).
// HI names the row's class: 0x01 row 2 ('+' '/'), 0x02 row 3 (digits), 0x04 rows 4 and 6
// ('@A-O', '`a-o'), 0x08 rows 5 and 7 ('P-Z[..', 'p-z{..'), 0x10 every other row. LO[n] has the
// bit of each class in which column n is NOT in the alphabet (0x10 always).
constexpr uint32_t kHi03 = 0x02011010u, kHi47 = 0x08040804u;
constexpr uint32_t kLo03 = 0x11111115u, kLo47 = 0x11111111u, kLo8B = 0x1A131111u,
                   kLoCF = 0x1A1B1B1Bu;
// Sextet = c + ROLL[(c >> 4) - (c == '/')] modulo 256: '+' + 19, '/' + 16 (the row-2 entry moved
// down one), digits + 4, 'A-Z' - 65, 'a-z' - 71.
constexpr uint32_t kRoll03 = 0x04131000u, kRoll47 = 0xB9B9BFBFu;

// The sextets of 4 characters (one per byte, first character in byte 0; garbage for characters
// outside the alphabet) and, in *inval, a non-zero byte for each such character.
__device__ __forceinline__ uint32_t b64_sextets4(uint32_t x, uint32_t* inval) {
  const uint32_t hsel = (x >> 4) & 0x07070707u;
  const uint32_t lo = x & 0x0F0F0F0Fu;
  const uint32_t s = lo & 0x07070707u;
  const uint32_t hi = __builtin_amdgcn_perm(kHi47, kHi03, hsel);
  const uint32_t p0 = __builtin_amdgcn_perm(kLo47, kLo03, s);
  const uint32_t p1 = __builtin_amdgcn_perm(kLoCF, kLo8B, s);
  const uint32_t m = ((lo >> 3) & 0x01010101u) * 0xFFu;
  *inval = (hi & ((m & p1) | (~m & p0))) | (x & 0x80808080u);
  // bytes equal to '/': exact zero-byte test of x ^ "////"
  const uint32_t z = x ^ 0x2F2F2F2Fu;
  const uint32_t eq = ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z | 0x7F7F7F7Fu) >> 7;
  const uint32_t roll = __builtin_amdgcn_perm(kRoll47, kRoll03, hsel - eq);
  // bytewise x + roll without carries between bytes
  return ((x & 0x7F7F7F7Fu) + (roll & 0x7F7F7F7Fu)) ^ ((x ^ roll) & 0x80808080u);
}

// Byte mask of the first n bytes of a dword (n <= 0: none, n >= 4: all).
__device__ __forceinline__ uint32_t first_bytes(int n) {
  return n <= 0 ? 0u : n >= 4 ? 0xFFFFFFFFu : (1u << (8 * n)) - 1u;
}

// ---- a lane's window ----------------------------------------------------------------------------
// The 16 characters at bytes + off + c (off: the string's first character, c: the window's first
// character in the string, a multiple of 4), of which the first nch (4, 8, 12 or 16) lie in the string:
// x[t] the characters of quad t (first in byte 0), v[t] its 24-bit group (byte 0 of the group in
// bits 16 .. 23; garbage where a character is outside the alphabet), inv[t] a non-zero byte for
// each character outside the alphabet.
struct Window {
  uint32_t x[4], v[4], inv[4];
};

// Read bound: the aligned 16-byte word under the window's first character and, only when the
// nch characters reach into it, the next one - at most 15 bytes before a string and fewer than 16
// past it are read, whatever the string's start phase.
// off and c come apart so that the phase of a window at c = 16 k is visibly the string's
// (off & 15, the same for every lane of an image): the alignment switch below is then a scalar
// branch. Taken from the sum off + c, the phase is a per-lane value to the compiler and the
// switch an exec-masked one (measured: 1-2 % on the packed decoders). Where a wave's lanes do
// differ in phase - b64_yuv_kernel, whose waves can span two byte ranges - it diverges, rightly.
__device__ __forceinline__ Window load_window(const uint8_t* bytes, int64_t off, int c, int nch) {
  const int ph = (int)((off + (c & 15)) & 15);
  const uint8_t* base = bytes + (off + c - ph);
  const uint4 lo = *reinterpret_cast<const uint4*>(base);
  const uint4 hi = ph + nch > 16 ? *reinterpret_cast<const uint4*>(base + 16)
                                 : make_uint4(0, 0, 0, 0);
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  const uint32_t sh = (uint32_t)(ph & 3);
  Window win;
  switch (ph >> 2) {  // (wave-uniform where the lanes of a wave share the phase: see above)
#define GALE_ALIGN_WORDS(D)                                    \
  _Pragma("unroll") for (int t = 0; t < 4; ++t) win.x[t] =     \
      __builtin_amdgcn_alignbyte(w[t + (D) + 1], w[t + (D)], sh);
    case 0: GALE_ALIGN_WORDS(0) break;
    case 1: GALE_ALIGN_WORDS(1) break;
    case 2: GALE_ALIGN_WORDS(2) break;
    default: GALE_ALIGN_WORDS(3) break;
#undef GALE_ALIGN_WORDS
  }
  // 4 characters -> 4 sextets -> 24 bits
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const uint32_t sx = b64_sextets4(win.x[t], &win.inv[t]) & 0x3F3F3F3Fu;
    // halves: (s0 << 6 | s1), (s2 << 6 | s3); then s0 << 18 | s1 << 12 | s2 << 6 | s3
    const uint32_t h = ((sx & 0x003F003Fu) << 6) | ((sx >> 8) & 0x003F003Fu);
    win.v[t] = ((h & 0xFFFu) << 12) | (h >> 16);
  }
  return win;
}

// Whether the window holds a character outside the alphabet among its data characters or a
// non-'=' in the padding. nd: data characters of the string from the window's start on.
__device__ __forceinline__ bool window_bad(const Window& win, int nd, int nch) {
  if (nd >= 16)  // every character of the window is a data character
    return (win.inv[0] | win.inv[1] | win.inv[2] | win.inv[3]) != 0;
  // the string's last lane: data characters, then '=', then not judged
  uint32_t j = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const uint32_t dm = first_bytes(nd - 4 * t);
    j |= (win.inv[t] & dm) | ((win.x[t] ^ 0x3D3D3D3Du) & first_bytes(nch - 4 * t) & ~dm);
  }
  return j != 0;
}

// (selects on the by-value coefficients: a dynamic index would spill them to scratch)
__device__ __forceinline__ float prep_a(const InputPrep& p, int ch) {
  return ch == 0 ? p.a[0] : ch == 1 ? p.a[1] : ch == 2 ? p.a[2] : p.a[3];
}
__device__ __forceinline__ float prep_b(const InputPrep& p, int ch) {
  return ch == 0 ? p.b[0] : ch == 1 ? p.b[1] : ch == 2 ? p.b[2] : p.b[3];
}
// (float)v of channel ch, through fmaf(v, a[ch], b[ch]) with PREP
template <bool PREP, typename T>
__device__ __forceinline__ float prepped(T v, int ch, const InputPrep& prep) {
  const float f = (float)v;
  return PREP ? __builtin_fmaf(f, prep_a(prep, ch), prep_b(prep, ch)) : f;
}

// Chunk `chunk` (kB64ChunkChars characters) of the string at bytes + d.off, by the 256 threads of
// a workgroup (tid = the thread's index in it): lane group k = chunk * 256 + tid decodes
// characters [16k, 16k + 16) into values [12k, 12k + 12) of the image at out + d.slot * H*W*C.
// Returns whether this lane saw a bad character or bad padding; every thread of the workgroup
// must call it (the staged store is per wave). stage: the workgroup's LDS staging rows.
// PREP: fmaf(v, a[c], b[c]) at the store (`prep` is never read without it). NCHW (with PREP):
// the string's bytes are ordered [C][H][W], transposed at the store. CT: the channel count when
// a lane's channel pattern is a compile-time one (1 or 3: 12 values per lane are whole pixels),
// 0 = general C.
template <bool PREP, bool NCHW, int CT>
__device__ __forceinline__ bool b64_decode_body(const B64Image& d, int chunk, int tid,
                                                const uint8_t* bytes, int H, int W, int C,
                                                float* out, const InputPrep& prep, Stage* stage) {
  const int per = H * W * C;
  const int L = 4 * ((per + 2) / 3);
  const int pad = (3 - per % 3) % 3;
  const int k = chunk * kLanesPerChunk + tid;  // this lane's 16-character group
  const int c0 = 16 * k;
  bool bad = false;
  // NHWC stores go through LDS when the image's base is 16-byte aligned (wave-uniform): a lane's
  // 12 floats are 48 bytes apart from its neighbour's, so its three 16-byte stores would each
  // touch every third 16 bytes of the wave's 3 KB; staged, each store instruction of the wave
  // writes 1 KB contiguous.
  float* const img_dst = out + (int64_t)d.slot * per;
  const bool staged = !NCHW && (reinterpret_cast<uintptr_t>(img_dst) & 15) == 0;
  const int lane = tid & 63;
  float4* const wl = stage[tid >> 6];
  if (c0 < L) {
    const int nch = min(16, L - c0);     // characters of the string in the window (4, 8, 12, 16)
    const int nd = L - pad - c0;         // data characters from the window's start on
    // (every lane of an image has the string's phase)
    const Window win = load_window(bytes, d.off, c0, nch);
    bad = window_bad(win, nd, nch);
    float f[12];  // 24 bits -> 3 values
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f[3 * t] = (float)((win.v[t] >> 16) & 0xFFu);
      f[3 * t + 1] = (float)((win.v[t] >> 8) & 0xFFu);
      f[3 * t + 2] = (float)(win.v[t] & 0xFFu);
    }
    const int v0 = 12 * k;               // first value of this lane (< per, see the launchers)
    const int nv = min(12, per - v0);    // values of the image in this lane
    float* dst = img_dst;
    if (NCHW) {
      const int hw = H * W;
      int ch = v0 / hw, p = v0 - ch * hw;
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        if (j < nv) {
          const int cs = min(ch, 3);
          dst[(int64_t)p * C + ch] = __builtin_fmaf(f[j], prep_a(prep, cs), prep_b(prep, cs));
        }
        if (++p == hw) { p = 0; ++ch; }
      }
    } else {
      if (PREP) {
        int ch = CT ? 0 : v0 % C;
#pragma unroll
        for (int j = 0; j < 12; ++j) {
          const int cs = CT ? j % CT : min(ch, 3);
          f[j] = __builtin_fmaf(f[j], prep_a(prep, cs), prep_b(prep, cs));
          if (!CT && ++ch == C) ch = 0;
        }
      }
      dst += v0;
      if (staged) {
        wl[3 * lane] = make_float4(f[0], f[1], f[2], f[3]);
        wl[3 * lane + 1] = make_float4(f[4], f[5], f[6], f[7]);
        wl[3 * lane + 2] = make_float4(f[8], f[9], f[10], f[11]);
      } else {
#pragma unroll
        for (int j = 0; j < 12; ++j)
          if (j < nv) dst[j] = f[j];
      }
    }
  }
  if (staged) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the wave's own LDS writes)
    const int wv0 = 12 * (k - lane);             // the wave's first value; 48 (k - lane) bytes in
    const int nvw = min(12 * 64, per - wv0);     // its values of the image (<= 0: none)
    float* wdst = img_dst + wv0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int q = 64 * i + lane;
      if (4 * q + 4 <= nvw) {
        reinterpret_cast<float4*>(wdst)[q] = wl[q];
      } else {
        const float* ws = reinterpret_cast<const float*>(wl);
        for (int e = 4 * q; e < nvw; ++e) wdst[e] = ws[e];
      }
    }
  }
  return bad;
}

// `prep` with a channel index past the four coefficient slots (C > 4) needs uniform coefficients.
inline bool prep_fits(const InputPrep* prep, int C) {
  if (!prep || prep->identity() || C <= 4) return true;
  for (int i = 1; i < 4; ++i)
    if (prep->a[i] != prep->a[0] || prep->b[i] != prep->b[0]) return false;
  return true;
}

}  // namespace b64
}  // namespace gale
