"""Input preprocessing: scale, per-channel mean / std and the record's nesting order.

A trained classifier expects ``y = (x * scale - mean[c]) / std[c]`` (torchvision ``ToTensor`` +
``Normalize``: mean and std in the units after scaling). gale applies it where the record text
is parsed - the GPU JSON parser's store, or the stub replica's host decoder - so clients can send
raw pixels. The numerics are defined once, here:

* ``a[c] = float32(scale / std[c])`` and ``b[c] = float32(-mean[c] / std[c])``, computed in
  double and rounded once;
* ``y = fma(x, a[c], b[c])`` in binary32 with a single rounding, ``x`` the correctly rounded
  binary32 value of the record's token.

Host (``codec::apply_input_prep``) and device (``json_parse_prep_kernel``) results are
bit-identical. ``layout="nchw"`` says the record's ``instances`` array nests ``[N][C][H][W]``;
the model's tensors stay NHWC.

``YuvConvert`` (below) defines what may come first: ``b64`` records that carry YUV 4:2:0 video
frames (``--input-pixel-format i420 | nv12``) are converted to 0..255 RGB in integers before the
fma above.

``PixelUnpack`` (below) is the other thing that may come first: ``b64`` records whose pixels are
packed as ``bgr24``, ``rgba``, ``bgra`` or ``gray`` are unpacked to interleaved RGB bytes.

``InputResize`` (below) defines the step that may follow: records that carry images of another
size are resized (bilinear, or with ``antialias`` the support-scaled triangle filter) and
centre-cropped to the model's on the preprocessed values.
"""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np

LAYOUTS = ("nhwc", "nchw")
MAX_CHANNEL_COEFFS = 4  # the coefficients travel by value in the parse kernel's arguments


def parse_floats(text) -> Tuple[float, ...]:
    """``"0.4914,0.4822,0.4465"`` (or a sequence / scalar) -> tuple of floats; empty -> ()."""
    if text is None:
        return ()
    if isinstance(text, (int, float)):
        return (float(text),)
    if isinstance(text, str):
        parts = [p.strip() for p in text.split(",")]
        parts = [p for p in parts if p]
        try:
            return tuple(float(p) for p in parts)
        except ValueError:
            raise ValueError(f"not a comma-separated list of numbers: {text!r}") from None
    return tuple(float(v) for v in text)


@dataclass(frozen=True)
class InputPrep:
    """The preprocessing of one model input with C channels (``a`` / ``b``: C float32 values)."""

    C: int
    a: Tuple[float, ...]
    b: Tuple[float, ...]
    layout: str = "nhwc"
    scale: float = 1.0  # (the record units: fp8 calibration draws U[0,1) / scale)

    @classmethod
    def build(cls, C: int, scale: float = 1.0, mean: Sequence[float] = (),
              std: Sequence[float] = (), layout: str = "nhwc") -> "InputPrep":
        if layout not in LAYOUTS:
            raise ValueError(f"input_layout={layout!r}: expected one of {LAYOUTS}")
        mean, std = parse_floats(mean), parse_floats(std)
        scale = float(scale)
        for name, vals in (("input_scale", (scale,)), ("input_mean", mean), ("input_std", std)):
            if not all(math.isfinite(v) for v in vals):
                raise ValueError(f"{name}: non-finite value")
        if any(s == 0.0 for s in std):
            raise ValueError("input_std: a std of 0")
        for name, vals in (("input_mean", mean), ("input_std", std)):
            if len(vals) not in (0, 1, C):
                raise ValueError(f"{name}: {len(vals)} values for a {C}-channel input "
                                 f"(expected 1 or {C})")
            if len(vals) > 1 and C > MAX_CHANNEL_COEFFS:
                raise ValueError(f"{name}: per-channel values need C <= {MAX_CHANNEL_COEFFS} "
                                 f"(the model has {C}); give one value")
        m = [(mean[i] if len(mean) > 1 else mean[0]) if mean else 0.0 for i in range(C)]
        s = [(std[i] if len(std) > 1 else std[0]) if std else 1.0 for i in range(C)]
        a = tuple(float(np.float32(scale / s[c])) for c in range(C))
        b = tuple(float(np.float32(-m[c] / s[c])) + 0.0 for c in range(C))  # (-0.0 -> 0.0)
        if not all(math.isfinite(v) for v in a + b):
            raise ValueError("input preprocessing: scale / std or mean / std is not finite")
        if scale == 0.0:
            raise ValueError("input_scale: 0 would erase the input")
        return cls(C=C, a=a, b=b, layout=layout, scale=scale)

    @classmethod
    def from_config(cls, cfg, C: int) -> "InputPrep":
        return cls.build(C, cfg.input_scale, cfg.input_mean, cfg.input_std, cfg.input_layout)

    @property
    def nchw(self) -> bool:
        return self.layout == "nchw"

    @property
    def identity(self) -> bool:
        return not self.nchw and all(v == 1.0 for v in self.a) and all(v == 0.0 for v in self.b)

    def coeffs(self) -> Tuple[list, list]:
        """``a`` / ``b`` as the four by-value slots of the native ``InputPrep`` (channels past the
        last one repeat it, so a broadcast scalar fills all four)."""
        pad = lambda v: [v[min(i, len(v) - 1)] for i in range(MAX_CHANNEL_COEFFS)]  # noqa: E731
        if self.C > MAX_CHANNEL_COEFFS:  # validated uniform
            return [self.a[0]] * MAX_CHANNEL_COEFFS, [self.b[0]] * MAX_CHANNEL_COEFFS
        return pad(self.a), pad(self.b)

    def engine_entries(self) -> Dict[str, Any]:
        a, b = self.coeffs()
        return dict(input_a=a, input_b=b, input_nchw=self.nchw)

    def kernel_kwargs(self) -> Dict[str, Any]:
        """Keyword arguments of the ``json_parse_instances`` binding."""
        a, b = self.coeffs()
        return dict(a=a, b=b, nchw=self.nchw)

    def apply(self, x):
        """The model input of NHWC record values ``x`` ([..., C]; numpy or torch): the binary32
        fma with one rounding (``fma_f32``), bit-identical to what the engine feeds the model."""
        is_torch = hasattr(x, "numpy") and not isinstance(x, np.ndarray)
        xv = x.detach().cpu().numpy() if is_torch else np.asarray(x)
        xv = xv.astype(np.float32, copy=False)
        if xv.shape[-1] != self.C:
            raise ValueError(f"last dimension {xv.shape[-1]} != {self.C} channels")
        y = fma_f32(xv, np.asarray(self.a, np.float32), np.asarray(self.b, np.float32))
        if is_torch:
            import torch

            return torch.from_numpy(y)
        return y


def fma_f32(x: np.ndarray, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """``float32(x * a + b)`` with a single rounding, elementwise (broadcasting), in numpy.

    The product of two binary32 values is exact in binary64 (48 significand bits). The sum p + b
    is then split without error (two-sum) into s + e; narrowing s alone would round twice, so s
    is first nudged to an odd significand whenever e != 0 (round-to-odd), after which one
    narrowing to binary32 is the correctly rounded result (53 >= 2 * 24 + 2).
    """
    p = x.astype(np.float64) * a.astype(np.float64)
    bb = np.broadcast_to(b.astype(np.float64), p.shape)
    s = p + bb
    t = s - p
    e = (p - (s - t)) + (bb - t)  # exact error of the sum
    bits = np.ascontiguousarray(s).view(np.int64).copy()
    inexact = (e != 0) & np.isfinite(s)
    even = (bits & 1) == 0
    # toward the true value: s + e lies between s and its neighbour in the direction of e
    up = (e > 0) == (s > 0)  # magnitude grows
    adj = np.where(inexact & even, np.where(up, 1, -1), 0).astype(np.int64)
    # s == 0 with e != 0 cannot happen (then s would be e); magnitudes move by one ulp
    out = (bits + adj).view(np.float64).reshape(s.shape)
    with np.errstate(over="ignore"):
        return out.astype(np.float32)


RESIZE_MAX = 4096  # largest source / resize / model side the resize tables are built for


def parse_size(text, name: str) -> Tuple[int, ...]:
    """``"40,36"`` -> (40, 36), ``"256"`` -> (256,), empty -> (); ValueError naming the option."""
    if text is None:
        return ()
    if isinstance(text, int):
        return (int(text),)
    if not isinstance(text, str):
        text = ",".join(str(v) for v in text)
    parts = [p.strip() for p in text.split(",")]
    if parts == [""]:
        return ()
    if len(parts) > 2 or not all(p.isdigit() for p in parts):
        raise ValueError(f"{name}: expected H,W or one number, got {text!r}")
    return tuple(int(p) for p in parts)


def _axis_table(n_src: int, n_rs: int, n_out: int):
    """Per output index of one axis: (i0, i1, w) of the half-pixel bilinear sample of a source of
    n_src pixels resized to n_rs, read at the centre crop's n_out pixels (floor offset)."""
    off = (n_rs - n_out) // 2
    i0 = np.zeros(n_out, np.int32)
    i1 = np.zeros(n_out, np.int32)
    w = np.zeros(n_out, np.float32)
    den = 2 * n_rs
    for i in range(n_out):
        num = (2 * (i + off) + 1) * n_src - n_rs
        if num < 0:
            continue
        q, rem = divmod(num, den)
        if q >= n_src - 1:
            i0[i] = i1[i] = n_src - 1
            continue
        i0[i], i1[i] = q, q + 1
        w[i] = np.float32(np.float64(rem) / np.float64(den))
    return i0, i1, w


def _lerp_f32(a: np.ndarray, b: np.ndarray, w: np.ndarray) -> np.ndarray:
    """a where w == 0 (b is not used), else fma(w, b - a, a): one binary32 subtraction (binary64
    subtraction narrowed: correctly rounded for binary32 operands) and one fma rounding."""
    with np.errstate(over="ignore", invalid="ignore"):
        d = (b.astype(np.float64) - a.astype(np.float64)).astype(np.float32)
        ww = np.broadcast_to(w, a.shape)
        zero = ww == 0
        r = fma_f32(np.where(zero, np.float32(0), ww), np.where(zero, np.float32(0), d), a)
    return np.where(zero, a, r).astype(np.float32)


RESIZE_AA_MAX_SCALE = 8  # antialias: n_src <= 8 * n_rs per axis ...
RESIZE_AA_MAX_TAPS = 2 * RESIZE_AA_MAX_SCALE + 1  # ... so an entry has at most 17 taps


def _aa_axis_table(n_src: int, n_rs: int, n_out: int):
    """The antialiased (support-scaled triangle) filter of one axis: per output index the first
    tap and the tap count (int32 [n_out]) and all weights concatenated in index order (float32).

    With off = (n_rs - n_out) // 2 and S = max(n_src, n_rs), the integer
    ``u(i, k) = 2 S - |(2 k + 1) n_rs - (2 (i + off) + 1) n_src|`` is 2 S times the triangle
    weight; the taps of i are the k in [0, n_src) with u > 0 (a contiguous, non-empty run) and
    ``w = float32(float64(u) / float64(U))``, U the sum of the run's u."""
    off = (n_rs - n_out) // 2
    S = max(n_src, n_rs)
    start = np.zeros(n_out, np.int32)
    count = np.zeros(n_out, np.int32)
    ws = []
    for i in range(n_out):
        c = (2 * (i + off) + 1) * n_src
        # u > 0 <=> c - 2 S < (2 k + 1) n_rs < c + 2 S
        lo = max((c - 2 * S - n_rs) // (2 * n_rs) + 1, 0)
        hi = min(-((n_rs - c - 2 * S) // (2 * n_rs)) - 1, n_src - 1)  # (ceil) - 1
        u = [2 * S - abs((2 * k + 1) * n_rs - c) for k in range(lo, hi + 1)]
        assert u and min(u) > 0, (n_src, n_rs, n_out, i)
        assert lo == 0 or 2 * S - abs((2 * lo - 1) * n_rs - c) <= 0
        assert hi == n_src - 1 or 2 * S - abs((2 * hi + 3) * n_rs - c) <= 0
        U = sum(u)
        assert len(u) <= RESIZE_AA_MAX_TAPS and U <= 1 << 26, (n_src, n_rs, n_out, i)
        start[i], count[i] = lo, len(u)
        ws.extend(np.float32(np.float64(v) / np.float64(U)) for v in u)
    return start, count, np.array(ws, np.float32)


def _taps_f32(v: np.ndarray, axis: int, start, count, w) -> np.ndarray:
    """The tap sum along ``axis`` of v: per output index i the value itself where count == 1 (a
    bit copy), else ``w0 * v0`` (one binary32 multiply) followed by ``fmaf(wk, vk, acc)`` for
    k = 1 .. count - 1 in ascending order."""
    v = np.moveaxis(v, axis, -1)
    offs = np.concatenate(([0], np.cumsum(count)[:-1])).astype(np.int64)
    start = start.astype(np.int64)
    first = v[..., start]
    with np.errstate(over="ignore", invalid="ignore"):
        acc = (first.astype(np.float64) * w[offs].astype(np.float64)).astype(np.float32)
        for j in range(1, int(count.max())):
            live = count > j
            if not live.any():
                break
            wj = np.where(live, w[np.minimum(offs + j, len(w) - 1)], np.float32(0))
            vj = np.where(live, v[..., np.where(live, start + j, start)], np.float32(0))
            acc = np.where(live, fma_f32(vj, wj.astype(np.float32), acc), acc)
    out = np.where(count == 1, first, acc).astype(np.float32)
    return np.moveaxis(out, -1, axis)


@dataclass(frozen=True)
class InputResize:
    """Bilinear resize (half-pixel centres, no antialiasing) of HS x WS source images to HR x WR
    and centre crop (floor offset) to the model's H x W, on the preprocessed fp32 NHWC values.

    The numerics are fixed to the bit (``codec::build_resize_tables`` / ``resize_crop_host`` and
    the ``resize_crop`` kernel mirror them): per output row y, with oy = (HR - H) // 2,
    ``num = (2 (y + oy) + 1) HS - HR``, ``den = 2 HR``; num < 0 -> (0, 0, w 0); else
    y0 = num // den, clamped (HS-1, HS-1, w 0) at the last row, else y1 = y0 + 1 and
    w = float32(rem / den). ``lerp(a, b, w)`` is a for w == 0, else ``fmaf(w, b - a, a)``;
    columns first, then rows.

    ``antialias=True`` replaces the two-tap lerp on both axes by the support-scaled triangle
    filter of PIL / torch ``antialias=True`` in the tap form of ``_aa_axis_table`` /
    ``_taps_f32`` (``codec::build_resize_aa_tables`` / ``resize_crop_aa_host`` and the
    ``resize_crop_aa`` kernel mirror it): columns first, the column sums rounded to binary32,
    then rows. Each axis must satisfy n_src <= 8 n_rs (at most 17 taps per entry)."""

    HS: int
    WS: int
    HR: int
    WR: int
    H: int
    W: int
    antialias: bool = False

    @classmethod
    def build(cls, H: int, W: int, size="", resize="", antialias=False) -> "InputResize":
        """From the option texts: ``size`` "HS,WS" (empty = the model's), ``resize`` "HR,WR" or
        "S" (torchvision Resize(S) on HS,WS; empty = the model's). ValueError names the option."""
        sz = parse_size(size, "input_size")
        if len(sz) == 1:
            raise ValueError(f"input_size: expected HS,WS, got {size!r}")
        HS, WS = sz if sz else (H, W)
        for v in (HS, WS):
            if not 1 <= v <= RESIZE_MAX:
                raise ValueError(f"input_size: {v} outside 1..{RESIZE_MAX}")
        rs = parse_size(resize, "input_resize")
        if len(rs) == 1:
            S = rs[0]
            if not 1 <= S <= RESIZE_MAX:
                raise ValueError(f"input_resize: {S} outside 1..{RESIZE_MAX}")
            if HS <= WS:
                HR, WR = S, S * WS // HS
            else:
                HR, WR = S * HS // WS, S
        else:
            HR, WR = rs if rs else (H, W)
        for v in (HR, WR):
            if not 1 <= v <= RESIZE_MAX:
                raise ValueError(f"input_resize: {v} outside 1..{RESIZE_MAX}")
        if HR < H or WR < W:
            raise ValueError(f"input_resize: {HR},{WR} is smaller than the model's {H},{W} "
                             "(no padding)")
        rs = cls(HS=HS, WS=WS, HR=HR, WR=WR, H=H, W=W, antialias=bool(antialias))
        if rs.antialias:
            if not rs.active:
                raise ValueError("input_antialias: needs an input resize (--input-size / "
                                 "--input-resize are the model's size)")
            rs._check_aa_limit()
        return rs

    def _check_aa_limit(self) -> None:
        for n_src, n_rs in ((self.HS, self.HR), (self.WS, self.WR)):
            if n_src > RESIZE_AA_MAX_SCALE * n_rs:
                raise ValueError(f"input_antialias: {n_src} -> {n_rs} is a downscale of more "
                                 f"than {RESIZE_AA_MAX_SCALE}x")

    @property
    def active(self) -> bool:
        return (self.HS, self.WS, self.HR, self.WR) != (self.H, self.W, self.H, self.W)

    def engine_entries(self) -> Dict[str, Any]:
        if not self.active:
            return {}
        d = dict(rec_H=self.HS, rec_W=self.WS, resize_H=self.HR, resize_W=self.WR)
        if self.antialias:
            d["resize_antialias"] = 1
        return d

    def tables(self):
        """(y0, y1, wy, x0, x1, wx): int32 / int32 / float32 per output row, then per column."""
        return (*_axis_table(self.HS, self.HR, self.H), *_axis_table(self.WS, self.WR, self.W))

    def aa_tables(self):
        """(ys, yn, wy, xs, xn, wx) of the antialiased filter: int32 [H] first tap and tap count
        and the float32 weights of all rows concatenated in row order (row y starts at
        ``yn[:y].sum()``), then the same per column."""
        self._check_aa_limit()
        return (*_aa_axis_table(self.HS, self.HR, self.H),
                *_aa_axis_table(self.WS, self.WR, self.W))

    def apply(self, x):
        """The numpy oracle: [..., HS, WS, C] fp32 (numpy or torch) -> [..., H, W, C]."""
        is_torch = hasattr(x, "numpy") and not isinstance(x, np.ndarray)
        xv = x.detach().cpu().numpy() if is_torch else np.asarray(x)
        xv = xv.astype(np.float32, copy=False)
        if xv.ndim < 3 or xv.shape[-3:-1] != (self.HS, self.WS):
            raise ValueError(f"expected [..., {self.HS}, {self.WS}, C], got {xv.shape}")
        if self.antialias:
            ys, yn, wy, xs, xn, wx = self.aa_tables()
            out = _taps_f32(_taps_f32(xv, -2, xs, xn, wx), -3, ys, yn, wy)
            out = np.ascontiguousarray(out)
        else:
            y0, y1, wy, x0, x1, wx = self.tables()
            r0, r1 = xv[..., y0, :, :], xv[..., y1, :, :]
            wxc = wx[:, None]
            t = _lerp_f32(r0[..., x0, :], r0[..., x1, :], wxc)
            u = _lerp_f32(r1[..., x0, :], r1[..., x1, :], wxc)
            out = _lerp_f32(t, u, wy[:, None, None])
        if is_torch:
            import torch

            return torch.from_numpy(out)
        return out


PIXEL_FORMATS = ("rgb", "i420", "nv12")
YUV_MATRICES = ("bt601", "bt709")
YUV_RANGES = ("limited", "full")
YUV_SHIFT = 20  # the coefficients' fixed point


@functools.lru_cache(maxsize=None)
def _yuv_rationals(matrix: str, range_: str):
    """(sy, crv, cgu, cgv, cbu) of the real-valued matrix, as exact fractions."""
    from fractions import Fraction as F

    kr, kb = {"bt601": (F(299, 1000), F(114, 1000)),
              "bt709": (F(2126, 10000), F(722, 10000))}[matrix]
    kg = 1 - kr - kb
    sy, sc = {"limited": (F(255, 219), F(255, 224)), "full": (F(1), F(1))}[range_]
    return (sy, 2 * (1 - kr) * sc, -2 * kb * (1 - kb) / kg * sc, -2 * kr * (1 - kr) / kg * sc,
            2 * (1 - kb) * sc)


def _round_half_even(q) -> int:
    n, d = q.numerator, q.denominator
    fl, rem = divmod(n, d)
    if 2 * rem > d or (2 * rem == d and fl % 2):
        return fl + 1
    return fl


@dataclass(frozen=True)
class YuvConvert:
    """YUV 4:2:0 frames (``--input-pixel-format i420 | nv12``) to RGB, in integers.

    A frame of HS x WS pixels (both even) is ``B = HS*WS*3/2`` bytes: I420 ``Y[HS][WS]``,
    ``U[HS/2][WS/2]``, ``V[HS/2][WS/2]``; NV12 ``Y[HS][WS]``, ``UV[HS/2][WS/2][2]``. Pixel (y, x)
    takes ``Y[y][x]`` and the chroma sample ``(y >> 1, x >> 1)`` (nearest neighbour). With
    ``yo = 16`` (limited) or 0 (full), in signed 32-bit arithmetic (``>>``: arithmetic shift)::

        R = clamp((cy (Y - yo)                  + crv (V - 128) + 2^19) >> 20, 0, 255)
        G = clamp((cy (Y - yo) + cgu (U - 128) + cgv (V - 128) + 2^19) >> 20, 0, 255)
        B = clamp((cy (Y - yo) + cbu (U - 128)                  + 2^19) >> 20, 0, 255)

    The coefficients are the exact rationals ``sy``, ``2(1-Kr) sc``, ``-2Kb(1-Kb)/Kg sc``,
    ``-2Kr(1-Kr)/Kg sc``, ``2(1-Kb) sc`` times 2^20, rounded half to even (Kg = 1 - Kr - Kb;
    bt601 Kr, Kb = 0.299, 0.114; bt709 0.2126, 0.0722; limited sy = 255/219, sc = 255/224; full
    1, 1). ``codec::yuv420_to_rgb_host`` (csrc/codec/yuv.h, which holds them as literals) and the
    ``b64_yuv_instances`` kernel give the same bits. There is no pre-clamp of ``Y - yo``."""

    format: str = "i420"
    matrix: str = "bt601"
    range: str = "limited"

    def __post_init__(self):
        if self.format not in PIXEL_FORMATS[1:]:
            raise ValueError(f"input_pixel_format={self.format!r}: expected one of "
                             f"{PIXEL_FORMATS[1:]} for a YUV conversion")
        if self.matrix not in YUV_MATRICES:
            raise ValueError(f"input_yuv_matrix={self.matrix!r}: expected one of {YUV_MATRICES}")
        if self.range not in YUV_RANGES:
            raise ValueError(f"input_yuv_range={self.range!r}: expected one of {YUV_RANGES}")

    @classmethod
    def from_config(cls, cfg) -> Optional["YuvConvert"]:
        """The conversion of a configuration, None for ``rgb``. (GaleConfig.validate refuses the
        combinations that have none.)"""
        if cfg.input_pixel_format not in PIXEL_FORMATS[1:]:  # (rgb, or a PixelUnpack format)
            return None
        return cls(cfg.input_pixel_format, cfg.input_yuv_matrix or "bt601",
                   cfg.input_yuv_range or "limited")

    def rationals(self):
        return _yuv_rationals(self.matrix, self.range)

    @property
    def yo(self) -> int:
        return 16 if self.range == "limited" else 0

    def coeffs(self) -> Tuple[int, int, int, int, int]:
        """(cy, crv, cgu, cgv, cbu)."""
        return tuple(_round_half_even(q * (1 << YUV_SHIFT)) for q in self.rationals())

    @staticmethod
    def frame_bytes(HS: int, WS: int) -> int:
        if HS <= 0 or WS <= 0 or HS % 2 or WS % 2:
            raise ValueError(f"a 4:2:0 frame needs even, positive sizes, got {HS},{WS}")
        return HS * WS * 3 // 2

    def engine_entries(self) -> Dict[str, Any]:
        return dict(pixel_format=self.format, yuv_matrix=self.matrix, yuv_range=self.range)

    def kernel_kwargs(self) -> Dict[str, Any]:
        """Keyword arguments of the ``b64_yuv_instances`` binding."""
        return dict(format=self.format, coeffs=[*self.coeffs(), self.yo])

    def accumulators(self, Y, U, V):
        """The three int64 accumulators (rounding term included) of int arrays Y, U, V."""
        cy, crv, cgu, cgv, cbu = self.coeffs()
        Y, U, V = (np.asarray(v).astype(np.int64) for v in (Y, U, V))
        yy = cy * (Y - self.yo) + (1 << (YUV_SHIFT - 1))
        u, v = U - 128, V - 128
        return yy + crv * v, yy + cgu * u + cgv * v, yy + cbu * u

    def planes(self, frame, HS: int, WS: int):
        """uint8 [..., B] frames -> (Y [..., HS, WS], U, V [..., HS/2, WS/2])."""
        B = self.frame_bytes(HS, WS)
        f = np.asarray(frame, np.uint8)
        if f.shape[-1] != B:
            raise ValueError(f"expected [..., {B}] bytes, got {f.shape}")
        lead, hw = f.shape[:-1], HS * WS
        Y = f[..., :hw].reshape(*lead, HS, WS)
        if self.format == "nv12":
            uv = f[..., hw:].reshape(*lead, HS // 2, WS // 2, 2)
            return Y, uv[..., 0], uv[..., 1]
        U = f[..., hw:hw + hw // 4].reshape(*lead, HS // 2, WS // 2)
        V = f[..., hw + hw // 4:].reshape(*lead, HS // 2, WS // 2)
        return Y, U, V

    def apply(self, frame, HS: int, WS: int) -> np.ndarray:
        """The numpy oracle: uint8 [..., B] frames -> uint8 [..., HS, WS, 3] RGB."""
        Y, U, V = self.planes(frame, HS, WS)
        up = lambda c: np.repeat(np.repeat(c, 2, axis=-2), 2, axis=-1)  # noqa: E731
        acc = self.accumulators(Y, up(U), up(V))
        assert all(np.abs(a).max(initial=0) < 1 << 31 for a in acc)
        return np.stack([np.clip(a >> YUV_SHIFT, 0, 255) for a in acc], axis=-1).astype(np.uint8)


# the packed formats: name -> (bytes per pixel, byte offset in a pixel of R, G, B)
PACKED_FORMATS = {"bgr24": (3, (2, 1, 0)), "rgba": (4, (0, 1, 2)), "bgra": (4, (2, 1, 0)),
                  "gray": (1, (0, 0, 0))}


@dataclass(frozen=True)
class PixelUnpack:
    """Packed pixels (``--input-pixel-format bgr24 | rgba | bgra | gray``) to interleaved RGB.

    An image of HS x WS pixels (any positive sizes) is ``B = HS*WS*P`` bytes, pixels in
    ``[HS][WS]`` order, P bytes per pixel::

        bgr24  P = 3   B, G, R       RGB = (byte 2, byte 1, byte 0)
        rgba   P = 4   R, G, B, A    RGB = (byte 0, byte 1, byte 2)
        bgra   P = 4   B, G, R, A    RGB = (byte 2, byte 1, byte 0)
        gray   P = 1   Y             RGB = (byte 0, byte 0, byte 0)

    Alpha is ignored: not composited, not un-premultiplied (PIL's ``convert("RGB")``). The names
    are ffmpeg's ``pix_fmt``s. ``codec::packed_to_rgb_host`` (csrc/codec/pixfmt.h) and the
    ``b64_packed_instances`` kernel give the same bytes; the ``InputPrep`` coefficients that
    follow are indexed by model channel (R, G, B), whatever the order on the wire."""

    format: str = "bgr24"

    def __post_init__(self):
        if self.format not in PACKED_FORMATS:
            raise ValueError(f"input_pixel_format={self.format!r}: expected one of "
                             f"{tuple(PACKED_FORMATS)} for a packed format")

    @classmethod
    def from_config(cls, cfg) -> Optional["PixelUnpack"]:
        """The unpack of a configuration, None for ``rgb`` and the YUV formats. (GaleConfig.validate
        refuses the combinations that have none.)"""
        if cfg.input_pixel_format not in PACKED_FORMATS:
            return None
        return cls(cfg.input_pixel_format)

    @property
    def bytes_per_pixel(self) -> int:
        return PACKED_FORMATS[self.format][0]

    @property
    def offsets(self) -> Tuple[int, int, int]:
        """Byte offset in a pixel of model channels R, G, B."""
        return PACKED_FORMATS[self.format][1]

    def frame_bytes(self, HS: int, WS: int) -> int:
        if HS <= 0 or WS <= 0:
            raise ValueError(f"an image needs positive sizes, got {HS},{WS}")
        return HS * WS * self.bytes_per_pixel

    def engine_entries(self) -> Dict[str, Any]:
        return dict(pixel_format=self.format)

    def kernel_kwargs(self) -> Dict[str, Any]:
        """Keyword arguments of the ``b64_packed_instances`` binding."""
        return dict(format=self.format)

    def apply(self, frame, HS: int, WS: int) -> np.ndarray:
        """The numpy oracle: uint8 [..., B] images -> uint8 [..., HS, WS, 3] RGB."""
        B = self.frame_bytes(HS, WS)
        f = np.asarray(frame, np.uint8)
        if f.shape[-1] != B:
            raise ValueError(f"expected [..., {B}] bytes, got {f.shape}")
        px = f.reshape(*f.shape[:-1], HS, WS, self.bytes_per_pixel)
        return np.ascontiguousarray(px[..., list(self.offsets)])


# the element types of a typed tensor record: name -> (bytes per element, numpy wire dtype)
ELEM_TYPES = {"u8": (1, "u1"), "u16": (2, "<u2"), "f16": (2, "<f2"), "bf16": (2, "<u2"),
              "f32": (4, "<f4")}


@dataclass(frozen=True)
class ElemType:
    """The element type of ``rgb`` b64 strings (``--input-dtype u8 | u16 | f16 | bf16 | f32``).

    A string is the image's ``HS*WS*C`` elements, little-endian, ``E`` bytes each, in ``[H][W][C]``
    order (``[C][H][W]`` with ``--input-layout nchw``)::

        u8    E = 1   the plain b64 record
        u16   E = 2   unsigned
        f16   E = 2   IEEE binary16
        bf16  E = 2   the top 16 bits of binary32
        f32   E = 4   binary32

    The model input of element x at channel c is ``fma(float32(x), a[c], b[c])`` with the
    ``InputPrep`` coefficients; ``float32(x)`` is exact for every type (f16 subnormals included),
    and with the identity prep the float32 bits are stored as they are. An f16 / bf16 / f32 element
    whose exponent field is all ones (Inf, NaN) makes its record ``bad_number``, judged on the
    element as sent. ``codec::typed_to_float_host`` (csrc/codec/elemtype.h) and the
    ``b64_typed_instances`` kernel give the same bits."""

    dtype: str = "u8"

    def __post_init__(self):
        if self.dtype not in ELEM_TYPES:
            raise ValueError(f"input_dtype={self.dtype!r}: expected one of {tuple(ELEM_TYPES)}")

    @classmethod
    def from_config(cls, cfg) -> Optional["ElemType"]:
        """The element type of a configuration, None for ``u8``. (GaleConfig.validate refuses the
        combinations that have none.)"""
        if cfg.input_dtype == "u8":
            return None
        return cls(cfg.input_dtype)

    @property
    def bytes_per_element(self) -> int:
        return ELEM_TYPES[self.dtype][0]

    def frame_bytes(self, HS: int, WS: int, C: int) -> int:
        if HS <= 0 or WS <= 0 or C <= 0:
            raise ValueError(f"a tensor needs positive sizes, got {HS},{WS},{C}")
        return HS * WS * C * self.bytes_per_element

    def engine_entries(self) -> Dict[str, Any]:
        return dict(input_dtype=self.dtype)

    def kernel_kwargs(self) -> Dict[str, Any]:
        """Keyword arguments of the ``b64_typed_instances`` binding."""
        return dict(dtype=self.dtype)

    def to_float(self, data) -> np.ndarray:
        """uint8 [..., n * E] wire bytes -> float32 [..., n]: ``float32(x)`` of every element."""
        raw = np.ascontiguousarray(np.asarray(data, np.uint8))
        E = self.bytes_per_element
        if raw.shape[-1] % E:
            raise ValueError(f"expected whole {self.dtype} elements, got {raw.shape[-1]} bytes")
        v = raw.view(ELEM_TYPES[self.dtype][1])
        if self.dtype == "bf16":
            return (v.astype(np.uint32) << 16).view(np.float32)
        return v.astype(np.float32)

    def nonfinite(self, data) -> np.ndarray:
        """bool [..., n]: the elements with an all-ones exponent field (never for u8 / u16)."""
        x = self.to_float(data)
        if self.dtype in ("u8", "u16"):
            return np.zeros(x.shape, bool)
        return ~np.isfinite(x)

    def to_wire(self, x) -> np.ndarray:
        """float [...] values -> uint8 [..., E] wire bytes of each, rounded to the type (nearest
        even; the integer types round and saturate): what a client holding ``x`` sends."""
        x = np.asarray(x, np.float32)
        if self.dtype in ("u8", "u16"):
            hi = 255 if self.dtype == "u8" else 65535
            v = np.clip(np.rint(x), 0, hi).astype(ELEM_TYPES[self.dtype][1])
        elif self.dtype == "bf16":
            b = np.ascontiguousarray(x).view(np.uint32).astype(np.uint64)
            v = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype("<u2")  # (finite x: no NaN care)
        else:
            with np.errstate(over="ignore"):
                v = x.astype(ELEM_TYPES[self.dtype][1])
        v = np.ascontiguousarray(v)
        return v.view(np.uint8).reshape(*v.shape, self.bytes_per_element)

    def apply(self, data, HS: int, WS: int, C: int, prep: Optional[InputPrep] = None) -> np.ndarray:
        """The numpy oracle: uint8 [..., B] strings' bytes -> float32 [..., HS, WS, C] model
        inputs (NHWC, whatever the prep's layout): the exact conversion, then ``prep.apply``."""
        B = self.frame_bytes(HS, WS, C)
        raw = np.asarray(data, np.uint8)
        if raw.shape[-1] != B:
            raise ValueError(f"expected [..., {B}] bytes, got {raw.shape}")
        x = self.to_float(raw)
        lead = x.shape[:-1]
        if prep is not None and prep.nchw:
            x = np.moveaxis(x.reshape(*lead, C, HS, WS), -3, -1)
        else:
            x = x.reshape(*lead, HS, WS, C)
        x = np.ascontiguousarray(x)
        if prep is None or prep.identity:
            return x
        return prep.apply(x)


def prep_or_none(prep: Optional[InputPrep]) -> Optional[InputPrep]:
    return None if prep is None or prep.identity else prep
