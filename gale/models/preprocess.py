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

    FORMATS = PIXEL_FORMATS[1:]  # (the formats of this layout; Yuv422Convert has its own)
    format: str = "i420"
    matrix: str = "bt601"
    range: str = "limited"

    def __post_init__(self):
        if self.format not in self.FORMATS:
            raise ValueError(f"input_pixel_format={self.format!r}: expected one of "
                             f"{self.FORMATS} for a YUV conversion")
        if self.matrix not in YUV_MATRICES:
            raise ValueError(f"input_yuv_matrix={self.matrix!r}: expected one of {YUV_MATRICES}")
        if self.range not in YUV_RANGES:
            raise ValueError(f"input_yuv_range={self.range!r}: expected one of {YUV_RANGES}")

    @classmethod
    def from_config(cls, cfg) -> Optional["YuvConvert"]:
        """The conversion of a configuration, None for ``rgb``. (GaleConfig.validate refuses the
        combinations that have none.)"""
        if cfg.input_pixel_format not in cls.FORMATS:  # (rgb, or another class's format)
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


YUV_CHROMA = ("nearest", "linear")


@dataclass(frozen=True)
class YuvLinearConvert(YuvConvert):
    """``YuvConvert`` with triangle-filtered chroma (``--input-yuv-chroma linear``): libjpeg's
    ``h2v2_fancy_upsample``, a centre-sited 3:1 filter in both directions, in integers.

    For output pixel (y, x) and a chroma plane ``C`` of ``HS/2 x WS/2``::

        cy0 = y >> 1     cyn = clamp(cy0 + (y & 1 ? +1 : -1), 0, HS/2 - 1)
        cx0 = x >> 1     cxn = clamp(cx0 + (x & 1 ? +1 : -1), 0, WS/2 - 1)
        col(cx) = 3 C[cy0][cx] + C[cyn][cx]
        C'(y, x) = (3 col(cx0) + col(cxn) + (x & 1 ? 7 : 8)) >> 4

    ``U'`` and ``V'`` then go with ``Y[y][x]`` through ``YuvConvert``'s formulas unchanged, so a
    frame gives the bits of a ``yuv444p`` frame that carries ``(Y, U', V')``.
    ``codec::yuv420_linear_to_rgb_host`` and the ``b64_yuv_linear_instances`` kernel give the same
    bits. b64 records only; WS at most ``YUV_LINEAR_MAX_WS`` (the kernel's LDS bound)."""

    def engine_entries(self) -> Dict[str, Any]:
        return dict(super().engine_entries(), yuv_chroma="linear")

    @staticmethod
    def upsample(C) -> np.ndarray:
        """uint8 [..., HS/2, WS/2] -> int64 [..., HS, WS]: the formulas above, directly."""
        C = np.asarray(C).astype(np.int64)
        ch, cw = C.shape[-2:]
        y, x = np.arange(2 * ch), np.arange(2 * cw)
        cyn = np.clip((y >> 1) + np.where(y & 1, 1, -1), 0, ch - 1)
        cxn = np.clip((x >> 1) + np.where(x & 1, 1, -1), 0, cw - 1)
        col = 3 * C[..., y >> 1, :] + C[..., cyn, :]
        return (3 * col[..., x >> 1] + col[..., cxn] + np.where(x & 1, 7, 8)) >> 4

    def apply(self, frame, HS: int, WS: int) -> np.ndarray:
        """The numpy oracle: uint8 [..., B] frames -> uint8 [..., HS, WS, 3] RGB."""
        Y, U, V = self.planes(frame, HS, WS)
        acc = self.accumulators(Y, self.upsample(U), self.upsample(V))
        assert all(np.abs(a).max(initial=0) < 1 << 31 for a in acc)
        return np.stack([np.clip(a >> YUV_SHIFT, 0, 255) for a in acc], axis=-1).astype(np.uint8)


YUV_LINEAR_MAX_WS = 8186  # (csrc/codec/yuv.h kYuv420LinearMaxWS)

# the packed 4:2:2 formats: name -> byte offset in a macropixel of (Y0, Y1, U, V)
YUV422_FORMATS = {"yuyv422": (0, 2, 1, 3), "uyvy422": (1, 3, 0, 2)}


@dataclass(frozen=True)
class Yuv422Convert(YuvConvert):
    """Packed YUV 4:2:2 frames (``--input-pixel-format yuyv422 | uyvy422``) to RGB: the integer
    conversion of ``YuvConvert`` - same formulas, coefficient tables, ``yo``, no pre-clamp - on
    another frame layout.

    A frame of HS x WS pixels (WS even, HS any) is ``B = 2*HS*WS`` bytes, ``[HS][WS/2]``
    macropixels of 4 bytes: yuyv422 ``Y0 U Y1 V``, uyvy422 ``U Y0 V Y1``. Pixel (y, x) takes
    ``Y[x & 1]``, ``U`` and ``V`` of macropixel ``(y, x >> 1)``: the horizontal half of the 4:2:0
    rule (nearest chroma, no siting filter). ``codec::yuv422_to_rgb_host`` (csrc/codec/yuv.h) and
    the ``b64_yuv422_instances`` / ``raw_yuv422_instances`` kernels give the same bits."""

    FORMATS = tuple(YUV422_FORMATS)
    format: str = "yuyv422"

    @staticmethod
    def frame_bytes(HS: int, WS: int) -> int:
        if HS <= 0 or WS <= 0 or WS % 2:
            raise ValueError(f"a 4:2:2 frame needs positive sizes and an even WS, got {HS},{WS}")
        return HS * WS * 2

    def kernel_kwargs(self) -> Dict[str, Any]:
        """Keyword arguments of the ``b64_yuv422_instances`` / ``raw_yuv422_instances``
        bindings."""
        return dict(format=self.format, coeffs=[*self.coeffs(), self.yo])

    def planes(self, frame, HS: int, WS: int):
        """uint8 [..., B] frames -> (Y [..., HS, WS], U, V [..., HS, WS/2])."""
        B = self.frame_bytes(HS, WS)
        f = np.asarray(frame, np.uint8)
        if f.shape[-1] != B:
            raise ValueError(f"expected [..., {B}] bytes, got {f.shape}")
        mp = f.reshape(*f.shape[:-1], HS, WS // 2, 4)
        y0, y1, u, v = YUV422_FORMATS[self.format]
        Y = np.stack([mp[..., y0], mp[..., y1]], axis=-1).reshape(*f.shape[:-1], HS, WS)
        return Y, mp[..., u], mp[..., v]

    def apply(self, frame, HS: int, WS: int) -> np.ndarray:
        """The numpy oracle: uint8 [..., B] frames -> uint8 [..., HS, WS, 3] RGB."""
        Y, U, V = self.planes(frame, HS, WS)
        acc = self.accumulators(Y, np.repeat(U, 2, axis=-1), np.repeat(V, 2, axis=-1))
        assert all(np.abs(a).max(initial=0) < 1 << 31 for a in acc)
        return np.stack([np.clip(a >> YUV_SHIFT, 0, 255) for a in acc], axis=-1).astype(np.uint8)


# the planar 4:2:2 / 4:4:4 formats: name -> horizontal chroma shift s
YUVP_FORMATS = {"yuv422p": 1, "yuv444p": 0}


@dataclass(frozen=True)
class YuvPlanarConvert(YuvConvert):
    """Planar YUV 4:2:2 / 4:4:4 frames (``--input-pixel-format yuv422p | yuv444p``, what a JPEG
    decoder hands back) to RGB: the integer conversion of ``YuvConvert`` - same formulas,
    coefficient tables, ``yo``, no pre-clamp - on another frame layout.

    With s = 1 (yuv422p, WS even) or 0 (yuv444p, any WS) and any HS, a frame is ``Y[HS][WS]``,
    ``U[HS][WS >> s]``, ``V[HS][WS >> s]``, ``B = HS*WS + 2*(HS*WS >> s)`` bytes. Pixel (y, x)
    takes ``Y[y][x]``, ``U[y][x >> s]``, ``V[y][x >> s]`` (nearest chroma, no siting filter).
    ``codec::yuvp_to_rgb_host`` (csrc/codec/yuv.h) and the ``b64_yuvp_instances`` /
    ``raw_yuvp_instances`` kernels give the same bits."""

    FORMATS = tuple(YUVP_FORMATS)
    format: str = "yuv444p"

    @property
    def shift(self) -> int:
        return YUVP_FORMATS[self.format]

    def frame_bytes(self, HS: int, WS: int) -> int:
        if HS <= 0 or WS <= 0 or WS % (1 << self.shift):
            raise ValueError(f"a {self.format} frame needs positive sizes"
                             f"{' and an even WS' if self.shift else ''}, got {HS},{WS}")
        return HS * WS + 2 * (HS * (WS >> self.shift))

    def kernel_kwargs(self) -> Dict[str, Any]:
        """Keyword arguments of the ``b64_yuvp_instances`` / ``raw_yuvp_instances`` bindings."""
        return dict(format=self.format, coeffs=[*self.coeffs(), self.yo])

    def planes(self, frame, HS: int, WS: int):
        """uint8 [..., B] frames -> (Y [..., HS, WS], U, V [..., HS, WS >> s])."""
        B = self.frame_bytes(HS, WS)
        f = np.asarray(frame, np.uint8)
        if f.shape[-1] != B:
            raise ValueError(f"expected [..., {B}] bytes, got {f.shape}")
        lead, hw, wc = f.shape[:-1], HS * WS, WS >> self.shift
        return (f[..., :hw].reshape(*lead, HS, WS), f[..., hw:hw + HS * wc].reshape(*lead, HS, wc),
                f[..., hw + HS * wc:].reshape(*lead, HS, wc))

    def apply(self, frame, HS: int, WS: int) -> np.ndarray:
        """The numpy oracle: uint8 [..., B] frames -> uint8 [..., HS, WS, 3] RGB."""
        Y, U, V = self.planes(frame, HS, WS)
        up = lambda c: np.repeat(c, 1 << self.shift, axis=-1)  # noqa: E731
        acc = self.accumulators(Y, up(U), up(V))
        assert all(np.abs(a).max(initial=0) < 1 << 31 for a in acc)
        return np.stack([np.clip(a >> YUV_SHIFT, 0, 255) for a in acc], axis=-1).astype(np.uint8)


# the 10-bit 4:2:0 formats: name -> right shift of a 16-bit word to its sample
YUV420_HI_FORMATS = {"p010le": 6, "yuv420p10le": 0}
YUV10_SHIFT = 18  # their coefficients' fixed point: 2^20 overflows 32 bits with 10-bit samples


@dataclass(frozen=True)
class Yuv420HiConvert(YuvConvert):
    """Raw 10-bit YUV 4:2:0 frames (``--input-pixel-format p010le | yuv420p10le``) to RGB, in
    integers, in quarter steps of the 8-bit scale.

    A frame of HS x WS pixels (both even) is ``B = 3*HS*WS`` bytes of little-endian 16-bit words:
    p010le ``Y[HS][WS]``, ``UV[HS/2][WS/2][2]`` with the sample in the top ten bits (``word >> 6``);
    yuv420p10le ``Y[HS][WS]``, ``U[HS/2][WS/2]``, ``V[HS/2][WS/2]`` with it in the low ten
    (``word & 1023``). Pixel (y, x) takes ``Y[y][x]`` and chroma ``(y >> 1, x >> 1)``. With
    ``yo = 64`` (limited) or 0 (full), in signed 32-bit arithmetic::

        q_R = clamp((cy (Y - yo)                  + crv (V - 512) + 2^17) >> 18, 0, 1020)
        q_G = clamp((cy (Y - yo) + cgu (U - 512) + cgv (V - 512) + 2^17) >> 18, 0, 1020)
        q_B = clamp((cy (Y - yo) + cbu (U - 512)                  + 2^17) >> 18, 0, 1020)

    and the model input of channel c is ``fmaf(float(q) * 0.25f, a[c], b[c])``: the range
    [0, 255] of an 8-bit record, with two more bits. The coefficients are ``YuvConvert``'s
    rationals (limited: sy = 255/219, sc = 255/224, since 64 .. 940 is 4 x (16 .. 235); full:
    sy = sc = 1020/1023) times 2^18, rounded half to even. ``codec::yuv420p10_to_rgb_host``
    (csrc/codec/yuv.h, which holds them as literals) and the ``raw_yuv420p10_instances`` kernel
    give the same bits."""

    FORMATS = tuple(YUV420_HI_FORMATS)
    format: str = "p010le"

    def rationals(self):
        from fractions import Fraction as F

        r = _yuv_rationals(self.matrix, self.range)  # (full: sy = sc = 1)
        return r if self.range == "limited" else tuple(q * F(1020, 1023) for q in r)

    @property
    def yo(self) -> int:
        return 64 if self.range == "limited" else 0

    def coeffs(self) -> Tuple[int, int, int, int, int]:
        """(cy, crv, cgu, cgv, cbu) at the scale 2^18."""
        return tuple(_round_half_even(q * (1 << YUV10_SHIFT)) for q in self.rationals())

    @staticmethod
    def frame_bytes(HS: int, WS: int) -> int:
        if HS <= 0 or WS <= 0 or HS % 2 or WS % 2:
            raise ValueError(f"a 4:2:0 frame needs even, positive sizes, got {HS},{WS}")
        return HS * WS * 3

    def kernel_kwargs(self) -> Dict[str, Any]:
        """Keyword arguments of the ``raw_yuv420p10_instances`` binding."""
        return dict(format=self.format, coeffs=[*self.coeffs(), self.yo])

    def accumulators(self, Y, U, V):
        """The three int64 accumulators (rounding term included) of 10-bit int arrays Y, U, V."""
        cy, crv, cgu, cgv, cbu = self.coeffs()
        Y, U, V = (np.asarray(v).astype(np.int64) for v in (Y, U, V))
        yy = cy * (Y - self.yo) + (1 << (YUV10_SHIFT - 1))
        u, v = U - 512, V - 512
        return yy + crv * v, yy + cgu * u + cgv * v, yy + cbu * u

    def planes(self, frame, HS: int, WS: int):
        """uint8 [..., B] frames -> 10-bit samples (Y [..., HS, WS], U, V [..., HS/2, WS/2])."""
        B = self.frame_bytes(HS, WS)
        f = np.ascontiguousarray(np.asarray(frame, np.uint8))
        if f.shape[-1] != B:
            raise ValueError(f"expected [..., {B}] bytes, got {f.shape}")
        w = (f.view("<u2") >> YUV420_HI_FORMATS[self.format]) & 1023
        lead, hw = f.shape[:-1], HS * WS
        Y = w[..., :hw].reshape(*lead, HS, WS)
        if self.format == "p010le":
            uv = w[..., hw:].reshape(*lead, HS // 2, WS // 2, 2)
            return Y, uv[..., 0], uv[..., 1]
        return (Y, w[..., hw:hw + hw // 4].reshape(*lead, HS // 2, WS // 2),
                w[..., hw + hw // 4:].reshape(*lead, HS // 2, WS // 2))

    def apply(self, frame, HS: int, WS: int) -> np.ndarray:
        """The numpy oracle: uint8 [..., B] frames -> uint16 [..., HS, WS, 3] quarter steps q."""
        Y, U, V = self.planes(frame, HS, WS)
        up = lambda c: np.repeat(np.repeat(c, 2, axis=-2), 2, axis=-1)  # noqa: E731
        acc = self.accumulators(Y, up(U), up(V))
        assert all(np.abs(a).max(initial=0) < 1 << 31 for a in acc)
        return np.stack([np.clip(a >> YUV10_SHIFT, 0, 1020) for a in acc],
                        axis=-1).astype(np.uint16)

    @staticmethod
    def to_float(q, prep=None) -> np.ndarray:
        """The model-side floats of quarter steps q: ``fmaf(float(q) * 0.25f, a[c], b[c])`` with
        the coefficients of ``prep`` (an ``InputPrep``; None: the identity). The product by 0.25
        is exact, so this is ``prep.apply`` of it."""
        x = np.asarray(q).astype(np.float32) * np.float32(0.25)
        return x if prep is None else prep.apply(x)


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


# the Bayer orders: name -> (site (0, 0) is green, the even rows' non-green colour is blue)
BAYER_FORMATS = {"bayer_rggb8": (False, False), "bayer_bggr8": (False, True),
                 "bayer_grbg8": (True, False), "bayer_gbrg8": (True, True)}
BAYER_DEMOSAICS = ("bilinear", "malvar", "hamilton")


def _hamilton_green(p: np.ndarray):
    """The edge-directed green of ``BayerConvert``'s hamilton rule at every position of ``p`` two
    or more from its border, as if each were an R / B site: (the unclamped estimate, the choice
    1 = gH, 2 = gV, 3 = gA), int arrays [..., H - 4, W - 4]."""
    H, W = p.shape[-2:]
    at = lambda dy, dx: p[..., 2 + dy:H - 2 + dy, 2 + dx:W - 2 + dx]  # noqa: E731
    s = at(0, 0)
    hs, hd = at(0, -1) + at(0, 1), 2 * s - at(0, -2) - at(0, 2)
    vs, vd = at(-1, 0) + at(1, 0), 2 * s - at(-2, 0) - at(2, 0)
    dh = np.abs(at(0, -1) - at(0, 1)) + np.abs(hd)
    dv = np.abs(at(-1, 0) - at(1, 0)) + np.abs(vd)
    choice = np.where(dh < dv, 1, np.where(dv < dh, 2, 3))
    g = np.where(choice == 1, (2 * hs + hd + 2) >> 2,
                 np.where(choice == 2, (2 * vs + vd + 2) >> 2,
                          (2 * (hs + vs) + hd + vd + 4) >> 3))
    return g, choice


def _demosaic(s: np.ndarray, green_first: bool, blue_first: bool, demosaic: str,
              M: int) -> np.ndarray:
    """Integer samples [..., HS, WS] of 0 .. M -> RGB [..., HS, WS, 3] by the rules that
    ``BayerConvert`` writes out; ``M`` is the clamp of the malvar and hamilton filters."""
    HS, WS = s.shape[-2:]
    y, x = np.ogrid[:HS, :WS]
    green = ((x + y) & 1 == 1) != green_first
    lead = [(0, 0)] * (s.ndim - 2)
    if demosaic == "hamilton":
        if HS < 4 or WS < 4:
            raise ValueError(f"the hamilton demosaic needs HS, WS >= 4, got {HS},{WS}")
        # S reflected two deep; K = S - G^ at R / B sites (0 elsewhere, never read) one deep
        cross = np.clip(_hamilton_green(np.pad(s, lead + [(2, 2), (2, 2)], mode="reflect"))[0], 0, M)
        kp = np.pad(np.where(green, 0, s - cross), lead + [(1, 1), (1, 1)], mode="reflect")
        k = lambda dy, dx: kp[..., 1 + dy:1 + dy + HS, 1 + dx:1 + dx + WS]  # noqa: E731
        h = np.clip(s + ((k(0, -1) + k(0, 1) + 1) >> 1), 0, M)
        v = np.clip(s + ((k(-1, 0) + k(1, 0) + 1) >> 1), 0, M)
        diag = np.clip(cross + ((k(-1, -1) + k(-1, 1) + k(1, -1) + k(1, 1) + 2) >> 2), 0, M)
    elif demosaic == "malvar":
        if HS < 4 or WS < 4:
            raise ValueError(f"the malvar demosaic needs HS, WS >= 4, got {HS},{WS}")
        # rows / columns -2, -1, n, n + 1 are rows / columns 2, 1, n - 2, n - 3
        p = np.pad(s, lead + [(2, 2), (2, 2)], mode="reflect")
        at = lambda dy, dx: p[..., 2 + dy:2 + dy + HS, 2 + dx:2 + dx + WS]  # noqa: E731
        q = lambda n: np.clip((n + 8) >> 4, 0, M)  # noqa: E731
        h1, h2 = at(0, -1) + at(0, 1), at(0, -2) + at(0, 2)
        v1, v2 = at(-1, 0) + at(1, 0), at(-2, 0) + at(2, 0)
        d = at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1)
        h = q(10 * s + 8 * h1 - 2 * d - 2 * h2 + v2)
        v = q(10 * s + 8 * v1 - 2 * d - 2 * v2 + h2)
        cross = q(8 * s + 4 * (h1 + v1) - 2 * (h2 + v2))
        diag = q(12 * s + 4 * d - 3 * (h2 + v2))
    else:
        # rows / columns -1 and n are rows / columns 1 and n - 2
        p = np.concatenate([s[..., 1:2, :], s, s[..., -2:-1, :]], axis=-2)
        p = np.concatenate([p[..., :, 1:2], p, p[..., :, -2:-1]], axis=-1)
        at = lambda dy, dx: p[..., 1 + dy:1 + dy + HS, 1 + dx:1 + dx + WS]  # noqa: E731
        h = (at(0, -1) + at(0, 1) + 1) >> 1
        v = (at(-1, 0) + at(1, 0) + 1) >> 1
        cross = (at(-1, 0) + at(1, 0) + at(0, -1) + at(0, 1) + 2) >> 2
        diag = (at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1) + 2) >> 2
    blue_row = (y & 1 == 1) != blue_first  # the row's non-green colour is blue
    own, opp = np.where(green, h, s), np.where(green, v, diag)
    return np.stack([np.where(blue_row, opp, own), np.where(green, s, cross),
                     np.where(blue_row, own, opp)], axis=-1)


@dataclass(frozen=True)
class BayerConvert:
    """Raw 8-bit Bayer mosaic frames (``--input-pixel-format bayer_rggb8 | bayer_bggr8 |
    bayer_grbg8 | bayer_gbrg8``) to interleaved RGB, in integers.

    A frame of HS x WS pixels (both even) is ``B = HS*WS`` bytes ``S[HS][WS]``; the name gives the
    colours of the tile (0,0) (0,1) / (1,0) (1,1). Indices outside the frame are mirrored without
    repeating the edge sample (-1 -> 1, n -> n - 2), which keeps a neighbour's colour parity.
    With ``s = S[y][x]`` and the eight neighbours at mirrored indices::

        R or B site:  own = s,  G = (N+S+E+W+2) >> 2,  opposite = (NW+NE+SW+SE+2) >> 2
        G site:       G = s,  this row's colour = (W+E+1) >> 1,  the other = (N+S+1) >> 1

    the usual rounded bilinear demosaic. ``codec::bayer_to_rgb_host`` (csrc/codec/bayer.h) and the
    ``raw_bayer_instances`` kernel give the same bytes; the ``InputPrep`` coefficients that
    follow are indexed by model channel (R, G, B): per-channel scales are white-balance gains.

    ``demosaic="malvar"`` (``--input-bayer-demosaic malvar``) is the 5 x 5 gradient-corrected
    linear filter of Malvar, He and Cutler (ICASSP 2004) instead, its four kernels times 2 so
    that every coefficient is an integer over 16. HS, WS >= 4; indices are reflected the same way
    two deep (-2 -> 2, -1 -> 1, n -> n - 2, n + 1 -> n - 3). With::

        H1 = S[y][x-1] + S[y][x+1]    H2 = S[y][x-2] + S[y][x+2]
        V1 = S[y-1][x] + S[y+1][x]    V2 = S[y-2][x] + S[y+2][x]
        D  = S[y-1][x-1] + S[y-1][x+1] + S[y+1][x-1] + S[y+1][x+1]
        q(n) = clamp((n + 8) >> 4, 0, 255)              (signed, >> arithmetic)

        R or B site:  own = s,  G = q(8s + 4(H1 + V1) - 2(H2 + V2)),
                      opposite = q(12s + 4D - 3(H2 + V2))
        G site:       G = s,  this row's colour = q(10s + 8 H1 - 2D - 2 H2 + V2),
                      the other = q(10s + 8 V1 - 2D - 2 V2 + H2)

    Every numerator lies in [-3060, 7140] (G at R / B: [-2040, 6120]) and so does every partial
    sum: signed 16-bit arithmetic is exact. ``codec::bayer_malvar_to_rgb_host`` and the
    ``raw_bayer_malvar_instances`` kernel (csrc/kernels/bayer_malvar.hip) give the same bytes.

    ``demosaic="hamilton"`` (``--input-bayer-demosaic hamilton``) is the edge-directed
    interpolation of Hamilton and Adams (US 5,629,734) in integers: green is chosen per site
    between a horizontal, a vertical and an averaged estimate, red and blue are interpolated as
    colour differences against that green. HS, WS >= 4; ``S`` is reflected two deep as for malvar.
    Green at an R or B site, with ``s = S[y][x]`` and W, E, N, S / WW, EE, NN, SS the samples one
    and two away::

        dH = |W - E| + |2s - WW - EE|              dV = |N - S| + |2s - NN - SS|
        gH = (2(W + E) + 2s - WW - EE + 2) >> 2    gV = (2(N + S) + 2s - NN - SS + 2) >> 2
        gA = (2(W + E + N + S) + 4s - WW - EE - NN - SS + 4) >> 3   (signed, >> arithmetic)
        G^ = clamp(dH < dV ? gH : dV < dH ? gV : gA, 0, 255)

    and ``G^ = s`` at a G site. The colour difference ``K[y][x] = S[y][x] - G^[y][x]`` uses the
    clamped ``G^``, exists at R / B sites only, is never read at a G site, and its indices are
    reflected one deep (-1 -> 1, n -> n - 2); dH / gH and dV / gV are symmetric, so this equals
    ``G^`` on a three-deep reflection of ``S``. Then::

        G site:    this row's colour = clamp(s + ((K[y][x-1] + K[y][x+1] + 1) >> 1), 0, 255)
                   the other         = clamp(s + ((K[y-1][x] + K[y+1][x] + 1) >> 1), 0, 255)
        R/B site:  own = s,  G = G^,  opposite = clamp(G^ + ((K[y-1][x-1] + K[y-1][x+1]
                                                 + K[y+1][x-1] + K[y+1][x+1] + 2) >> 2), 0, 255)

    There is no diagonal direction decision. gH and gV lie in [-127, 383] (gA within them), K in
    [-255, 255], a sum of four K in [-1020, 1020]: signed 16-bit arithmetic is exact.
    ``codec::bayer_hamilton_to_rgb_host`` and the ``raw_bayer_hamilton_instances`` kernel
    (csrc/kernels/bayer_hamilton.hip) give the same bytes. 8-bit mosaics only."""

    format: str = "bayer_rggb8"
    demosaic: str = "bilinear"

    def __post_init__(self):
        if self.format not in BAYER_FORMATS:
            raise ValueError(f"input_pixel_format={self.format!r}: expected one of "
                             f"{tuple(BAYER_FORMATS)} for a Bayer mosaic")
        if self.demosaic not in BAYER_DEMOSAICS:
            raise ValueError(f"input_bayer_demosaic={self.demosaic!r}: expected one of "
                             f"{BAYER_DEMOSAICS}")

    @classmethod
    def from_config(cls, cfg) -> Optional["BayerConvert"]:
        """The demosaic of a configuration, None for every other pixel format."""
        if cfg.input_pixel_format not in BAYER_FORMATS:
            return None
        return cls(cfg.input_pixel_format, cfg.input_bayer_demosaic)

    @staticmethod
    def frame_bytes(HS: int, WS: int) -> int:
        if HS <= 0 or WS <= 0 or HS % 2 or WS % 2:
            raise ValueError(f"a Bayer mosaic needs even, positive sizes, got {HS},{WS}")
        return HS * WS

    def engine_entries(self) -> Dict[str, Any]:
        d = dict(pixel_format=self.format)
        if self.demosaic != "bilinear":
            d["bayer_demosaic"] = self.demosaic
        return d

    def kernel_kwargs(self) -> Dict[str, Any]:
        """Keyword arguments of the ``raw_bayer_instances`` / ``raw_bayer_malvar_instances`` /
        ``raw_bayer_hamilton_instances`` bindings."""
        return dict(order=self.format)

    def apply(self, frame, HS: int, WS: int) -> np.ndarray:
        """The numpy oracle: uint8 [..., B] frames -> uint8 [..., HS, WS, 3] RGB."""
        B = self.frame_bytes(HS, WS)
        f = np.asarray(frame, np.uint8)
        if f.shape[-1] != B:
            raise ValueError(f"expected [..., {B}] bytes, got {f.shape}")
        green_first, blue_first = BAYER_FORMATS[self.format]
        s = f.reshape(*f.shape[:-1], HS, WS).astype(np.int32)
        rgb = _demosaic(s, green_first, blue_first, self.demosaic, 255)
        return rgb.astype(np.uint8)

    def green_choice(self, frame, HS: int, WS: int) -> np.ndarray:
        """Which green estimate the hamilton rule takes: uint8 [..., HS, WS], 0 at a G site,
        1 / 2 / 3 where gH / gV / gA is chosen at an R / B site."""
        s = np.asarray(frame, np.uint8).reshape(-1, HS, WS).astype(np.int32)
        choice = _hamilton_green(np.pad(s, [(0, 0), (2, 2), (2, 2)], mode="reflect"))[1]
        y, x = np.ogrid[:HS, :WS]
        green = ((x + y) & 1 == 1) != BAYER_FORMATS[self.format][0]
        return np.where(green, 0, choice).astype(np.uint8)

    @staticmethod
    def to_float(rgb, prep=None) -> np.ndarray:
        """The model-side floats of an RGB image: ``fmaf(float(RGB[c]), a[c], b[c])`` with the
        coefficients of ``prep`` (an ``InputPrep``; None: the identity)."""
        x = np.asarray(rgb).astype(np.float32)
        return x if prep is None else prep.apply(x)


# the deeper Bayer mosaics: name -> (green_first, blue_first, bits, packing); packing "le16":
# little-endian 16-bit words masked to the depth, "mipi": the CSI-2 packed groups
BAYER_HI_FORMATS = {
    f"bayer_{order}{form}": (*BAYER_FORMATS[f"bayer_{order}8"], bits, packing)
    for order in ("rggb", "bggr", "grbg", "gbrg")
    for form, bits, packing in (("10le", 10, "le16"), ("12le", 12, "le16"), ("16le", 16, "le16"),
                                ("10p", 10, "mipi"), ("12p", 12, "mipi"))}


@dataclass(frozen=True)
class BayerHiConvert:
    """Raw 10-, 12- and 16-bit Bayer mosaic frames (``--input-pixel-format bayer_<order><form>``,
    order ``rggb | bggr | grbg | gbrg``) to interleaved RGB at full depth, in integers.

    A frame of HS x WS samples (both even) of ``bits`` bits, ``M = 2**bits - 1``::

        10le 12le 16le  2*HS*WS bytes    little-endian 16-bit words, sample = word & M (the upper
                                         bits of a 10- / 12-bit word are ignored)
        10p             5*HS*WS/4 bytes  WS % 4 == 0, no row padding; 4 pixels in 5 bytes: bytes
                                         0..3 hold bits 9:2 of pixels 0..3, byte 4 their bits 1:0
                                         (pixel 0 in bits 1:0, pixel 3 in bits 7:6)
        12p             3*HS*WS/2 bytes  2 pixels in 3 bytes: p0[11:4], p1[11:4],
                                         p1[3:0] << 4 | p0[3:0]

    (V4L2 SRGGB10 / 12 / 16, SRGGB10P, SRGGB12P.) Every bit pattern is a frame. RGB is
    ``BayerConvert``'s bilinear or malvar rule on the samples, the malvar clamp being
    ``q(n) = clamp((n + 8) >> 4, 0, M)``; nothing is scaled to 8 bits, ``--input-scale`` is the
    user's for their depth. ``codec::bayer_hi_to_rgb_host`` (csrc/codec/bayer_hi.h) and the
    ``raw_bayer_hi_instances`` kernel (csrc/kernels/bayer_hi.hip) give the same bits."""

    format: str = "bayer_rggb16le"
    demosaic: str = "bilinear"

    def __post_init__(self):
        if self.format not in BAYER_HI_FORMATS:
            raise ValueError(f"input_pixel_format={self.format!r}: expected one of "
                             f"{tuple(BAYER_HI_FORMATS)} for a 10/12/16-bit Bayer mosaic")
        if self.demosaic not in ("bilinear", "malvar"):  # (hamilton: 8-bit mosaics only)
            raise ValueError(f"input_bayer_demosaic={self.demosaic!r}: expected bilinear or "
                             f"malvar for a 10/12/16-bit Bayer mosaic ({self.format})")

    @classmethod
    def from_config(cls, cfg) -> Optional["BayerHiConvert"]:
        """The demosaic of a configuration, None for every other pixel format."""
        if cfg.input_pixel_format not in BAYER_HI_FORMATS:
            return None
        return cls(cfg.input_pixel_format, cfg.input_bayer_demosaic)

    @property
    def bits(self) -> int:
        return BAYER_HI_FORMATS[self.format][2]

    @property
    def packing(self) -> str:
        return BAYER_HI_FORMATS[self.format][3]

    def frame_bytes(self, HS: int, WS: int) -> int:
        if HS <= 0 or WS <= 0 or HS % 2 or WS % 2:
            raise ValueError(f"a Bayer mosaic needs even, positive sizes, got {HS},{WS}")
        if self.packing == "le16":
            return 2 * HS * WS
        if self.bits == 10 and WS % 4:
            raise ValueError(f"{self.format}: four pixels in five bytes need WS % 4 == 0, got {WS}")
        return HS * WS * self.bits // 8

    def engine_entries(self) -> Dict[str, Any]:
        d = dict(pixel_format=self.format)
        if self.demosaic != "bilinear":
            d["bayer_demosaic"] = self.demosaic
        return d

    def kernel_kwargs(self) -> Dict[str, Any]:
        """Keyword arguments of the ``raw_bayer_hi_instances`` binding."""
        return dict(format=self.format, malvar=self.demosaic == "malvar")

    def unpack(self, frame, HS: int, WS: int) -> np.ndarray:
        """uint8 [..., B] frames -> uint16 [..., HS, WS] samples."""
        B = self.frame_bytes(HS, WS)
        f = np.asarray(frame, np.uint8)
        if f.shape[-1] != B:
            raise ValueError(f"expected [..., {B}] bytes, got {f.shape}")
        lead = f.shape[:-1]
        if self.packing == "le16":
            w = f.reshape(*lead, HS * WS, 2).astype(np.uint16)
            s = (w[..., 0] | w[..., 1] << 8) & ((1 << self.bits) - 1)
        elif self.bits == 10:
            g = f.reshape(*lead, HS * WS // 4, 5).astype(np.uint16)
            s = g[..., :4] << 2 | (g[..., 4:] >> np.arange(0, 8, 2, dtype=np.uint16)) & 3
        else:
            g = f.reshape(*lead, HS * WS // 2, 3).astype(np.uint16)
            s = g[..., :2] << 4 | (g[..., 2:] >> np.arange(0, 8, 4, dtype=np.uint16)) & 15
        return s.reshape(*lead, HS, WS).astype(np.uint16)

    def apply(self, frame, HS: int, WS: int) -> np.ndarray:
        """The numpy oracle: uint8 [..., B] frames -> uint16 [..., HS, WS, 3] RGB."""
        green_first, blue_first, bits, _ = BAYER_HI_FORMATS[self.format]
        s = self.unpack(frame, HS, WS).astype(np.int64)
        return _demosaic(s, green_first, blue_first, self.demosaic,
                         (1 << bits) - 1).astype(np.uint16)

    to_float = staticmethod(BayerConvert.to_float)


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
