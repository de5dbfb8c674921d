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
"""

from __future__ import annotations

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


def prep_or_none(prep: Optional[InputPrep]) -> Optional[InputPrep]:
    return None if prep is None or prep.identity else prep
