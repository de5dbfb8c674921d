"""Synthetic InstObj traffic (the reference's producers are external; README.md:22-27 documents
the record shape ``{"instances": [[[[...]]]]}``).

Images are uniform [0, 1) floats (normalised pixels) of the model's input shape, encoded with
Java ``Float.toString`` formatting by the native encoder (what a Jackson-based producer would
emit), one or more images per record.
"""

from __future__ import annotations

import base64
import json
from typing import List, Optional, Sequence, Tuple

import numpy as np

from gale._native import native


def synthetic_images(n: int, shape: Sequence[int], seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return rng.random((n,) + tuple(shape), dtype=np.float32)


def encode_records(images: np.ndarray, images_per_record: int = 1) -> List[bytes]:
    """[N, H, W, C] fp32 -> list of InstObj JSON records (bytes)."""
    C = native()
    out = []
    for i in range(0, images.shape[0], images_per_record):
        out.append(C.encode_instances(np.ascontiguousarray(images[i:i + images_per_record])))
    return out


def synthetic_pixels(n: int, shape: Sequence[int], seed: int = 0) -> np.ndarray:
    """Raw 8-bit pixels (integers 0..255) of the model's input shape: what a client sends when
    the topology scales and normalises on the GPU (--input-scale / --input-mean / --input-std)."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n,) + tuple(shape), dtype=np.uint8)


def encode_records_text(images: np.ndarray, images_per_record: int = 1,
                        layout: str = "nhwc") -> List[bytes]:
    """[N, H, W, C] -> InstObj records written by Python's compact ``json.dumps``: integer
    arrays without a decimal point (``[[[[125,122,113],...``), and with ``layout="nchw"`` each
    record's array nested [N][C][H][W] (what a PyTorch client holds; --input-layout nchw)."""
    if layout not in ("nhwc", "nchw"):
        raise ValueError(f"layout={layout!r}: expected nhwc or nchw")
    if layout == "nchw":
        images = images.transpose(0, 3, 1, 2)
    out = []
    for i in range(0, images.shape[0], images_per_record):
        out.append(json.dumps({"instances": images[i:i + images_per_record].tolist()},
                              separators=(",", ":")).encode())
    return out


def encode_records_b64(images_u8: np.ndarray, images_per_record: int = 1,
                       layout: str = "nhwc") -> List[bytes]:
    """uint8 [N, H, W, C] -> ``{"instances":[{"b64":"..."},...]}`` records (--input-format b64):
    each image's H*W*C bytes in standard base64, ordered [H][W][C], or [C][H][W] with
    ``layout="nchw"`` (--input-layout nchw)."""
    if layout not in ("nhwc", "nchw"):
        raise ValueError(f"layout={layout!r}: expected nhwc or nchw")
    images_u8 = np.asarray(images_u8)
    if images_u8.dtype != np.uint8 or images_u8.ndim != 4:
        raise ValueError("encode_records_b64: uint8 [N, H, W, C] images")
    if layout == "nchw":
        images_u8 = images_u8.transpose(0, 3, 1, 2)
    out = []
    for i in range(0, images_u8.shape[0], images_per_record):
        elems = [b'{"b64":"' + base64.b64encode(np.ascontiguousarray(im).tobytes()) + b'"}'
                 for im in images_u8[i:i + images_per_record]]
        out.append(b'{"instances":[' + b",".join(elems) + b"]}")
    return out


def pack_yuv420(Y: np.ndarray, U: np.ndarray, V: np.ndarray, pixel_format: str) -> np.ndarray:
    """uint8 planes Y [N, HS, WS], U / V [N, HS/2, WS/2] -> uint8 [N, HS*WS*3/2] frames: I420
    (Y, U, V planes) or NV12 (Y plane, interleaved UV plane)."""
    Y, U, V = (np.asarray(p) for p in (Y, U, V))
    if any(p.dtype != np.uint8 or p.ndim != 3 for p in (Y, U, V)):
        raise ValueError("pack_yuv420: uint8 [N, rows, cols] planes")
    N, HS, WS = Y.shape
    if HS % 2 or WS % 2 or U.shape != (N, HS // 2, WS // 2) or V.shape != U.shape:
        raise ValueError(f"pack_yuv420: Y {Y.shape} needs even sizes and U, V of "
                         f"{(N, HS // 2, WS // 2)}, got {U.shape}, {V.shape}")
    if pixel_format == "i420":
        chroma = [U.reshape(N, -1), V.reshape(N, -1)]
    elif pixel_format == "nv12":
        chroma = [np.stack([U, V], axis=-1).reshape(N, -1)]
    else:
        raise ValueError(f"pixel_format={pixel_format!r}: expected i420 or nv12")
    return np.ascontiguousarray(np.concatenate([Y.reshape(N, -1), *chroma], axis=1))


def encode_records_yuv(Y: np.ndarray, U: np.ndarray, V: np.ndarray, pixel_format: str,
                       images_per_record: int = 1) -> List[bytes]:
    """uint8 planes (``pack_yuv420``) -> ``{"instances":[{"b64":"..."},...]}`` records of YUV
    4:2:0 frames (--input-format b64 --input-pixel-format i420 | nv12): each frame's HS*WS*3/2
    bytes in standard base64 (never padded: the byte count is a multiple of 3)."""
    frames = pack_yuv420(Y, U, V, pixel_format)
    out = []
    for i in range(0, frames.shape[0], images_per_record):
        elems = [b'{"b64":"' + base64.b64encode(fr.tobytes()) + b'"}'
                 for fr in frames[i:i + images_per_record]]
        out.append(b'{"instances":[' + b",".join(elems) + b"]}")
    return out


def synthetic_yuv_planes(n: int, HS: int, WS: int, seed: int = 0):
    """Deterministic uint8 planes (Y [n, HS, WS], U, V [n, HS/2, WS/2]) of synthetic frames."""
    if HS % 2 or WS % 2:
        raise ValueError(f"a 4:2:0 frame needs even sizes, got {HS},{WS}")
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n, HS, WS), dtype=np.uint8),
            rng.integers(0, 256, (n, HS // 2, WS // 2), dtype=np.uint8),
            rng.integers(0, 256, (n, HS // 2, WS // 2), dtype=np.uint8))


def pack_yuv422(Y: np.ndarray, U: np.ndarray, V: np.ndarray, pixel_format: str) -> np.ndarray:
    """uint8 planes Y [N, HS, WS], U / V [N, HS, WS/2] -> uint8 [N, 2*HS*WS] packed 4:2:2 frames:
    yuyv422 (``Y0 U Y1 V`` macropixels) or uyvy422 (``U Y0 V Y1``); the inverse of
    ``gale.models.preprocess.Yuv422Convert.planes``."""
    from gale.models.preprocess import YUV422_FORMATS

    Y, U, V = (np.asarray(p) for p in (Y, U, V))
    if any(p.dtype != np.uint8 or p.ndim != 3 for p in (Y, U, V)):
        raise ValueError("pack_yuv422: uint8 [N, rows, cols] planes")
    N, HS, WS = Y.shape
    if WS % 2 or U.shape != (N, HS, WS // 2) or V.shape != U.shape:
        raise ValueError(f"pack_yuv422: Y {Y.shape} needs an even width and U, V of "
                         f"{(N, HS, WS // 2)}, got {U.shape}, {V.shape}")
    if pixel_format not in YUV422_FORMATS:
        raise ValueError(f"pixel_format={pixel_format!r}: expected yuyv422 or uyvy422")
    y0, y1, u, v = YUV422_FORMATS[pixel_format]
    mp = np.empty((N, HS, WS // 2, 4), np.uint8)
    mp[..., y0], mp[..., y1], mp[..., u], mp[..., v] = Y[..., 0::2], Y[..., 1::2], U, V
    return mp.reshape(N, -1)


def encode_records_yuv422(Y: np.ndarray, U: np.ndarray, V: np.ndarray, pixel_format: str,
                          images_per_record: int = 1, encoding: str = "b64") -> List[bytes]:
    """uint8 planes (``pack_yuv422``) -> records of packed 4:2:2 frames (--input-pixel-format
    yuyv422 | uyvy422). ``encoding`` b64: ``{"instances":[{"b64":"..."},...]}`` with each
    frame's 2*HS*WS bytes in standard base64, '=' padded; raw: each record value is its frames'
    bytes back to back (--input-format raw)."""
    if encoding not in ("b64", "raw"):
        raise ValueError(f"encoding={encoding!r}: expected b64 or raw")
    frames = pack_yuv422(Y, U, V, pixel_format)
    out = []
    for i in range(0, frames.shape[0], images_per_record):
        part = frames[i:i + images_per_record]
        if encoding == "raw":
            out.append(part.tobytes())
        else:
            elems = [b'{"b64":"' + base64.b64encode(fr.tobytes()) + b'"}' for fr in part]
            out.append(b'{"instances":[' + b",".join(elems) + b"]}")
    return out


def synthetic_yuv422_planes(n: int, HS: int, WS: int, seed: int = 0):
    """Deterministic uint8 planes (Y [n, HS, WS], U, V [n, HS, WS/2]) of synthetic frames."""
    if WS % 2:
        raise ValueError(f"a 4:2:2 frame needs an even width, got {HS},{WS}")
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n, HS, WS), dtype=np.uint8),
            rng.integers(0, 256, (n, HS, WS // 2), dtype=np.uint8),
            rng.integers(0, 256, (n, HS, WS // 2), dtype=np.uint8))


def pack_yuvp(Y: np.ndarray, U: np.ndarray, V: np.ndarray, pixel_format: str) -> np.ndarray:
    """uint8 planes Y [N, HS, WS], U / V [N, HS, WS >> s] -> uint8 [N, B] planar frames (Y, U, V
    planes back to back): yuv422p (s = 1, WS even) or yuv444p (s = 0)."""
    from gale.models.preprocess import YUVP_FORMATS

    Y, U, V = (np.asarray(p) for p in (Y, U, V))
    if any(p.dtype != np.uint8 or p.ndim != 3 for p in (Y, U, V)):
        raise ValueError("pack_yuvp: uint8 [N, rows, cols] planes")
    if pixel_format not in YUVP_FORMATS:
        raise ValueError(f"pixel_format={pixel_format!r}: expected yuv422p or yuv444p")
    s = YUVP_FORMATS[pixel_format]
    N, HS, WS = Y.shape
    if WS % (1 << s) or U.shape != (N, HS, WS >> s) or V.shape != U.shape:
        raise ValueError(f"pack_yuvp: {pixel_format} with Y {Y.shape} needs "
                         f"{'an even width and ' if s else ''}U, V of {(N, HS, WS >> s)}, got "
                         f"{U.shape}, {V.shape}")
    return np.ascontiguousarray(np.concatenate([p.reshape(N, -1) for p in (Y, U, V)], axis=1))


def encode_records_yuvp(Y: np.ndarray, U: np.ndarray, V: np.ndarray, pixel_format: str,
                        images_per_record: int = 1, encoding: str = "b64") -> List[bytes]:
    """uint8 planes (``pack_yuvp``) -> records of planar 4:2:2 / 4:4:4 frames
    (--input-pixel-format yuv422p | yuv444p). ``encoding`` b64:
    ``{"instances":[{"b64":"..."},...]}`` with each frame's bytes in standard base64, '=' padded;
    raw: each record value is its frames' bytes back to back (--input-format raw)."""
    if encoding not in ("b64", "raw"):
        raise ValueError(f"encoding={encoding!r}: expected b64 or raw")
    frames = pack_yuvp(Y, U, V, pixel_format)
    out = []
    for i in range(0, frames.shape[0], images_per_record):
        part = frames[i:i + images_per_record]
        if encoding == "raw":
            out.append(part.tobytes())
        else:
            elems = [b'{"b64":"' + base64.b64encode(fr.tobytes()) + b'"}' for fr in part]
            out.append(b'{"instances":[' + b",".join(elems) + b"]}")
    return out


def synthetic_yuvp_planes(n: int, HS: int, WS: int, pixel_format: str, seed: int = 0):
    """Deterministic uint8 planes (Y [n, HS, WS], U, V [n, HS, WS >> s]) of synthetic frames."""
    s = 1 if pixel_format == "yuv422p" else 0
    if WS % (1 << s):
        raise ValueError(f"a 4:2:2 frame needs an even width, got {HS},{WS}")
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n, HS, WS), dtype=np.uint8),
            rng.integers(0, 256, (n, HS, WS >> s), dtype=np.uint8),
            rng.integers(0, 256, (n, HS, WS >> s), dtype=np.uint8))


def pack_yuv420p10(Y: np.ndarray, U: np.ndarray, V: np.ndarray, pixel_format: str,
                   junk: Optional[np.ndarray] = None) -> np.ndarray:
    """10-bit samples Y [N, HS, WS], U / V [N, HS/2, WS/2] (integers 0 .. 1023) -> uint8
    [N, 3*HS*WS] frames of little-endian 16-bit words: p010le (Y, interleaved UV, the sample in
    the top ten bits) or yuv420p10le (Y, U, V planes, the sample in the low ten). ``junk``
    (uint16 [N, 3*HS*WS/2], optional): its six bits that a reader ignores are set in every word."""
    from gale.models.preprocess import YUV420_HI_FORMATS

    Y, U, V = (np.asarray(p) for p in (Y, U, V))
    if pixel_format not in YUV420_HI_FORMATS:
        raise ValueError(f"pixel_format={pixel_format!r}: expected p010le or yuv420p10le")
    if any(p.ndim != 3 or p.dtype.kind not in "iu" or p.min(initial=0) < 0
           or p.max(initial=0) > 1023 for p in (Y, U, V)):
        raise ValueError("pack_yuv420p10: integer [N, rows, cols] planes of 0 .. 1023")
    N, HS, WS = Y.shape
    if HS % 2 or WS % 2 or U.shape != (N, HS // 2, WS // 2) or V.shape != U.shape:
        raise ValueError(f"pack_yuv420p10: Y {Y.shape} needs even sizes and U, V of "
                         f"{(N, HS // 2, WS // 2)}, got {U.shape}, {V.shape}")
    chroma = [np.stack([U, V], axis=-1)] if pixel_format == "p010le" else [U, V]
    w = np.concatenate([p.reshape(N, -1) for p in (Y, *chroma)], axis=1).astype(np.uint16)
    sh = YUV420_HI_FORMATS[pixel_format]
    w = w << sh
    if junk is not None:
        w |= np.asarray(junk, np.uint16) & np.uint16(~(1023 << sh) & 0xFFFF)
    return np.ascontiguousarray(w.astype("<u2")).view(np.uint8).reshape(N, -1)


def encode_records_yuv420p10(Y: np.ndarray, U: np.ndarray, V: np.ndarray, pixel_format: str,
                             images_per_record: int = 1,
                             junk: Optional[np.ndarray] = None) -> List[bytes]:
    """10-bit samples (``pack_yuv420p10``) -> raw records of 10-bit 4:2:0 frames
    (--input-pixel-format p010le | yuv420p10le, --input-format raw): each record value is its
    frames' bytes back to back."""
    frames = pack_yuv420p10(Y, U, V, pixel_format, junk)
    return [frames[i:i + images_per_record].tobytes()
            for i in range(0, frames.shape[0], images_per_record)]


def synthetic_yuv420p10_planes(n: int, HS: int, WS: int, seed: int = 0):
    """Deterministic 10-bit samples (Y [n, HS, WS], U, V [n, HS/2, WS/2]) of synthetic frames."""
    if HS % 2 or WS % 2:
        raise ValueError(f"a 4:2:0 frame needs even sizes, got {HS},{WS}")
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1024, (n, HS, WS), dtype=np.uint16),
            rng.integers(0, 1024, (n, HS // 2, WS // 2), dtype=np.uint16),
            rng.integers(0, 1024, (n, HS // 2, WS // 2), dtype=np.uint16))


def mosaic_bayer(rgb_u8: np.ndarray, pixel_format: str) -> np.ndarray:
    """uint8 RGB images [..., HS, WS, 3] (HS, WS even) -> uint8 [..., HS, WS]: the colour-filter
    mosaic a sensor of that order sees, every site keeping its own colour of the image."""
    from gale.models.preprocess import BAYER_FORMATS

    rgb = np.asarray(rgb_u8)
    if pixel_format not in BAYER_FORMATS:
        raise ValueError(f"pixel_format={pixel_format!r}: expected one of {tuple(BAYER_FORMATS)}")
    if rgb.dtype != np.uint8 or rgb.ndim < 3 or rgb.shape[-1] != 3 or rgb.shape[-3] % 2 \
            or rgb.shape[-2] % 2:
        raise ValueError(f"mosaic_bayer: uint8 [..., HS, WS, 3] with even HS, WS, got {rgb.shape}")
    green_first, blue_first = BAYER_FORMATS[pixel_format]
    y, x = np.ogrid[:rgb.shape[-3], :rgb.shape[-2]]
    green = ((x + y) & 1 == 1) != green_first
    blue_row = (y & 1 == 1) != blue_first
    return np.where(green, rgb[..., 1], np.where(blue_row, rgb[..., 2], rgb[..., 0]))


def encode_records_bayer(rgb_u8: np.ndarray, pixel_format: str,
                         images_per_record: int = 1) -> List[bytes]:
    """uint8 RGB images [N, HS, WS, 3] -> raw records of Bayer mosaics (``mosaic_bayer``;
    --input-pixel-format bayer_*8, --input-format raw): each record value is its frames' HS*WS
    bytes back to back."""
    frames = mosaic_bayer(rgb_u8, pixel_format)
    frames = frames.reshape(frames.shape[0], -1)
    return [frames[i:i + images_per_record].tobytes()
            for i in range(0, frames.shape[0], images_per_record)]


def pack_bayer_hi(mosaic: np.ndarray, pixel_format: str,
                  junk: Optional[np.ndarray] = None) -> np.ndarray:
    """Samples [N, HS, WS] (integers 0 .. 2**bits - 1) -> uint8 [N, B] frames of a 10/12/16-bit
    Bayer format (``gale.models.preprocess.BayerHiConvert``: little-endian words, or the MIPI
    groups of 5 bytes for 4 pixels / 3 bytes for 2). ``junk`` (uint16 [N, HS, WS], optional, the
    10le / 12le words only): its bits above the depth, which a reader ignores, are set."""
    from gale.models.preprocess import BayerHiConvert

    bc, m = BayerHiConvert(pixel_format), np.asarray(mosaic)
    if m.ndim != 3 or m.dtype.kind not in "iu" or m.min(initial=0) < 0 \
            or m.max(initial=0) >> bc.bits:
        raise ValueError(f"pack_bayer_hi: integer [N, HS, WS] samples of {bc.bits} bits")
    N, HS, WS = m.shape
    bc.frame_bytes(HS, WS)  # (ValueError on a size that is no frame)
    s = m.astype(np.uint16)
    if bc.packing == "le16":
        if junk is not None:
            s = s | (np.asarray(junk, np.uint16) & np.uint16(0xFFFF >> bc.bits << bc.bits))
        return np.ascontiguousarray(s.astype("<u2")).view(np.uint8).reshape(N, -1)
    if junk is not None:
        raise ValueError(f"pack_bayer_hi: {pixel_format} has no ignored bits")
    n, low = (4, 2) if bc.bits == 10 else (2, 4)  # pixels a group, their bits in the last byte
    g = s.reshape(N, -1, n)
    last = (((g & ((1 << low) - 1)) << (low * np.arange(n, dtype=np.uint16))).sum(-1))
    return np.concatenate([g >> low, last[..., None]], axis=-1).astype(np.uint8).reshape(N, -1)


def encode_records_bayer_hi(mosaic: np.ndarray, pixel_format: str, images_per_record: int = 1,
                            junk: Optional[np.ndarray] = None) -> List[bytes]:
    """Samples (``pack_bayer_hi``) -> raw records of 10/12/16-bit Bayer mosaics
    (--input-pixel-format bayer_*10le | 12le | 16le | 10p | 12p, --input-format raw): each record
    value is its frames' bytes back to back."""
    frames = pack_bayer_hi(mosaic, pixel_format, junk)
    return [frames[i:i + images_per_record].tobytes()
            for i in range(0, frames.shape[0], images_per_record)]


def pack_pixels(rgb_u8: np.ndarray, pixel_format: str,
                alpha: Optional[np.ndarray] = None) -> np.ndarray:
    """uint8 RGB images [N, HS, WS, 3] -> uint8 [N, HS*WS*P] packed images (the inverse of
    ``gale.models.preprocess.PixelUnpack.apply``): ``bgr24`` / ``rgba`` / ``bgra`` reorder the
    bytes, with ``alpha`` [N, HS, WS] (default 255) as the fourth byte; ``gray`` needs
    R == G == B and keeps one byte."""
    from gale.models.preprocess import PixelUnpack

    un = PixelUnpack(pixel_format)
    x = np.asarray(rgb_u8)
    if x.dtype != np.uint8 or x.ndim != 4 or x.shape[3] != 3:
        raise ValueError("pack_pixels: uint8 [N, HS, WS, 3] images")
    N, HS, WS, _ = x.shape
    P = un.bytes_per_pixel
    if alpha is not None and P != 4:
        raise ValueError(f"pack_pixels: {pixel_format} has no alpha byte")
    if P == 1:
        if not (np.array_equal(x[..., 0], x[..., 1]) and np.array_equal(x[..., 0], x[..., 2])):
            raise ValueError("pack_pixels: gray needs R == G == B")
        return np.ascontiguousarray(x[..., 0].reshape(N, -1))
    out = np.full((N, HS, WS, P), 255, np.uint8)
    if alpha is not None:
        a = np.asarray(alpha)
        if a.dtype != np.uint8 or a.shape != (N, HS, WS):
            raise ValueError(f"pack_pixels: alpha must be uint8 {(N, HS, WS)}, got {a.shape}")
        out[..., 3] = a
    for c, off in enumerate(un.offsets):
        out[..., off] = x[..., c]
    return out.reshape(N, -1)


def encode_records_packed(rgb_u8: np.ndarray, pixel_format: str, images_per_record: int = 1,
                          alpha: Optional[np.ndarray] = None) -> List[bytes]:
    """uint8 RGB images (``pack_pixels``) -> ``{"instances":[{"b64":"..."},...]}`` records of
    packed pixels (--input-format b64 --input-pixel-format bgr24 | rgba | bgra | gray): each
    image's HS*WS*P bytes in standard base64, '=' padded."""
    packed = pack_pixels(rgb_u8, pixel_format, alpha)
    out = []
    for i in range(0, packed.shape[0], images_per_record):
        elems = [b'{"b64":"' + base64.b64encode(im.tobytes()) + b'"}'
                 for im in packed[i:i + images_per_record]]
        out.append(b'{"instances":[' + b",".join(elems) + b"]}")
    return out


def encode_records_typed(x: np.ndarray, dtype: str, images_per_record: int = 1,
                         layout: str = "nhwc") -> List[bytes]:
    """[N, H, W, C] values -> ``{"instances":[{"b64":"..."},...]}`` records of typed tensors
    (--input-format b64 --input-dtype u8 | u16 | f16 | bf16 | f32): each image's H*W*C elements
    rounded to ``dtype`` (``gale.models.preprocess.ElemType.to_wire``), little-endian, in
    standard base64, ordered [H][W][C], or [C][H][W] with ``layout="nchw"``."""
    from gale.models.preprocess import ElemType

    if layout not in ("nhwc", "nchw"):
        raise ValueError(f"layout={layout!r}: expected nhwc or nchw")
    x = np.asarray(x)
    if x.ndim != 4:
        raise ValueError("encode_records_typed: [N, H, W, C] images")
    if layout == "nchw":
        x = x.transpose(0, 3, 1, 2)
    wire = ElemType(dtype).to_wire(np.ascontiguousarray(x)).reshape(x.shape[0], -1)
    out = []
    for i in range(0, wire.shape[0], images_per_record):
        elems = [b'{"b64":"' + base64.b64encode(im.tobytes()) + b'"}'
                 for im in wire[i:i + images_per_record]]
        out.append(b'{"instances":[' + b",".join(elems) + b"]}")
    return out


def encode_records_raw(x: np.ndarray, images_per_record: int = 1, dtype: str = "u8",
                       pixel_format: str = "rgb", layout: str = "nhwc",
                       alpha: Optional[np.ndarray] = None) -> List[bytes]:
    """[N, H, W, C] values -> raw binary records (--input-format raw): each record value is its
    images' bytes back to back, nothing around them. ``pixel_format`` rgb: the H*W*C elements
    rounded to ``dtype`` (``ElemType.to_wire``), little-endian, ordered [H][W][C] or [C][H][W]
    with ``layout="nchw"``; a packed format: uint8 RGB images packed by ``pack_pixels``."""
    from gale.models.preprocess import ElemType

    if layout not in ("nhwc", "nchw"):
        raise ValueError(f"layout={layout!r}: expected nhwc or nchw")
    x = np.asarray(x)
    if x.ndim != 4:
        raise ValueError("encode_records_raw: [N, H, W, C] images")
    if pixel_format != "rgb":
        if dtype != "u8" or layout != "nhwc":
            raise ValueError(f"pixel_format={pixel_format!r} carries uint8 pixels in nhwc order")
        wire = pack_pixels(x, pixel_format, alpha)
    else:
        if layout == "nchw":
            x = x.transpose(0, 3, 1, 2)
        wire = ElemType(dtype).to_wire(np.ascontiguousarray(x)).reshape(x.shape[0], -1)
    return [wire[i:i + images_per_record].tobytes()
            for i in range(0, wire.shape[0], images_per_record)]


def encode_batches(records: Sequence[bytes], records_per_batch: int = 64) -> List[bytes]:
    """Group records into Kafka RecordBatch v2 blobs (for the broker's shared-append preload)."""
    K = native().kafka
    return [K.encode_batch([(None, r, -1, None) for r in records[i:i + records_per_batch]], 0, 0)
            for i in range(0, len(records), records_per_batch)]


def preload(broker, topic: str, partition: int, batches: Sequence[bytes], total_records: int,
            records_per_batch: int) -> Tuple[int, int]:
    """Append ``total_records`` records to (topic, partition) by cycling through ``batches``
    (each appended by reference). Returns (first offset, records appended)."""
    first = None
    n = 0
    i = 0
    while n < total_records:
        off = broker.append_batch_repeated(topic, partition, batches[i % len(batches)], 1)
        first = off if first is None else first
        n += records_per_batch
        i += 1
    return first, n
