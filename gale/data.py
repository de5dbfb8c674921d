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
