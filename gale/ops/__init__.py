"""PyTorch-facing wrappers of the gale gfx950 kernels (``gale._C``).

Each op takes device tensors, launches the hand-written HIP kernel on the current torch stream
and returns a new tensor. There is deliberately no eager-PyTorch fallback: if the native library
is missing or the tensor is not on a GPU the call fails loudly (the serving path must never run
silently on a non-native implementation).
"""

from __future__ import annotations

from typing import Optional

import torch

from gale._native import native
from gale.models.graph import conv_n_tiles, pack_conv_weight, round_up


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _check(t: torch.Tensor, dtype: torch.dtype, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"gale op: {name} must be a GPU tensor (no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"gale op: {name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"gale op: {name} must be contiguous")


def pack_conv(w_oihw: torch.Tensor, bias: torch.Tensor, cin_stored: Optional[int] = None,
              device=None):
    """Pack an fp32 [Cout, Cin, KH, KW] conv weight for the MFMA kernel.

    Returns (w_packed bf16 [Npad, Kpad], bias fp32 [Npad], desc-geometry dict).
    """
    cout, cin, kh, kw = w_oihw.shape
    cin_s = cin if cin_stored is None else cin_stored
    cout_s = round_up(cout, 4)
    K = kh * kw * cin_s
    Kpad = round_up(K, 32)
    Npad = round_up(cout_s, conv_n_tiles(cout_s) * 16)
    wp = pack_conv_weight(w_oihw.float().cpu(), cin_s, Npad, Kpad).to(torch.bfloat16)
    bp = torch.zeros(Npad)
    bp[:cout] = bias.float().cpu()
    dev = device if device is not None else torch.device("cuda")
    return wp.to(dev), bp.to(dev), dict(Cin=cin_s, Cout=cout_s, KH=kh, KW=kw, K=K, Kpad=Kpad,
                                        Npad=Npad)


def conv2d(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, geom: dict, stride: int = 1,
           pad: int = 0, relu: bool = False, residual: Optional[torch.Tensor] = None,
           res_mode: str = "identity", out_f32: bool = False) -> torch.Tensor:
    """NHWC conv on MFMA. x: [B,H,W,Cin] bf16 (or fp32 for the network input)."""
    B, H, W, C = x.shape
    if C != geom["Cin"]:
        raise ValueError(f"x has {C} channels, packed weight expects {geom['Cin']}")
    _check(w_packed, torch.bfloat16, "w_packed")
    _check(bias, torch.float32, "bias")
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("x must be bf16 or fp32")
    _check(x, x.dtype, "x")
    kh, kw = geom["KH"], geom["KW"]
    Ho = (H + 2 * pad - kh) // stride + 1
    Wo = (W + 2 * pad - kw) // stride + 1
    cout = geom["Cout"]
    y = torch.empty(B, Ho, Wo, cout, device=x.device,
                    dtype=torch.float32 if out_f32 else torch.bfloat16)
    d = dict(geom, H=H, W=W, Ho=Ho, Wo=Wo, stride=stride, pad=pad, relu=int(relu),
             in_f32=int(x.dtype == torch.float32), out_f32=int(out_f32))
    res_ptr = 0
    if residual is not None:
        _check(residual, torch.bfloat16, "residual")
        _, rh, rw, rc = residual.shape
        d.update(has_res=1, res_H=rh, res_W=rw, res_C=rc, res_stride=2 if res_mode == "pad" else 1)
        res_ptr = residual.data_ptr()
    native().conv2d(d, B, x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), 0, res_ptr,
                    y.data_ptr(), _stream())
    return y


def bottleneck56(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor,
                 b2: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor,
                 wd: Optional[torch.Tensor] = None,
                 bd: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One whole ResNet-50 56x56 bottleneck in one kernel (bottleneck_fused.hip).

    x: [B,56,56,256] bf16 (identity shortcut) or [B,56,56,64] with the projection (wd, bd) of
    block 0. Weights packed by ``pack_conv`` (w1 1x1 -> 64, w2 3x3 64 -> 64, w3 / wd 1x1 -> 256).
    Returns relu(conv3(relu(conv2(relu(conv1(x))))) + shortcut), bf16 [B,56,56,256].
    """
    B, H, W, C = x.shape
    down = wd is not None
    if not native().bottleneck56_supported(H, W, C, 64, 256, int(down)):
        raise ValueError(f"bottleneck56: unsupported input {tuple(x.shape)} (down={down})")
    _check(x, torch.bfloat16, "x")
    shapes = {"w1": (w1, (64, C)), "w2": (w2, (64, 576)), "w3": (w3, (256, 64))}
    if down:
        if bd is None:
            raise ValueError("bottleneck56: wd needs bd")
        shapes["wd"] = (wd, (256, 64))
    for name, (t, shp) in shapes.items():
        _check(t, torch.bfloat16, name)
        if tuple(t.shape) != shp:
            raise ValueError(f"bottleneck56: {name} must be {shp}, got {tuple(t.shape)}")
    for name, t, n in (("b1", b1, 64), ("b2", b2, 64), ("b3", b3, 256)) + \
            ((("bd", bd, 256),) if down else ()):
        _check(t, torch.float32, name)
        if t.numel() != n:
            raise ValueError(f"bottleneck56: {name} must have {n} entries")
    y = torch.empty(B, H, W, 256, device=x.device, dtype=torch.bfloat16)
    native().bottleneck56(B, x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                          b2.data_ptr(), w3.data_ptr(), b3.data_ptr(),
                          wd.data_ptr() if down else 0, bd.data_ptr() if down else 0,
                          y.data_ptr(), C, int(down), _stream())
    return y


def maxpool2d(x: torch.Tensor, k: int, s: int, p: int = 0) -> torch.Tensor:
    _check(x, torch.bfloat16, "x")
    B, H, W, C = x.shape
    Ho = (H + 2 * p - k) // s + 1
    Wo = (W + 2 * p - k) // s + 1
    y = torch.empty(B, Ho, Wo, C, device=x.device, dtype=torch.bfloat16)
    native().maxpool2d(B, H, W, C, k, s, p, Ho, Wo, x.data_ptr(), y.data_ptr(), _stream())
    return y


def avgpool_global(x: torch.Tensor) -> torch.Tensor:
    _check(x, torch.bfloat16, "x")
    B, H, W, C = x.shape
    y = torch.empty(B, C, device=x.device, dtype=torch.bfloat16)
    native().avgpool_global(B, H * W, C, x.data_ptr(), y.data_ptr(), _stream())
    return y


def head(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Global avg pool + dense(fp32 w [N, C]) + softmax. x: [B,H,W,C] bf16 -> [B,N] fp32."""
    _check(x, torch.bfloat16, "x")
    _check(w, torch.float32, "w")
    _check(b, torch.float32, "b")
    B, H, W, C = x.shape
    N = w.shape[0]
    out = torch.empty(B, N, device=x.device, dtype=torch.float32)
    native().head_pool_dense_softmax(B, H * W, C, N, x.data_ptr(), w.data_ptr(), b.data_ptr(),
                                     out.data_ptr(), _stream())
    return out


def softmax(x: torch.Tensor, n: Optional[int] = None) -> torch.Tensor:
    _check(x, torch.float32, "x")
    B, ld = x.shape
    n = ld if n is None else n
    out = torch.empty(B, n, device=x.device, dtype=torch.float32)
    native().softmax_rows(B, n, ld, x.data_ptr(), out.data_ptr(), _stream())
    return out


def topk(x: torch.Tensor, k: int):
    """The ``k`` best classes of each row of x (fp32 [rows, classes]) in score order (descending
    by the bits' order-preserving key, ties to the lower class; csrc/codec/json_codec.h), selected
    and formatted by the top-k kernel (csrc/kernels/topk.hip).

    Returns ``(texts, indices)``: uint8 [rows, k, FLOAT_TEXT_SLOT] Java ``Float.toString`` slots
    (characters from byte 0, length in byte 15) and int32 [rows, k] class indices."""
    _check(x, torch.float32, "x")
    if x.dim() != 2:
        raise ValueError("gale op: x must be [rows, classes]")
    rows, classes = x.shape
    if not 1 <= k <= min(classes, 64) or classes > 4096:
        raise ValueError("gale op: topk needs 1 <= k <= min(classes, 64) and classes <= 4096")
    texts = torch.empty(rows, k, native().FLOAT_TEXT_SLOT, device=x.device, dtype=torch.uint8)
    indices = torch.empty(rows, k, device=x.device, dtype=torch.int32)
    native().topk_java(rows, classes, k, x.data_ptr(), texts.data_ptr(), indices.data_ptr(),
                       _stream())
    return texts, indices


def resize_tables(HS: int, WS: int, HR: int, WR: int, H: int, W: int, device):
    """The six tables of an input resize (``codec::build_resize_tables``) as device tensors, in
    the order the ``resize_crop`` bindings take their pointers: y0, y1, wy, x0, x1, wx."""
    return [torch.from_numpy(t).to(device)
            for t in native().build_resize_tables(HS, WS, HR, WR, H, W)]


def resize_crop(x: torch.Tensor, resize, size, tables=None) -> torch.Tensor:
    """Bilinear resize (half-pixel centres, no antialiasing) of x (fp32 [N, HS, WS, C]) to
    ``resize`` = (HR, WR) and centre crop (floor offset) to ``size`` = (H, W), by the resize
    kernel (csrc/kernels/resize_crop.hip); bit-identical to ``InputResize.apply``
    (gale/models/preprocess.py). ``tables``: ``resize_tables(...)`` of the same dimensions on x's
    device, to reuse them across calls. Returns fp32 [N, H, W, C]."""
    _check(x, torch.float32, "x")
    if x.dim() != 4:
        raise ValueError("gale op: x must be [N, HS, WS, C]")
    N, HS, WS, C = x.shape
    (HR, WR), (H, W) = resize, size
    if N > 65535 or C < 1:
        raise ValueError("gale op: resize_crop needs N <= 65535 images and C >= 1")
    if tables is None:
        tables = resize_tables(HS, WS, HR, WR, H, W, x.device)  # (ValueError on bad sizes)
    if len(tables) != 6 or tables[0].numel() != H or tables[3].numel() != W:
        raise ValueError("gale op: resize_crop tables do not match size")
    for t in tables:
        if not t.is_cuda or t.device != x.device:
            raise ValueError("gale op: resize_crop tables must be on x's device")
    out = torch.empty(N, H, W, C, device=x.device, dtype=torch.float32)
    if N == 0:
        return out
    native().resize_crop(N, HS, WS, H, W, C, [t.data_ptr() for t in tables], x.data_ptr(),
                         out.data_ptr(), _stream())
    return out


class ResizeAaTables:
    """The device tables of an antialiased input resize in the ``resize_crop_aa`` kernel's layout
    (ys, yn, wy [H][ty], xs, xn, wx [W][tx]) with the dimensions and the launch figures (ty, tx,
    band, band_rows) they were built for."""

    def __init__(self, dims, tensors, launch):
        self.dims, self.tensors, self.launch = tuple(dims), list(tensors), tuple(launch)

    def ptrs(self):
        return [t.data_ptr() for t in self.tensors]


def resize_aa_tables(HS: int, WS: int, HR: int, WR: int, H: int, W: int, device) -> ResizeAaTables:
    """``codec::build_resize_aa_tables`` on ``device`` for the ``resize_crop_aa`` bindings
    (ValueError beyond the 8x antialias limit or on other bad sizes)."""
    *tabs, ty, tx, band, rows = native().build_resize_aa_tables(HS, WS, HR, WR, H, W, device=True)
    return ResizeAaTables((HS, WS, HR, WR, H, W), [torch.from_numpy(t).to(device) for t in tabs],
                          (ty, tx, band, rows))


def resize_crop_aa(x: torch.Tensor, resize, size, tables=None) -> torch.Tensor:
    """Antialiased resize (the support-scaled triangle filter of PIL / torch ``antialias=True``,
    half-pixel centres) of x (fp32 [N, HS, WS, C]) to ``resize`` = (HR, WR) and centre crop (floor
    offset) to ``size`` = (H, W), by the kernel in csrc/kernels/resize_crop_aa.hip; bit-identical
    to ``InputResize(..., antialias=True).apply`` (gale/models/preprocess.py). ``tables``:
    ``resize_aa_tables(...)`` of the same dimensions on x's device, to reuse them across calls.
    Returns fp32 [N, H, W, C]."""
    _check(x, torch.float32, "x")
    if x.dim() != 4:
        raise ValueError("gale op: x must be [N, HS, WS, C]")
    N, HS, WS, C = x.shape
    (HR, WR), (H, W) = resize, size
    if N > 65535 or C < 1:
        raise ValueError("gale op: resize_crop_aa needs N <= 65535 images and C >= 1")
    if tables is None:
        tables = resize_aa_tables(HS, WS, HR, WR, H, W, x.device)  # (ValueError on bad sizes)
    if not isinstance(tables, ResizeAaTables) or tables.dims != (HS, WS, HR, WR, H, W):
        raise ValueError("gale op: resize_crop_aa tables do not match x, resize and size")
    for t in tables.tensors:
        if not t.is_cuda or t.device != x.device:
            raise ValueError("gale op: resize_crop_aa tables must be on x's device")
    out = torch.empty(N, H, W, C, device=x.device, dtype=torch.float32)
    if N == 0:
        return out
    native().resize_crop_aa(N, [HS, WS, HR, WR, H, W, C], tables.ptrs(), list(tables.launch),
                            x.data_ptr(), out.data_ptr(), _stream())
    return out


def batchnorm(x: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor],
              relu: bool = False, residual: Optional[torch.Tensor] = None,
              res_mode: str = "identity", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Inference BatchNorm as a per-channel affine (scale = gamma/sqrt(var+eps),
    shift = beta - mean*scale; None = identity), + optional residual + ReLU. x: [B,H,W,C] bf16
    (C % 8 == 0); scale/shift: fp32 [>= C]. ``res_mode="pad"``: ResNet option-A shortcut
    (residual read at (2h, 2w), zero above its channel count). ``out`` may alias ``x``."""
    _check(x, torch.bfloat16, "x")
    B, H, W, C = x.shape
    if C % 8:
        raise ValueError("batchnorm: channel count must be a multiple of 8")
    sp = hp = 0
    if scale is not None:
        _check(scale, torch.float32, "scale")
        _check(shift, torch.float32, "shift")
        if scale.device != x.device or shift.device != x.device:
            raise ValueError("batchnorm: scale/shift must be on x's device")
        if scale.numel() < C or shift.numel() < C:
            raise ValueError("batchnorm: scale/shift shorter than the channel count")
        sp, hp = scale.data_ptr(), shift.data_ptr()
    rp, rh, rw, rc, rs = 0, 0, 0, 0, 1
    if residual is not None:
        _check(residual, torch.bfloat16, "residual")
        if residual.device != x.device:
            raise ValueError("batchnorm: residual must be on x's device")
        rb, rh, rw, rc = residual.shape
        if res_mode not in ("identity", "pad"):
            raise ValueError(f"batchnorm: unknown res_mode {res_mode!r}")
        rs = 2 if res_mode == "pad" else 1
        if rb != B:
            raise ValueError(f"batchnorm: residual batch {rb} != {B}")
        if res_mode == "identity" and (rh, rw, rc) != (H, W, C):
            raise ValueError(f"batchnorm: identity residual {tuple(residual.shape)} != "
                             f"{tuple(x.shape)}")
        if res_mode == "pad" and (rh < 2 * (H - 1) + 1 or rw < 2 * (W - 1) + 1 or rc > C):
            raise ValueError(f"batchnorm: pad residual {tuple(residual.shape)} does not cover "
                             f"{tuple(x.shape)} at stride 2")
        rp = residual.data_ptr()
    if out is None:
        y = torch.empty_like(x)
    else:
        _check(out, torch.bfloat16, "out")
        if out.shape != x.shape or out.device != x.device:
            raise ValueError(f"batchnorm: out {tuple(out.shape)} on {out.device} must match x "
                             f"{tuple(x.shape)} on {x.device}")
        y = out
    native().bn_act(B, H * W, W, C, x.data_ptr(), sp, hp, rp, rh, rw, rc, rs, int(relu),
                    y.data_ptr(), _stream())
    return y


def relu(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Standalone ReLU over a bf16 NHWC tensor (the conv epilogue fuses it on the fast path)."""
    return batchnorm(x, None, None, relu=True, out=out)


def cast_bf16(x: torch.Tensor, scale: float = 1.0, shift: float = 0.0) -> torch.Tensor:
    _check(x, torch.float32, "x")
    y = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    native().cast_f32_bf16(x.numel(), scale, shift, x.data_ptr(), y.data_ptr(), _stream())
    return y


def b64_decode_instances(staged: torch.Tensor, table: torch.Tensor, shape, out: torch.Tensor,
                         status: torch.Tensor, images: Optional[int] = None,
                         d_images: Optional[torch.Tensor] = None, prep=None) -> torch.Tensor:
    """Decode base64 uint8 image strings (input format ``b64``) into the fp32 NHWC batch tensor
    ``out`` [slots, H, W, C], in place; returns ``out``.

    ``staged``: uint8 bytes holding the strings, with 16 readable bytes past the last one.
    ``table``: int32 [n, 4] descriptors, one per image: the int64 byte offset of the string's
    first character (low word, high word), its slot in ``out`` and its record's index in
    ``status`` (int32, zeroed by the caller; a record with a bad character gets 2). ``d_images``:
    an int32 device word holding the image count (the launch is then sized for ``images``, or
    the whole table). ``prep``: a ``gale.models.preprocess.InputPrep``."""
    H, W, C = (int(v) for v in shape)
    _check(staged, torch.uint8, "staged")
    _check(table, torch.int32, "table")
    _check(out, torch.float32, "out")
    _check(status, torch.int32, "status")
    if table.dim() != 2 or table.shape[1] != native().B64_IMAGE_BYTES // 4:
        raise ValueError("gale op: table must be int32 [images, 4]")
    n = table.shape[0] if images is None else int(images)
    if n > table.shape[0]:
        raise ValueError("gale op: more images than descriptors")
    if out.numel() % (H * W * C) != 0:
        raise ValueError("gale op: out must hold whole [H, W, C] images")
    if d_images is not None:
        _check(d_images, torch.int32, "d_images")
    kw = prep.kernel_kwargs() if prep is not None else {}
    native().b64_decode_instances(n, table.data_ptr(), staged.data_ptr(), H, W, C,
                                  out.data_ptr(), status.data_ptr(), _stream(),
                                  d_images.data_ptr() if d_images is not None else 0, **kw)
    return out


def b64_yuv_instances(staged: torch.Tensor, table: torch.Tensor, size, out: torch.Tensor,
                      status: torch.Tensor, yuv, images: Optional[int] = None,
                      d_images: Optional[torch.Tensor] = None, prep=None,
                      pairs: int = 0) -> torch.Tensor:
    """Decode base64 YUV 4:2:0 frame strings (``--input-pixel-format i420 | nv12``) into the fp32
    NHWC batch tensor ``out`` [slots, HS, WS, 3] as RGB, in place; returns ``out``.

    ``staged`` / ``table`` / ``status`` / ``images`` / ``d_images`` / ``prep``: as
    ``b64_decode_instances`` (both launch forms). ``size``: (HS, WS), both even; every string is
    4 * (HS*WS*3/2) / 3 characters. ``yuv``: a ``gale.models.preprocess.YuvConvert`` (format and
    coefficient table). ``pairs``: row pairs per workgroup (0 = the launcher's choice). A shape or
    argument the launcher refuses raises ``ValueError`` before anything is launched."""
    HS, WS = (int(v) for v in size)
    _check(staged, torch.uint8, "staged")
    _check(table, torch.int32, "table")
    _check(out, torch.float32, "out")
    _check(status, torch.int32, "status")
    if table.dim() != 2 or table.shape[1] != native().B64_IMAGE_BYTES // 4:
        raise ValueError("gale op: table must be int32 [images, 4]")
    n = table.shape[0] if images is None else int(images)
    if n > table.shape[0]:
        raise ValueError("gale op: more images than descriptors")
    if HS > 0 and WS > 0 and out.numel() % (HS * WS * 3) != 0:
        raise ValueError("gale op: out must hold whole [HS, WS, 3] images")
    if d_images is not None:
        _check(d_images, torch.int32, "d_images")
    kw = prep.kernel_kwargs() if prep is not None else {}
    err = native().b64_yuv_instances(n, table.data_ptr(), staged.data_ptr(), HS, WS, 3,
                                     out.data_ptr(), status.data_ptr(), _stream(),
                                     d_images.data_ptr() if d_images is not None else 0,
                                     pairs=int(pairs), **yuv.kernel_kwargs(), **kw)
    if err == native().HIP_ERROR_INVALID_VALUE:
        raise ValueError(f"b64_yuv_instances: the launcher refused {HS}x{WS} {yuv.format} "
                         f"(pairs={pairs}, images={n})")
    if err != 0:
        raise RuntimeError(f"b64_yuv_instances: HIP error {err}")
    return out


def b64_packed_instances(staged: torch.Tensor, table: torch.Tensor, size, out: torch.Tensor,
                         status: torch.Tensor, unpack, images: Optional[int] = None,
                         d_images: Optional[torch.Tensor] = None, prep=None) -> torch.Tensor:
    """Decode base64 packed-pixel strings (``--input-pixel-format bgr24 | rgba | bgra | gray``)
    into the fp32 NHWC batch tensor ``out`` [slots, HS, WS, 3] as RGB, in place; returns ``out``.

    ``staged`` / ``table`` / ``status`` / ``images`` / ``d_images`` / ``prep``: as
    ``b64_decode_instances`` (both launch forms; the prep's coefficients are indexed by model
    channel). ``size``: (HS, WS); every string is 4 * ceil(HS*WS*P / 3) characters. ``unpack``:
    a ``gale.models.preprocess.PixelUnpack``. A shape or argument the launcher refuses raises
    ``ValueError`` before anything is launched."""
    HS, WS = (int(v) for v in size)
    _check(staged, torch.uint8, "staged")
    _check(table, torch.int32, "table")
    _check(out, torch.float32, "out")
    _check(status, torch.int32, "status")
    if table.dim() != 2 or table.shape[1] != native().B64_IMAGE_BYTES // 4:
        raise ValueError("gale op: table must be int32 [images, 4]")
    n = table.shape[0] if images is None else int(images)
    if n > table.shape[0]:
        raise ValueError("gale op: more images than descriptors")
    if HS > 0 and WS > 0 and out.numel() % (HS * WS * 3) != 0:
        raise ValueError("gale op: out must hold whole [HS, WS, 3] images")
    if d_images is not None:
        _check(d_images, torch.int32, "d_images")
    kw = prep.kernel_kwargs() if prep is not None else {}
    err = native().b64_packed_instances(n, table.data_ptr(), staged.data_ptr(), HS, WS, 3,
                                        out.data_ptr(), status.data_ptr(), _stream(),
                                        d_images.data_ptr() if d_images is not None else 0,
                                        **unpack.kernel_kwargs(), **kw)
    if err == native().HIP_ERROR_INVALID_VALUE:
        raise ValueError(f"b64_packed_instances: the launcher refused {HS}x{WS} "
                         f"{unpack.format} (images={n})")
    if err != 0:
        raise RuntimeError(f"b64_packed_instances: HIP error {err}")
    return out


def b64_typed_instances(staged: torch.Tensor, table: torch.Tensor, shape, out: torch.Tensor,
                        status: torch.Tensor, elem, images: Optional[int] = None,
                        d_images: Optional[torch.Tensor] = None, prep=None) -> torch.Tensor:
    """Decode base64 typed tensor strings (``--input-dtype u16 | f16 | bf16 | f32``) into the fp32
    NHWC batch tensor ``out`` [slots, HS, WS, C], in place; returns ``out``.

    ``staged`` / ``table`` / ``status`` / ``images`` / ``d_images`` / ``prep``: as
    ``b64_decode_instances`` (both launch forms, either layout; a record with a bad character or
    a non-finite element gets status 2). ``shape``: (HS, WS, C); every string is
    4 * ceil(HS*WS*C*E / 3) characters. ``elem``: a ``gale.models.preprocess.ElemType``. A shape or
    argument the launcher refuses raises ``ValueError`` before anything is launched."""
    HS, WS, C = (int(v) for v in shape)
    _check(staged, torch.uint8, "staged")
    _check(table, torch.int32, "table")
    _check(out, torch.float32, "out")
    _check(status, torch.int32, "status")
    if table.dim() != 2 or table.shape[1] != native().B64_IMAGE_BYTES // 4:
        raise ValueError("gale op: table must be int32 [images, 4]")
    n = table.shape[0] if images is None else int(images)
    if n > table.shape[0]:
        raise ValueError("gale op: more images than descriptors")
    if HS > 0 and WS > 0 and C > 0 and out.numel() % (HS * WS * C) != 0:
        raise ValueError("gale op: out must hold whole [HS, WS, C] images")
    if d_images is not None:
        _check(d_images, torch.int32, "d_images")
    kw = prep.kernel_kwargs() if prep is not None else {}
    err = native().b64_typed_instances(n, table.data_ptr(), staged.data_ptr(), HS, WS, C,
                                       out.data_ptr(), status.data_ptr(), _stream(),
                                       d_images.data_ptr() if d_images is not None else 0,
                                       **elem.kernel_kwargs(), **kw)
    if err == native().HIP_ERROR_INVALID_VALUE:
        raise ValueError(f"b64_typed_instances: the launcher refused {HS}x{WS}x{C} "
                         f"{elem.dtype} (images={n})")
    if err != 0:
        raise RuntimeError(f"b64_typed_instances: HIP error {err}")
    return out


def ingest_crc_b64(staged: torch.Tensor, shape, arena: Optional[torch.Tensor] = None,
                   table: Optional[torch.Tensor] = None, wg_bad: Optional[torch.Tensor] = None,
                   windows: Optional[torch.Tensor] = None, tables: Optional[torch.Tensor] = None,
                   crc_out: Optional[torch.Tensor] = None, prep=None) -> None:
    """The device ingest of a fetch of base64 image records in ONE launch: the raw CRC32C of
    ``windows`` into ``crc_out`` and every string of ``table`` decoded into ``arena``.

    ``staged``: uint8 bytes (the fetch's device mirror), with 16 readable bytes past the last
    string. ``table``: int32 [n, 4] descriptors as for ``b64_decode_instances`` (the record index
    is not read); ``arena``: fp32, whole [H, W, C] slots; ``wg_bad``: int32, one word per decode
    workgroup (n * ceil(L / B64_CHUNK_CHARS)), every one of them written: 2 = a bad character
    or bad padding in that chunk, else 0. ``windows``: int32 [m, 4] CRC windows (int64 end, int32
    length, pad), ``tables``: the device CRC tables, ``crc_out``: uint32-as-int32 [m]. Either
    half may be left out."""
    H, W, C = (int(v) for v in shape)
    _check(staged, torch.uint8, "staged")
    n = m = 0
    if table is not None:
        _check(table, torch.int32, "table")
        _check(arena, torch.float32, "arena")
        _check(wg_bad, torch.int32, "wg_bad")
        if table.dim() != 2 or table.shape[1] != native().B64_IMAGE_BYTES // 4:
            raise ValueError("gale op: table must be int32 [images, 4]")
        n = table.shape[0]
        per = H * W * C
        if arena.numel() % per != 0:
            raise ValueError("gale op: arena must hold whole [H, W, C] images")
        chars = 4 * ((per + 2) // 3)
        cpi = -(-chars // native().B64_CHUNK_CHARS)
        if wg_bad.numel() < n * cpi:
            raise ValueError("gale op: wg_bad needs one word per decode workgroup")
    if windows is not None:
        _check(windows, torch.int32, "windows")
        _check(tables, torch.int32, "tables")
        _check(crc_out, torch.int32, "crc_out")
        if windows.dim() != 2 or windows.shape[1] != 4:
            raise ValueError("gale op: windows must be int32 [windows, 4]")
        m = windows.shape[0]
        if crc_out.numel() < m:
            raise ValueError("gale op: crc_out shorter than the windows")
    kw = prep.kernel_kwargs() if prep is not None else {}
    native().ingest_crc_b64(staged.data_ptr(), windows.data_ptr() if m else 0, m,
                            tables.data_ptr() if m else 0, crc_out.data_ptr() if m else 0, n,
                            table.data_ptr() if n else 0, H, W, C,
                            arena.data_ptr() if n else 0, wg_bad.data_ptr() if n else 0,
                            _stream(), **kw)


# ---- fp8 (OCP e4m3fn) path: tensors of e4m3 codes are uint8 --------------------------------


def pack_conv_fp8(w_oihw: torch.Tensor, bias: torch.Tensor, cin_stored: Optional[int] = None,
                  device=None):
    """Pack an fp32 conv weight as e4m3 codes with per-output-channel scales.

    Returns (w codes uint8 [Npad, Kpad], bias fp32 [Npad], wscale fp32 [Npad], geometry dict).
    """
    from gale.models.quant import quantize_rows_e4m3

    cout, cin, kh, kw = w_oihw.shape
    cin_s = cin if cin_stored is None else cin_stored
    cout_s = round_up(cout, 4)
    K = kh * kw * cin_s
    Kpad = round_up(K, 32)
    Npad = round_up(cout_s, conv_n_tiles(cout_s) * 16)
    q, s = quantize_rows_e4m3(pack_conv_weight(w_oihw.float().cpu(), cin_s, Npad, Kpad))
    bp = torch.zeros(Npad)
    bp[:cout] = bias.float().cpu()
    dev = device if device is not None else torch.device("cuda")
    return q.to(dev), bp.to(dev), s.to(dev), dict(Cin=cin_s, Cout=cout_s, KH=kh, KW=kw, K=K,
                                                   Kpad=Kpad, Npad=Npad)


def conv2d_fp8(x: torch.Tensor, w_codes: torch.Tensor, bias: torch.Tensor, wscale: torch.Tensor,
               geom: dict, in_scale: float, out_scale: float = 1.0, stride: int = 1, pad: int = 0,
               relu: bool = False, residual: Optional[torch.Tensor] = None,
               res_scale: float = 1.0, res_mode: str = "identity",
               out_f32: bool = False) -> torch.Tensor:
    """NHWC conv on fp8 MFMA. x: e4m3 codes (uint8, value = code * in_scale) or fp32 (quantised
    with step in_scale while loaded). Returns e4m3 codes at out_scale, or fp32 (out_f32)."""
    B, H, W, C = x.shape
    if C != geom["Cin"]:
        raise ValueError(f"x has {C} channels, packed weight expects {geom['Cin']}")
    _check(w_codes, torch.uint8, "w_codes")
    _check(bias, torch.float32, "bias")
    _check(wscale, torch.float32, "wscale")
    if x.dtype not in (torch.uint8, torch.float32):
        raise TypeError("x must be e4m3 codes (uint8) or fp32")
    _check(x, x.dtype, "x")
    kh, kw = geom["KH"], geom["KW"]
    Ho = (H + 2 * pad - kh) // stride + 1
    Wo = (W + 2 * pad - kw) // stride + 1
    y = torch.empty(B, Ho, Wo, geom["Cout"], device=x.device,
                    dtype=torch.float32 if out_f32 else torch.uint8)
    d = dict(geom, H=H, W=W, Ho=Ho, Wo=Wo, stride=stride, pad=pad, relu=int(relu),
             in_f32=int(x.dtype == torch.float32), out_f32=int(out_f32), fp8=1,
             in_scale=float(in_scale), out_scale=float(out_scale), res_scale=float(res_scale))
    res_ptr = 0
    if residual is not None:
        _check(residual, torch.uint8, "residual")
        _, rh, rw, rc = residual.shape
        d.update(has_res=1, res_H=rh, res_W=rw, res_C=rc, res_stride=2 if res_mode == "pad" else 1)
        res_ptr = residual.data_ptr()
    native().conv2d(d, B, x.data_ptr(), w_codes.data_ptr(), bias.data_ptr(), wscale.data_ptr(),
                    res_ptr, y.data_ptr(), _stream())
    return y


def maxpool2d_fp8(x: torch.Tensor, k: int, s: int, p: int = 0) -> torch.Tensor:
    _check(x, torch.uint8, "x")
    B, H, W, C = x.shape
    Ho = (H + 2 * p - k) // s + 1
    Wo = (W + 2 * p - k) // s + 1
    y = torch.empty(B, Ho, Wo, C, device=x.device, dtype=torch.uint8)
    native().maxpool2d(B, H, W, C, k, s, p, Ho, Wo, x.data_ptr(), y.data_ptr(), _stream(), 1)
    return y


def avgpool_global_fp8(x: torch.Tensor) -> torch.Tensor:
    _check(x, torch.uint8, "x")
    B, H, W, C = x.shape
    y = torch.empty(B, C, device=x.device, dtype=torch.uint8)
    native().avgpool_global(B, H * W, C, x.data_ptr(), y.data_ptr(), _stream(), 1)
    return y


def head_fp8(x: torch.Tensor, in_scale: float, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    _check(x, torch.uint8, "x")
    _check(w, torch.float32, "w")
    _check(b, torch.float32, "b")
    B, H, W, C = x.shape
    N = w.shape[0]
    out = torch.empty(B, N, device=x.device, dtype=torch.float32)
    native().head_pool_dense_softmax(B, H * W, C, N, x.data_ptr(), w.data_ptr(), b.data_ptr(),
                                     out.data_ptr(), _stream(), 1, float(in_scale))
    return out
