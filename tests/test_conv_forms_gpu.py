"""The batch-selected launch forms of the MFMA conv (csrc/kernels/conv_mfma.hip), bit-exact.

conv2d() picks the kernel instantiation (pixel tiles per wave PR, hence the register double
buffer's group size U = 8 / PR) and the grid (a grid-stride walk over the pixel tiles when the
weights stay resident) from the size of the launch. The small batches of test_kernels_gpu.py all
end at PR = 1 with one workgroup per tile; the cases of conv_forms.py are the smallest launches
that select every other form, in bf16 and in fp8.

The checks have no tolerance. Inputs and residuals are integers in [-3, 3], weights multiples of
0.25 in [-0.75, 0.75] with one 0.875 per row (which makes the fp8 row scale exactly 2^-9 and every
code exact), biases multiples of 0.25: every operand is exact in bf16 and in e4m3 and every
partial sum is an exact fp32 value (K <= 4608: below 2^24 quanta), so the fp32 CPU convolution of
the same values is the exact result whatever its summation order and the kernel's only rounding
is the one to its output type. y is prefilled with a NaN pattern no launch can produce and is one
256-row tile longer than M: a tile the walk skipped shows up as NaNs inside, a write past M in the
tail. Each test first asserts, through conv_mfma_plan() and conv_route(), the kernel and form it
is about to launch.
"""

import pytest
import torch
import torch.nn.functional as F

import conv_forms
from gale import ops
from gale._native import native
from gale.models.quant import e4m3_codes, e4m3_round

pytestmark = pytest.mark.gpu

DEV = "cuda"
TAIL_ROWS = 256
# bit patterns of a NaN in each output type: the kernel's outputs are finite (fp8 saturates)
SENTINEL = {torch.bfloat16: (torch.int16, 0x7FC1), torch.uint8: (torch.uint8, 0x7F),
            torch.float32: (torch.int32, 0x7FC00001)}

_operands = {}  # the operands and exact reference of the case run last (bf16 and fp8 share them)


def _case(f):
    if f.name not in _operands:
        _operands.clear()
        g = torch.Generator().manual_seed(4100 + conv_forms.FORMS.index(f))
        x = torch.randint(-3, 4, (f.B, f.H, f.W, f.Cin), generator=g).float()
        w = torch.randint(-3, 4, (f.Cout, f.Cin, f.k, f.k), generator=g).float() * 0.25
        w[:, 0, 0, 0] = 0.875
        b = torch.randint(-8, 9, (f.Cout,), generator=g).float() * 0.25
        b[b == 0] = 0.25
        Ho, Wo = conv_forms.out_size(f)
        res = None
        y = F.conv2d(x.permute(0, 3, 1, 2), w, b, stride=f.stride, padding=f.pad)
        if f.res == "identity":
            res = torch.randint(-3, 4, (f.B, Ho, Wo, f.Cout), generator=g).float()
            y = y + res.permute(0, 3, 1, 2)
        elif f.res == "pad":
            res = x
            r = x.permute(0, 3, 1, 2)[:, :, ::2, ::2]
            y = y + F.pad(r, (0, 0, 0, 0, 0, f.Cout - f.Cin))
        if f.relu:
            y = F.relu(y)
        ref = y.permute(0, 2, 3, 1).reshape(f.B * Ho * Wo, f.Cout).contiguous()
        _operands[f.name] = (x, w, b, res, ref)
    return _operands[f.name]


def _launch(f, fp8, x, wp, bp, ws, geom, res, out_dtype, out_scale=1.0):
    """One conv2d launch of the case into a sentinel-filled y with a spare tile; returns the
    body [M, Cout] on the host after checking the spare tile."""
    C = native()
    assert geom == conv_forms.geometry(f)
    d = dict(conv_forms.desc(f, fp8, geom), in_scale=1.0, res_scale=1.0, out_scale=out_scale)
    conv_forms.check_plan(C.conv_mfma_plan(d, f.B, res is not None), f, fp8)
    Ho, Wo = conv_forms.out_size(f)
    M = f.B * Ho * Wo
    bits, pattern = SENTINEL[out_dtype]
    y = torch.full((M + TAIL_ROWS, geom["Cout"]), pattern, dtype=bits, device=DEV)
    force = not fp8 and f.Cin % 64 == 0  # wide bf16 layers would take the patch / GEMM kernels
    try:
        if force:
            C.set_conv_path(1)
        route = C.conv_route(d, f.B, res is not None)
        assert route["kernel"] == "mfma"
        conv_forms.check_plan(route, f, fp8)
        C.conv2d(d, f.B, x.data_ptr(), wp.data_ptr(), bp.data_ptr(),
                 ws.data_ptr() if fp8 else 0, res.data_ptr() if res is not None else 0,
                 y.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        if force:
            C.set_conv_path(0)
    y = y.cpu()
    assert torch.equal(y[M:], torch.full_like(y[M:], pattern)), "write past M"
    body = y[:M]
    skipped = int((body == pattern).all(dim=1).sum())
    assert skipped == 0, f"{skipped} output rows never written"
    return body.view(out_dtype)


def _run_bf16(f):
    x, w, b, res, ref = _case(f)
    wp, bp, geom = ops.pack_conv(w, b)
    xd = (x if f.in_f32 else x.to(torch.bfloat16)).to(DEV)
    rd = None if res is None else res.to(torch.bfloat16).to(DEV)
    out_dtype = torch.float32 if f.out_f32 else torch.bfloat16
    y = _launch(f, False, xd, wp, bp, None, geom, rd, out_dtype)
    assert torch.equal(y, ref.to(out_dtype))


def _run_fp8(f):
    x, w, b, res, ref = _case(f)
    wq, bq, ws, geom = ops.pack_conv_fp8(w, b)
    assert torch.equal(ws[:f.Cout].cpu(), torch.full((f.Cout,), 2.0 ** -9))
    xd = (x if f.in_f32 else e4m3_codes(x)).to(DEV)
    rd = None if res is None else e4m3_codes(res).to(DEV)
    if f.out_f32:
        y = _launch(f, True, xd, wq, bq, ws, geom, rd, torch.float32)
        assert torch.equal(y, ref)
        return
    # the smallest power of two that keeps every output inside e4m3's range
    out_scale, amax = 1.0, float(ref.abs().max())
    while amax / out_scale > 448:
        out_scale *= 2
    while amax / (out_scale / 2) <= 448:
        out_scale /= 2
    y = _launch(f, True, xd, wq, bq, ws, geom, rd, torch.uint8, out_scale)
    assert torch.equal(y.view(torch.float8_e4m3fn).float(), e4m3_round(ref / out_scale))


# (the form is the outer loop: both types of a case run back to back on one reference)
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("form", conv_forms.FORMS, ids=lambda f: f.name)
def test_conv_form_exact(form, dtype):
    (_run_fp8 if dtype == "fp8" else _run_bf16)(form)
