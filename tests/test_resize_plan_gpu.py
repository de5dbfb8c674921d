"""The byte layout a replica uploads for its input resize (pack, csrc/runtime/resize_plan.h)
under the kernels: the packed image goes to the device as ONE uint8 tensor and the six table
pointers of the resize_crop / resize_crop_aa bindings are base + the image's offsets, with the
launch figures taken from the image. Both forms of the launch, bit-exact against the numpy
oracle ``InputResize.apply``; the image is also placed 16 bytes into a larger tensor, so that
the base is not an allocation's start.

As in tests/test_input_antialias_gpu.py, dst lies inside a larger device tensor filled with a
sentinel bit pattern and src at the very end of its tensor, behind NaNs; every "untouched" claim
is checked against the sentinel."""

import numpy as np
import pytest
import torch

from gale._native import native
from gale.models.preprocess import InputResize
from test_input_antialias_cpu import random_images, u32

pytestmark = pytest.mark.gpu

C = native()
SENTINEL = np.uint32(0xEEEEEEEE)
PAD = 64  # sentinel floats before and after dst
N = 3     # images; the _dev form runs with a device count of 2 against this launch size

# (HS, WS, HR, WR, H, W, C)
SMALL = (21, 11, 7, 9, 5, 7, 3)      # tables of 20 / 28 bytes: every section is padded;
                                     # antialiased ty = 5 != tx = 3; rows of 21 floats
VEC = (40, 36, 34, 33, 32, 32, 3)    # 16-byte stores
EIGHT = (64, 40, 8, 5, 8, 4, 2)      # antialiased only: 16 taps on both axes, band 4
CASES = [(SMALL, False), (VEC, False), (SMALL, True), (VEC, True), (EIGHT, True)]


def stream():
    return torch.cuda.current_stream().cuda_stream


def sentinel_tensor(n):
    return torch.full((n,), int(SENTINEL.view(np.int32)), dtype=torch.int32, device="cuda")


def place_src(x):
    """x at the very end of a device tensor, NaNs before it."""
    buf = torch.full((37 + x.size,), float("nan"), dtype=torch.float32, device="cuda")
    buf[37:] = torch.from_numpy(x.reshape(-1)).cuda()
    return buf, buf[37:].data_ptr()


def upload(dims, antialias, lead):
    """The packed image as one uint8 device tensor, `lead` bytes into it; returns the tensor, the
    six pointers base + offset and the launch figures."""
    blob, offs, fig = C.resize_device_image(*dims[:6], antialias)
    buf = torch.full((lead + blob.size + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[lead:lead + blob.size] = torch.from_numpy(blob).cuda()
    base = buf.data_ptr() + lead
    assert base % 16 == 0
    return buf, [base + o for o in offs], list(fig)


def run_kernel(dims, antialias, x, lead, count=None):
    """Launch over the N images of x (count: the _dev form's device word); returns the whole dst
    tensor's words and the per-image float count."""
    HS, WS, HR, WR, H, W, Ch = dims
    tables, ptrs, fig = upload(dims, antialias, lead)
    per = H * W * Ch
    big = sentinel_tensor(PAD + N * per + PAD)
    src_buf, src = place_src(x)
    dst = big[PAD:].data_ptr()
    d = torch.tensor([0 if count is None else count], dtype=torch.int32, device="cuda")
    if antialias and count is None:
        C.resize_crop_aa(N, list(dims), ptrs, fig, src, dst, stream())
    elif antialias:
        C.resize_crop_aa_dev(N, d.data_ptr(), list(dims), ptrs, fig, src, dst, stream())
    elif count is None:
        C.resize_crop(N, HS, WS, H, W, Ch, ptrs, src, dst, stream())
    else:
        C.resize_crop_dev(N, d.data_ptr(), HS, WS, H, W, Ch, ptrs, src, dst, stream())
    torch.cuda.synchronize()
    return big.cpu().numpy().view(np.uint32), per


def check(words, per, want, written):
    """Images [0, written) hold the oracle's bits; every other word holds the sentinel."""
    assert np.array_equal(words[PAD:PAD + written * per], u32(want[:written]).reshape(-1))
    assert (words[:PAD] == SENTINEL).all()
    assert (words[PAD + written * per:] == SENTINEL).all()


@pytest.fixture(scope="module")
def cases():
    """Per shape and form: N random images (both signs, several binades) and the oracle's output."""
    out = {}
    for dims, antialias in CASES:
        HS, WS, HR, WR, H, W, Ch = dims
        x = random_images(np.random.default_rng(HS * 1000 + WS), N, HS, WS, Ch)
        out[dims, antialias] = (x, InputResize(HS, WS, HR, WR, H, W, antialias=antialias).apply(x))
    return out


def test_the_shapes_are_what_the_cases_claim():
    for antialias in (False, True):
        blob, offs, fig = C.resize_device_image(*SMALL[:6], antialias)
        ty, tx = fig[:2] if antialias else (1, 1)
        assert all(b - a > 4 * n for a, b, n in zip(offs, list(offs[1:]) + [blob.size],
                                                    (5, 5, 5 * ty, 7, 7, 7 * tx)))  # padded
    assert tuple(C.resize_device_image(*SMALL[:6], True)[2][:2]) == (5, 3)
    assert (SMALL[5] * SMALL[6]) % 4 != 0 and (VEC[5] * VEC[6]) % 4 == 0
    ty, tx, band, rows = C.resize_device_image(*EIGHT[:6], True)[2]
    assert (ty, tx, band) == (16, 16, 4) and rows + tx <= 64


@pytest.mark.parametrize("dims,antialias", CASES,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else
                         ("aa" if v else "plain"))
def test_kernels_read_the_packed_image_in_both_forms(cases, dims, antialias):
    x, want = cases[dims, antialias]
    for lead in (0, 16):  # the image at the start of its allocation / 16 bytes into it
        check(*run_kernel(dims, antialias, x, lead), want, N)
        check(*run_kernel(dims, antialias, x, lead, count=2), want, 2)
