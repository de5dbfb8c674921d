"""gale.ops.raw_instances (csrc/kernels/raw_convert.hip) bit for bit against the numpy oracles
(ElemType.apply, PixelUnpack.apply, fma_f32 through InputPrep.apply). A workgroup owns 4096 floats
of an image, a wave 1024, a lane four 16-byte units: the shapes are the smallest across those."""

import numpy as np
import pytest
import torch

from gale import ops
from gale._native import native
from gale.models.preprocess import ElemType, InputPrep
from test_input_raw_cpu import ELEMS, PACKED, bits, finite_wire, oracle

pytestmark = pytest.mark.gpu

C = native()
IMG = np.dtype([("off", "<i8"), ("slot", "<i4"), ("rec", "<i4")])
SENTINEL = float(np.float32(-7.0000005))   # (no converted value of these tests' data)
CIFAR = dict(mean="0.4914,0.4822,0.4465", std="0.2470,0.2435,0.2616")
PREPS = {1: InputPrep.build(1, 1 / 255, "0.1307", "0.3081"),
         3: InputPrep.build(3, 1 / 255, CIFAR["mean"], CIFAR["std"]),
         5: InputPrep.build(5, 1 / 255, "0.5", "0.25")}            # (C > 4: uniform)
SLOTS, GUARD = (3, 0, 4), 4     # image i -> slot SLOTS[i] of 5; slots 1 and 2 stay sentinel
# 1 and 105 floats: less than a lane's units. 3069: no multiple of 4, so slots 3 and 4 start off
# a 16-byte boundary. 5166 = 4096 + 1024 + 46: a second workgroup, ending inside its second wave
SIZES = [(1, 1), (5, 7), (33, 31), (42, 41)]


def convert(kind, wire, shape, prep, ph0, ph1, header=None, skew=0):
    """wire [3, B]: image 0 is record 0, staged at byte phase ph0 modulo 16; images 1 and 2 back
    to back are record 1, at ph1. Returns (floats [5 slots, HS, WS, C], status [2]) after checking
    the guard floats around the tensor. skew: the staged tensor is a slice starting that many bytes
    into its allocation (ph0 and ph1 are then phases of the offsets, not of the addresses)."""
    HS, WS, CH = shape
    B, per = wire.shape[1], HS * WS * CH
    o0 = 16 + ph0
    o1 = (o0 + B + 15) // 16 * 16 + 16 + ph1
    buf = np.full(o1 + 2 * B + 3 & ~3, 0xEE, np.uint8)   # (whole dwords, nothing to spare)
    buf[o0:o0 + B], buf[o1:o1 + 2 * B] = wire[0], wire[1:].ravel()
    tab = np.zeros(3, dtype=IMG)
    tab["off"], tab["slot"], tab["rec"] = (o0, o1, o1 + B), SLOTS, (0, 1, 1)
    flat = torch.full((2 * GUARD + 5 * per,), SENTINEL, device="cuda")
    out = flat[GUARD:GUARD + 5 * per]
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    fmt = kind if kind in PACKED else "rgb"
    ops.raw_instances(torch.from_numpy(np.concatenate([buf[:skew], buf])).cuda()[skew:],
                      torch.from_numpy(tab.view(np.int32).reshape(-1, 4).copy()).cuda(), shape,
                      out, status, dtype="u8" if kind in PACKED else kind, pixel_format=fmt,
                      d_images=None if header is None else
                      torch.tensor([header], dtype=torch.int32, device="cuda"), prep=prep)
    torch.cuda.synchronize()
    f = flat.cpu().numpy()
    assert (f[:GUARD] == SENTINEL).all() and (f[-GUARD:] == SENTINEL).all()
    return f[GUARD:-GUARD].reshape(5, *shape), status.cpu().numpy()


NCHW = InputPrep.build(3, 1 / 255, [0.1, 0.2, 0.3], [0.25], layout="nchw")
CASES = [(k, size + (c,), prep) for size in SIZES for k in ELEMS + PACKED
         for c in ((3,) if k in PACKED else (3, 1)) for prep in (None, PREPS[c])]
CASES += [("bf16", (5, 7, 5), None), ("bf16", (5, 7, 5), PREPS[5])]          # general C
CASES += [(k, size + (3,), NCHW) for size in SIZES[1:3] for k in ELEMS]    # [C][H][W] records


def check(got, status, want):
    assert list(status) == [0, 0]
    assert np.array_equal(bits(got[list(SLOTS)]), want) and (got[[1, 2]] == SENTINEL).all()


@pytest.mark.parametrize("kind,shape,prep", CASES,
                         ids=lambda v: str(v).replace(" ", "") if isinstance(v, (str, tuple))
                         else "id" if v is None else "nchw" if v.nchw else "prep")
def test_against_oracle(kind, shape, prep):
    """Every start phase modulo 16 for both records (image 2 follows image 1, so its phase moves
    by the image's bytes); permuted slots; unused slots and guards untouched; then the staged
    tensor as a slice at byte 5 of its allocation."""
    wire = finite_wire(kind, shape, sum(shape))
    want = bits(oracle(kind, wire, *shape, prep))
    for ph in range(16):
        check(*convert(kind, wire, shape, prep, ph, (3 * ph + 7) % 16), want)
    check(*convert(kind, wire, shape, prep, 0, 8, skew=5), want)


@pytest.mark.parametrize("kind", ["u16", "f16", "bf16"])
def test_every_16_bit_pattern(kind):
    """All 65 536 patterns (the non-finite ones zeroed) three times over, without and with a prep;
    f16 subnormals convert exactly."""
    p = np.arange(65536, dtype="<u2")
    p[ElemType(kind).nonfinite(p.view(np.uint8))] = 0
    wire = np.tile(p.view(np.uint8), (3, 1))
    for prep in (None, PREPS[1]):
        check(*convert(kind, wire, (256, 256, 1), prep, 2, 9),
              bits(oracle(kind, wire, 256, 256, 1, prep)))
    if kind == "f16":
        assert oracle(kind, wire, 256, 256, 1, None).ravel()[1] == 2.0 ** -24


NONFINITE = {"f16": (0x7C00, 0xFE00), "bf16": (0xFF80, 0x7FC1), "f32": (0x7F800000, 0xFFC00001)}


@pytest.mark.parametrize("header", [None, 3, 1])
@pytest.mark.parametrize("el", [0, 33 * 31 * 3 - 1], ids=["first", "last"])
@pytest.mark.parametrize("kind", list(NONFINITE))
def test_verdicts(kind, el, header):
    """Inf and NaN at the first or the last element of record 1's last image: status 2 for that
    record only, every image still written in its slot. header: the device-count form; with a
    count of 1 the images past it are not touched and nothing is judged."""
    shape = (33, 31, 3)
    E = ElemType(kind).bytes_per_element
    clean = finite_wire(kind, shape, E)
    want = bits(oracle(kind, clean, *shape, None)).reshape(3, -1)
    for pattern in NONFINITE[kind]:
        wire = clean.copy()
        wire[2, el * E:(el + 1) * E] = np.frombuffer(int(pattern).to_bytes(E, "little"), np.uint8)
        got, status = convert(kind, wire, shape, None, 6, 13, header=header)
        g = bits(got[list(SLOTS)]).reshape(3, -1)
        if header == 1:
            assert list(status) == [0, 0] and np.array_equal(g[0], want[0])
            assert (got[[1, 2, 0, 4]] == SENTINEL).all()
            continue
        keep = np.ones(g.shape, bool)
        keep[2, el] = False
        assert list(status) == [0, 2] and np.array_equal(g[keep], want[keep])
        assert not np.isfinite(got[SLOTS[2]].ravel()[el]) and (got[[1, 2]] == SENTINEL).all()


REFUSED = {
    "H=0": dict(HS=0), "W<0": dict(WS=-2), "C=0": dict(C=0),
    "imgs": dict(imgs=0), "bytes": dict(bytes=0), "out": dict(out=0), "status": dict(status=0),
    "dtype": dict(dtype="f64"), "format": dict(format="i420"),
    "typed+packed": dict(dtype="f16", format="rgba"),
    "packed C=1": dict(format="gray", C=1), "packed nchw": dict(format="bgr24", nchw=True),
    "images": dict(images=65536), "2^30": dict(HS=16384, WS=16384, C=5),
    "C=5 per-channel": dict(C=5, a=[0.5, 0.5, 0.5, 0.25], b=[0.0] * 4),
}


@pytest.mark.parametrize("why", list(REFUSED))
def test_launcher_refusals(why):
    """hipErrorInvalidValue before any launch; images == 0 launches nothing."""
    out = torch.full((3, 5, 7, 5), SENTINEL, device="cuda")
    status = torch.zeros(3, dtype=torch.int32, device="cuda")
    staged = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    tab = torch.zeros((3, 4), dtype=torch.int32, device="cuda")
    args = dict(images=3, imgs=tab.data_ptr(), bytes=staged.data_ptr(), HS=5, WS=7, C=3,
                out=out.data_ptr(), status=status.data_ptr(),
                stream=torch.cuda.current_stream().cuda_stream)
    assert C.raw_instances(**dict(args, **REFUSED[why])) == C.HIP_ERROR_INVALID_VALUE
    assert C.raw_instances(**dict(args, images=0)) == 0
    if why == "H=0":
        with pytest.raises(ValueError, match="refused"):
            ops.raw_instances(staged, tab, (0, 7, 3), out, status)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item() and not status.any().item()
