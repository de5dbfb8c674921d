"""Raw 8-bit Bayer mosaic records (--input-pixel-format bayer_*8) on the GPU: the kernel of
csrc/kernels/bayer.hip against the numpy oracle (BayerConvert) on the bits, its bounds, the
launcher's refusals, and the engine against raw rgb records of the oracle's image."""

import numpy as np
import pytest
import torch

from gale import ops
from gale._native import native
from gale.data import encode_records_raw
from gale.models.preprocess import BayerConvert
from test_bayer_cpu import ORDERS, PREP, frames_of
from test_input_raw_cpu import CIFAR, serve
from test_raw_engine_gpu import params_for

pytestmark = pytest.mark.gpu

C = native()
IMG = np.dtype([("off", "<i8"), ("slot", "<i4"), ("rec", "<i4")])
SENTINEL = -7.0
SLOTS = [4, 0, 2]  # of five: slots 1 and 3 keep their fill
# 2x2 every neighbour mirrored; 4x6 a tail block of 6 columns; 6x10 a full block and a tail of 2;
# 34x18 many row pairs, WS mod 4 == 2 (8-byte stores, the row phase alternates); 32x32 one wave
# spanning 16 row pairs (the 64-thread launch); 4x520 a row pair longer than a wave's 64 blocks
SHAPES = [(2, 2), (4, 6), (6, 10), (34, 18), (32, 32), (4, 520)]


def staged(frames, phase=0):
    """(device bytes, device descriptor table): frame i at byte phase `phase` of 16 in a buffer
    of guard bytes that ends with the last frame's aligned dword, in slot SLOTS[i]."""
    buf, offs = bytearray(b"\xee" * 16), []
    for fr in frames:
        buf += b"\xee" * ((phase - len(buf)) % 16)
        offs.append(len(buf))
        buf += fr.tobytes()
    buf += b"\xee" * (-len(buf) % 4)
    tab = np.zeros(3, dtype=IMG)
    tab["off"], tab["slot"], tab["rec"] = offs, SLOTS, range(3)
    return (torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).cuda(),
            torch.from_numpy(tab.view(np.int32).reshape(-1, 4).copy()).cuda())


def launch(raw, tab, size, bc, prep=None, out_off=0, **kw):
    """Floats [5, HS, WS, 3] by slot. The guard bands on either side of `out` and every status
    word keep their fill."""
    per = size[0] * size[1] * 3
    flat = torch.full((4 + out_off + 5 * per + 64,), SENTINEL, device="cuda")
    out = flat[4 + out_off:4 + out_off + 5 * per]
    assert out.data_ptr() % 16 == 4 * out_off
    status = torch.full((3,), 77, dtype=torch.int32, device="cuda")
    ops.raw_bayer_instances(raw, tab, size, out, status, bc, prep=prep, **kw)
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    assert (host[:4 + out_off] == SENTINEL).all() and (host[-64:] == SENTINEL).all()
    assert (status.cpu().numpy() == 77).all()
    got = host[4 + out_off:-64].reshape(5, *size, 3)
    assert (got[[1, 3]] == SENTINEL).all()
    return got


# every order x shape with the identity and a per-channel prep at phase 0; at byte phases 1, 2, 3
# and 5; and with `out` 4 bytes off a 16-byte boundary (the unaligned store path)
CASES = [dict(prep=p) for p in (None, PREP)] + [dict(phase=p) for p in (1, 2, 3, 5)] \
    + [dict(out_off=1, prep=PREP)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(
    "cifar" if k == "prep" else f"{k}{v}" for k, v in c.items() if v is not None) or "identity")
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("order", ORDERS)
def test_kernel_equals_the_oracle(order, size, case):
    bc, frames, prep = BayerConvert(order), frames_of(1, *size, size[0] * 1009 + size[1]), \
        case.get("prep")
    got = launch(*staged(frames, case.get("phase", 0)), size, bc, prep, case.get("out_off", 0))
    want = bc.to_float(bc.apply(frames, *size), prep)
    assert np.array_equal(got[SLOTS].view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("order", ORDERS)
def test_image_counts_below_the_table(order):
    """images = 2 of a table of 3, then d_images = 1 below images = 3: the unused slots keep
    their fill."""
    size, bc = (34, 18), BayerConvert(order)  # (two workgroups an image)
    frames = frames_of(1, *size, 11)
    want = bc.to_float(bc.apply(frames, *size), PREP)
    got = launch(*staged(frames, 2), size, bc, PREP, images=2)
    assert np.array_equal(got[SLOTS[0]], want[0]) and np.array_equal(got[SLOTS[1]], want[1])
    assert (got[SLOTS[2]] == SENTINEL).all()
    one = torch.tensor([1], dtype=torch.int32, device="cuda")
    got = launch(*staged(frames, 2), size, bc, PREP, d_images=one)
    assert np.array_equal(got[SLOTS[0]], want[0])
    assert (got[SLOTS[1]] == SENTINEL).all() and (got[SLOTS[2]] == SENTINEL).all()


REFUSED = [dict(imgs=0), dict(bytes=0), dict(out=0), dict(status=0), dict(HS=0), dict(WS=-2),
           dict(HS=3), dict(WS=5), dict(C=1), dict(C=4), dict(order="gray"),
           dict(order="bayer_rggb16"), dict(nchw=True), dict(images=65536),
           dict(HS=1 << 15, WS=1 << 15)]


@pytest.mark.parametrize("bad", REFUSED, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_launcher_refusals(bad):
    raw, tab = staged(frames_of(1, 2, 4, 3))
    out = torch.full((5 * 24,), SENTINEL, device="cuda")
    status = torch.zeros(3, dtype=torch.int32, device="cuda")
    ok = dict(images=3, imgs=tab.data_ptr(), bytes=raw.data_ptr(), HS=2, WS=4, C=3,
              out=out.data_ptr(), status=status.data_ptr(), stream=0, order="bayer_rggb8")
    assert C.raw_bayer_instances(**dict(ok, **bad)) == C.HIP_ERROR_INVALID_VALUE
    assert C.raw_bayer_instances(**dict(ok, images=0)) == 0
    if bad in (dict(HS=0), dict(WS=-2)):  # the wrapper raises ValueError for such a refusal
        with pytest.raises(ValueError, match="the launcher refused"):
            ops.raw_bayer_instances(raw, tab, (bad.get("HS", 2), bad.get("WS", 4)), out, status,
                                    BayerConvert("bayer_rggb8"))
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item()                       # nothing was launched


@pytest.mark.parametrize("size,extra", [((32, 32), {}), ((40, 36), dict(input_size="40,36"))],
                         ids=["model-size", "resized"])
def test_engine_equals_raw_rgb_records(size, extra):
    """Raw bayer_rggb8 records through a ResNet-20 topology, one of them over --max-batch and one
    bad_shape: every good record gets the softmaxes of the oracle's image sent as a raw rgb
    record, the bad one goes through --on-error; then the same through the input resize."""
    counts, order = [1, 2, 40, 1], "bayer_rggb8"
    bc, params = BayerConvert(order), params_for("resnet20", CIFAR)
    rng = np.random.default_rng(size[0])
    sets = {f"r{i}".encode(): rng.integers(0, 256, (n, size[0] * size[1]), dtype=np.uint8)
            for i, n in enumerate(counts)}
    kw = dict(params=params, dtype="bf16", max_batch=32, on_error="null", input_format="raw",
              **CIFAR, **extra)
    want, _ = serve([(k, encode_records_raw(bc.apply(f, *size), f.shape[0])[0])
                     for k, f in sets.items()] + [(b"short", b"\0" * 5)], **kw)
    got, stats = serve([(k, f.tobytes()) for k, f in sets.items()]
                       + [(b"short", sets[b"r1"].tobytes()[:-2])], input_pixel_format=order, **kw)
    assert got == want and got[b"short"] is None
    for i, n in enumerate(counts):  # n softmaxes of 10 classes
        v = got[f"r{i}".encode()]
        assert v is not None and v.count(b"],[") == n - 1 and v.count(b",") == 10 * n - 1
    assert stats["raw_records"] == len(counts) and stats["errors"] == 1, stats
    assert stats["images_out"] == sum(counts) and stats["split_records"] == 1, stats
