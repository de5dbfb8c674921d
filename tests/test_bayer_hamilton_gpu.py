"""The edge-directed Bayer demosaic (--input-bayer-demosaic hamilton) on the GPU: the kernel of
csrc/kernels/bayer_hamilton.hip against the numpy oracle (BayerConvert(order, "hamilton")) on the
bits, its bounds, the launcher's refusals, and the engine against raw rgb records of the oracle's
image. (That the frames take every green branch is asserted on the CPU, from the oracle's choice
plane: test_bayer_hamilton_cpu.py.)"""

import numpy as np
import pytest
import torch

from gale import ops
from gale._native import native
from gale.data import encode_records_raw
from gale.models.preprocess import BayerConvert
from test_bayer_cpu import ORDERS, PREP, frames_of
from test_bayer_gpu import CASES, REFUSED, SENTINEL, SLOTS, staged
from test_bayer_hamilton_cpu import SHAPES, edge_frames
from test_input_raw_cpu import CIFAR, serve
from test_raw_engine_gpu import params_for

pytestmark = pytest.mark.gpu

C = native()
ids = dict(ids=lambda s: "%dx%d" % s)


def launch(raw, tab, size, bc, prep=None, out_off=0, **kw):
    """test_bayer_gpu.launch for this kernel: floats [5, HS, WS, 3] by slot, fills kept."""
    per = size[0] * size[1] * 3
    flat = torch.full((4 + out_off + 5 * per + 64,), SENTINEL, device="cuda")
    out = flat[4 + out_off:4 + out_off + 5 * per]
    assert out.data_ptr() % 16 == 4 * out_off
    status = torch.full((3,), 77, dtype=torch.int32, device="cuda")
    ops.raw_bayer_hamilton_instances(raw, tab, size, out, status, bc, prep=prep, **kw)
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    assert (host[:4 + out_off] == SENTINEL).all() and (host[-64:] == SENTINEL).all()
    assert (status.cpu().numpy() == 77).all()
    got = host[4 + out_off:-64].reshape(5, *size, 3)
    assert (got[[1, 3]] == SENTINEL).all()
    return got


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(
    "cifar" if k == "prep" else f"{k}{v}" for k, v in c.items() if v is not None) or "identity")
@pytest.mark.parametrize("size", SHAPES, **ids)
@pytest.mark.parametrize("order", ORDERS)
def test_kernel_equals_the_oracle(order, size, case):
    bc, frames, prep = BayerConvert(order, "hamilton"), \
        frames_of(1, *size, size[0] * 1009 + size[1]), case.get("prep")
    got = launch(*staged(frames, case.get("phase", 0)), size, bc, prep, case.get("out_off", 0))
    want = bc.to_float(bc.apply(frames, *size), prep)
    assert np.array_equal(got[SLOTS].view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("which", [0, 1], ids=["low-stripes", "boards"])
@pytest.mark.parametrize("size", [s for s in SHAPES if s >= (6, 10)], **ids)
@pytest.mark.parametrize("order", ORDERS)
def test_ties_stripes_and_clamps(order, size, which):
    """Low-amplitude noise (ties), one-pixel rows and columns of 0 / 255 (each direction alone),
    checkerboards (both clamps), at byte phase 3."""
    bc, frames = BayerConvert(order, "hamilton"), edge_frames(size, which)
    got = launch(*staged(frames, 3), size, bc)
    want = bc.to_float(bc.apply(frames, *size))
    assert np.array_equal(got[SLOTS].view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("order", ORDERS)
def test_image_counts_below_the_table(order):
    """images = 2 of a table of 3, then d_images = 1: the unused slots keep their fill."""
    size, bc = (34, 34), BayerConvert(order, "hamilton")  # (four workgroups an image)
    frames = frames_of(1, *size, 11)
    want = bc.to_float(bc.apply(frames, *size), PREP)
    got = launch(*staged(frames, 2), size, bc, PREP, images=2)
    assert np.array_equal(got[SLOTS[0]], want[0]) and np.array_equal(got[SLOTS[1]], want[1])
    assert (got[SLOTS[2]] == SENTINEL).all()
    one = torch.tensor([1], dtype=torch.int32, device="cuda")
    got = launch(*staged(frames, 2), size, bc, PREP, d_images=one)
    assert np.array_equal(got[SLOTS[0]], want[0])
    assert (got[SLOTS[1]] == SENTINEL).all() and (got[SLOTS[2]] == SENTINEL).all()


# what raw_bayer_instances refuses (its HS = 0, WS = -2 cases included), and a size under 4
@pytest.mark.parametrize("bad", REFUSED + [dict(HS=2), dict(WS=2)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_launcher_refusals(bad):
    raw, tab = staged(frames_of(1, 4, 4, 3))
    out = torch.full((5 * 48,), SENTINEL, device="cuda")
    status = torch.zeros(3, dtype=torch.int32, device="cuda")
    ok = dict(images=3, imgs=tab.data_ptr(), bytes=raw.data_ptr(), HS=4, WS=4, C=3,
              out=out.data_ptr(), status=status.data_ptr(), stream=0, order="bayer_rggb8")
    assert C.raw_bayer_hamilton_instances(**dict(ok, **bad)) == C.HIP_ERROR_INVALID_VALUE
    assert C.raw_bayer_hamilton_instances(**dict(ok, images=0)) == 0
    if bad in (dict(HS=2), dict(WS=2)):  # the wrapper raises ValueError for such a refusal
        with pytest.raises(ValueError, match="the launcher refused"):
            ops.raw_bayer_hamilton_instances(raw, tab, (bad.get("HS", 4), bad.get("WS", 4)), out,
                                             status, BayerConvert("bayer_rggb8", "hamilton"))
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item()                       # nothing was launched


@pytest.mark.parametrize("size,extra", [((32, 32), {}), ((40, 36), dict(input_size="40,36"))],
                         ids=["model-size", "resized"])
def test_engine_equals_raw_rgb_records(size, extra):
    """Raw bayer_rggb8 records with bayer_demosaic hamilton through a ResNet-20 topology, one over
    --max-batch and one bad_shape: the softmaxes of the oracle's image sent as raw rgb."""
    counts, order = [1, 2, 40, 1], "bayer_rggb8"
    bc, params = BayerConvert(order, "hamilton"), params_for("resnet20", CIFAR)
    rng = np.random.default_rng(size[0])
    sets = {f"r{i}".encode(): rng.integers(0, 256, (n, size[0] * size[1]), dtype=np.uint8)
            for i, n in enumerate(counts)}
    kw = dict(params=params, dtype="bf16", max_batch=32, on_error="null", input_format="raw",
              **CIFAR, **extra)
    want, _ = serve([(k, encode_records_raw(bc.apply(f, *size), f.shape[0])[0])
                     for k, f in sets.items()] + [(b"short", b"\0" * 5)], **kw)
    recs = [(k, f.tobytes()) for k, f in sets.items()] + [(b"short", sets[b"r1"].tobytes()[:-2])]
    got, stats = serve(recs, input_pixel_format=order, input_bayer_demosaic="hamilton", **kw)
    assert got == want and got[b"short"] is None
    assert stats["raw_records"] == len(counts) and stats["errors"] == 1, stats
    assert stats["images_out"] == sum(counts) and stats["split_records"] == 1, stats
