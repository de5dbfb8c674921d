"""Raw 10/12/16-bit Bayer mosaic records (--input-pixel-format bayer_*10le | 12le | 16le | 10p |
12p) on the GPU: the kernel of csrc/kernels/bayer_hi.hip against the numpy oracle (BayerHiConvert)
on the bits, its bounds, the launcher's refusals, and the engine against raw rgb u16 records of
the oracle's image."""

import functools

import numpy as np
import pytest
import torch

from gale import ops
from gale._native import native
from gale.data import encode_records_raw, pack_bayer_hi
from gale.models.preprocess import BAYER_HI_FORMATS, BayerHiConvert
from test_bayer_cpu import PREP
from test_bayer_gpu import CASES, REFUSED, SENTINEL, SLOTS, staged
from test_input_raw_cpu import CIFAR, serve
from test_raw_engine_gpu import params_for

pytestmark = pytest.mark.gpu

C = native()
FORMS = ("10le", "12le", "16le", "10p", "12p")
ORDERS = ("rggb", "bggr", "grbg", "gbrg")
DEMOSAICS = ("bilinear", "malvar")
# from the kernel's tile of 16 rows x 64 columns:
SHAPES = [
    (4, 4),     # the minimum frame: every halo sample reflected, both sides inside one tile
    (16, 64),   # exactly one tile
    (18, 68),   # a tail tile of one quad row / two quad columns, its halo reflected into the tile before
    (6, 12),    # 10p rows of 15 bytes, 12p rows of 18: the row phase alternates (10p)
    (6, 10),    # 12p rows of 15 bytes (no 10p frame: WS mod 4)
    (32, 128),  # two tiles each way
]


def shapes_of(form):
    return [s for s in SHAPES if form != "10p" or s[1] % 4 == 0]


@functools.lru_cache(maxsize=None)
def frames_and_rgb(fmt, demosaic, size):
    """(uint8 [3, B] frames, uint16 [3, HS, WS, 3] oracle RGB): seeded noise (10le / 12le: with
    noise in the ignored upper bits), all-0 and all-M."""
    bits, rng = BAYER_HI_FORMATS[fmt][2], np.random.default_rng(size[0] * 1009 + size[1])
    m = rng.integers(0, 1 << bits, (3, *size), dtype=np.uint16)
    m[1], m[2] = 0, (1 << bits) - 1
    junk = rng.integers(0, 1 << 16, m.shape, dtype=np.uint16) if fmt.endswith("le") else None
    frames = pack_bayer_hi(m, fmt, junk)
    return frames, BayerHiConvert(fmt, demosaic).apply(frames, *size)


def launch(raw, tab, size, bc, prep=None, out_off=0, **kw):
    """test_bayer_gpu.launch for this kernel: floats [5, HS, WS, 3] by slot, fills kept."""
    per = size[0] * size[1] * 3
    flat = torch.full((4 + out_off + 5 * per + 64,), SENTINEL, device="cuda")
    out = flat[4 + out_off:4 + out_off + 5 * per]
    assert out.data_ptr() % 16 == 4 * out_off
    status = torch.full((3,), 77, dtype=torch.int32, device="cuda")
    ops.raw_bayer_hi_instances(raw, tab, size, out, status, bc, prep=prep, **kw)
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    assert (host[:4 + out_off] == SENTINEL).all() and (host[-64:] == SENTINEL).all()
    assert (status.cpu().numpy() == 77).all()
    got = host[4 + out_off:-64].reshape(5, *size, 3)
    assert (got[[1, 3]] == SENTINEL).all()
    return got


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(
    "cifar" if k == "prep" else f"{k}{v}" for k, v in c.items() if v is not None) or "identity")
@pytest.mark.parametrize("form,size", [(f, s) for f in FORMS for s in shapes_of(f)],
                         ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("demosaic", DEMOSAICS)
def test_kernel_equals_the_oracle(demosaic, order, form, size, case):
    bc, prep = BayerHiConvert(f"bayer_{order}{form}", demosaic), case.get("prep")
    frames, rgb = frames_and_rgb(bc.format, demosaic, size)
    got = launch(*staged(frames, case.get("phase", 0)), size, bc, prep, case.get("out_off", 0))
    want = bc.to_float(rgb, prep)
    assert np.array_equal(got[SLOTS].view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("size", [(6, 12), (18, 68)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", ORDERS)
def test_checkerboard_clamps_both_ways(order, form, size):
    """2 x 2 cells of 0 / M, the inverse, and noise: the clamp is hit on both sides."""
    bc = BayerHiConvert(f"bayer_{order}{form}", "malvar")
    y, x = np.ogrid[:size[0], :size[1]]
    m = np.empty((3, *size), np.uint16)
    m[0] = (((x >> 1) + (y >> 1)) & 1) * ((1 << bc.bits) - 1)
    m[1] = ((1 << bc.bits) - 1) - m[0]
    m[2] = np.random.default_rng(1).integers(0, 1 << bc.bits, size)
    frames = pack_bayer_hi(m, bc.format)
    rgb = bc.apply(frames, *size)
    assert rgb.min() == 0 and rgb.max() == (1 << bc.bits) - 1
    got = launch(*staged(frames, 3), size, bc)
    assert np.array_equal(got[SLOTS].view(np.int32), bc.to_float(rgb).view(np.int32))


@pytest.mark.parametrize("form", FORMS)
def test_image_counts_below_the_table(form):
    """images = 2 of a table of 3, then d_images = 1: the unused slots keep their fill."""
    size, bc = (18, 68), BayerHiConvert(f"bayer_gbrg{form}", "malvar")  # (four workgroups an image)
    frames, rgb = frames_and_rgb(bc.format, "malvar", size)
    want = bc.to_float(rgb, PREP)
    got = launch(*staged(frames, 2), size, bc, PREP, images=2)
    assert np.array_equal(got[SLOTS[0]], want[0]) and np.array_equal(got[SLOTS[1]], want[1])
    assert (got[SLOTS[2]] == SENTINEL).all()
    one = torch.tensor([1], dtype=torch.int32, device="cuda")
    got = launch(*staged(frames, 2), size, bc, PREP, d_images=one)
    assert np.array_equal(got[SLOTS[0]], want[0])
    assert (got[SLOTS[1]] == SENTINEL).all() and (got[SLOTS[2]] == SENTINEL).all()


# what raw_bayer_instances refuses (its unknown names as `format`), then this launcher's own: a
# bits / packing pair that is no form, 10p with WS mod 4, malvar under 4
HI_REFUSED = [{("format" if k == "order" else k): v for k, v in d.items()} for d in REFUSED] + [
    dict(format="bayer_rggb8"), dict(bits=14), dict(packing=3), dict(bits=16, packing=2),
    dict(format="bayer_rggb10p", WS=6), dict(malvar=True, HS=2), dict(malvar=True, WS=2)]


@pytest.mark.parametrize("bad", HI_REFUSED,
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_launcher_refusals(bad):
    raw, tab = staged(np.zeros((3, 32), np.uint8))
    out = torch.full((5 * 48,), SENTINEL, device="cuda")
    status = torch.zeros(3, dtype=torch.int32, device="cuda")
    ok = dict(images=3, imgs=tab.data_ptr(), bytes=raw.data_ptr(), HS=4, WS=4, C=3,
              out=out.data_ptr(), status=status.data_ptr(), stream=0, format="bayer_rggb16le")
    assert C.raw_bayer_hi_instances(**dict(ok, **bad)) == C.HIP_ERROR_INVALID_VALUE
    assert C.raw_bayer_hi_instances(**dict(ok, images=0)) == 0
    if "malvar" in bad:  # the wrapper raises ValueError for such a refusal
        with pytest.raises(ValueError, match="the launcher refused"):
            ops.raw_bayer_hi_instances(raw, tab, (bad.get("HS", 4), bad.get("WS", 4)), out, status,
                                       BayerHiConvert("bayer_rggb16le", "malvar"))
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item()                       # nothing was launched


@pytest.mark.parametrize("fmt", ["bayer_grbg10p", "bayer_rggb16le"])
def test_engine_equals_raw_rgb_u16_records(fmt):
    """Raw records with bayer_demosaic malvar through a ResNet-20 topology, one over --max-batch
    and one short: the softmaxes of the oracle's RGB sent as raw rgb --input-dtype u16 records
    with the same --input-scale."""
    counts, size = [1, 2, 40, 1], (32, 32)
    bc, params = BayerHiConvert(fmt, "malvar"), params_for("resnet20", CIFAR)
    rng = np.random.default_rng(bc.bits)
    sets = {f"r{i}".encode(): pack_bayer_hi(rng.integers(0, 1 << bc.bits, (n, *size)), fmt)
            for i, n in enumerate(counts)}
    kw = dict(params=params, dtype="bf16", max_batch=32, on_error="null", input_format="raw",
              **CIFAR)
    want, _ = serve([(k, encode_records_raw(bc.apply(f, *size), f.shape[0], "u16")[0])
                     for k, f in sets.items()] + [(b"short", b"\0" * 5)], input_dtype="u16", **kw)
    recs = [(k, f.tobytes()) for k, f in sets.items()] + [(b"short", sets[b"r1"].tobytes()[:-2])]
    got, stats = serve(recs, input_pixel_format=fmt, input_bayer_demosaic="malvar", **kw)
    assert got == want and got[b"short"] is None
    for i, n in enumerate(counts):  # n softmaxes of 10 classes
        v = got[f"r{i}".encode()]
        assert v is not None and v.count(b"],[") == n - 1 and v.count(b",") == 10 * n - 1
    assert stats["raw_records"] == len(counts) and stats["errors"] == 1, stats
    assert stats["images_out"] == sum(counts) and stats["split_records"] == 1, stats
