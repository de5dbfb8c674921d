"""Raw 10-bit YUV 4:2:0 frame records (--input-pixel-format p010le | yuv420p10le) on the GPU: the
kernel of csrc/kernels/yuv420_hi.hip against the numpy oracle (Yuv420HiConvert) on the bits, its
bounds, the launcher's refusals, and the engine against f32 rgb records of the oracle's floats."""

import numpy as np
import pytest
import torch

from gale import ops
from gale._native import native
from gale.data import encode_records_typed, encode_records_yuv420p10, pack_yuv420p10
from gale.models.preprocess import Yuv420HiConvert
from test_input_raw_cpu import CIFAR, serve
from test_raw_engine_gpu import params_for
from test_yuv10_cpu import FORMATS, PREP, SIZES, planes

pytestmark = pytest.mark.gpu

C = native()
IMG = np.dtype([("off", "<i8"), ("slot", "<i4"), ("rec", "<i4")])
SENTINEL = -7.0
# either format with another table: both values of yo, both matrices
CONVERT = {"p010le": Yuv420HiConvert("p010le", "bt709", "limited"),
           "yuv420p10le": Yuv420HiConvert("yuv420p10le", "bt601", "full")}
SLOTS = [2, 0, 1]
# SIZES: 2x2 one quad, a lone partial block; 2x10 a whole block and a 2-column tail; 4x8 two row
# pairs of one block; 6x18 WS mod 4 == 2 (8-byte stores, alternating planar chroma phase, 2-column
# tail); 32x32 a wave spanning 16 row pairs; 2x1040 wave boundaries inside a row pair; 34x130 289
# blocks, the second workgroup mostly empty.
# One case per hazard on the baseline of both formats x every size (identity prep, phase 0, a
# 16-byte aligned out): the CIFAR prep; frames at byte phases 1, 2, 3 and 15 of the buffer; out
# 4 bytes off a 16-byte boundary.
CASES = [dict(fmt=f, size=s) for f in FORMATS for s in SIZES]
CASES += [dict(fmt=f, size=s, prep=PREP) for f in FORMATS for s in [(6, 18), (32, 32)]]
CASES += [dict(fmt=f, size=s, phase=p) for f in FORMATS for s in [(6, 18), (4, 8), (34, 130)]
          for p in (1, 2, 3, 15)]
CASES += [dict(fmt=f, size=s, out_off=1) for f in FORMATS for s in [(2, 10), (32, 32)]]


def case_id(c):
    extra = [("cifar" if k == "prep" else f"{k}{v}") for k, v in c.items() if k not in ("fmt", "size")]
    return "-".join([c["fmt"], "%dx%d" % c["size"], *extra])


def frames_of(fmt, size):
    """uint8 [3, B]: cube corners, seeded noise, junk in the ignored bits of every word."""
    p, junk = planes(3, *size, size[0] * 10007 + size[1])
    return pack_yuv420p10(*p, fmt, junk)


def staged(frames, phase=0):
    """(device bytes, device descriptor table): frame i at byte phase `phase` of 16 in a buffer
    of guard bytes, in slot SLOTS[i]."""
    buf, offs = bytearray(b"\xee" * 16), []
    for fr in frames:
        buf += b"\xee" * ((phase - len(buf)) % 16)
        offs.append(len(buf))
        buf += fr.tobytes()
    buf += b"\xee" * 16
    tab = np.zeros(3, dtype=IMG)
    tab["off"], tab["slot"], tab["rec"] = offs, SLOTS, range(3)
    return (torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).cuda(),
            torch.from_numpy(tab.view(np.int32).reshape(-1, 4).copy()).cuda())


def launch(raw, tab, size, yc, prep=None, out_off=0, **kw):
    """Floats [3, HS, WS, 3] by slot. The floats on either side of `out` (a guard region after
    it) and every status word keep their fill."""
    per = size[0] * size[1] * 3
    flat = torch.full((4 + out_off + 3 * per + 64,), SENTINEL, device="cuda")
    out = flat[4 + out_off:4 + out_off + 3 * per]
    assert out.data_ptr() % 16 == 4 * out_off
    status = torch.full((3,), 77, dtype=torch.int32, device="cuda")
    ops.raw_yuv420p10_instances(raw, tab, size, out, status, yc, prep=prep, **kw)
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    assert (host[:4 + out_off] == SENTINEL).all() and (host[-64:] == SENTINEL).all()
    assert (status.cpu().numpy() == 77).all()
    return host[4 + out_off:-64].reshape(3, *size, 3)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_kernel_equals_the_oracle(case):
    fmt, size, prep = case["fmt"], case["size"], case.get("prep")
    yc, frames = CONVERT[fmt], frames_of(fmt, size)
    got = launch(*staged(frames, case.get("phase", 0)), size, yc, prep, case.get("out_off", 0))
    want = yc.to_float(yc.apply(frames, *size), prep)
    assert np.array_equal(got[SLOTS].view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("fmt", FORMATS)
def test_distance_to_the_real_matrix(fmt):
    """Behind the CIFAR prep the kernel stays within (0.5 + 2047 * 2^-19) * 0.25 |a| of the
    float64 matrix (clamped like the kernel: a clamp brings two values no further apart)."""
    size, yc = (34, 130), CONVERT[fmt]
    frames = frames_of(fmt, size)
    got = launch(*staged(frames, 3), size, yc, PREP)[SLOTS].astype(np.float64)
    Y, U, V = (p.astype(np.float64) for p in yc.planes(frames, *size))
    u, v = (np.repeat(np.repeat(c, 2, -2), 2, -1) - 512 for c in (U, V))
    r, y = [float(x) for x in yc.rationals()], Y - yc.yo
    real = np.stack([r[0] * y + r[1] * v, r[0] * y + r[2] * u + r[3] * v, r[0] * y + r[4] * u], -1)
    a, b = (np.asarray(x, np.float32)[:3].astype(np.float64) for x in PREP.coeffs())
    excess = np.abs(got - (np.clip(real, 0, 1020) * 0.25 * a + b)) / (0.25 * np.abs(a))
    print(f"{fmt}: largest distance {excess.max()} quarter steps")
    assert excess.max() <= 0.5 + 2047 * 2.0 ** -19


@pytest.mark.parametrize("fmt", FORMATS)
def test_image_counts_below_the_table(fmt):
    """images = 2 of a table of 3, then d_images = 1 below images = 3: the unused slots keep
    their fill."""
    size, yc = (34, 130), CONVERT[fmt]  # (two workgroups an image)
    frames = frames_of(fmt, size)
    want = yc.to_float(yc.apply(frames, *size), PREP)
    got = launch(*staged(frames, 2), size, yc, PREP, images=2)
    assert np.array_equal(got[SLOTS[0]], want[0]) and np.array_equal(got[SLOTS[1]], want[1])
    assert (got[SLOTS[2]] == SENTINEL).all()
    one = torch.tensor([1], dtype=torch.int32, device="cuda")
    got = launch(*staged(frames, 2), size, yc, PREP, d_images=one)
    assert np.array_equal(got[SLOTS[0]], want[0])
    assert (got[SLOTS[1]] == SENTINEL).all() and (got[SLOTS[2]] == SENTINEL).all()


REFUSED = [dict(imgs=0), dict(bytes=0), dict(out=0), dict(status=0), dict(HS=0), dict(WS=-2),
           dict(HS=3), dict(WS=5), dict(C=1), dict(C=4), dict(format="nv12"),
           dict(format="yuv444p"), dict(nchw=True), dict(images=65536),
           dict(HS=1 << 15, WS=1 << 15)]


@pytest.mark.parametrize("bad", REFUSED, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_launcher_refusals(bad):
    raw, tab = staged(frames_of("p010le", (2, 4)))
    out = torch.full((3 * 24,), SENTINEL, device="cuda")
    status = torch.zeros(3, dtype=torch.int32, device="cuda")
    ok = dict(images=3, imgs=tab.data_ptr(), bytes=raw.data_ptr(), HS=2, WS=4, C=3,
              out=out.data_ptr(), status=status.data_ptr(), stream=0, format="p010le")
    assert C.raw_yuv420p10_instances(**dict(ok, **bad)) == C.HIP_ERROR_INVALID_VALUE
    assert C.raw_yuv420p10_instances(**dict(ok, images=0)) == 0
    if bad in (dict(HS=0), dict(WS=-2)):  # the wrapper raises ValueError for such a refusal
        with pytest.raises(ValueError, match="the launcher refused"):
            ops.raw_yuv420p10_instances(raw, tab, (bad.get("HS", 2), bad.get("WS", 4)), out,
                                        status, CONVERT["p010le"])
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item()                       # nothing was launched


def test_engine_equals_f32_rgb_records():
    """Raw p010le records through a ResNet-20 topology, one of them over --max-batch: every
    record gets the softmaxes of the same images sent as f32 rgb b64 records of the oracle's
    floats."""
    counts, fmt = [1, 2, 1, 3, 40, 1], "p010le"
    yc = Yuv420HiConvert(fmt, "bt709", "full")
    params = params_for("resnet20", CIFAR)
    sets = {f"r{i}".encode(): planes(n, 32, 32, 90 + i) for i, n in enumerate(counts)}
    kw = dict(params=params, dtype="bf16", max_batch=32, on_error="null", **CIFAR)
    rgb = {k: yc.to_float(yc.apply(pack_yuv420p10(*p, fmt, j), 32, 32)) for k, (p, j) in sets.items()}
    want, _ = serve([(k, encode_records_typed(x, "f32", x.shape[0])[0]) for k, x in rgb.items()],
                    input_format="b64", input_dtype="f32", **kw)
    got, stats = serve([(k, encode_records_yuv420p10(*p, fmt, p[0].shape[0], j)[0])
                        for k, (p, j) in sets.items()], input_format="raw",
                       input_pixel_format=fmt, input_yuv_matrix="bt709", input_yuv_range="full",
                       **kw)
    assert got == want
    for i, n in enumerate(counts):  # n softmaxes of 10 classes
        v = got[f"r{i}".encode()]
        assert v is not None and v.count(b"],[") == n - 1 and v.count(b",") == 10 * n - 1
    assert stats["yuv_records"] == stats["raw_records"] == len(counts), stats
    assert stats["errors"] == 0 and stats["images_out"] == sum(counts), stats
    assert stats["split_records"] == 1, stats
