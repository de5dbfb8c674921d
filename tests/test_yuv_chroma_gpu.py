"""Triangle-filter chroma for b64 i420 / nv12 records (--input-yuv-chroma linear) on the GPU: the
kernel of csrc/kernels/b64_yuv_linear.hip against the numpy oracle (YuvLinearConvert) on the bits,
its bounds, verdicts, the launcher's refusals, and the engine against f32 rgb records of the
oracle's floats."""

import base64

import numpy as np
import pytest
import torch

from gale import ops
from gale._native import native
from gale.data import encode_records_typed, encode_records_yuv, pack_yuv420
from gale.models.preprocess import YuvLinearConvert
from test_input_raw_cpu import CIFAR, serve
from test_raw_engine_gpu import params_for
from test_yuv_chroma_cpu import FORMATS, PREP, planes

pytestmark = pytest.mark.gpu

C = native()
IMG = np.dtype([("off", "<i8"), ("slot", "<i4"), ("rec", "<i4")])
SENTINEL = -7.0
# either format with another table: both values of yo, both matrices
CONVERT = {"i420": YuvLinearConvert("i420", "bt709", "limited"),
           "nv12": YuvLinearConvert("nv12", "bt601", "full")}
SLOTS = [2, 0, 1]
# 2x2 one chroma sample, every neighbour clamps to it; 2x4 / 4x2 one interior seam in one
# direction; 4x4 one in both; 6x18 WS mod 4 == 2 (8-byte stores) and a partial last block; 32x32 a
# wave spanning 16 row pairs; 2x1040 wave boundaries inside a row pair; 34x130 a second workgroup
# of 2 row pairs; 12x8 with 1 and 2 row pairs a workgroup: the halo rows are the neighbours' own.
SIZES = [(2, 2), (2, 4), (4, 2), (4, 4), (6, 18), (32, 32), (2, 1040), (34, 130)]
CASES = [dict(fmt=f, size=s) for f in FORMATS for s in SIZES]
CASES += [dict(fmt=f, size=(12, 8), pairs=p) for f in FORMATS for p in (1, 2)]
# on two sizes: the CIFAR prep; out 4 bytes off a 16-byte boundary; strings at odd byte offsets
CASES += [dict(fmt=f, size=s, **kw) for f in FORMATS for s in [(6, 18), (32, 32)]
          for kw in (dict(prep=PREP), dict(out_off=1), dict(phase=5), dict(phase=11))]


def case_id(c):
    extra = [("cifar" if k == "prep" else f"{k}{v}") for k, v in c.items() if k not in ("fmt", "size")]
    return "-".join([c["fmt"], "%dx%d" % c["size"], *extra])


def frames_of(fmt, size, n=3):
    return pack_yuv420(*planes(n, *size, size[0] * 10007 + size[1]), fmt)


def staged(strings, phase=0, slots=SLOTS):
    """(device bytes, device descriptor table): string i at byte phase `phase` of 16 in a buffer
    of record text and guard bytes, in slot slots[i], record i."""
    buf, offs = bytearray(b'{"instances":[{"b64":"'), []
    for s in strings:
        buf += b" " * ((phase - len(buf)) % 16)
        offs.append(len(buf))
        buf += s + b'"},{"b64":"'
    buf += b"\xee" * 16
    tab = np.zeros(len(strings), dtype=IMG)
    tab["off"], tab["slot"], tab["rec"] = offs, slots, range(len(strings))
    return (torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).cuda(),
            torch.from_numpy(tab.view(np.int32).reshape(-1, 4).copy()).cuda())


def launch(raw, tab, size, yc, prep=None, out_off=0, **kw):
    """(floats [n, HS, WS, 3] by slot, statuses [n]). The floats on either side of `out` (a guard
    region after it) keep their fill."""
    n, per = tab.shape[0], size[0] * size[1] * 3
    flat = torch.full((4 + out_off + n * per + 64,), SENTINEL, device="cuda")
    out = flat[4 + out_off:4 + out_off + n * per]
    assert out.data_ptr() % 16 == 4 * out_off
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    ops.b64_yuv_linear_instances(raw, tab, size, out, status, yc, prep=prep, **kw)
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    assert (host[:4 + out_off] == SENTINEL).all() and (host[-64:] == SENTINEL).all()
    return host[4 + out_off:-64].reshape(n, *size, 3), status.cpu().numpy()


def oracle(yc, frames, size, prep=None):
    x = yc.apply(frames, *size).astype(np.float32)
    return x if prep is None else prep.apply(x)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_kernel_equals_the_oracle(case):
    fmt, size, prep = case["fmt"], case["size"], case.get("prep")
    yc, frames = CONVERT[fmt], frames_of(fmt, size)
    got, status = launch(*staged([base64.b64encode(f.tobytes()) for f in frames],
                                 case.get("phase", 0)),
                         size, yc, prep, case.get("out_off", 0), pairs=case.get("pairs", 0))
    assert not status.any()
    assert np.array_equal(got[SLOTS].view(np.int32), oracle(yc, frames, size, prep).view(np.int32))


@pytest.mark.parametrize("fmt", FORMATS)
def test_verdicts(fmt):
    """12x8 in workgroups of 2 row pairs: luma is bytes 0 .. 95; byte 113 lies in U row 4 (i420)
    or UV row 2 (nv12), the halo row of one workgroup and an own row of its neighbour. One bad
    character in records 1, 2, 3: in luma, in that row, in the last quad. Record 0 stays good
    and exact."""
    size, yc = (12, 8), CONVERT[fmt]
    frames = frames_of(fmt, size, 4)
    s = [bytearray(base64.b64encode(f.tobytes())) for f in frames]
    for rec, at in ((1, 4 * (10 // 3) + 1), (2, 4 * (113 // 3) + 2), (3, len(s[0]) - 1)):
        s[rec][at:at + 1] = b"-"
    got, status = launch(*staged([bytes(x) for x in s], 7, [3, 1, 0, 2]), size, yc, pairs=2)
    assert list(status) == [0, 2, 2, 2]
    want = oracle(yc, frames, size)
    assert np.array_equal(got[3], want[0])
    assert (got != SENTINEL).all()                      # every frame was written, in its slot
    assert np.array_equal(got[1][4:], want[1][4:])      # far from record 1's bad bytes (row 1)


@pytest.mark.parametrize("fmt", FORMATS)
def test_image_counts_below_the_table(fmt):
    """images = 2 of a table of 3, then d_images = 1 below images = 3: the unused slots keep
    their fill."""
    size, yc = (34, 130), CONVERT[fmt]  # (two workgroups an image)
    frames = frames_of(fmt, size)
    st = staged([base64.b64encode(f.tobytes()) for f in frames], 3)
    want = oracle(yc, frames, size, PREP)
    got, _ = launch(*st, size, yc, PREP, images=2)
    assert np.array_equal(got[SLOTS[0]], want[0]) and np.array_equal(got[SLOTS[1]], want[1])
    assert (got[SLOTS[2]] == SENTINEL).all()
    one = torch.tensor([1], dtype=torch.int32, device="cuda")
    got, _ = launch(*st, size, yc, PREP, d_images=one)
    assert np.array_equal(got[SLOTS[0]], want[0])
    assert (got[SLOTS[1]] == SENTINEL).all() and (got[SLOTS[2]] == SENTINEL).all()


REFUSED = [dict(imgs=0), dict(bytes=0), dict(out=0), dict(status=0), dict(HS=0), dict(WS=-2),
           dict(HS=3), dict(WS=5), dict(C=1), dict(C=4), dict(format="yuv444p"),
           dict(format="p010le"), dict(nchw=True), dict(images=65536), dict(pairs=2),
           dict(WS=C.YUV_LINEAR_MAX_WS + 2), dict(HS=1 << 15, WS=1 << 15)]


@pytest.mark.parametrize("bad", REFUSED, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_launcher_refusals(bad):
    raw, tab = staged([base64.b64encode(f.tobytes()) for f in frames_of("i420", (2, 4))])
    out = torch.full((3 * 24,), SENTINEL, device="cuda")
    status = torch.zeros(3, dtype=torch.int32, device="cuda")
    ok = dict(images=3, imgs=tab.data_ptr(), bytes=raw.data_ptr(), HS=2, WS=4, C=3,
              out=out.data_ptr(), status=status.data_ptr(), stream=0, format="i420")
    assert C.b64_yuv_linear_instances(**dict(ok, **bad)) == C.HIP_ERROR_INVALID_VALUE
    assert C.b64_yuv_linear_instances(**dict(ok, images=0)) == 0
    if bad in (dict(HS=0), dict(pairs=2)):  # the wrapper raises ValueError for such a refusal
        with pytest.raises(ValueError, match="the launcher refused"):
            ops.b64_yuv_linear_instances(raw, tab, (bad.get("HS", 2), 4), out, status,
                                         CONVERT["i420"], pairs=bad.get("pairs", 0))
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item() and not status.any().item()   # nothing was launched


def test_engine_equals_f32_rgb_records():
    """i420 linear records through a ResNet-20 topology, one of them over --max-batch: every
    record gets the softmaxes of the same images sent as f32 rgb b64 records of the oracle's
    floats."""
    counts, fmt = [1, 2, 1, 3, 40, 1], "i420"
    yc = YuvLinearConvert(fmt, "bt601", "full")
    params = params_for("resnet20", CIFAR)
    sets = {f"r{i}".encode(): planes(n, 32, 32, 90 + i) for i, n in enumerate(counts)}
    kw = dict(params=params, dtype="bf16", max_batch=32, on_error="null", input_format="b64",
              **CIFAR)
    rgb = {k: oracle(yc, pack_yuv420(*p, fmt), (32, 32)) for k, p in sets.items()}
    want, _ = serve([(k, encode_records_typed(x, "f32", x.shape[0])[0]) for k, x in rgb.items()],
                    input_dtype="f32", **kw)
    got, stats = serve([(k, encode_records_yuv(*p, fmt, p[0].shape[0])[0])
                        for k, p in sets.items()], input_pixel_format=fmt,
                       input_yuv_range="full", input_yuv_chroma="linear", **kw)
    assert got == want
    for i, n in enumerate(counts):  # n softmaxes of 10 classes
        v = got[f"r{i}".encode()]
        assert v is not None and v.count(b"],[") == n - 1 and v.count(b",") == 10 * n - 1
    assert stats["yuv_records"] == stats["b64_records"] == len(counts), stats
    assert stats["errors"] == 0 and stats["images_out"] == sum(counts), stats
    assert stats["split_records"] == 1, stats
