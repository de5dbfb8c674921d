"""Planar YUV 4:2:2 / 4:4:4 frame records (--input-pixel-format yuv422p | yuv444p) on the GPU:
both launchers of csrc/kernels/yuv_planar.hip against the numpy oracle (YuvPlanarConvert),
verdicts, device count, refusals, and the engine on every step site against RGB b64 records of the
oracle's images. Every comparison is on the bits."""

import base64

import numpy as np
import pytest
import torch

from gale import ops
from gale._native import native
from gale.config import GaleConfig
from gale.data import encode_records_b64, encode_records_yuvp, pack_yuvp
from gale.engine import Engine
from gale.models import get_model, init_params
from gale.models.preprocess import InputPrep, YuvPlanarConvert
from gale.models.reference import calibrate_bn

pytestmark = pytest.mark.gpu

C = native()
K = C.kafka
IMG = np.dtype([("off", "<i8"), ("slot", "<i4"), ("rec", "<i4")])
CIFAR_MEAN_S = "0.4914,0.4822,0.4465"
CIFAR_STD_S = "0.2470,0.2435,0.2616"
PREP = InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S)
SENTINEL = -7.0
EDGE = (0, 16, 128, 235, 240, 255)
# either format with another table: both values of yo, both matrices
CONVERT = {"yuv422p": YuvPlanarConvert("yuv422p", "bt601", "full"),
           "yuv444p": YuvPlanarConvert("yuv444p", "bt709", "limited")}
# The kernel's units: a lane's run of 12 (4:4:4) / 24 (4:2:2) pixels, a wave of 768 / 1536, a
# workgroup of 3072.
# yuv444p: 1x1 B = 3, one quad, U and V at byte phases 1 and 2 of it; 1x2 plane phase 2; 2x2
# exactly one window; 3x3 HS*WS mod 3 = 0 and 5x7 mod 3 = 2, both odd x odd with 27 / 105 floats
# an image, so slots 1 and 2 sit at misaligned bases (the per-lane store path); 3x4 one whole run,
# 1x13 a second lane; 24x32 one whole wave, 1x769 a second (and a 3-float tail after whole
# 16-byte units); 48x64 one whole workgroup, 7x439 a second.
# yuv422p: 1x2 '==' padding (6 floats: the per-lane store path), 1x4 one '=', 3x2 none; 4x6 one
# whole run, 1x26 a second lane (78 floats: misaligned slots); 24x64 one whole wave, 1x1538 a
# second; 48x64 one whole workgroup, 29x106 a second.
SIZES = {"yuv444p": [(1, 1), (1, 2), (2, 2), (3, 3), (5, 7), (3, 4), (1, 13), (24, 32), (1, 769),
                     (48, 64), (7, 439)],
         "yuv422p": [(1, 2), (1, 4), (3, 2), (4, 6), (1, 26), (24, 64), (1, 1538), (48, 64),
                     (29, 106)]}
CASES = [(f, s) for f in SIZES for s in SIZES[f]]
SLOTS = [2, 0, 1]
# how the three frames are staged: b64 strings at three 16-byte phases; raw frames at byte phases
# 1, 2, 3 (dword loads realigned) and at 16-byte boundaries (the vector loads where a plane's
# own phase allows)
STAGINGS = {"b64": (0, 5, 11), "raw": (1, 2, 3), "raw16": (0, 0, 0)}


def frames_of(HS, WS, fmt):
    """uint8 [3, B]: random planes, half of the samples from EDGE so that both clamps fire."""
    rng = np.random.default_rng(HS * 10007 + WS)

    def draw(shape):
        return np.where(rng.random(shape) < 0.5, rng.choice(EDGE, shape),
                        rng.integers(0, 256, shape)).astype(np.uint8)

    wc = WS >> CONVERT[fmt].shift
    return pack_yuvp(draw((3, HS, WS)), draw((3, HS, wc)), draw((3, HS, wc)), fmt)


def staged(frames, staging):
    """(device bytes, device descriptor table): frame i in slot SLOTS[i], record i."""
    b64 = staging == "b64"
    buf, offs = bytearray(b"\xee" * 16), []
    for fr, ph in zip(frames, STAGINGS[staging]):
        while len(buf) % (16 if b64 or staging == "raw16" else 4) != ph:
            buf += b"\xee"
        offs.append(len(buf))
        buf += base64.b64encode(fr.tobytes()) + b'"},{' if b64 else fr.tobytes()
    buf += b"\xee" * 16
    tab = np.zeros(3, dtype=IMG)
    tab["off"], tab["slot"], tab["rec"] = offs, SLOTS, range(3)
    return (torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).cuda(),
            torch.from_numpy(tab.view(np.int32).reshape(-1, 4).copy()).cuda())


def launch(staging, raw, tab, size, yc, prep=None, d_images=None):
    """(floats [3, HS, WS, 3] by slot, statuses [3]); the four floats on either side of the
    output are checked to be untouched."""
    per = size[0] * size[1] * 3
    flat = torch.full((3 * per + 8,), SENTINEL, device="cuda")
    out, status = flat[4:4 + 3 * per], torch.zeros(3, dtype=torch.int32, device="cuda")
    assert out.data_ptr() % 16 == 0
    op = ops.b64_yuvp_instances if staging == "b64" else ops.raw_yuvp_instances
    op(raw, tab, size, out, status, yc, d_images=d_images, prep=prep)
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    assert (host[:4] == SENTINEL).all() and (host[-4:] == SENTINEL).all()
    return host[4:-4].reshape(3, *size, 3), status.cpu().numpy()


def expected(frames, size, yc, prep):
    want = yc.apply(frames, *size).astype(np.float32)
    return prep.apply(want) if prep is not None else want


@pytest.mark.parametrize("prep", [None, PREP], ids=["identity", "cifar"])
@pytest.mark.parametrize("staging", list(STAGINGS))
@pytest.mark.parametrize("fmt,size", CASES, ids=[f"{f}-{s[0]}x{s[1]}" for f, s in CASES])
def test_kernel_equals_the_oracle(fmt, size, staging, prep):
    yc, frames = CONVERT[fmt], frames_of(*size, fmt)
    got, status = launch(staging, *staged(frames, staging), size, yc, prep)
    want = expected(frames, size, yc, prep)
    assert np.array_equal(got[SLOTS].view(np.uint32), want.view(np.uint32))
    assert not status.any()


# yuv422p 7x10: Y bytes 0 .. 69, U 70 .. 104, V 105 .. 139; B = 140, L = 188, the last character
# '='; bytes 69 (Y) and 70 (U) share quad 23, characters 92 .. 95. yuv444p 5x7: bytes 34 (Y) and
# 35 (U) share quad 11, characters 44 .. 47.
VERDICTS = [("yuv422p", (7, 10), 0, b"-"), ("yuv422p", (7, 10), 93, b"_"),
            ("yuv422p", (7, 10), 186, b"_"), ("yuv422p", (7, 10), 187, b"A"),
            ("yuv444p", (5, 7), 46, b"=")]


@pytest.mark.parametrize("fmt,size,at,ch", VERDICTS,
                         ids=["first-y", "shared-y-u", "last-v", "padding", "444-shared-y-u"])
def test_b64_verdicts(fmt, size, at, ch):
    """Record 1 of 3 gets the bad character; the other two images are intact."""
    yc, frames = CONVERT[fmt], frames_of(*size, fmt)
    raw, tab = staged(frames, "b64")
    off = int(tab.cpu().numpy().view(IMG)["off"][1, 0])
    L = 4 * ((frames.shape[1] + 2) // 3)
    tail = bytes(raw[off + L - 1:off + L + 1].cpu().numpy())
    assert tail[1:] == b'"' and (tail[:1] == b"=") == (fmt == "yuv422p")
    raw[off + at] = ch[0]
    got, status = launch("b64", raw, tab, size, yc)
    assert list(status) == [0, 2, 0]
    want = expected(frames, size, yc, None)
    assert np.array_equal(got[SLOTS[0]], want[0]) and np.array_equal(got[SLOTS[2]], want[2])


@pytest.mark.parametrize("fmt", list(CONVERT))
@pytest.mark.parametrize("staging", ["b64", "raw"])
def test_device_count_below_the_launch_size(staging, fmt):
    size, yc = (26, 60), CONVERT[fmt]  # (1560 pixels: past one wave in either format)
    frames = frames_of(*size, fmt)
    two = torch.tensor([2], dtype=torch.int32, device="cuda")
    got, _ = launch(staging, *staged(frames, staging), size, yc, PREP, d_images=two)
    want = expected(frames, size, yc, PREP)
    assert np.array_equal(got[SLOTS[0]], want[0]) and np.array_equal(got[SLOTS[1]], want[1])
    assert (got[SLOTS[2]] == SENTINEL).all()


REFUSED = [dict(imgs=0), dict(bytes=0), dict(out=0), dict(status=0), dict(HS=0), dict(WS=-2),
           dict(WS=3, format="yuv422p"), dict(C=1), dict(format="i420"), dict(format="yuyv422"),
           dict(nchw=True), dict(images=65536), dict(HS=1 << 15, WS=1 << 15)]


@pytest.mark.parametrize("bad", REFUSED, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
@pytest.mark.parametrize("name", ["b64_yuvp_instances", "raw_yuvp_instances"])
def test_launcher_refusals(name, bad):
    raw, tab = staged(frames_of(3, 2, "yuv444p"), "b64" if name.startswith("b64") else "raw")
    out = torch.full((3 * 18,), SENTINEL, device="cuda")
    status = torch.zeros(3, dtype=torch.int32, device="cuda")
    ok = dict(images=3, imgs=tab.data_ptr(), bytes=raw.data_ptr(), HS=3, WS=2, C=3,
              out=out.data_ptr(), status=status.data_ptr(), stream=0, format="yuv444p")
    assert getattr(C, name)(**dict(ok, **bad)) == C.HIP_ERROR_INVALID_VALUE
    assert getattr(C, name)(**dict(ok, images=0)) == 0
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item()                       # nothing was launched


# ---- the engine ---------------------------------------------------------------------------------

COUNTS = [1, 2, 1, 3, 1, 1, 4, 1, 2, 1, 3, 2]
PREP_KW = dict(input_scale=1 / 255, input_mean=CIFAR_MEAN_S, input_std=CIFAR_STD_S)
SITES = {"direct": {}, "plain": dict(graph_step=False), "graph": dict(step_launch="graph"),
         "graph-noencode": dict(step_launch="graph", gpu_encode=False)}
TOPOLOGIES = [("b64", "yuv422p"), ("raw", "yuv444p")]  # one topology per encoding


def serve(recs, params, input_format="b64", **kw):
    broker = K.Broker()
    broker.start()
    try:
        broker.create_topic("in", 1)
        broker.create_topic("out", 1)
        for key, rec in recs:
            broker.append("in", 0, [rec], [key])
        cfg = GaleConfig(topology_name="g", input_topic="in", output_topic="out",
                         model="resnet20", dtype="bf16", input_format=input_format,
                         bootstrap=f"127.0.0.1:{broker.port}", start_offset="earliest",
                         max_batch=32, max_wait_us=500, output_key="input", on_error="null", **kw)
        eng = Engine(cfg.validate(), devices=[0], max_records=len(recs), params=params)
        eng.start()
        assert eng.wait(120), eng.stats()
        eng.stop()
        out = broker.read("out", 0)
    finally:
        broker.stop()
    assert len(out) == len(recs)
    return eng.stats(), {r["key"]: r["value"] for r in out}


@pytest.fixture(scope="module")
def r20():
    net = get_model("resnet20")
    params = init_params(net, seed=0, calibrate=False)
    x = np.random.default_rng(77).integers(0, 256, (16,) + tuple(net.input_shape))
    calibrate_bn(net, params, torch.from_numpy(PREP.apply(x.astype(np.float32))))
    return params


def check_topologies(size, params, **kw):
    """Either topology gives, key by key, the text of the same engine fed RGB b64 records of the
    oracle's images (yuv444p's planes are yuv422p's with every chroma column doubled, so one RGB
    run serves both); returns its statistics by encoding."""
    rng = np.random.default_rng(61)
    sets = {f"r{i}".encode(): tuple(rng.integers(0, 256, (n, size[0], w), dtype=np.uint8)
                                    for w in (size[1], size[1] // 2, size[1] // 2))
            for i, n in enumerate(COUNTS)}
    yc = YuvPlanarConvert("yuv422p", "bt709", "full")
    rgb = [(k, yc.apply(pack_yuvp(*p, "yuv422p"), *size)) for k, p in sets.items()]
    wstats, want = serve([(k, encode_records_b64(x, x.shape[0])[0]) for k, x in rgb], params, **kw)
    assert wstats["yuv_records"] == 0 and all(v is not None for v in want.values())
    stats = {}
    for enc, fmt in TOPOLOGIES:
        wide = 2 if fmt == "yuv444p" else 1
        recs = [(k, encode_records_yuvp(Y, np.repeat(U, wide, -1), np.repeat(V, wide, -1), fmt,
                                        Y.shape[0], enc)[0]) for k, (Y, U, V) in sets.items()]
        stats[enc], got = serve(recs, params, enc, input_pixel_format=fmt,
                                input_yuv_matrix="bt709", input_yuv_range="full", **kw)
        assert got == want, (enc, fmt)
        assert stats[enc]["yuv_records"] == len(sets) and stats[enc]["errors"] == 0, stats[enc]
        assert stats[enc]["images_out"] == sum(COUNTS), stats[enc]
    assert stats["b64"]["b64_records"] == len(sets) == stats["raw"]["raw_records"]
    return stats


@pytest.mark.parametrize("site", [*SITES, "resize"])
def test_engine_every_step_site(r20, site):
    """Each step site at 32x32, and --input-size 41,36 (an odd HS) with --input-resize: the decode
    writes the resize's source tensor."""
    size, kw = ((41, 36), dict(input_size="41,36", input_resize="34,33")) if site == "resize" \
        else ((32, 32), SITES[site])
    stats = check_topologies(size, r20, **PREP_KW, **kw)
    for s in stats.values():
        assert (s["graph_step_batches"] > 0) == (site != "plain"), s
        assert s["resized_images"] == (sum(COUNTS) if site == "resize" else 0), s
