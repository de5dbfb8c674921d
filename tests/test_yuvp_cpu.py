"""Planar YUV 4:2:2 / 4:4:4 frame records (--input-pixel-format yuv422p | yuv444p) on the host:
twin and parsers against the oracle, the ties to packed 4:2:2 and between the two formats, byte
counts, configuration, the stub engine and the sanitizer program. Every comparison is on the bits."""

import base64
import os
import shutil
import subprocess

import numpy as np
import pytest

from gale._native import native
from gale.config import GaleConfig
from gale.data import encode_records_b64, encode_records_yuvp, pack_yuv422, pack_yuvp
from gale.models.preprocess import InputPrep, Yuv422Convert, YuvPlanarConvert

C = native()
K = C.kafka
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = [(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]
FORMATS = ("yuv422p", "yuv444p")
# (HS, WS) -> padding characters of a yuv422p string; yuv444p (any of them, and the odd widths)
# never has any
SIZES = {(1, 2): 2, (1, 4): 1, (3, 2): 0, (5, 6): 0, (7, 10): 1}
ODD = [(1, 1), (3, 3), (5, 7)]
EDGE = (0, 16, 128, 235, 240, 255)
CIFAR_MEAN_S = "0.4914,0.4822,0.4465"
CIFAR_STD_S = "0.2470,0.2435,0.2616"
PREP = InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S)


def planes(n, HS, WS, fmt, seed):
    """Y [n, HS, WS], U, V [n, HS, WS >> s]: half of the samples from EDGE (both clamps fire)."""
    rng = np.random.default_rng(seed)

    def draw(shape):
        return np.where(rng.random(shape) < 0.5, rng.choice(EDGE, shape),
                        rng.integers(0, 256, shape)).astype(np.uint8)

    wc = WS >> (fmt == "yuv422p")
    return draw((n, HS, WS)), draw((n, HS, wc)), draw((n, HS, wc))


@pytest.mark.parametrize("fmt,HS,WS", [(f, *s) for f in FORMATS for s in SIZES]
                         + [("yuv444p", *s) for s in ODD])
@pytest.mark.parametrize("matrix,range_", TABLES)
def test_host_twin_and_parsers_equal_the_oracle(matrix, range_, fmt, HS, WS):
    yc = YuvPlanarConvert(fmt, matrix, range_)
    Y, U, V = planes(4, HS, WS, fmt, HS * 100 + WS)
    frames = pack_yuvp(Y, U, V, fmt)
    B = HS * WS * (2 if fmt == "yuv422p" else 3)
    assert frames.shape == (4, B) and yc.frame_bytes(HS, WS) == B == C.yuvp_bytes(HS, WS, fmt)
    text = base64.b64encode(frames[0].tobytes())
    pad = SIZES.get((HS, WS), 0) if fmt == "yuv422p" else 0
    assert len(text) == 4 * ((B + 2) // 3) and len(text) - len(text.rstrip(b"=")) == pad
    want = yc.apply(frames, HS, WS)
    k, (a, b) = [*yc.coeffs(), yc.yo], PREP.coeffs()
    for i, fr in enumerate(frames):
        rgb, f32 = C.yuvp_to_rgb_host(fr.tobytes(), HS, WS, fmt, k)
        assert np.array_equal(rgb, want[i]) and np.array_equal(f32, want[i].astype(np.float32))
        _, f32p = C.yuvp_to_rgb_host(fr.tobytes(), HS, WS, fmt, k, a=a, b=b)
        assert np.array_equal(f32p.view(np.uint32),
                              PREP.apply(want[i].astype(np.float32)).view(np.uint32))
    for enc in ("b64", "raw"):
        st, out = C.parse_instances_yuvp_host(encode_records_yuvp(Y, U, V, fmt, 4, enc)[0],
                                              HS, WS, fmt, k, raw=enc == "raw")
        assert st == 0 and np.array_equal(out, want.astype(np.float32)), enc


def test_ties_to_packed_422_and_between_the_formats():
    """A yuv422p frame gives what Yuv422Convert gives for the same planes packed as yuyv422, and
    a yuv444p frame whose chroma columns are pairwise equal gives the yuv422p result."""
    HS, WS = 6, 10
    Y, U, V = planes(3, HS, WS, "yuv422p", 5)
    got = YuvPlanarConvert("yuv422p", "bt709", "full").apply(pack_yuvp(Y, U, V, "yuv422p"), HS, WS)
    want = Yuv422Convert("yuyv422", "bt709", "full").apply(pack_yuv422(Y, U, V, "yuyv422"), HS, WS)
    assert np.array_equal(got, want)
    wide = pack_yuvp(Y, np.repeat(U, 2, axis=-1), np.repeat(V, 2, axis=-1), "yuv444p")
    assert np.array_equal(YuvPlanarConvert("yuv444p", "bt709", "full").apply(wide, HS, WS), want)


# ---- configuration ------------------------------------------------------------------------------

def cfg(**kw):
    return GaleConfig(topology_name="t", input_topic="in", output_topic="out", **kw).validate()


REFUSED = [
    (dict(input_format="json"), "--input-format b64 or raw", dict(input_format="json")),
    (dict(input_format="b64", input_layout="nchw"), "--input-layout nchw", dict(input_nchw=True)),
    (dict(input_format="raw", model="lenet5"), "C = 1", dict(C=1)),
    (dict(input_format="raw", input_dtype="f16"), "--input-dtype f16", dict(input_dtype="f16")),
    (dict(input_format="raw", b64_ingest=True), "--b64-ingest", dict(b64_ingest=True)),
]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("kw,match,engine_kw", REFUSED, ids=[r[1] for r in REFUSED])
def test_refusals_name_their_option(fmt, kw, match, engine_kw):
    with pytest.raises(ValueError, match=match):
        cfg(**{"input_pixel_format": fmt, **kw})
    # the native engine refuses the same combination in a dict built by hand
    d = cfg(input_format="raw", input_pixel_format=fmt).engine_dict(32, 32, 3, 10)
    with pytest.raises(ValueError):
        C.Engine(dict(d, **engine_kw))


def test_odd_width_is_refused_for_422_only():
    odd = dict(input_format="b64", input_size="32,33", input_resize="32,32")
    with pytest.raises(ValueError, match="--input-size.*even WS"):
        cfg(input_pixel_format="yuv422p", **odd)
    d = cfg(input_format="raw", input_pixel_format="yuv422p").engine_dict(32, 32, 3, 10)
    with pytest.raises(ValueError):
        C.Engine(dict(d, rec_H=32, rec_W=33))
    c = cfg(input_pixel_format="yuv444p", **odd)
    C.Engine(c.engine_dict(32, 32, 3, 10))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("kw", [dict(input_format="b64"), dict(input_format="raw"),
                                dict(input_format="b64", b64_ingest=True),
                                dict(input_format="raw", input_size="41,36",
                                     input_resize="34,33"),
                                dict(input_format="b64", input_yuv_matrix="bt709",
                                     input_yuv_range="full")],
                         ids=["b64", "raw", "b64-ingest", "raw-input-size", "matrix-range"])
def test_accepted_combinations(fmt, kw):
    c = cfg(input_pixel_format=fmt, **kw)
    assert c.input_yuv() == YuvPlanarConvert(fmt, kw.get("input_yuv_matrix", "bt601"),
                                             kw.get("input_yuv_range", "limited"))
    C.Engine(c.engine_dict(32, 32, 3, 10))


# ---- the stub engine end to end -----------------------------------------------------------------

MAX_BATCH, CLASSES = 4, 10
COUNTS = [1, 2, 1, 6, 3]        # r3: one record over max_batch (fragments of 4 and 2)


def run_stub(records, input_format, **opts):
    broker = K.Broker()
    broker.start()
    try:
        broker.create_topic("in", 1)
        broker.create_topic("out", 1)
        for key, value in records:
            broker.append("in", 0, [value], [key])
        c = cfg(bootstrap=f"127.0.0.1:{broker.port}", start_offset="earliest", stub=True,
                max_batch=MAX_BATCH, max_wait_us=500, output_key="input", on_error="null",
                input_format=input_format, input_scale=1 / 255, input_mean=CIFAR_MEAN_S,
                input_std=CIFAR_STD_S, **opts)
        d = c.engine_dict(32, 32, 3, CLASSES)
        d["max_records"] = len(records)
        eng = C.Engine(d)
        eng.add_stub_replica(MAX_BATCH, 0, True, -1)
        eng.start()
        assert eng.wait(30000), eng.stats()
        eng.stop()
        out = broker.read("out", 0)
    finally:
        broker.stop()
    assert len(out) == len(records)
    return {r["key"]: r["value"] for r in out}, dict(eng.stats())


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("enc", ["b64", "raw"])
def test_stub_engine_equals_rgb_records_of_the_oracle(enc, fmt):
    HS, WS = 32, 32
    sets = {f"r{i}".encode(): planes(n, HS, WS, fmt, 23 + i) for i, n in enumerate(COUNTS)}
    yc = YuvPlanarConvert(fmt, "bt601", "full")  # (what a JPEG carries)
    rgb = {k: yc.apply(pack_yuvp(*p, fmt), HS, WS) for k, p in sets.items()}
    want, wstats = run_stub([(k, encode_records_b64(x, x.shape[0])[0]) for k, x in rgb.items()],
                            "b64")
    assert wstats["yuv_records"] == 0
    recs = [(k, encode_records_yuvp(*p, fmt, p[0].shape[0], enc)[0]) for k, p in sets.items()]
    recs.insert(2, (b"short", recs[0][1][:-4]))                     # bad_shape in either encoding
    got, stats = run_stub(recs, enc, input_pixel_format=fmt, input_yuv_range="full")
    assert got.pop(b"short") is None
    assert got == want and all(v is not None for v in want.values())
    assert stats["yuv_records"] == len(COUNTS), stats
    assert stats["split_records"] == 1 and stats["errors"] == 1, stats


# ---- stand-alone sanitizer run ------------------------------------------------------------------

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None,
                    reason="needs ROCm clang++ and make")
def test_yuvp_codec_under_address_and_ub_sanitizers():
    target = "build/asan/yuvp_check"
    b = subprocess.run(["make", "-C", ROOT, target], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, target), "4000"], capture_output=True, text=True,
                       timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "all checks passed" in out
    assert "AddressSanitizer" not in out and "runtime error" not in out
