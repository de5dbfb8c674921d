"""Raw 8-bit Bayer mosaic records (--input-pixel-format bayer_rggb8 | bayer_bggr8 | bayer_grbg8 |
bayer_gbrg8) on the host: the oracle against a hand-computed frame and flat colours, the twin and
the parser against the oracle, configuration, verdicts, the stub engine and the sanitizer program.
Every comparison of outputs is on the bits."""

import os
import shutil
import subprocess

import numpy as np
import pytest

from gale._native import native
from gale.config import GaleConfig, from_sources
from gale.data import encode_records_bayer, mosaic_bayer
from gale.models.preprocess import BAYER_FORMATS, BayerConvert, InputPrep
from test_input_raw_cpu import BAD_SHAPE, CIFAR, EMPTY, OK, serve

C = native()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = tuple(BAYER_FORMATS)
PREP = InputPrep.build(3, CIFAR["input_scale"], CIFAR["input_mean"], CIFAR["input_std"])


def frames_of(n, HS, WS, seed):
    """uint8 [n + 2, HS*WS]: n frames of seeded noise, an all-0 and an all-255 frame."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.integers(0, 256, (n, HS * WS), dtype=np.uint8),
                           np.zeros((1, HS * WS), np.uint8), np.full((1, HS * WS), 255, np.uint8)])


def test_oracle_equals_a_hand_computed_frame():
    """bayer_rggb8, every pixel worked out on paper from the contract (mirror: -1 -> 1, 4 -> 2)."""
    frame = np.array([[1, 2, 3, 4], [5, 6, 7, 9], [8, 12, 10, 20], [30, 40, 50, 61]], np.uint8)
    want = np.array([
        [(1, 4, 6), (2, 2, 6), (3, 5, 8), (3, 4, 9)],
        [(5, 5, 6), (6, 7, 6), (7, 7, 8), (7, 10, 9)],
        [(8, 15, 23), (9, 12, 23), (10, 22, 29), (10, 20, 35)],
        [(8, 30, 40), (9, 26, 40), (10, 50, 51), (10, 35, 61)]], np.uint8)
    assert np.array_equal(BayerConvert("bayer_rggb8").apply(frame.reshape(-1), 4, 4), want)
    # bggr sees the same sites with red and blue exchanged
    assert np.array_equal(BayerConvert("bayer_bggr8").apply(frame.reshape(-1), 4, 4),
                          want[..., ::-1])


@pytest.mark.parametrize("order", ORDERS)
def test_flat_colour_demosaics_to_itself(order):
    """Edges and corners included: the mirror keeps the colour parity, the tables name the sites."""
    rgb = np.empty((6, 10, 3), np.uint8)
    rgb[:] = (200, 31, 97)
    mosaic = mosaic_bayer(rgb, order)
    assert mosaic.shape == (6, 10) and set(np.unique(mosaic)) == {200, 31, 97}
    assert np.array_equal(BayerConvert(order).apply(mosaic.reshape(-1), 6, 10), rgb)


@pytest.mark.parametrize("HS,WS", [(2, 2), (2, 4), (4, 2), (6, 10), (32, 32)], ids=str)
@pytest.mark.parametrize("order", ORDERS)
def test_host_twin_and_parser_equal_the_oracle(order, HS, WS):
    bc, frames, B = BayerConvert(order), frames_of(2, HS, WS, HS * 100 + WS), HS * WS
    assert bc.frame_bytes(HS, WS) == B == C.bayer_bytes(HS, WS)
    rgb = bc.apply(frames, HS, WS)
    a, b = PREP.coeffs()
    for i, fr in enumerate(frames):
        u8, f32 = C.bayer_to_rgb_host(fr.tobytes(), HS, WS, order)
        assert np.array_equal(u8, rgb[i]) and np.array_equal(f32, bc.to_float(rgb[i]))
        _, f32p = C.bayer_to_rgb_host(fr.tobytes(), HS, WS, order, a=a, b=b)
        assert np.array_equal(f32p.view(np.uint32), bc.to_float(rgb[i], PREP).view(np.uint32))
    rec = frames.tobytes()
    st, out = C.parse_instances_raw_bayer_host(rec, HS, WS, order)
    assert st == OK and np.array_equal(out, bc.to_float(rgb))
    # verdicts: records of 0, B - 1, B + 1 and 2 B bytes; the splitter gives whole frames
    for n, want in ((0, EMPTY), (B - 1, BAD_SHAPE), (B + 1, BAD_SHAPE), (2 * B, OK)):
        assert C.parse_instances_raw_bayer_host(rec[:n], HS, WS, order)[0] == want, n
    assert C.parse_instances_raw_bayer_host(rec, HS + 1, WS, order)[0] == BAD_SHAPE
    assert C.parse_instances_raw_bayer_host(rec, HS, WS, "gray")[0] == BAD_SHAPE
    assert C.split_instances_raw(4 * B, B, 3) == [(0, 3 * B), (3 * B, 4 * B)]


# ---- configuration ------------------------------------------------------------------------------

def cfg(**kw):
    return GaleConfig(topology_name="t", input_topic="in", output_topic="out", **kw).validate()


REFUSED = [
    (dict(input_format="json"), "--input-format raw", dict(input_format="json")),
    (dict(input_format="b64"), "--input-format raw", dict(input_format="b64")),
    (dict(input_layout="nchw"), "--input-layout nchw", dict(input_nchw=True)),
    (dict(model="lenet5"), "C = 1", dict(C=1)),
    (dict(input_size="33,32", input_resize="32,32"), "--input-size.*even", dict(rec_H=33)),
    (dict(input_size="32,33", input_resize="32,32"), "--input-size.*even", dict(rec_W=33)),
    (dict(input_dtype="f16"), "--input-dtype f16", dict(input_dtype="f16")),
    (dict(input_yuv_matrix="bt709"), "--input-yuv-matrix", dict(yuv_matrix="bt709")),
    (dict(input_yuv_range="full"), "--input-yuv-range", dict(yuv_range="full")),
    (dict(input_yuv_chroma="linear"), "--input-yuv-chroma linear", dict(yuv_chroma="linear")),
    (dict(b64_ingest=True), "--b64-ingest", dict(b64_ingest=True)),
]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw,match,engine_kw", REFUSED, ids=[
    "json", "b64", "nchw", "C=1", "odd-HS", "odd-WS", "dtype", "matrix", "range", "chroma",
    "ingest"])
def test_refusals_name_their_option(order, kw, match, engine_kw):
    with pytest.raises(ValueError, match=match):
        cfg(**{"input_format": "raw", "input_pixel_format": order, **kw})
    # the native engine refuses the same combination in a dict built by hand
    d = cfg(input_format="raw", input_pixel_format=order).engine_dict(32, 32, 3, 10)
    assert d["pixel_format"] == order
    C.Engine(d)
    with pytest.raises(ValueError):
        C.Engine(dict(d, **engine_kw))


def test_option_precedence(tmp_path):
    toml = tmp_path / "gale.toml"
    toml.write_text('[gale]\ntopology_name = "t"\ninput_format = "raw"\n'
                    'input_pixel_format = "bayer_rggb8"\n')
    env = {"GALE_INPUT_PIXEL_FORMAT": "bayer_grbg8"}
    assert from_sources({}, {}, str(toml)).input_pixel_format == "bayer_rggb8"
    assert from_sources({}, env, str(toml)).input_pixel_format == "bayer_grbg8"
    assert from_sources({"input_pixel_format": "bayer_gbrg8"}, env,
                        str(toml)).input_pixel_format == "bayer_gbrg8"


# ---- the stub engine ----------------------------------------------------------------------------

def test_stub_engine_splits_on_frame_boundaries():
    """The predictions of the frames sent one image a record; the record of 9 images over
    --max-batch 4 is split on frame boundaries and joined into one output."""
    counts, order = [1, 2, 9, 1], "bayer_gbrg8"
    rng = np.random.default_rng(5)
    sets = {f"r{i}".encode(): rng.integers(0, 256, (n, 32, 32, 3), dtype=np.uint8)
            for i, n in enumerate(counts)}
    kw = dict(max_batch=4, on_error="null", input_format="raw", input_pixel_format=order, **CIFAR)
    recs = [(k, encode_records_bayer(x, order, x.shape[0])[0]) for k, x in sets.items()]
    got, st = serve(recs + [(b"short", recs[2][1][:-2])], **kw)
    assert got.pop(b"short") is None
    assert (st["raw_records"], st["errors"], st["split_records"]) == (len(counts), 1, 1), st
    singles = [(k + b"/%d" % i, r) for k, x in sets.items()
               for i, r in enumerate(encode_records_bayer(x, order, 1))]
    one, _ = serve(singles, **kw)
    for k, x in sets.items():
        rows = [one[k + b"/%d" % i] for i in range(x.shape[0])]
        pre = b'{"predictions":['
        assert got[k] == pre + b",".join(r[len(pre):-2] for r in rows) + b"]}", k


# ---- stand-alone sanitizer run ------------------------------------------------------------------

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None,
                    reason="needs ROCm clang++ and make")
def test_bayer_codec_under_address_and_ub_sanitizers():
    target = "build/asan/bayer_check"
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
