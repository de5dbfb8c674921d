"""Raw 10/12/16-bit Bayer mosaic records (--input-pixel-format bayer_<order>{10le,12le,16le,10p,
12p}) on the host: the oracle against a hand-computed frame and flat colours, the twin and the
parser against the oracle, verdicts, configuration, the stub engine and the sanitizer program.
Every comparison of outputs is on the bits."""

import os
import shutil
import subprocess

import numpy as np
import pytest

from gale._native import native
from gale.data import encode_records_raw, mosaic_bayer, pack_bayer_hi
from gale.models.preprocess import BayerHiConvert
from test_bayer_cpu import CLANG, PREP, REFUSED, ROOT, cfg
from test_input_raw_cpu import BAD_SHAPE, CIFAR, EMPTY, OK, serve

C = native()
FORMS = ("10le", "12le", "16le", "10p", "12p")
ORDERS = ("rggb", "bggr", "grbg", "gbrg")
DEMOSAICS = ("bilinear", "malvar")


@pytest.mark.parametrize("form", FORMS)
def test_oracle_equals_a_hand_computed_frame(form):
    """The frame and RGB of test_bayer_cpu's hand-computed case with every sample shifted to the
    depth (k = bits - 8). A deep average is 2^k S / 2^sh exactly (S the tap sum, sh = 1 or 2), so
    rounding it half up to 8 bits gives that test's RGB at every pixel, and a site's own sample is
    the shifted one."""
    frame = np.array([[1, 2, 3, 4], [5, 6, 7, 9], [8, 12, 10, 20], [30, 40, 50, 61]], np.uint16)
    want = np.array([
        [(1, 4, 6), (2, 2, 6), (3, 5, 8), (3, 4, 9)],
        [(5, 5, 6), (6, 7, 6), (7, 7, 8), (7, 10, 9)],
        [(8, 15, 23), (9, 12, 23), (10, 22, 29), (10, 20, 35)],
        [(8, 30, 40), (9, 26, 40), (10, 50, 51), (10, 35, 61)]], np.int64)
    bc = BayerHiConvert(f"bayer_rggb{form}")
    k = bc.bits - 8
    rgb = bc.apply(pack_bayer_hi((frame << k)[None], bc.format), 4, 4)[0].astype(np.int64)
    assert np.array_equal((rgb + (1 << (k - 1))) >> k, want)
    assert rgb[0, 0, 0] == 1 << k and rgb[1, 1, 2] == 6 << k and rgb[3, 2, 1] == 50 << k
    assert rgb[0, 0, 1] == (2 + 2 + 5 + 5) << k >> 2 and rgb[0, 1, 0] == (1 + 3) << k >> 1


@pytest.mark.parametrize("demosaic", DEMOSAICS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", ORDERS)
def test_flat_colour_demosaics_to_itself(order, form, demosaic):
    bc = BayerHiConvert(f"bayer_{order}{form}", demosaic)
    rgb = np.empty((1, 6, 12, 3), np.uint8)
    rgb[:] = (200, 31, 97)
    mosaic = mosaic_bayer(rgb, f"bayer_{order}8").astype(np.uint16) << (bc.bits - 8)
    got = bc.apply(pack_bayer_hi(mosaic, bc.format), 6, 12)
    assert np.array_equal(got, rgb.astype(np.uint16) << (bc.bits - 8))


@pytest.mark.parametrize("HS,WS", [(4, 4), (6, 12), (32, 32)], ids=str)
@pytest.mark.parametrize("demosaic", DEMOSAICS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", ORDERS)
def test_host_twin_and_parser_equal_the_oracle(order, form, demosaic, HS, WS):
    bc = BayerHiConvert(f"bayer_{order}{form}", demosaic)
    rng = np.random.default_rng(HS * 100 + WS)
    m = rng.integers(0, 1 << bc.bits, (4, HS, WS), dtype=np.uint16)
    m[2], m[3] = 0, (1 << bc.bits) - 1
    frames = pack_bayer_hi(m, bc.format)
    B = frames.shape[1]
    assert bc.frame_bytes(HS, WS) == B == C.bayer_hi_bytes(HS, WS, bc.format)
    assert np.array_equal(bc.unpack(frames, HS, WS), m)
    rgb = bc.apply(frames, HS, WS)
    if bc.packing == "le16" and bc.bits < 16:  # random upper bits: the frame of the masked words
        frames = pack_bayer_hi(m, bc.format, rng.integers(0, 1 << 16, m.shape, dtype=np.uint16))
        assert not np.array_equal(frames.view("<u2") >> bc.bits, np.zeros_like(frames.view("<u2")))
        assert np.array_equal(bc.apply(frames, HS, WS), rgb)
    a, b = PREP.coeffs()
    for i, fr in enumerate(frames):
        u16, f32 = C.bayer_hi_to_rgb_host(fr.tobytes(), HS, WS, bc.format, demosaic)
        assert np.array_equal(u16, rgb[i]) and np.array_equal(f32, bc.to_float(rgb[i]))
        _, f32p = C.bayer_hi_to_rgb_host(fr.tobytes(), HS, WS, bc.format, demosaic, a=a, b=b)
        assert np.array_equal(f32p.view(np.uint32), bc.to_float(rgb[i], PREP).view(np.uint32))
    rec = frames.tobytes()
    st, out = C.parse_instances_raw_bayer_hi_host(rec, HS, WS, bc.format, demosaic=demosaic)
    assert st == OK and np.array_equal(out, bc.to_float(rgb))
    # verdicts: records of 0, B - 1, B + 1 and 2 B bytes; the splitter gives whole frames
    for n, want in ((0, EMPTY), (B - 1, BAD_SHAPE), (B + 1, BAD_SHAPE), (2 * B, OK)):
        assert C.parse_instances_raw_bayer_hi_host(rec[:n], HS, WS, bc.format,
                                                   demosaic=demosaic)[0] == want, n
    assert C.parse_instances_raw_bayer_hi_host(rec, HS, WS, f"bayer_{order}8")[0] == BAD_SHAPE
    assert C.split_instances_raw(4 * B, B, 3) == [(0, 3 * B), (3 * B, 4 * B)]


# ---- configuration ------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["bayer_rggb10le", "bayer_bggr16le", "bayer_grbg10p", "bayer_gbrg12p"])
@pytest.mark.parametrize("kw,match,engine_kw", REFUSED + [
    (dict(input_size="32,6", input_resize="32,32"), "WS % 4", dict(rec_W=6))], ids=[
    "json", "b64", "nchw", "C=1", "odd-HS", "odd-WS", "dtype", "matrix", "range", "chroma",
    "ingest", "WS=6"])
def test_refusals_name_their_option(fmt, kw, match, engine_kw):
    """test_bayer_cpu's table for the deep formats, and four pixels in five bytes with WS = 6."""
    ok = cfg(input_format="raw", input_pixel_format=fmt)
    d = ok.engine_dict(32, 32, 3, 10)
    assert d["pixel_format"] == fmt and ok.input_unpack() == BayerHiConvert(fmt)
    C.Engine(d)
    if match == "WS % 4" and not fmt.endswith("10p"):  # (a frame of every other form)
        C.Engine(cfg(input_format="raw", input_pixel_format=fmt, **kw).engine_dict(32, 32, 3, 10))
        return
    with pytest.raises(ValueError, match=match):
        cfg(**{"input_format": "raw", "input_pixel_format": fmt, **kw})
    # the native engine refuses the same combination in a dict built by hand
    with pytest.raises(ValueError):
        C.Engine(dict(d, **engine_kw))


# ---- the stub engine ----------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["bayer_gbrg10p", "bayer_rggb12le"])
def test_stub_engine_splits_on_frame_boundaries(fmt):
    """The record of 9 frames over --max-batch 4 is split on frame boundaries and joined; every
    output is that of the oracle's image sent as a raw rgb u16 record, and a short record is an
    error."""
    counts = [1, 2, 9, 1]
    bc, rng = BayerHiConvert(fmt, "malvar"), np.random.default_rng(5)
    sets = {f"r{i}".encode(): pack_bayer_hi(rng.integers(0, 1 << bc.bits, (n, 32, 32)), fmt)
            for i, n in enumerate(counts)}
    kw = dict(max_batch=4, on_error="null", input_format="raw", **CIFAR)
    want, _ = serve([(k, encode_records_raw(bc.apply(f, 32, 32), f.shape[0], "u16")[0])
                     for k, f in sets.items()], input_dtype="u16", **kw)
    kw.update(input_pixel_format=fmt, input_bayer_demosaic="malvar")
    got, st = serve([(k, f.tobytes()) for k, f in sets.items()]
                    + [(b"short", sets[b"r2"].tobytes()[:-2])], **kw)
    assert got.pop(b"short") is None and got == want
    assert (st["raw_records"], st["errors"], st["split_records"]) == (len(counts), 1, 1), st


# ---- stand-alone sanitizer run ------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None,
                    reason="needs ROCm clang++ and make")
def test_bayer_hi_codec_under_address_and_ub_sanitizers():
    target = "build/asan/bayer_hi_check"
    b = subprocess.run(["make", "-C", ROOT, target], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, target), "2000"], capture_output=True, text=True,
                       timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "all checks passed" in out
    assert "AddressSanitizer" not in out and "runtime error" not in out
