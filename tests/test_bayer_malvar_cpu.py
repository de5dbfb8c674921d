"""The gradient-corrected Bayer demosaic (--input-bayer-demosaic malvar) on the host: the oracle
against a hand-computed frame and flat colours, the twin and the parser against the oracle,
configuration, the stub engine and the sanitizer program. Every comparison is on the bits."""

import os
import shutil
import subprocess

import numpy as np
import pytest

from gale._native import native
from gale.config import from_sources
from gale.data import encode_records_raw, mosaic_bayer
from gale.models.preprocess import BayerConvert
from test_bayer_cpu import CLANG, ORDERS, PREP, ROOT, cfg, frames_of
from test_input_raw_cpu import BAD_SHAPE, CIFAR, OK, serve

C = native()


def test_oracle_equals_a_hand_computed_frame():
    """bayer_rggb8, 4 x 6: both edges and an interior column pair, every pixel worked out on paper
    from the contract (reflection: -2 -> 2, -1 -> 1, n -> n - 2, n + 1 -> n - 3). Eleven
    numerators are negative, e.g. B at (0, 0): 12*10 + 4*0 - 3*(40 + 60) = -180 -> 0; one is over
    255: G at (2, 2): 8*250 + 4*(480 + 455) - 2*(90 + 270) = 5020 -> 314 -> 255."""
    frame = np.array([[10, 200, 20, 250, 0, 255], [255, 0, 255, 10, 240, 5],
                      [30, 240, 250, 240, 60, 120], [140, 90, 200, 70, 255, 0]], np.uint8)
    want = np.array([
        [(10, 220, 0), (0, 200, 0), (20, 186, 0), (16, 250, 11), (0, 229, 0), (0, 255, 46)],
        [(52, 255, 10), (59, 225, 0), (152, 255, 15), (74, 241, 10), (41, 240, 18), (29, 213, 5)],
        [(30, 166, 0), (151, 240, 64), (250, 255, 163), (172, 240, 33), (60, 198, 0), (0, 120, 0)],
        [(0, 140, 39), (178, 230, 90), (216, 200, 68), (187, 255, 70), (98, 255, 78), (32, 169, 0)],
    ], np.uint8)
    assert np.array_equal(BayerConvert("bayer_rggb8", "malvar").apply(frame.reshape(-1), 4, 6), want)
    # bggr sees the same sites with red and blue exchanged
    assert np.array_equal(BayerConvert("bayer_bggr8", "malvar").apply(frame.reshape(-1), 4, 6),
                          want[..., ::-1])


@pytest.mark.parametrize("order", ORDERS)
def test_flat_colour_demosaics_to_itself(order):
    rgb = np.empty((6, 10, 3), np.uint8)
    rgb[:] = (200, 31, 97)
    mosaic = mosaic_bayer(rgb, order)
    assert np.array_equal(BayerConvert(order, "malvar").apply(mosaic.reshape(-1), 6, 10), rgb)


@pytest.mark.parametrize("HS,WS", [(4, 4), (4, 6), (6, 10), (32, 32)], ids=str)
@pytest.mark.parametrize("order", ORDERS)
def test_host_twin_and_parser_equal_the_oracle(order, HS, WS):
    bc, frames = BayerConvert(order, "malvar"), frames_of(2, HS, WS, HS * 100 + WS)
    rgb = bc.apply(frames, HS, WS)
    assert not np.array_equal(rgb, BayerConvert(order).apply(frames, HS, WS))
    a, b = PREP.coeffs()
    for i, fr in enumerate(frames):
        u8, f32 = C.bayer_malvar_to_rgb_host(fr.tobytes(), HS, WS, order)
        assert np.array_equal(u8, rgb[i]) and np.array_equal(f32, bc.to_float(rgb[i]))
        _, f32p = C.bayer_malvar_to_rgb_host(fr.tobytes(), HS, WS, order, a=a, b=b)
        assert np.array_equal(f32p.view(np.uint32), bc.to_float(rgb[i], PREP).view(np.uint32))
    rec = frames.tobytes()
    st, out = C.parse_instances_raw_bayer_host(rec, HS, WS, order, demosaic="malvar")
    assert st == OK and np.array_equal(out, bc.to_float(rgb))
    assert C.parse_instances_raw_bayer_host(rec[:-1], HS, WS, order, demosaic="malvar")[0] == BAD_SHAPE
    # a size under 4 is a frame of the bilinear demosaic only
    assert C.parse_instances_raw_bayer_host(rec[:8], 2, 4, order)[0] == OK
    assert C.parse_instances_raw_bayer_host(rec[:8], 2, 4, order, demosaic="malvar")[0] == BAD_SHAPE
    with pytest.raises(ValueError):
        C.bayer_malvar_to_rgb_host(rec[:8], 4, 2, order)
    with pytest.raises(ValueError):
        bc.apply(frames[:, :8], 2, 4)


# ---- configuration ------------------------------------------------------------------------------

BAYER = dict(input_format="raw", input_pixel_format="bayer_grbg8")
# (configuration that validates without the option, the refusal's text, the same in an engine dict)
REFUSED = [
    (dict(input_format="raw"), "--input-bayer-demosaic malvar needs", {}),
    (dict(input_format="b64"), "--input-bayer-demosaic malvar needs", {}),
    (dict(input_format="b64", input_pixel_format="i420"), "--input-bayer-demosaic malvar needs", {}),
    (dict(input_format="raw", input_pixel_format="gray"), "--input-bayer-demosaic malvar needs", {}),
    (dict(BAYER, input_size="2,32", input_resize="32,32"), "--input-bayer-demosaic.*>= 4", {}),
    (dict(BAYER, input_size="32,2", input_resize="32,32"), "--input-bayer-demosaic.*>= 4", {}),
    (BAYER, "input_bayer_demosaic", dict(input_bayer_demosaic="vng")),
]


@pytest.mark.parametrize("kw,match,bad", REFUSED,
                         ids=["rgb-raw", "rgb-b64", "i420", "gray", "HS=2", "WS=2", "name"])
def test_refusals_name_the_option(kw, match, bad):
    ok = cfg(**kw, input_bayer_demosaic="bilinear")  # named or defaulted: accepted, no engine key
    d = ok.engine_dict(32, 32, 3, 10)
    assert d == cfg(**kw).engine_dict(32, 32, 3, 10) and "bayer_demosaic" not in d
    C.Engine(d)
    with pytest.raises(ValueError, match=match):
        cfg(**{**kw, "input_bayer_demosaic": "malvar", **bad})
    # the native engine refuses the same combination in a dict built by hand
    with pytest.raises(ValueError, match="bayer_demosaic"):
        C.Engine(dict(d, bayer_demosaic=bad.get("input_bayer_demosaic", "malvar")))


def test_option_precedence_and_engine_key(tmp_path):
    toml = tmp_path / "gale.toml"
    toml.write_text('[gale]\ntopology_name = "t"\ninput_topic = "in"\noutput_topic = "out"\n'
                    'input_format = "raw"\n'
                    'input_pixel_format = "bayer_rggb8"\ninput-bayer-demosaic = "malvar"\n')
    env = {"GALE_INPUT_BAYER_DEMOSAIC": "bilinear"}
    assert from_sources({}, {}, str(toml)).input_bayer_demosaic == "malvar"
    assert from_sources({}, env, str(toml)).input_bayer_demosaic == "bilinear"
    c = from_sources({"input_bayer_demosaic": "malvar"}, env, str(toml))
    assert c.input_bayer_demosaic == "malvar"
    d = c.engine_dict(32, 32, 3, 10)
    assert d["bayer_demosaic"] == "malvar" and d["pixel_format"] == "bayer_rggb8"
    C.Engine(d)
    assert c.input_unpack() == BayerConvert("bayer_rggb8", "malvar")


# ---- the stub engine ----------------------------------------------------------------------------

def test_stub_engine_equals_raw_rgb_records_of_the_oracle():
    """The record of 9 frames over --max-batch 4 is split on frame boundaries and joined; every
    output is that of the oracle's image sent as a raw rgb record, and of the frames sent singly."""
    counts, order = [1, 2, 9, 1], "bayer_gbrg8"
    bc, rng = BayerConvert(order, "malvar"), np.random.default_rng(5)
    sets = {f"r{i}".encode(): rng.integers(0, 256, (n, 32 * 32), dtype=np.uint8)
            for i, n in enumerate(counts)}
    kw = dict(max_batch=4, on_error="null", input_format="raw", **CIFAR)
    want, _ = serve([(k, encode_records_raw(bc.apply(f, 32, 32), f.shape[0])[0])
                     for k, f in sets.items()], **kw)
    kw.update(input_pixel_format=order, input_bayer_demosaic="malvar")
    got, st = serve([(k, f.tobytes()) for k, f in sets.items()], **kw)
    assert got == want and (st["raw_records"], st["split_records"]) == (len(counts), 1), st
    one, _ = serve([(b"%d" % i, f.tobytes()) for i, f in enumerate(sets[b"r2"])], **kw)
    pre = b'{"predictions":['
    assert got[b"r2"] == pre + b",".join(one[b"%d" % i][len(pre):-2] for i in range(9)) + b"]}"


# ---- stand-alone sanitizer run ------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None,
                    reason="needs ROCm clang++ and make")
def test_malvar_codec_under_address_and_ub_sanitizers():
    target = "build/asan/bayer_malvar_check"
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
