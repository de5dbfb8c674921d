"""The edge-directed Bayer demosaic (--input-bayer-demosaic hamilton) on the host: the oracle
against a hand-computed frame and flat colours, its bounds and the branches its test frames take,
the twin and the parser against the oracle, configuration, the stub engine and the sanitizer
program. Every comparison is on the bits."""

import os
import shutil
import subprocess

import numpy as np
import pytest

from gale._native import native
from gale.config import from_sources
from gale.data import encode_records_raw, mosaic_bayer
from gale.models.preprocess import BayerConvert, BayerHiConvert, _hamilton_green
from test_bayer_cpu import CLANG, ORDERS, PREP, ROOT, cfg, frames_of
from test_input_raw_cpu import BAD_SHAPE, CIFAR, OK, serve

C = native()
# the shapes of the kernel's tests (tiles of 32 x 32): every neighbour reflected; a tail of 2
# columns, WS % 4 == 2; one whole tile; both seams with partial tiles of 2, the halo column 34 being
# column WS; both seams with WS % 4 == 0; 17 tiles in a row, one wave each
SHAPES = [(4, 4), (4, 6), (6, 10), (32, 32), (34, 34), (36, 40), (4, 520)]


def edge_frames(size, which):
    """uint8 [3, HS*WS]: the frames that noise does not give. 0: noise of 0..3 (ties are common),
    rows of 0 / 255, columns of 0 / 255; 1: a checkerboard of 2 x 2 cells of 0 / 255, its inverse
    (both clamps) and noise of 0..3 on 252."""
    HS, WS = size
    rng = np.random.default_rng(HS * 31 + WS + which)
    low = rng.integers(0, 4, (HS, WS))
    y, x = np.ogrid[:HS, :WS]
    zero = np.zeros((HS, WS), np.int64)
    if which == 0:
        f = [low, (y & 1) * 255 + zero, (x & 1) * 255 + zero]
    else:
        board = (((x >> 1) + (y >> 1)) & 1) * 255
        f = [board, 255 - board, 252 + low]
    return np.stack(f).astype(np.uint8).reshape(3, -1)


def test_oracle_equals_a_hand_computed_frame():
    """bayer_rggb8, 4 x 6, every pixel worked out from the contract. The three branches, e.g.:
    (0, 0) s = 10: dH = 0 + |20 - 20 - 20| = 20 < dV = 0 + |20 - 30 - 30| = 40, gH = (0 + 20 - 40 + 2)
    >> 2 = -5 -> 0; (2, 2) s = 250: dH = 0 + |500 - 30 - 60| = 410 > dV = 55 + |500 - 20 - 250| = 285,
    gV = (910 + 230 + 2) >> 2 = 285 -> 255; (0, 4) s = 45: dH = 5 + 25 = dV = 0 + 30, gA =
    (2 * 985 + 25 - 30 + 4) >> 3 = 246."""
    frame = np.array([[10, 0, 20, 250, 45, 255], [255, 0, 255, 10, 240, 5],
                      [30, 240, 250, 240, 60, 120], [140, 90, 200, 70, 255, 0]], np.uint8)
    want = np.array([
        [(10, 0, 0), (0, 0, 0), (20, 121, 0), (99, 250, 9), (45, 246, 9), (54, 255, 22)],
        [(174, 255, 2), (186, 253, 0), (202, 255, 8), (127, 251, 10), (44, 240, 3), (42, 238, 5)],
        [(30, 203, 34), (151, 240, 71), (250, 255, 68), (142, 240, 35), (60, 251, 61), (0, 120, 0)],
        [(0, 140, 55), (86, 175, 90), (195, 200, 73), (142, 240, 70), (64, 255, 111), (0, 118, 0)],
    ], np.uint8)
    bc = BayerConvert("bayer_rggb8", "hamilton")
    assert np.array_equal(bc.apply(frame.reshape(-1), 4, 6), want)
    assert bc.green_choice(frame, 4, 6).tolist() == [[[1, 0, 1, 0, 3, 0], [0, 1, 0, 1, 0, 1],
                                                      [2, 0, 2, 0, 2, 0], [0, 1, 0, 1, 0, 2]]]
    # bggr sees the same sites with red and blue exchanged
    assert np.array_equal(BayerConvert("bayer_bggr8", "hamilton").apply(frame.reshape(-1), 4, 6),
                          want[..., ::-1])


@pytest.mark.parametrize("order", ORDERS)
def test_flat_colour_demosaics_to_itself(order):
    rgb = np.empty((6, 10, 3), np.uint8)
    rgb[:] = (200, 31, 97)
    mosaic = mosaic_bayer(rgb, order)
    assert np.array_equal(BayerConvert(order, "hamilton").apply(mosaic.reshape(-1), 6, 10), rgb)


def test_bounds_and_the_three_deep_reflection():
    """The docstring's ranges on noise and on the extremes, and K reflected one deep = G^ on S
    reflected three deep (what the kernel stages)."""
    HS, WS = 34, 22
    s = np.concatenate([frames_of(6, HS, WS, 3), edge_frames((HS, WS), 0), edge_frames((HS, WS), 1)])
    s = s.reshape(-1, HS, WS).astype(np.int32)
    p3 = np.pad(s, [(0, 0), (3, 3), (3, 3)], mode="reflect")
    g, _ = _hamilton_green(np.pad(s, [(0, 0), (2, 2), (2, 2)], mode="reflect"))
    assert -127 <= g.min() and g.max() <= 383
    k = s - np.clip(g, 0, 255)
    assert -255 <= k.min() and k.max() <= 255
    assert np.array_equal(_hamilton_green(p3)[0],
                          np.pad(g, [(0, 0), (1, 1), (1, 1)], mode="reflect"))


@pytest.mark.parametrize("size", [s for s in SHAPES if s >= (6, 10)], ids=str)
@pytest.mark.parametrize("order", ORDERS)
def test_the_kernel_tests_frames_take_every_branch(order, size):
    """The frames test_bayer_hamilton_gpu.py launches at a shape - its noise and both edge sets -
    take gH, gV and gA at least 8 times each (noise alone ties once in hundreds of sites)."""
    frames = np.concatenate([frames_of(1, *size, size[0] * 1009 + size[1]),
                             edge_frames(size, 0), edge_frames(size, 1)])
    choice = BayerConvert(order, "hamilton").green_choice(frames, *size)
    counts = np.bincount(choice.reshape(-1), minlength=4)
    assert counts[0] == choice.size // 2 and (counts[1:] >= 8).all(), counts


@pytest.mark.parametrize("HS,WS", [(4, 4), (4, 6), (6, 10), (32, 32)], ids=str)
@pytest.mark.parametrize("order", ORDERS)
def test_host_twin_and_parser_equal_the_oracle(order, HS, WS):
    bc = BayerConvert(order, "hamilton")
    frames = np.concatenate([frames_of(2, HS, WS, HS * 100 + WS), edge_frames((HS, WS), 0)])
    rgb = bc.apply(frames, HS, WS)
    assert not np.array_equal(rgb, BayerConvert(order, "malvar").apply(frames, HS, WS))
    a, b = PREP.coeffs()
    for i, fr in enumerate(frames):
        u8, f32 = C.bayer_hamilton_to_rgb_host(fr.tobytes(), HS, WS, order)
        assert np.array_equal(u8, rgb[i]) and np.array_equal(f32, bc.to_float(rgb[i]))
        _, f32p = C.bayer_hamilton_to_rgb_host(fr.tobytes(), HS, WS, order, a=a, b=b)
        assert np.array_equal(f32p.view(np.uint32), bc.to_float(rgb[i], PREP).view(np.uint32))
    rec = frames.tobytes()
    st, out = C.parse_instances_raw_bayer_host(rec, HS, WS, order, demosaic="hamilton")
    assert st == OK and np.array_equal(out, bc.to_float(rgb))
    assert C.parse_instances_raw_bayer_host(rec[:-1], HS, WS, order, demosaic="hamilton")[0] == BAD_SHAPE
    assert C.parse_instances_raw_bayer_host(rec[:8], 2, 4, order, demosaic="hamilton")[0] == BAD_SHAPE
    with pytest.raises(ValueError):
        C.bayer_hamilton_to_rgb_host(rec[:8], 4, 2, order)
    with pytest.raises(ValueError):
        bc.apply(frames[:, :8], 2, 4)


# ---- configuration ------------------------------------------------------------------------------

BAYER = dict(input_format="raw", input_pixel_format="bayer_grbg8")
# (configuration that validates without the option, the refusal's text)
REFUSED = [
    (dict(input_format="raw"), "--input-bayer-demosaic hamilton needs"),
    (dict(input_format="b64", input_pixel_format="i420"), "--input-bayer-demosaic hamilton needs"),
    (dict(input_format="raw", input_pixel_format="gray"), "--input-bayer-demosaic hamilton needs"),
    (dict(input_format="raw", input_pixel_format="bayer_rggb10le"),
     "--input-bayer-demosaic hamilton needs"),
    (dict(input_format="raw", input_pixel_format="bayer_gbrg12p"),
     "--input-bayer-demosaic hamilton needs"),
    (dict(BAYER, input_size="2,32", input_resize="32,32"), "--input-bayer-demosaic hamilton.*>= 4"),
    (dict(BAYER, input_size="32,2", input_resize="32,32"), "--input-bayer-demosaic hamilton.*>= 4"),
]


@pytest.mark.parametrize("kw,match", REFUSED,
                         ids=["rgb", "i420", "gray", "10le", "12p", "HS=2", "WS=2"])
def test_refusals_name_the_option(kw, match):
    d = cfg(**kw).engine_dict(32, 32, 3, 10)
    assert "bayer_demosaic" not in d
    C.Engine(d)
    with pytest.raises(ValueError, match=match):
        cfg(**kw, input_bayer_demosaic="hamilton")
    # the native engine refuses the same combination in a dict built by hand
    with pytest.raises(ValueError, match="bayer_demosaic hamilton"):
        C.Engine(dict(d, bayer_demosaic="hamilton"))


def test_the_deep_mosaics_keep_their_two_names():
    with pytest.raises(ValueError, match="bilinear or malvar"):
        BayerHiConvert("bayer_rggb10le", "hamilton")
    assert BayerHiConvert("bayer_rggb10le", "malvar").demosaic == "malvar"


def test_option_precedence_and_engine_key(tmp_path):
    toml = tmp_path / "gale.toml"
    toml.write_text('[gale]\ntopology_name = "t"\ninput_topic = "in"\noutput_topic = "out"\n'
                    'input_format = "raw"\n'
                    'input_pixel_format = "bayer_rggb8"\ninput-bayer-demosaic = "hamilton"\n')
    env = {"GALE_INPUT_BAYER_DEMOSAIC": "malvar"}
    assert from_sources({}, {}, str(toml)).input_bayer_demosaic == "hamilton"
    assert from_sources({}, env, str(toml)).input_bayer_demosaic == "malvar"
    c = from_sources({"input_bayer_demosaic": "hamilton"}, env, str(toml))
    assert c.input_bayer_demosaic == "hamilton"
    d = c.engine_dict(32, 32, 3, 10)
    assert d["bayer_demosaic"] == "hamilton" and d["pixel_format"] == "bayer_rggb8"
    C.Engine(d)
    assert c.input_unpack() == BayerConvert("bayer_rggb8", "hamilton")
    assert c.input_unpack().kernel_kwargs() == dict(order="bayer_rggb8")


# ---- the stub engine ----------------------------------------------------------------------------

def test_stub_engine_equals_raw_rgb_records_of_the_oracle():
    """The record of 9 frames over --max-batch 4 is split on frame boundaries and joined; every
    output is that of the oracle's image sent as a raw rgb record."""
    counts, order = [1, 2, 9, 1], "bayer_gbrg8"
    bc, rng = BayerConvert(order, "hamilton"), np.random.default_rng(5)
    sets = {f"r{i}".encode(): rng.integers(0, 256, (n, 32 * 32), dtype=np.uint8)
            for i, n in enumerate(counts)}
    kw = dict(max_batch=4, on_error="null", input_format="raw", **CIFAR)
    want, _ = serve([(k, encode_records_raw(bc.apply(f, 32, 32), f.shape[0])[0])
                     for k, f in sets.items()], **kw)
    kw.update(input_pixel_format=order, input_bayer_demosaic="hamilton")
    got, st = serve([(k, f.tobytes()) for k, f in sets.items()], **kw)
    assert got == want and (st["raw_records"], st["split_records"]) == (len(counts), 1), st


# ---- stand-alone sanitizer run ------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None,
                    reason="needs ROCm clang++ and make")
def test_hamilton_codec_under_address_and_ub_sanitizers():
    target = "build/asan/bayer_hamilton_check"
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
