"""Input resize (--input-size / --input-resize) without a GPU: the tables against an independent
rational derivation and against the native builder, the numpy oracle against exact rational
arithmetic with one rounding per stated operation, the host twin against the oracle, crops as bit
copies, a sanity check against torch's bilinear interpolation, configuration sources and
refusals, the stub engine end to end, and the stand-alone sanitizer driver."""

import base64
import json
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gale._native import native
from gale.cli import parse_topology_args, produce_shape
from gale.config import GaleConfig, from_sources
from gale.models.preprocess import InputPrep, InputResize

C = native()
K = C.kafka
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CIFAR_MEAN_S = "0.4914,0.4822,0.4465"
CIFAR_STD_S = "0.2470,0.2435,0.2616"

# (HS, WS, HR, WR, H, W, C): an upscale where both clamps are hit, two mixed resizes
SHAPES = [(5, 7, 32, 33, 32, 32, 3), (37, 41, 33, 35, 32, 32, 3), (30, 33, 29, 31, 28, 28, 1)]
CROP = (40, 36, 40, 36, 32, 32, 3)


def f32_round(x: Fraction) -> np.float32:
    """The binary32 nearest to the rational x, ties to even."""
    if x == 0:
        return np.float32(0.0)
    sign = -1 if x < 0 else 1
    x = abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    if e < -126:
        m, e = round(x / Fraction(2) ** -149), -149
        return np.float32(sign * math.ldexp(m, e))
    m = round(x / Fraction(2) ** (e - 23))
    if e > 127 or (m == 1 << 24 and e == 127):
        return np.float32(sign * math.inf)
    return np.float32(sign * math.ldexp(m, e - 23))


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. tables ---------------------------------------------------------------------------------

def axis_by_fractions(n_src, n_rs, n_out):
    """The half-pixel source coordinate of each output pixel as a rational: its floor and the
    correctly rounded fraction, with the two clamps."""
    off = (n_rs - n_out) // 2
    i0, i1, w = [], [], []
    for i in range(n_out):
        pos = (Fraction(2 * (i + off) + 1, 2)) * Fraction(n_src, n_rs) - Fraction(1, 2)
        if pos < 0:
            i0.append(0), i1.append(0), w.append(np.float32(0))
            continue
        fl = pos.numerator // pos.denominator
        if fl >= n_src - 1:
            i0.append(n_src - 1), i1.append(n_src - 1), w.append(np.float32(0))
            continue
        i0.append(fl), i1.append(fl + 1), w.append(f32_round(pos - fl))
    return np.array(i0, np.int32), np.array(i1, np.int32), np.array(w, np.float32)


TABLE_DIMS = SHAPES + [CROP, (9, 6, 9, 6, 8, 4, 1), (7, 5, 9, 11, 6, 7, 3),
                       (375, 500, 256, 341, 224, 224, 3), (1, 1, 4096, 4096, 4096, 4095, 1),
                       (4096, 4095, 4096, 4096, 1, 2, 1)]


@pytest.mark.parametrize("dims", TABLE_DIMS, ids=lambda d: "x".join(map(str, d[:6])))
def test_tables_match_rational_derivation_and_native_builder(dims):
    HS, WS, HR, WR, H, W, _ = dims
    got = InputResize(HS, WS, HR, WR, H, W).tables()
    want = axis_by_fractions(HS, HR, H) + axis_by_fractions(WS, WR, W)
    nat = C.build_resize_tables(HS, WS, HR, WR, H, W)
    assert len(got) == len(nat) == 6
    for g, w, n in zip(got, want, nat):
        assert g.dtype == w.dtype == n.dtype and g.shape == w.shape == n.shape
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
        assert np.array_equal(g.view(np.uint32), n.view(np.uint32))
    for i0, i1, w, n_src in ((got[0], got[1], got[2], HS), (got[3], got[4], got[5], WS)):
        assert (i0 >= 0).all() and (i1 < n_src).all() and (i0 <= i1).all()
        assert (w >= 0).all() and (w < 1).all() and (np.diff(i0) >= 0).all()


# ---- 2. the oracle and the host twin -----------------------------------------------------------

def lerp_exact(a, b, w):
    if w == 0:
        return a
    d = f32_round(Fraction(float(b)) - Fraction(float(a)))
    return f32_round(Fraction(float(w)) * Fraction(float(d)) + Fraction(float(a)))


def apply_by_fractions(x, rs: InputResize):
    y0, y1, wy, x0, x1, wx = axis_by_fractions(rs.HS, rs.HR, rs.H) + \
        axis_by_fractions(rs.WS, rs.WR, rs.W)
    out = np.zeros((rs.H, rs.W, x.shape[-1]), np.float32)
    for y in range(rs.H):
        for xx in range(rs.W):
            for c in range(x.shape[-1]):
                t = lerp_exact(x[y0[y], x0[xx], c], x[y0[y], x1[xx], c], wx[xx])
                u = lerp_exact(x[y1[y], x0[xx], c], x[y1[y], x1[xx], c], wx[xx])
                out[y, xx, c] = lerp_exact(t, u, wy[y])
    return out


def random_images(rng, n, HS, WS, Ch):
    """fp32 values of both signs over several binades (so the roundings are not trivial)."""
    x = rng.standard_normal((n, HS, WS, Ch)) * 10.0 ** rng.integers(-2, 3, (n, HS, WS, Ch))
    return x.astype(np.float32)


@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_oracle_is_one_rounding_per_operation_and_host_twin_matches(dims):
    HS, WS, HR, WR, H, W, Ch = dims
    rs = InputResize(HS, WS, HR, WR, H, W)
    x = random_images(np.random.default_rng(HS * 100 + WS), 3, HS, WS, Ch)
    got = rs.apply(x)
    assert got.shape == (3, H, W, Ch) and got.dtype == np.float32
    want0 = apply_by_fractions(x[0], rs)
    assert np.array_equal(u32(got[0]), u32(want0))
    host = C.resize_crop_host(x, HR, WR, H, W)
    assert host.shape == got.shape and np.array_equal(u32(host), u32(got))
    # torch tensors go through the same oracle
    assert np.array_equal(u32(rs.apply(torch.from_numpy(x)).numpy()), u32(got))


def test_crop_is_a_bit_copy_also_next_to_max_and_nan():
    HS, WS, HR, WR, H, W, Ch = CROP
    rs = InputResize(HS, WS, HR, WR, H, W)
    x = random_images(np.random.default_rng(3), 2, HS, WS, Ch)
    # +-max and NaN inside the window and right outside it (rows 3 / 36, columns 1 / 34)
    for (i, y, xx, c, v) in [(0, 3, 5, 0, 3.4e38), (0, 4, 5, 0, -3.4e38), (0, 4, 6, 1, np.nan),
                             (0, 36, 7, 2, np.nan), (1, 10, 1, 0, 3.4e38), (1, 10, 2, 0, -3.4e38),
                             (1, 35, 34, 1, np.nan), (1, 35, 33, 1, -3.4e38),
                             (1, 20, 20, 2, np.inf)]:
        x[i, y, xx, c] = v
    want = x[:, 4:36, 2:34]
    assert np.array_equal(u32(rs.apply(x)), u32(want))
    assert np.array_equal(u32(C.resize_crop_host(x, HR, WR, H, W)), u32(want))
    _, _, wy, _, _, wx = rs.tables()
    assert not wy.any() and not wx.any()


@pytest.mark.parametrize("dims", SHAPES + [CROP], ids=lambda d: "x".join(map(str, d)))
def test_close_to_torch_bilinear(dims):
    HS, WS, HR, WR, H, W, Ch = dims
    x = np.random.default_rng(11).integers(0, 256, (2, HS, WS, Ch)).astype(np.float32)
    got = InputResize(HS, WS, HR, WR, H, W).apply(x)
    t = F.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), size=(HR, WR), mode="bilinear",
                      align_corners=False, antialias=False).permute(0, 2, 3, 1).numpy()
    oy, ox = (HR - H) // 2, (WR - W) // 2
    err = float(np.abs(got - t[:, oy:oy + H, ox:ox + W]).max())
    bound = float(np.abs(x).max()) * max(HS, WS) * 2.0 ** -20
    print(f"{dims}: max |oracle - torch| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    if (HS, WS) == (HR, WR):
        assert err == 0.0


def test_host_twin_refuses_bad_dimensions():
    x = np.zeros((1, 5, 7, 3), np.float32)
    for hr, wr, h, w in [(3, 8, 4, 4), (8, 3, 4, 4), (4097, 8, 4, 4), (8, 8, 0, 4)]:
        with pytest.raises(ValueError):
            C.resize_crop_host(x, hr, wr, h, w)
    with pytest.raises(ValueError):
        C.build_resize_tables(0, 4, 4, 4, 4, 4)
    with pytest.raises(ValueError):
        C.build_resize_tables(4, 4, 4, 4097, 4, 4)


# ---- 3. configuration --------------------------------------------------------------------------

def test_config_sources_and_precedence(tmp_path):
    cli = parse_topology_args(["t", "in", "out", "--input-size", "40,36", "--input-resize",
                               "34,33"])
    assert (cli.input_size, cli.input_resize) == ("40,36", "34,33")
    rs = cli.input_resize_plan()
    assert (rs.HS, rs.WS, rs.HR, rs.WR, rs.H, rs.W) == (40, 36, 34, 33, 32, 32) and rs.active
    base = dict(topology_name="t", input_topic="in", output_topic="out")
    env = from_sources(cli=base, env={"GALE_INPUT_SIZE": "30,33", "GALE_INPUT_RESIZE": "29,31",
                                      "GALE_MODEL": "lenet5"})
    rs = env.input_resize_plan()
    assert (rs.HS, rs.WS, rs.HR, rs.WR, rs.H, rs.W) == (30, 33, 29, 31, 28, 28)
    toml = tmp_path / "gale.toml"
    toml.write_text('[gale]\ninput-size = "48,40"\ninput-resize = "36"\n')
    t = from_sources(cli=base, env={}, toml_path=str(toml))
    rs = t.input_resize_plan()
    assert (rs.HS, rs.WS, rs.HR, rs.WR) == (48, 40, 43, 36)  # 36 * 48 // 40 = 43
    # CLI > env > TOML
    both = from_sources(cli=dict(base, input_size="40,36"), env={"GALE_INPUT_SIZE": "30,33",
                                                                "GALE_INPUT_RESIZE": "33,34"},
                        toml_path=str(toml))
    assert (both.input_size, both.input_resize) == ("40,36", "33,34")
    d = cli.engine_dict(32, 32, 3, 10)
    assert (d["rec_H"], d["rec_W"], d["resize_H"], d["resize_W"]) == (40, 36, 34, 33)


def test_single_number_follows_torchvision_resize():
    rs = GaleConfig(topology_name="t", model="resnet50", input_size="375,500",
                    input_resize="256").validate().input_resize_plan()
    assert (rs.HS, rs.WS, rs.HR, rs.WR, rs.H, rs.W) == (375, 500, 256, 341, 224, 224)
    rs = InputResize.build(224, 224, "500,375", "256")
    assert (rs.HR, rs.WR) == (341, 256)
    rs = InputResize.build(224, 224, "256,256", "256")
    assert (rs.HR, rs.WR) == (256, 256)
    # --input-size alone: a plain resize to the model's size
    rs = InputResize.build(32, 32, "40,36", "")
    assert (rs.HS, rs.WS, rs.HR, rs.WR) == (40, 36, 32, 32) and rs.active


@pytest.mark.parametrize("size,resize,name", [
    ("0,36", "", "--input-size"), ("40,4097", "", "--input-size"), ("40", "", "--input-size"),
    ("40,36,3", "", "--input-size"), ("a,b", "", "--input-size"), ("40;36", "", "--input-size"),
    ("-40,36", "", "--input-size"), ("40.5,36", "", "--input-size"),
    ("40,36", "31,33", "--input-resize"), ("40,36", "33,31", "--input-resize"),
    ("40,36", "4097,33", "--input-resize"), ("40,36", "33,0", "--input-resize"),
    ("40,36", "0", "--input-resize"), ("40,36", "4097", "--input-resize"),
    ("40,36", "31", "--input-resize"), ("40,36", "x", "--input-resize"),
    ("40,36", "33,34,35", "--input-resize"), ("1,4096", "32", "--input-resize"),
    ("", "31,31", "--input-resize"),
])
def test_refusals_name_the_option(size, resize, name):
    with pytest.raises(ValueError, match=name):
        GaleConfig(topology_name="t", input_size=size, input_resize=resize).validate()


def test_inactive_when_the_values_equal_the_models():
    base = GaleConfig(topology_name="t").validate()
    assert not base.input_resize_plan().active
    same = GaleConfig(topology_name="t", input_size="32,32", input_resize="32,32").validate()
    assert not same.input_resize_plan().active
    assert same.input_resize_plan().engine_entries() == {}
    d0, d1 = base.engine_dict(32, 32, 3, 10), same.engine_dict(32, 32, 3, 10)
    assert d0 == d1 and "rec_H" not in d0
    s = GaleConfig(topology_name="t", input_resize="32").validate().input_resize_plan()
    assert not s.active
    assert GaleConfig(topology_name="t", input_resize="33").validate().input_resize_plan().active


def test_produce_shape():
    assert produce_shape((32, 32, 3), "") == (32, 32, 3)
    assert produce_shape((32, 32, 3), "40,36") == (40, 36, 3)
    for bad in ("40", "0,3", "4097,3", "a,b"):
        with pytest.raises(ValueError):
            produce_shape((32, 32, 3), bad)


def test_produce_size_writes_source_size_records(capsys):
    """`produce --size 40,36` for both encodings and both layouts, read back from the broker."""
    from gale import cli

    broker = K.Broker()
    broker.start()
    try:
        broker.create_topic("in", 1)
        base = ["produce", "in", "--bootstrap", f"127.0.0.1:{broker.port}", "--size", "40,36",
                "--images", "2", "--images-per-record", "2"]
        for extra in (["--encoding", "b64", "--pixels", "byte"],
                      ["--encoding", "b64", "--pixels", "byte", "--layout", "nchw"],
                      ["--pixels", "byte", "--layout", "nchw"], []):
            assert cli.main(base + extra) == 0
        recs = [json.loads(r["value"])["instances"] for r in broker.read("in", 0)]
    finally:
        broker.stop()
    capsys.readouterr()
    assert [len(base64.b64decode(i["b64"])) for i in recs[0]] == [40 * 36 * 3] * 2
    assert [len(base64.b64decode(i["b64"])) for i in recs[1]] == [40 * 36 * 3] * 2
    assert np.array(recs[2]).shape == (2, 3, 40, 36)
    assert np.array(recs[3]).shape == (2, 40, 36, 3)


# ---- 4. stub engine end to end -----------------------------------------------------------------

CLASSES = 10
MAX_BATCH = 4
COUNTS = [1, 2, 6, 3, 1]  # (6 > max_batch: served as two fragments and joined)


def float_record(x) -> bytes:
    return C.encode_instances(np.ascontiguousarray(x, dtype=np.float32))


def pixel_record(x_u8, fmt, layout) -> bytes:
    v = x_u8.transpose(0, 3, 1, 2) if layout == "nchw" else x_u8
    if fmt == "b64":
        inst = [{"b64": base64.b64encode(np.ascontiguousarray(im).tobytes()).decode()} for im in v]
    else:
        inst = v.tolist()
    return json.dumps({"instances": inst}, separators=(",", ":")).encode()


def run_stub(records, model_hwc, **opts):
    broker = K.Broker()
    broker.start()
    try:
        broker.create_topic("in", 1)
        broker.create_topic("out", 1)
        for key, value in records:
            broker.append("in", 0, [value], [key])
        cfg = GaleConfig(topology_name="t", input_topic="in", output_topic="out",
                         bootstrap=f"127.0.0.1:{broker.port}", start_offset="earliest", stub=True,
                         max_batch=MAX_BATCH, max_wait_us=500, output_key="input",
                         on_error="null", **opts).validate()
        d = cfg.engine_dict(*model_hwc, CLASSES)
        d["max_records"] = len(records)
        eng = C.Engine(d)
        eng.add_stub_replica(MAX_BATCH, 0, True, -1)
        eng.start()
        assert eng.wait(30000), eng.stats()
        eng.stop()
        stats = dict(eng.stats())
        out = broker.read("out", 0)
    finally:
        broker.stop()
    return {r["key"]: r["value"] for r in out}, stats


@pytest.fixture(scope="module")
def stub_case():
    """Pixels at 40x36, and what the engine gives for apply(prep(x)) as float text, no options."""
    rng = np.random.default_rng(17)
    xs = {f"r{i}".encode(): rng.integers(0, 256, (n, 40, 36, 3), dtype=np.uint8)
          for i, n in enumerate(COUNTS)}
    prep = InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S)
    rs = InputResize(40, 36, 34, 33, 32, 32)
    recs = [(k, float_record(rs.apply(prep.apply(x.astype(np.float32))))) for k, x in xs.items()]
    recs.insert(2, (b"bad", b'{"instances": [[[1, 2'))
    want, stats = run_stub(recs, (32, 32, 3))
    assert stats["resized_images"] == 0
    assert want[b"bad"] is None and all(want[k] is not None for k in xs)
    return xs, want


@pytest.mark.parametrize("fmt", ["json", "b64"])
@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
def test_stub_engine_resizes_source_size_records(stub_case, fmt, layout):
    xs, want = stub_case
    recs = [(k, pixel_record(x, fmt, layout)) for k, x in xs.items()]
    recs.insert(2, (b"bad", b'{"instances": [[[1, 2'))
    got, stats = run_stub(recs, (32, 32, 3), input_size="40,36", input_resize="34,33",
                          input_scale=1 / 255, input_mean=CIFAR_MEAN_S, input_std=CIFAR_STD_S,
                          input_format=fmt, input_layout=layout)
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], k
    assert stats["resized_images"] == sum(COUNTS)
    assert json.loads(got[b"r2"])["predictions"].__len__() == 6


# ---- 5. stand-alone sanitizer run ---------------------------------------------------------------

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None,
                    reason="needs ROCm clang++ and make")
def test_resize_under_address_and_ub_sanitizers():
    target = "build/asan/resize_check"
    b = subprocess.run(["make", "-C", ROOT, target], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, target)], capture_output=True, text=True, timeout=300,
                       env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "resize_check OK" in out
