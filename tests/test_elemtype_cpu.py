"""Typed tensor records (--input-dtype u16 | f16 | bf16 | f32) without a GPU: the numpy oracle
(gale.models.preprocess.ElemType) against struct / numpy conversions on every 16-bit pattern and
on f32 patterns, the configuration rules, the host parser against the oracle with every verdict,
a stub engine against the same values sent as JSON numbers, and the stand-alone sanitizer driver
(csrc/tests/elemtype_check.cpp). Every float comparison is on the bits."""

import base64
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from gale._native import native
from gale.cli import parse_topology_args
from gale.config import GaleConfig, from_sources
from gale.data import encode_records_text, encode_records_typed
from gale.models.preprocess import ELEM_TYPES, ElemType, InputPrep

C = native()
K = C.kafka
OK, BAD_SHAPE, BAD_NUMBER = 0, 3, 5
TYPED = ("u16", "f16", "bf16", "f32")
CIFAR_MEAN_S = "0.4914,0.4822,0.4465"
CIFAR_STD_S = "0.2470,0.2435,0.2616"
SHAPES = [(1, 1, 1), (1, 2, 1), (5, 7, 1), (5, 7, 3)]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def all_u16_patterns(dtype):
    """The 65 536 patterns as wire bytes [65536 * 2], the non-finite ones replaced with 0."""
    p = np.arange(65536, dtype="<u2")
    e = ElemType(dtype)
    p[e.nonfinite(p.view(np.uint8))] = 0
    return p.view(np.uint8)


def f32_patterns(n=100_000, seed=3):
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype("<u4")
    p[(p & 0x7F800000) == 0x7F800000] &= 0xBFFFFFFF          # finite
    special = [0x80000000, 0x00000001, 0x7F7FFFFF]          # -0, least subnormal, largest finite
    p[:3] = special[:len(p[:3])]
    return p.view(np.uint8)


# ---- 1. the numpy oracle ------------------------------------------------------------------------

def test_oracle_on_every_16_bit_pattern():
    pats = np.arange(65536)
    u = ElemType("u16").to_float(all_u16_patterns("u16"))
    assert np.array_equal(bits(u), bits(pats.astype(np.float32)))
    h = all_u16_patterns("f16")
    want = np.array([struct.unpack("<e", h[2 * i:2 * i + 2].tobytes())[0] for i in pats],
                    dtype=np.float64)
    got = ElemType("f16").to_float(h)
    assert np.array_equal(bits(got), bits(want.astype(np.float32)))
    assert np.isfinite(got).all() and (got[1:0x400] > 0).all()          # (subnormals are kept)
    b = all_u16_patterns("bf16")
    want = np.array([struct.unpack("<f", b"\0\0" + b[2 * i:2 * i + 2].tobytes())[0]
                     for i in pats], dtype=np.float32)
    assert np.array_equal(bits(ElemType("bf16").to_float(b)), bits(want))
    # what was replaced: exactly the all-ones exponents
    for t, mask in (("f16", 0x7C00), ("bf16", 0x7F80)):
        nf = ElemType(t).nonfinite(np.arange(65536, dtype="<u2").view(np.uint8))
        assert np.array_equal(nf, (pats & mask) == mask)
    assert not ElemType("u16").nonfinite(np.arange(65536, dtype="<u2").view(np.uint8)).any()


def test_oracle_on_f32_patterns():
    p = f32_patterns()
    got = ElemType("f32").to_float(p)
    assert np.array_equal(bits(got), p.view("<u4"))
    assert np.isfinite(got).all() and np.signbit(got[0]) and got[0] == 0 and 0 < got[1] < 1e-44
    assert got[2] == np.finfo(np.float32).max
    # the identity prep leaves the bits alone; a prep is InputPrep.apply of the exact values
    x = p[:4 * 105]
    assert np.array_equal(bits(ElemType("f32").apply(x, 5, 7, 3)).ravel(), x.view("<u4"))
    prep = InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S)
    y = ElemType("f32").apply(x, 5, 7, 3, prep)
    assert np.array_equal(bits(y), bits(prep.apply(x.view("<f4").reshape(5, 7, 3))))


def test_oracle_layout_and_wire():
    rng = np.random.default_rng(4)
    x = rng.integers(0, 256, (2, 5, 7, 3)).astype(np.float32)
    for t in TYPED:
        e = ElemType(t)
        assert e.bytes_per_element == ELEM_TYPES[t][0] == C.elem_bytes(t)
        wire = e.to_wire(x).reshape(2, -1)
        assert wire.shape[1] == e.frame_bytes(5, 7, 3)
        assert np.array_equal(e.apply(wire, 5, 7, 3), x)     # (0..255 is exact in every type)
        nchw = InputPrep.build(3, 0.5, layout="nchw")
        wire_t = e.to_wire(x.transpose(0, 3, 1, 2)).reshape(2, -1)
        assert np.array_equal(e.apply(wire_t, 5, 7, 3, nchw), x * 0.5)
    # rounding to the type: nearest even
    assert ElemType("bf16").to_wire(np.float32(1.00390625)).view("<u2")[0] == 0x3F80
    assert ElemType("bf16").to_wire(np.float32(1.01171875)).view("<u2")[0] == 0x3F82
    assert ElemType("u16").to_wire(np.float32(70000.0)).view("<u2")[0] == 65535
    with pytest.raises(ValueError, match="input_dtype"):
        ElemType("f64")
    with pytest.raises(ValueError):
        ElemType("f16").apply(np.zeros(7, np.uint8), 1, 2, 2)


# ---- 2. configuration ---------------------------------------------------------------------------

def test_refusals_name_the_option():
    base = dict(topology_name="t", input_format="b64")
    for t in TYPED:
        assert GaleConfig(input_dtype=t, **base).validate().input_elem() == ElemType(t)
        with pytest.raises(ValueError, match=f"--input-dtype {t} needs --input-format b64"):
            GaleConfig(topology_name="t", input_dtype=t).validate()
        for pf in ("i420", "nv12", "bgr24", "rgba", "bgra", "gray"):
            with pytest.raises(ValueError, match=f"--input-dtype {t}.*--input-pixel-format rgb"):
                GaleConfig(input_dtype=t, input_pixel_format=pf, **base).validate()
        # nchw, any channel count and a record-side size are the rgb rules
        GaleConfig(input_dtype=t, input_layout="nchw", input_scale=0.5, **base).validate()
        GaleConfig(input_dtype=t, model="lenet5", input_mean="0.1307", input_std="0.3081",
                   **base).validate()
        GaleConfig(input_dtype=t, input_size="40,36", **base).validate()
    with pytest.raises(ValueError, match="input_dtype"):
        GaleConfig(input_dtype="f64", **base).validate()
    with pytest.raises(SystemExit):
        parse_topology_args(["t", "in", "out", "--input-format", "b64", "--input-dtype", "half"])
    assert GaleConfig(topology_name="t").validate().input_elem() is None
    # the existing rule for per-channel coefficients with C > 4, by its option
    with pytest.raises(ValueError, match="input_mean.*C <= 4"):
        InputPrep.build(5, 1.0, "1,2,3,4,5", "")


def test_native_engine_refuses_the_same_combinations():
    d = GaleConfig(topology_name="t", input_topic="in", output_topic="out",
                   input_format="b64").validate().engine_dict(4, 3, 3, 10)
    C.Engine(dict(d, input_dtype="f16"))
    C.Engine(dict(d, input_dtype="u8"))
    with pytest.raises(ValueError, match="input_dtype: u8, u16, f16, bf16 or f32"):
        C.Engine(dict(d, input_dtype="f64"))
    with pytest.raises(ValueError, match="input_dtype f16 needs input_format b64"):
        C.Engine(dict(d, input_dtype="f16", input_format="json"))
    for pf in ("i420", "bgra"):
        with pytest.raises(ValueError, match="input_dtype bf16 needs pixel_format rgb"):
            C.Engine(dict(d, input_dtype="bf16", pixel_format=pf))
    d5 = dict(d, C=5, input_dtype="f32")
    C.Engine(dict(d5, input_a=[0.5] * 4, input_b=[1.0] * 4))
    with pytest.raises(ValueError, match="input_dtype f32.*C <= 4"):
        C.Engine(dict(d5, input_a=[0.5, 0.5, 0.5, 0.25], input_b=[0.0] * 4))


def test_precedence(tmp_path):
    cli = parse_topology_args(["t", "in", "out", "--input-format", "b64", "--input-dtype", "f16"])
    env = from_sources(cli=dict(topology_name="t", input_format="b64"),
                       env={"GALE_INPUT_DTYPE": "f16"})
    toml = tmp_path / "g.toml"
    toml.write_text('[gale]\ninput-format = "b64"\ninput-dtype = "f16"\n')
    tom = from_sources(cli=dict(topology_name="t"), env={}, toml_path=str(toml))
    for cfg in (cli, env, tom):
        assert cfg.input_dtype == "f16"
        assert cfg.engine_dict(32, 32, 3, 10)["input_dtype"] == "f16"
    over_toml = from_sources(cli=dict(topology_name="t"), env={"GALE_INPUT_DTYPE": "bf16"},
                             toml_path=str(toml))
    assert over_toml.input_dtype == "bf16"
    over_env = from_sources(cli=dict(topology_name="t", input_dtype="f32"),
                            env={"GALE_INPUT_DTYPE": "bf16"}, toml_path=str(toml))
    assert over_env.input_dtype == "f32"


def test_engine_dict_gains_the_key_only_off_the_default():
    for kw in (dict(), dict(input_format="b64"),
               dict(input_format="b64", input_pixel_format="bgra")):
        plain = GaleConfig(topology_name="t", **kw).validate().engine_dict(32, 32, 3, 10)
        u8 = GaleConfig(topology_name="t", input_dtype="u8", **kw).validate() \
            .engine_dict(32, 32, 3, 10)
        assert "input_dtype" not in plain and u8 == plain
    b = GaleConfig(topology_name="t", input_format="b64").validate().engine_dict(32, 32, 3, 10)
    for t in TYPED:
        d = GaleConfig(topology_name="t", input_format="b64", input_dtype=t).validate() \
            .engine_dict(32, 32, 3, 10)
        assert d == dict(b, input_dtype=t)


# ---- 3. the host parser -------------------------------------------------------------------------

def wire_images(t, shape, n, seed):
    """n random finite images of the type, wire bytes uint8 [n, B]."""
    H, W, CH = shape
    per = H * W * CH
    if t == "f32":
        return f32_patterns(n * per, seed).reshape(n, -1).copy()
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, 65536, n * per)
    return all_u16_patterns(t).reshape(-1, 2)[idx].reshape(n, -1).copy()


def record(wire):
    return b'{"instances":[' + b",".join(b'{"b64":"' + base64.b64encode(w.tobytes()) + b'"}'
                                         for w in wire) + b"]}"


@pytest.mark.parametrize("t", TYPED)
@pytest.mark.parametrize("shape", SHAPES)
def test_host_parser_equals_the_oracle(shape, t):
    H, W, CH = shape
    e = ElemType(t)
    B = e.frame_bytes(H, W, CH)
    wire = wire_images(t, shape, 3, 11)
    rec = record(wire)
    pad = (3 - B % 3) % 3
    assert rec.count(b"=") == 3 * pad
    st, got = C.parse_instances_typed_host(rec, H, W, CH, t)
    assert st == OK and got.shape == (3, H * W * CH)
    assert np.array_equal(bits(got), bits(e.to_float(wire)))
    assert np.array_equal(bits(got.reshape(3, H, W, CH)), bits(e.apply(wire, H, W, CH)))
    assert C.parse_instances_typed_host(rec, H, W, CH, t, max_images=2)[0] == 7   # too_large
    assert C.parse_instances_typed_host(record(wire[:1]), H + 2, W, CH, t)[0] == BAD_SHAPE
    assert C.parse_instances_typed_host(rec, H, W, CH, "f64")[0] == BAD_SHAPE
    one, fin = C.typed_to_float_host(wire[0].tobytes(), t)
    assert fin and np.array_equal(bits(one), bits(got[0]))


def test_the_shapes_give_both_paddings():
    pads = {E: {(3 - h * w * c * E % 3) % 3 for h, w, c in SHAPES} for E in (2, 4)}
    assert pads == {2: {0, 1, 2}, 4: {0, 1, 2}}


def plant(s: bytes, at: int, what: bytes) -> bytes:
    return s[:at] + what + s[at + len(what):]


NONFINITE = {"f16": (0x7C00, 0xFC00, 0x7E00, 0x7C01), "bf16": (0x7F80, 0xFF80, 0x7FC0, 0x7F81),
             "f32": (0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001)}   # +Inf -Inf qNaN NaN(bit 0)


@pytest.mark.parametrize("t", TYPED)
@pytest.mark.parametrize("shape", SHAPES)
def test_host_parser_verdicts(shape, t):
    H, W, CH = shape
    e = ElemType(t)
    E, per = e.bytes_per_element, H * W * CH
    wire = wire_images(t, shape, 2, 12)
    good = record(wire)
    q = good.index(b'"b64":"') + 7
    L = 4 * ((per * E + 2) // 3)
    pad = (3 - per * E % 3) % 3
    for at in (0, L - pad - 1):
        assert C.parse_instances_typed_host(plant(good, q + at, b"-"), H, W, CH, t)[0] == BAD_NUMBER
    if pad:
        for k in range(pad):
            assert C.parse_instances_typed_host(plant(good, q + L - 1 - k, b"A"), H, W, CH,
                                                t)[0] == BAD_NUMBER
    assert C.parse_instances_typed_host(plant(good, q + L - pad - 1, b"="), H, W, CH,
                                        t)[0] == BAD_NUMBER
    for pattern in NONFINITE.get(t, ()):
        for img in (0, 1):
            for el in (0, per - 1):
                w = wire.copy()
                w[img, el * E:(el + 1) * E] = np.frombuffer(
                    int(pattern).to_bytes(E, "little"), np.uint8)
                assert e.nonfinite(w).sum() == 1
                st, out = C.parse_instances_typed_host(record(w), H, W, CH, t)
                assert st == BAD_NUMBER and out.shape[0] == 0, (hex(pattern), img, el)
                assert not C.typed_to_float_host(w[img].tobytes(), t)[1]
    if t == "u16":      # every pattern is a number
        w = wire.copy()
        w[:] = 0xFF
        assert C.parse_instances_typed_host(record(w), H, W, CH, t)[0] == OK


# ---- 4. stub engine end to end ------------------------------------------------------------------

def serve_stub(recs, H, W, CH, **kw):
    """key -> output value of a stub topology fed (key, record) pairs; and its stats."""
    broker = K.Broker()
    broker.start()
    try:
        broker.create_topic("in", 1)
        broker.create_topic("out", 1)
        for key, rec in recs:
            broker.append("in", 0, [rec], [key])
        cfg = GaleConfig(topology_name="t", input_topic="in", output_topic="out",
                         bootstrap=f"127.0.0.1:{broker.port}", start_offset="earliest",
                         stub=True, max_batch=4, max_wait_us=500, output_key="input",
                         **kw).validate()
        d = cfg.engine_dict(H, W, CH, 10)
        d["max_records"] = len(recs)
        eng = C.Engine(d)
        eng.add_stub_replica(4, 0, True, -1)
        eng.start()
        assert eng.wait(30000), eng.stats()
        eng.stop()
        st = eng.stats()
        out = broker.read("out", 0)
    finally:
        broker.stop()
    assert len(out) == len(recs)
    return {r["key"]: r["value"] for r in out}, st


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
def test_stub_engine_f16_equals_json_numbers(layout):
    H, W, CH = 4, 3, 3
    rng = np.random.default_rng(8)
    prep = dict(input_scale=1 / 255, input_mean=CIFAR_MEAN_S, input_std=CIFAR_STD_S,
                input_layout=layout)
    xs = {}
    for i, n in enumerate([1, 2, 3, 9, 1]):                  # 9 > max_batch 4: fragments
        # f16 values with fractions and subnormals, exact in float32 and in JSON text
        x = (rng.integers(0, 2048, (n, H, W, CH)) / 8).astype(np.float16).astype(np.float32)
        x[0, 0, 0, 0] = 2.0 ** -24
        xs[f"r{i}".encode()] = x
    text = [(k, encode_records_text(x, x.shape[0], layout)[0]) for k, x in xs.items()]
    typed = [(k, encode_records_typed(x, "f16", x.shape[0], layout)[0]) for k, x in xs.items()]
    assert sum(len(r) for _, r in typed) < sum(len(r) for _, r in text)
    want, wst = serve_stub(text, H, W, CH, on_error="error-json", **prep)
    w = ElemType("f16").to_wire(xs[b"r2"] if layout == "nhwc"
                                else xs[b"r2"].transpose(0, 3, 1, 2)).reshape(3, -1).copy()
    w[2, -2:] = (0x00, 0x7C)                                 # +Inf, the last element
    typed += [(b"inf", record(w)), (b"badchar", plant(typed[1][1], 30, b"-"))]
    got, st = serve_stub(typed, H, W, CH, on_error="error-json", input_format="b64",
                         input_dtype="f16", **prep)
    inf, badchar = got.pop(b"inf"), got.pop(b"badchar")
    assert got == want and all(b"predictions" in v for v in want.values())  # byte for byte
    assert b"bad_number" in inf and b"error" in inf and b"bad_number" in badchar
    assert wst["typed_records"] == 0 and wst["errors"] == 0
    assert st["typed_records"] == st["b64_records"] == len(xs) + 2 and st["errors"] == 2
    assert st["split_records"] == 1 and st["packed_records"] == 0 == st["yuv_records"]


# ---- 5. stand-alone sanitizer run ---------------------------------------------------------------

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None,
                    reason="needs ROCm clang++ and make")
def test_elemtype_under_address_and_ub_sanitizers():
    target = "build/asan/elemtype_check"
    b = subprocess.run(["make", "-C", ROOT, target], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, target)], capture_output=True, text=True, timeout=300,
                       env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "elemtype_check OK" in out
