"""YUV 4:2:0 frame records (--input-pixel-format i420 | nv12) on the host: the integer
definition (coefficients, accumulator range, distance from the real-valued matrix), the host twin
against the numpy oracle, the b64 verdict table with L = 4 B / 3, the splitter, the configuration
refusals and sources, the stub engine end to end against RGB records of the oracle's images, and
the stand-alone sanitizer program. Every comparison is bit-exact."""

import base64
import itertools
import json
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from gale._native import native
from gale.cli import cmd_produce, parse_topology_args
from gale.config import GaleConfig, from_sources
from gale.data import encode_records_b64, encode_records_yuv, pack_yuv420, synthetic_yuv_planes
from gale.models.preprocess import InputPrep, InputResize, YuvConvert

C = native()
K = C.kafka
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TABLES = [(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]
FORMATS = ("i420", "nv12")
# chroma planes starting at byte phase 1, 2 and 0 modulo 3, an odd chroma width, one CIFAR frame
SIZES = [(2, 2), (2, 4), (4, 6), (6, 10), (32, 32)]
EDGE = (0, 16, 128, 235, 240, 255)
CIFAR_MEAN_S = "0.4914,0.4822,0.4465"
CIFAR_STD_S = "0.2470,0.2435,0.2616"

# the issue's table, copied by hand: the literals of csrc/codec/yuv.h must equal it
LITERALS = {
    ("bt601", "limited"): (1220945, 1673555, -410793, -852458, 2115221),
    ("bt601", "full"): (1048576, 1470104, -360853, -748826, 1858077),
    ("bt709", "limited"): (1220945, 1879825, -223607, -558796, 2215014),
    ("bt709", "full"): (1048576, 1651297, -196424, -490864, 1945738),
}


def kcoeffs(yc):
    return [*yc.coeffs(), yc.yo]


# ---- 1. the definition --------------------------------------------------------------------------

def half_even(q: Fraction) -> int:
    fl = q.numerator // q.denominator
    rem = q - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2):
        return fl + 1
    return fl


def rationals(matrix, range_):
    """Written out again here, from the issue's formulas."""
    kr, kb = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)),
              "bt709": (Fraction(2126, 10000), Fraction(722, 10000))}[matrix]
    kg = 1 - kr - kb
    sy, sc = (Fraction(255, 219), Fraction(255, 224)) if range_ == "limited" else (1, 1)
    return (Fraction(sy), 2 * (1 - kr) * sc, -2 * kb * (1 - kb) / kg * sc,
            -2 * kr * (1 - kr) / kg * sc, 2 * (1 - kb) * sc)


@pytest.mark.parametrize("matrix,range_", TABLES)
def test_twenty_literals_are_the_rounded_fractions(matrix, range_):
    want = tuple(half_even(q * 2 ** 20) for q in rationals(matrix, range_))
    assert want == LITERALS[(matrix, range_)]
    yo = 16 if range_ == "limited" else 0
    assert tuple(C.yuv_coeffs(matrix, range_)) == want + (yo,)       # the C++ literals
    yc = YuvConvert("i420", matrix, range_)
    assert yc.coeffs() == want and yc.yo == yo                       # the Python definition
    with pytest.raises(ValueError):
        C.yuv_coeffs("bt2020", range_)


@pytest.mark.parametrize("matrix,range_", TABLES)
def test_all_triples_accumulator_and_distance(matrix, range_):
    """All 2^24 (Y, U, V): |accumulator| < 2^31 (rounding term included) and the unclamped
    result within 0.5 + 3 * 255 * 2^-21 of the real-valued matrix."""
    yc = YuvConvert("i420", matrix, range_)
    sy, crv, cgu, cgv, cbu = (float(q) for q in rationals(matrix, range_))
    bound = 0.5 + 3 * 255 * 2.0 ** -21
    U, V = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    u, v = U - 128.0, V - 128.0
    worst_acc, worst_d = 0, 0.0
    for Y in range(256):
        acc = yc.accumulators(np.full_like(U, Y), U, V)
        worst_acc = max(worst_acc, *(int(np.abs(a).max()) for a in acc))
        yy = sy * (Y - yc.yo)
        real = (yy + crv * v, yy + cgu * u + cgv * v, yy + cbu * u)
        for a, r in zip(acc, real):
            worst_d = max(worst_d, float(np.abs((a >> 20) - r).max()))
    print(f"\n{matrix} {range_}: max |acc| {worst_acc}, max distance {worst_d:.6f}")
    assert worst_acc < 2 ** 31
    assert worst_acc <= 573636921       # the issue's figure is the maximum over the four tables
    assert worst_d <= bound


# ---- 2. the host twin against the oracle --------------------------------------------------------

def forced_planes(HS, WS, rng):
    """Frames whose pixels run through every (Y, U, V) of EDGE^3 (both clamps fire), at every
    position of the 2x2 block in turn; random elsewhere."""
    triples = list(itertools.product(EDGE, repeat=3))
    n = -(-len(triples) * 4 // (HS * WS)) + 1
    Y = rng.integers(0, 256, (n, HS, WS), dtype=np.uint8)
    U = rng.integers(0, 256, (n, HS // 2, WS // 2), dtype=np.uint8)
    V = rng.integers(0, 256, (n, HS // 2, WS // 2), dtype=np.uint8)
    blocks = [(i, by, bx) for i in range(n) for by in range(HS // 2) for bx in range(WS // 2)]
    for (y, u, v), (i, by, bx) in zip(triples, blocks):
        Y[i, 2 * by:2 * by + 2, 2 * bx:2 * bx + 2] = y
        U[i, by, bx], V[i, by, bx] = u, v
    assert len(blocks) >= len(triples)
    return Y, U, V


def planes_for(HS, WS, seed):
    rng = np.random.default_rng(seed)
    Y, U, V = synthetic_yuv_planes(3, HS, WS, seed)
    fy, fu, fv = forced_planes(HS, WS, rng)
    return np.concatenate([Y, fy]), np.concatenate([U, fu]), np.concatenate([V, fv])


def test_forced_triples_fire_both_clamps():
    yc = YuvConvert("i420")
    acc = yc.accumulators(*np.meshgrid(EDGE, EDGE, EDGE, indexing="ij"))
    res = np.stack(acc) >> 20
    assert (res < 0).any() and (res > 255).any()


@pytest.mark.parametrize("HS,WS", SIZES)
def test_host_twin_equals_the_oracle(HS, WS):
    Y, U, V = planes_for(HS, WS, 100 + HS * WS)
    prep = InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S)
    a, b = prep.coeffs()
    for (matrix, range_), fmt in itertools.product(TABLES, FORMATS):
        yc = YuvConvert(fmt, matrix, range_)
        frames = pack_yuv420(Y, U, V, fmt)
        assert frames.shape[1] == YuvConvert.frame_bytes(HS, WS)
        want = yc.apply(frames, HS, WS)
        # the oracle is the per-pixel formula, written out on a sample
        cy, crv, cgu, cgv, cbu = yc.coeffs()
        for (i, y, x) in [(0, 0, 0), (1, HS - 1, WS - 1), (2, HS // 2, 1)]:
            yy = cy * (int(Y[i, y, x]) - yc.yo) + (1 << 19)
            u, v = int(U[i, y >> 1, x >> 1]) - 128, int(V[i, y >> 1, x >> 1]) - 128
            px = [yy + crv * v, yy + cgu * u + cgv * v, yy + cbu * u]
            assert list(want[i, y, x]) == [min(max(p >> 20, 0), 255) for p in px]
        for i, fr in enumerate(frames):
            rgb, f32 = C.yuv420_to_rgb_host(fr.tobytes(), HS, WS, fmt, kcoeffs(yc))
            assert np.array_equal(rgb, want[i]), (HS, WS, fmt, matrix, range_, i)
            assert np.array_equal(f32, want[i].astype(np.float32))
            _, f32p = C.yuv420_to_rgb_host(fr.tobytes(), HS, WS, fmt, kcoeffs(yc), a=a, b=b)
            assert np.array_equal(f32p.view(np.uint32),
                                  prep.apply(want[i].astype(np.float32)).view(np.uint32))


@pytest.mark.parametrize("HS,WS", SIZES)
def test_i420_and_nv12_records_decode_identically(HS, WS):
    Y, U, V = planes_for(HS, WS, 7)
    outs = {}
    for fmt in FORMATS:
        yc = YuvConvert(fmt, "bt709", "full")
        rec = encode_records_yuv(Y, U, V, fmt, Y.shape[0])[0]
        st, out = C.parse_instances_yuv_host(rec, HS, WS, fmt, kcoeffs(yc))
        assert st == 0 and out.shape == (Y.shape[0], HS, WS, 3)
        assert np.array_equal(out, yc.apply(pack_yuv420(Y, U, V, fmt), HS, WS).astype(np.float32))
        outs[fmt] = out
    assert np.array_equal(outs["i420"].view(np.uint32), outs["nv12"].view(np.uint32))
    # ... and equal the RGB decoder's output for the oracle's image sent as an RGB record
    rgb = YuvConvert("i420", "bt709", "full").apply(pack_yuv420(Y, U, V, "i420"), HS, WS)
    st, out = C.parse_instances_b64_host(encode_records_b64(rgb, rgb.shape[0])[0], HS, WS, 3)
    assert st == 0 and np.array_equal(out.view(np.uint32), outs["i420"].view(np.uint32))


# ---- 3. the verdict table with L = 4 B / 3, the splitter ----------------------------------------

OK, BAD_ENVELOPE, UNKNOWN_KEY, BAD_SHAPE, EMPTY, BAD_NUMBER, NULL_INSTANCES, TOO_LARGE = \
    0, 1, 2, 3, 4, 5, 6, 7


def rec_of(*elems: str) -> bytes:
    return ('{"instances":[' + ",".join(elems) + "]}").encode()


@pytest.mark.parametrize("fmt", FORMATS)
def test_verdict_table(fmt):
    HS, WS = 4, 6
    B = YuvConvert.frame_bytes(HS, WS)
    L = 4 * B // 3
    assert B == 36 and L == 48
    yc = YuvConvert(fmt)
    Y, U, V = synthetic_yuv_planes(2, HS, WS, 3)
    s = [base64.b64encode(f.tobytes()).decode() for f in pack_yuv420(Y, U, V, fmt)]
    assert all(len(x) == L and "=" not in x for x in s)

    def both(rec):
        scan = C.scan_instances_b64_bytes(rec, B)[0]
        full = C.parse_instances_yuv_host(rec, HS, WS, fmt, kcoeffs(yc))[0]
        return scan, full

    el = lambda x: '{"b64":"%s"}' % x  # noqa: E731
    assert both(rec_of(el(s[0]), el(s[1]))) == (OK, OK)
    assert C.scan_instances_b64_bytes(rec_of(el(s[0]), el(s[1])), B)[3] == 2
    assert both(rec_of(el(s[0][:-1]))) == (BAD_SHAPE, BAD_SHAPE)            # one short
    assert both(rec_of(el(s[0] + "A"))) == (BAD_SHAPE, BAD_SHAPE)           # one long
    assert both(rec_of('{"b64":7}')) == (BAD_SHAPE, BAD_SHAPE)              # not a string
    assert both(rec_of('{"b64":[1]}')) == (BAD_SHAPE, BAD_SHAPE)
    assert both(rec_of('{"b64":"%s","k":1}' % s[0])) == (UNKNOWN_KEY, UNKNOWN_KEY)  # second key
    assert both(rec_of('{"b65":"%s"}' % s[0])) == (UNKNOWN_KEY, UNKNOWN_KEY)
    assert both(rec_of()) == (EMPTY, EMPTY)
    assert both(b'{"instances":null}') == (NULL_INSTANCES, NULL_INSTANCES)
    assert both(rec_of(el(s[0]))[:-1]) == (BAD_ENVELOPE, BAD_ENVELOPE)
    # the characters are the decoder's: '=' anywhere (there is no padding), any other outsider
    for at in (0, 17, L - 1):
        for ch in "=-_ \\":
            bad = s[1][:at] + ch + s[1][at + 1:]
            assert both(rec_of(el(s[0]), el(bad))) == (OK, BAD_NUMBER), (at, ch)
    assert C.parse_instances_yuv_host(rec_of(el(s[0]), el(s[1])), HS, WS, fmt, kcoeffs(yc),
                                      max_images=1)[0] == TOO_LARGE
    # an RGB-size string is the wrong length for a frame, and the other way round
    rgb = base64.b64encode(bytes(HS * WS * 3)).decode()
    assert both(rec_of(el(rgb))) == (BAD_SHAPE, BAD_SHAPE)
    assert C.scan_instances_b64(rec_of(el(s[0])), HS, WS, 3)[0] == BAD_SHAPE
    # the (H, W, C) forms are the byte-count forms of H*W*C
    r = rec_of(el(s[0]), el(s[1]))
    assert C.scan_instances_b64(r, HS // 2, WS, 3) == C.scan_instances_b64_bytes(r, B)
    assert C.scan_instances_b64_bytes(r, 0)[0] == BAD_SHAPE


def test_splitter_yields_byte_identical_fragments():
    HS, WS = 6, 10
    B = YuvConvert.frame_bytes(HS, WS)
    Y, U, V = synthetic_yuv_planes(5, HS, WS, 9)
    rec = encode_records_yuv(Y, U, V, "nv12", 5)[0]
    _, off, ln, n = C.scan_instances_b64_bytes(rec, B)
    arr = rec[off:off + ln]
    spans = C.split_instances_b64_bytes(arr, B)
    offs = C.b64_image_offsets_bytes(arr, B)
    singles = encode_records_yuv(Y, U, V, "nv12", 1)
    assert n == 5 and len(spans) == 5 and len(offs) == 5
    for i, (b, e) in enumerate(spans):
        assert b'{"instances":[' + arr[b:e] + b"]}" == singles[i]
        assert arr[offs[i]:offs[i] + 4 * B // 3] == base64.b64encode(
            pack_yuv420(Y, U, V, "nv12")[i].tobytes())
    assert C.split_instances_b64_bytes(arr, B + 3) is None
    assert C.split_instances_b64(arr, HS // 2, WS, 3) == spans


# ---- 4. configuration ---------------------------------------------------------------------------

def cfg(**kw):
    return GaleConfig(topology_name="t", **kw).validate()


def test_refusals_name_their_option():
    ok = dict(input_format="b64", input_pixel_format="i420")
    cfg(**ok)
    cfg(**dict(ok, input_pixel_format="nv12", input_yuv_matrix="bt709", input_yuv_range="full"))
    with pytest.raises(ValueError, match="--input-format b64"):
        cfg(input_pixel_format="i420")
    with pytest.raises(ValueError, match="--input-layout nchw"):
        cfg(**ok, input_layout="nchw")
    with pytest.raises(ValueError, match="--input-pixel-format nv12.*C = 1"):
        cfg(input_format="b64", input_pixel_format="nv12", model="lenet5")
    with pytest.raises(ValueError, match="--input-size.*even"):
        cfg(**ok, input_size="33,32")
    with pytest.raises(ValueError, match="--input-size.*even"):
        cfg(**ok, input_size="40,35", input_resize="34,33")
    with pytest.raises(ValueError, match="--input-yuv-matrix"):
        cfg(input_yuv_matrix="bt709")
    with pytest.raises(ValueError, match="--input-yuv-range"):
        cfg(input_format="b64", input_yuv_range="full")
    with pytest.raises(ValueError, match="input_pixel_format"):
        cfg(input_format="b64", input_pixel_format="yuyv")
    with pytest.raises(ValueError, match="input_yuv_matrix"):
        cfg(**ok, input_yuv_matrix="bt2020")
    # the native engine refuses the same combinations (a dict built by hand)
    d = cfg(**ok, input_topic="in", output_topic="out").engine_dict(32, 32, 3, 10)
    assert (d["pixel_format"], d["yuv_matrix"], d["yuv_range"]) == ("i420", "bt601", "limited")
    C.Engine(d)
    for bad in (dict(input_format="json"), dict(input_nchw=True), dict(C=1), dict(rec_H=33, rec_W=32),
                dict(pixel_format="yuyv"), dict(yuv_matrix="bt2020")):
        with pytest.raises(ValueError, match="pixel_format|yuv_matrix"):
            C.Engine(dict(d, **bad))
    # rgb: nothing new reaches the engine
    assert "pixel_format" not in cfg(input_format="b64").engine_dict(32, 32, 3, 10)


def test_three_sources_and_their_precedence(tmp_path):
    toml = tmp_path / "g.toml"
    toml.write_text('[gale]\ninput-format = "b64"\ninput-pixel-format = "i420"\n'
                    'input-yuv-matrix = "bt709"\ninput-yuv-range = "full"\n')
    c = from_sources(cli=dict(topology_name="t"), env={}, toml_path=str(toml))
    assert (c.input_pixel_format, c.input_yuv_matrix, c.input_yuv_range) == \
        ("i420", "bt709", "full")
    env = {"GALE_INPUT_PIXEL_FORMAT": "nv12", "GALE_INPUT_YUV_RANGE": "limited"}
    c = from_sources(cli=dict(topology_name="t"), env=env, toml_path=str(toml))
    assert (c.input_pixel_format, c.input_yuv_matrix, c.input_yuv_range) == \
        ("nv12", "bt709", "limited")
    c = from_sources(cli=dict(topology_name="t", input_pixel_format="i420",
                              input_yuv_matrix="bt601"), env=env, toml_path=str(toml))
    assert (c.input_pixel_format, c.input_yuv_matrix, c.input_yuv_range) == \
        ("i420", "bt601", "limited")
    yc = c.input_yuv()
    assert (yc.format, yc.matrix, yc.range) == ("i420", "bt601", "limited")
    c = parse_topology_args(["t", "in", "out", "--input-format", "b64", "--input-pixel-format",
                             "nv12", "--input-yuv-range", "full"])
    assert c.input_yuv() == YuvConvert("nv12", "bt601", "full")
    assert cfg().input_yuv() is None
    with pytest.raises(SystemExit):
        parse_topology_args(["t", "in", "out", "--input-pixel-format", "bgr"])


def test_produce_pixel_format_needs_b64(capsys):
    with pytest.raises(SystemExit) as e:
        cmd_produce(["topic", "--pixel-format", "i420"])
    assert e.value.code == 2 and "--encoding b64" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cmd_produce(["topic", "--pixel-format", "nv12", "--encoding", "b64", "--model", "lenet5"])
    with pytest.raises(ValueError):
        pack_yuv420(np.zeros((1, 3, 2), np.uint8), np.zeros((1, 1, 1), np.uint8),
                    np.zeros((1, 1, 1), np.uint8), "i420")


# ---- 5. the stub engine end to end --------------------------------------------------------------

MAX_BATCH, CLASSES = 4, 10
COUNTS = [1, 2, 1, 6, 3]        # r3: one record over max_batch (fragments of 4 and 2)


def run_stub(records, model_hwc, **opts):
    broker = K.Broker()
    broker.start()
    try:
        broker.create_topic("in", 1)
        broker.create_topic("out", 1)
        for key, value in records:
            broker.append("in", 0, [value], [key])
        c = GaleConfig(topology_name="t", input_topic="in", output_topic="out",
                       bootstrap=f"127.0.0.1:{broker.port}", start_offset="earliest", stub=True,
                       max_batch=MAX_BATCH, max_wait_us=500, output_key="input",
                       on_error="null", input_format="b64", **opts).validate()
        d = c.engine_dict(*model_hwc, CLASSES)
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
    assert len(out) == len(records)
    return {r["key"]: r["value"] for r in out}, stats


def yuv_case(HS, WS, seed):
    rng = np.random.default_rng(seed)
    return {f"r{i}".encode(): tuple(rng.integers(0, 256, (n, h, w), dtype=np.uint8)
                                    for h, w in ((HS, WS), (HS // 2, WS // 2), (HS // 2, WS // 2)))
            for i, n in enumerate(COUNTS)}


def bad_yuv_record(planes, fmt):
    rec = bytearray(encode_records_yuv(*planes, fmt, planes[0].shape[0])[0])
    at = bytes(rec).rindex(b'"b64":"') + 7 + 5
    rec[at:at + 1] = b"="
    return bytes(rec)


@pytest.mark.parametrize("resize", [False, True])
@pytest.mark.parametrize("fmt", FORMATS)
def test_stub_engine_equals_rgb_records_of_the_oracle(fmt, resize):
    HS, WS = (40, 36) if resize else (32, 32)
    planes = yuv_case(HS, WS, 23)
    yc = YuvConvert(fmt, "bt709", "limited")
    opts = dict(input_scale=1 / 255, input_mean=CIFAR_MEAN_S, input_std=CIFAR_STD_S)
    if resize:
        opts.update(input_size="40,36", input_resize="34,33")
    rgb = {k: yc.apply(pack_yuv420(*p, fmt), HS, WS) for k, p in planes.items()}
    want, wstats = run_stub([(k, encode_records_b64(x, x.shape[0])[0]) for k, x in rgb.items()],
                            (32, 32, 3), **opts)
    assert wstats["yuv_records"] == 0 and wstats["b64_records"] == len(COUNTS)
    recs = [(k, encode_records_yuv(*p, fmt, p[0].shape[0])[0]) for k, p in planes.items()]
    recs.insert(2, (b"badchar", bad_yuv_record(planes[b"r1"], fmt)))
    recs.insert(4, (b"rgbsize", encode_records_b64(rgb[b"r0"], 1)[0]))
    got, stats = run_stub(recs, (32, 32, 3), input_pixel_format=fmt, input_yuv_matrix="bt709",
                          **opts)
    assert got.pop(b"badchar") is None and got.pop(b"rgbsize") is None
    assert set(got) == set(want)
    for k in want:
        assert want[k] is not None and got[k] == want[k], k
    assert len(json.loads(got[b"r3"])["predictions"]) == 6
    assert stats["yuv_records"] == len(COUNTS) + 1 == stats["b64_records"], stats
    assert stats["split_records"] == 1 and stats["errors"] == 2, stats
    assert stats["resized_images"] == (sum(COUNTS) if resize else 0)
    if resize:      # and the model input is the resize oracle of the prepped oracle image
        prep = InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S)
        rs = InputResize(40, 36, 34, 33, 32, 32)
        x = rs.apply(prep.apply(rgb[b"r0"].astype(np.float32)))
        ref, _ = run_stub([(b"f", b'{"instances":[{"b64":"' + base64.b64encode(
            rgb[b"r0"][0].tobytes()) + b'"}]}')], (32, 32, 3), **opts)
        assert x.shape == (1, 32, 32, 3) and ref[b"f"] == got[b"r0"]


# ---- 6. stand-alone sanitizer run ---------------------------------------------------------------

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None,
                    reason="needs ROCm clang++ and make")
def test_yuv_codec_under_address_and_ub_sanitizers():
    target = "build/asan/yuv_check"
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
