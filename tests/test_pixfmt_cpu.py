"""Packed-pixel records (--input-pixel-format bgr24 | rgba | bgra | gray) on the host: the
definition against a per-pixel restatement and against PIL, the host twin against the numpy
oracle, the record decoder against the RGB decoder on the oracle's images, the b64 verdict table
with L = 4 ceil(B / 3), the splitter, the configuration refusals and sources, produce, the stub
engine end to end against RGB records of the oracle's images, and the stand-alone sanitizer
program. Every comparison is bit-exact."""

import base64
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from gale._native import native
from gale.cli import cmd_produce, parse_topology_args
from gale.config import GaleConfig, from_sources
from gale.data import encode_records_b64, encode_records_packed, pack_pixels
from gale.models.preprocess import InputPrep, InputResize, PixelUnpack

C = native()
K = C.kafka
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FORMATS = ("bgr24", "rgba", "bgra", "gray")
# the issue's table, copied by hand: (bytes per pixel, offset of R, G, B in a pixel)
TABLE = {"bgr24": (3, (2, 1, 0)), "rgba": (4, (0, 1, 2)), "bgra": (4, (2, 1, 0)),
         "gray": (1, (0, 0, 0))}
# 1x1, the three padding lengths for P = 1 and 4, odd sizes, one CIFAR image
SIZES = [(1, 1), (4, 4), (5, 7), (6, 10), (3, 11), (32, 32)]
CIFAR_MEAN_S = "0.4914,0.4822,0.4465"
CIFAR_STD_S = "0.2470,0.2435,0.2616"
PREP = InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S)

OK, BAD_ENVELOPE, UNKNOWN_KEY, BAD_SHAPE, EMPTY, BAD_NUMBER, NULL_INSTANCES, TOO_LARGE = \
    0, 1, 2, 3, 4, 5, 6, 7


def random_packed(n, HS, WS, fmt, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, HS * WS * TABLE[fmt][0]), dtype=np.uint8)


def b64_record(images) -> bytes:
    return b'{"instances":[' + b",".join(b'{"b64":"' + base64.b64encode(im.tobytes()) + b'"}'
                                         for im in images) + b"]}"


# ---- 1. the definition --------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("HS,WS", SIZES[:5])
def test_oracle_equals_a_per_pixel_restatement(HS, WS, fmt):
    P, off = TABLE[fmt]
    un = PixelUnpack(fmt)
    assert (un.bytes_per_pixel, un.offsets) == (P, off) and un.frame_bytes(HS, WS) == HS * WS * P
    src = random_packed(2, HS, WS, fmt, 1)
    got = un.apply(src, HS, WS)
    assert got.shape == (2, HS, WS, 3) and got.dtype == np.uint8
    for i in range(2):
        raw = src[i].tobytes()
        for y in range(HS):
            for x in range(WS):
                px = raw[(y * WS + x) * P:(y * WS + x + 1) * P]
                assert tuple(got[i, y, x]) == tuple(px[o] for o in off)
    with pytest.raises(ValueError):
        un.apply(src[:, :-1], HS, WS)
    with pytest.raises(ValueError):
        un.frame_bytes(0, WS)
    with pytest.raises(ValueError, match="input_pixel_format"):
        PixelUnpack("bgr")


@pytest.mark.parametrize("HS,WS", [(5, 7), (32, 32)])
def test_oracle_equals_pil(HS, WS):
    Image = pytest.importorskip("PIL.Image")
    want = {
        "rgba": lambda b: Image.frombytes("RGBA", (WS, HS), b).convert("RGB"),
        "bgr24": lambda b: Image.frombytes("RGB", (WS, HS), b, "raw", "BGR"),
        "bgra": lambda b: Image.frombytes("RGBA", (WS, HS), b, "raw", "BGRA").convert("RGB"),
        "gray": lambda b: Image.frombytes("L", (WS, HS), b).convert("RGB"),
    }
    for fmt in FORMATS:
        src = random_packed(1, HS, WS, fmt, 2)[0]
        pil = np.asarray(want[fmt](src.tobytes()))
        assert np.array_equal(PixelUnpack(fmt).apply(src, HS, WS), pil), fmt


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("HS,WS", SIZES)
def test_host_twin_equals_the_oracle(HS, WS, fmt):
    src = random_packed(3, HS, WS, fmt, 3)
    rgb = PixelUnpack(fmt).apply(src, HS, WS)
    a, b = PREP.coeffs()
    assert C.packed_bpp(fmt) == TABLE[fmt][0] and C.packed_bpp("rgb") == 0
    for i in range(3):
        u8, f32 = C.packed_to_rgb_host(src[i].tobytes(), HS, WS, fmt)
        assert np.array_equal(u8, rgb[i]) and np.array_equal(f32, rgb[i].astype(np.float32))
        _, fp = C.packed_to_rgb_host(src[i].tobytes(), HS, WS, fmt, a, b)
        # (coefficients indexed by model channel, whatever the order on the wire)
        assert np.array_equal(fp.view(np.uint32),
                              PREP.apply(rgb[i].astype(np.float32)).view(np.uint32))
    for bad in ((src[0].tobytes()[:-1], HS, WS, fmt), (src[0].tobytes(), HS, WS, "bgr"),
                (b"", 0, WS, fmt)):
        with pytest.raises(ValueError):
            C.packed_to_rgb_host(*bad)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("HS,WS", SIZES)
def test_record_decoder_equals_the_rgb_decoder_on_the_oracles_image(HS, WS, fmt):
    src = random_packed(3, HS, WS, fmt, 4)
    rgb = PixelUnpack(fmt).apply(src, HS, WS)
    st, got = C.parse_instances_packed_host(b64_record(src), HS, WS, fmt)
    wst, want = C.parse_instances_b64_host(encode_records_b64(rgb, 3)[0], HS, WS, 3)
    assert st == OK == wst and got.shape == (3, HS, WS, 3)
    assert np.array_equal(got.view(np.uint32), np.asarray(want).reshape(got.shape).view(np.uint32))
    # ... and with prep: the stub applies it to the decoder's floats
    a, b = PREP.coeffs()
    gp, wp = (np.array(v, dtype=np.float32).reshape(3, HS, WS, 3) for v in (got, want))
    gp, wp = (C.apply_input_prep(v, HS, WS, 3, False, a, b) for v in (gp, wp))
    assert np.array_equal(np.asarray(gp).view(np.uint32), np.asarray(wp).view(np.uint32))
    assert np.array_equal(np.asarray(gp).reshape(3, HS, WS, 3).view(np.uint32),
                          PREP.apply(rgb.astype(np.float32)).view(np.uint32))


def test_pack_pixels_inverts_the_oracle():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)
    alpha = rng.integers(0, 256, (2, 5, 7), dtype=np.uint8)
    for fmt in ("bgr24", "rgba", "bgra"):
        p = pack_pixels(x, fmt, alpha if fmt != "bgr24" else None)
        assert p.shape == (2, 35 * TABLE[fmt][0])
        assert np.array_equal(PixelUnpack(fmt).apply(p, 5, 7), x)
        if fmt != "bgr24":
            assert np.array_equal(p.reshape(2, 5, 7, 4)[..., 3], alpha)
            assert (pack_pixels(x, fmt).reshape(2, 5, 7, 4)[..., 3] == 255).all()
    g = np.repeat(x[..., :1], 3, axis=-1)
    assert np.array_equal(PixelUnpack("gray").apply(pack_pixels(g, "gray"), 5, 7), g)
    with pytest.raises(ValueError, match="R == G == B"):
        pack_pixels(x, "gray")
    with pytest.raises(ValueError, match="alpha"):
        pack_pixels(x, "bgr24", alpha)
    with pytest.raises(ValueError):
        pack_pixels(x, "rgb")
    recs = encode_records_packed(x, "bgra", 2, alpha)
    assert recs == [b64_record(pack_pixels(x, "bgra", alpha))]


# ---- 2. the verdict table with L = 4 ceil(B / 3), the splitter ----------------------------------

def rec_of(*elems: str) -> bytes:
    return ('{"instances":[' + ",".join(elems) + "]}").encode()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("HS,WS", [(4, 4), (5, 7), (6, 10)])
def test_verdict_table(HS, WS, fmt):
    """One row per status of the b64 table; 4x4, 5x7 and 6x10 give gray and rgba / bgra strings
    two, one and no '='."""
    P = TABLE[fmt][0]
    B = HS * WS * P
    L = 4 * ((B + 2) // 3)
    pad = (3 - B % 3) % 3
    s = [base64.b64encode(f.tobytes()).decode() for f in random_packed(2, HS, WS, fmt, 6)]
    assert all(len(x) == L and x.count("=") == pad and x.endswith("=" * pad) for x in s)

    def both(rec):
        scan = C.scan_instances_b64_bytes(rec, B)[0]
        full = C.parse_instances_packed_host(rec, HS, WS, fmt)[0]
        assert C.parse_instances_b64_host(rec, HS, WS, P)[0] == full   # the rgb decoder's verdict
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
    # the characters are the decoder's: an outsider (or '=') in the data part ...
    for at in (0, 17, L - pad - 1):
        for ch in "=-_ \\":
            bad = s[1][:at] + ch + s[1][at + 1:]
            assert both(rec_of(el(s[0]), el(bad))) == (OK, BAD_NUMBER), (at, ch)
    # ... and anything but '=' in the padding
    for at in range(L - pad, L):
        for ch in "A/-":
            bad = s[1][:at] + ch + s[1][at + 1:]
            assert both(rec_of(el(s[0]), el(bad))) == (OK, BAD_NUMBER), (at, ch)
    assert C.parse_instances_packed_host(rec_of(el(s[0]), el(s[1])), HS, WS, fmt,
                                         max_images=1)[0] == TOO_LARGE
    # an RGB-size string is the wrong length (bgr24: the right one - the formats share L), and an
    # unknown format or a non-positive size is BAD_SHAPE
    rgb = base64.b64encode(bytes(HS * WS * 3)).decode()
    assert both(rec_of(el(rgb))) == ((OK, OK) if P == 3 else (BAD_SHAPE, BAD_SHAPE))
    r = rec_of(el(s[0]), el(s[1]))
    for f in ("rgb", "bgr", "yuyv", ""):
        assert C.parse_instances_packed_host(r, HS, WS, f)[0] == BAD_SHAPE
    assert C.parse_instances_packed_host(r, 0, WS, fmt)[0] == BAD_SHAPE
    assert C.parse_instances_packed_host(r, HS, -WS, fmt)[0] == BAD_SHAPE
    # the (H, W, C) forms are the byte-count forms of H*W*C
    assert C.scan_instances_b64(r, HS, WS, P) == C.scan_instances_b64_bytes(r, B)


@pytest.mark.parametrize("fmt", FORMATS)
def test_splitter_yields_byte_identical_fragments(fmt):
    HS, WS = 5, 7
    src = random_packed(5, HS, WS, fmt, 9)
    B = src.shape[1]
    L = 4 * ((B + 2) // 3)
    rec = b64_record(src)
    _, off, ln, n = C.scan_instances_b64_bytes(rec, B)
    arr = rec[off:off + ln]
    spans = C.split_instances_b64_bytes(arr, B)
    offs = C.b64_image_offsets_bytes(arr, B)
    assert n == 5 and len(spans) == 5 and len(offs) == 5
    for i, (b, e) in enumerate(spans):
        assert b'{"instances":[' + arr[b:e] + b"]}" == b64_record(src[i:i + 1])
        assert arr[offs[i]:offs[i] + L] == base64.b64encode(src[i].tobytes())
    assert C.split_instances_b64_bytes(arr, B + 3) is None


# ---- 3. configuration ---------------------------------------------------------------------------

def cfg(**kw):
    return GaleConfig(topology_name="t", **kw).validate()


@pytest.mark.parametrize("fmt", FORMATS)
def test_refusals_name_their_option(fmt):
    ok = dict(input_format="b64", input_pixel_format=fmt)
    cfg(**ok)
    cfg(**ok, input_size="33,31")                     # odd sizes: the even rule is a YUV rule
    assert cfg(**ok).input_unpack() == PixelUnpack(fmt) and cfg(**ok).input_yuv() is None
    with pytest.raises(ValueError, match="--input-format b64"):
        cfg(input_pixel_format=fmt)
    with pytest.raises(ValueError, match=f"--input-pixel-format {fmt}.*--input-layout nchw"):
        cfg(**ok, input_layout="nchw")
    with pytest.raises(ValueError, match=f"--input-pixel-format {fmt}.*C = 1"):
        cfg(**ok, model="lenet5")
    with pytest.raises(ValueError, match="--input-yuv-matrix"):
        cfg(**ok, input_yuv_matrix="bt709")
    with pytest.raises(ValueError, match="--input-yuv-range"):
        cfg(**ok, input_yuv_range="full")
    # the native engine refuses the same combinations (a dict built by hand)
    d = cfg(**ok, input_topic="in", output_topic="out").engine_dict(32, 32, 3, 10)
    assert d["pixel_format"] == fmt and "yuv_matrix" not in d and "yuv_range" not in d
    C.Engine(d)
    C.Engine(dict(d, rec_H=33, rec_W=31))
    for bad in (dict(input_format="json"), dict(input_nchw=True), dict(C=1),
                dict(yuv_matrix="bt709"), dict(yuv_range="full"), dict(pixel_format="yuyv"),
                dict(pixel_format="bgr")):
        with pytest.raises(ValueError, match="pixel_format|yuv_matrix"):
            C.Engine(dict(d, **bad))


def test_gray_with_lenet5_points_at_rgb():
    with pytest.raises(ValueError, match="rgb already carries one byte per pixel"):
        cfg(input_format="b64", input_pixel_format="gray", model="lenet5")


def test_bgr_and_yuyv_stay_refused_and_rgb_is_unchanged():
    with pytest.raises(SystemExit):
        parse_topology_args(["t", "in", "out", "--input-pixel-format", "bgr"])
    with pytest.raises(ValueError, match="input_pixel_format"):
        cfg(input_format="b64", input_pixel_format="yuyv")
    with pytest.raises(ValueError, match="input_pixel_format"):
        cfg(input_format="b64", input_pixel_format="bgr")
    # rgb: nothing new reaches the engine, and the YUV entries are what they were
    d = cfg(input_format="b64").engine_dict(32, 32, 3, 10)
    assert not {"pixel_format", "yuv_matrix", "yuv_range"} & set(d)
    assert cfg(input_format="b64").input_unpack() is None and cfg().input_unpack() is None
    y = cfg(input_format="b64", input_pixel_format="nv12").engine_dict(32, 32, 3, 10)
    assert (y["pixel_format"], y["yuv_matrix"], y["yuv_range"]) == ("nv12", "bt601", "limited")
    assert cfg(input_format="b64", input_pixel_format="nv12").input_unpack() is None


def test_three_sources_and_their_precedence(tmp_path):
    toml = tmp_path / "g.toml"
    toml.write_text('[gale]\ninput-format = "b64"\ninput-pixel-format = "bgr24"\n')
    c = from_sources(cli=dict(topology_name="t"), env={}, toml_path=str(toml))
    assert c.input_pixel_format == "bgr24" and c.input_unpack() == PixelUnpack("bgr24")
    env = {"GALE_INPUT_PIXEL_FORMAT": "gray"}
    c = from_sources(cli=dict(topology_name="t"), env=env, toml_path=str(toml))
    assert c.input_pixel_format == "gray"
    c = from_sources(cli=dict(topology_name="t", input_pixel_format="rgba"), env=env,
                     toml_path=str(toml))
    assert c.input_pixel_format == "rgba" and c.input_unpack().bytes_per_pixel == 4
    c = parse_topology_args(["t", "in", "out", "--input-format", "b64", "--input-pixel-format",
                             "bgra"])
    assert c.input_unpack() == PixelUnpack("bgra")
    bad = tmp_path / "bad.toml"
    bad.write_text('[gale]\ninput-format = "b64"\ninput-pixel-format = "bgr"\n')
    with pytest.raises(ValueError, match="input_pixel_format"):
        from_sources(cli=dict(topology_name="t"), env={}, toml_path=str(bad)).validate()


def test_produce_pixel_format(capsys):
    for fmt in FORMATS:
        with pytest.raises(SystemExit) as e:
            cmd_produce(["topic", "--pixel-format", fmt, "--pixels", "byte"])
        assert e.value.code == 2 and "--encoding b64" in capsys.readouterr().err
        with pytest.raises(SystemExit) as e:
            cmd_produce(["topic", "--pixel-format", fmt, "--encoding", "b64", "--pixels", "byte",
                         "--model", "lenet5"])
        assert e.value.code == 2 and "3-channel" in capsys.readouterr().err
        with pytest.raises(SystemExit) as e:
            cmd_produce(["topic", "--pixel-format", fmt, "--encoding", "b64", "--pixels", "byte",
                         "--layout", "nchw"])
        assert e.value.code == 2 and "byte order" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cmd_produce(["topic", "--pixel-format", "bgr", "--encoding", "b64"])


# ---- 4. the stub engine end to end --------------------------------------------------------------

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


def bad_record(images):
    rec = bytearray(b64_record(images))
    at = bytes(rec).rindex(b'"b64":"') + 7 + 5
    rec[at:at + 1] = b"-"
    return bytes(rec)


@pytest.mark.parametrize("resize", [False, True])
@pytest.mark.parametrize("fmt", FORMATS)
def test_stub_engine_equals_rgb_records_of_the_oracle(fmt, resize):
    HS, WS = (40, 36) if resize else (32, 32)
    rng = np.random.default_rng(23)
    B = PixelUnpack(fmt).frame_bytes(HS, WS)
    sets = {f"r{i}".encode(): rng.integers(0, 256, (n, B), dtype=np.uint8)
            for i, n in enumerate(COUNTS)}
    opts = dict(input_scale=1 / 255, input_mean=CIFAR_MEAN_S, input_std=CIFAR_STD_S)
    if resize:
        opts.update(input_size="40,36", input_resize="34,33")
    rgb = {k: PixelUnpack(fmt).apply(p, HS, WS) for k, p in sets.items()}
    want, wstats = run_stub([(k, encode_records_b64(x, x.shape[0])[0]) for k, x in rgb.items()],
                            (32, 32, 3), **opts)
    assert wstats["packed_records"] == 0 and wstats["b64_records"] == len(COUNTS)
    recs = [(k, b64_record(p)) for k, p in sets.items()]
    recs.insert(2, (b"badchar", bad_record(sets[b"r1"])))
    if fmt != "bgr24":      # (an RGB image is a bgr24 image to the scan: same byte count)
        recs.insert(4, (b"rgbsize", encode_records_b64(rgb[b"r0"], 1)[0]))
    got, stats = run_stub(recs, (32, 32, 3), input_pixel_format=fmt, **opts)
    assert got.pop(b"badchar") is None
    assert fmt == "bgr24" or got.pop(b"rgbsize") is None
    assert set(got) == set(want)
    for k in want:
        assert want[k] is not None and got[k] == want[k], k
    assert len(json.loads(got[b"r3"])["predictions"]) == 6
    assert stats["packed_records"] == len(COUNTS) + 1 == stats["b64_records"], stats
    assert stats["yuv_records"] == 0, stats
    assert stats["split_records"] == 1, stats
    assert stats["errors"] == (1 if fmt == "bgr24" else 2), stats
    assert stats["resized_images"] == (sum(COUNTS) if resize else 0)
    if resize:      # and the model input is the resize oracle of the prepped oracle image
        rs = InputResize(40, 36, 34, 33, 32, 32)
        x = rs.apply(PREP.apply(rgb[b"r0"].astype(np.float32)))
        ref, _ = run_stub([(b"f", b64_record(rgb[b"r0"]))], (32, 32, 3), **opts)
        assert x.shape == (1, 32, 32, 3) and ref[b"f"] == got[b"r0"]


def produce_and_serve(fmt):
    """`produce --pixel-format fmt` into an embedded broker, served by a stub engine."""
    broker = K.Broker()
    broker.start()
    try:
        broker.create_topic("in", 1)
        broker.create_topic("out", 1)
        boot = f"127.0.0.1:{broker.port}"
        assert cmd_produce(["in", "--bootstrap", boot, "--images", "12", "--images-per-record",
                            "3", "--pixels", "byte", "--encoding", "b64", "--model", "resnet20",
                            "--pixel-format", fmt]) == 0
        c = GaleConfig(topology_name="t", input_topic="in", output_topic="out", bootstrap=boot,
                       start_offset="earliest", stub=True, max_batch=MAX_BATCH, max_wait_us=500,
                       on_error="null", input_format="b64", input_pixel_format=fmt,
                       input_scale=1 / 255, input_mean=CIFAR_MEAN_S,
                       input_std=CIFAR_STD_S).validate()
        d = c.engine_dict(32, 32, 3, CLASSES)
        d["max_records"] = 4
        eng = C.Engine(d)
        eng.add_stub_replica(MAX_BATCH, 0, True, -1)
        eng.start()
        assert eng.wait(30000), eng.stats()
        eng.stop()
        stats = dict(eng.stats())
        return [r["value"] for r in broker.read("out", 0)], stats
    finally:
        broker.stop()


def test_produced_records_are_served_as_their_rgb_records(capsys):
    """produce --pixel-format bgr24 | rgba | bgra sends the synthetic pixels of rgb in that byte
    order: the predictions are those of the rgb records."""
    want, wstats = produce_and_serve("rgb")
    assert len(want) == 4 and None not in want and wstats["packed_records"] == 0
    for fmt in ("bgr24", "rgba", "bgra"):
        got, stats = produce_and_serve(fmt)
        assert got == want and stats["packed_records"] == 4, fmt
    got, stats = produce_and_serve("gray")
    assert len(got) == 4 and None not in got and stats["packed_records"] == 4
    capsys.readouterr()


# ---- 5. stand-alone sanitizer run ---------------------------------------------------------------

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None,
                    reason="needs ROCm clang++ and make")
def test_pixfmt_codec_under_address_and_ub_sanitizers():
    target = "build/asan/pixfmt_check"
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
