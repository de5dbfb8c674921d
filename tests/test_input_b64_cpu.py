"""Base64 uint8 image records (--input-format b64) without a GPU: the host scanner and decoder
against base64.b64encode / numpy, every verdict of the format's table, the splitter, the stub
engine end to end, the configuration sources, and a stand-alone sanitizer run of the codec."""

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
from gale.data import encode_records_b64, encode_records_text
from gale.models.preprocess import InputPrep

C = native()
K = C.kafka
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK, BAD_ENVELOPE, UNKNOWN_KEY, BAD_SHAPE, EMPTY, BAD_NUMBER, NULL_INSTANCES, TOO_LARGE = range(8)
assert [C.status_name(i) for i in range(8)] == [
    "ok", "bad_envelope", "unknown_key", "bad_shape", "empty", "bad_number", "null_instances",
    "too_large"]

CIFAR_MEAN_S = "0.4914,0.4822,0.4465"
CIFAR_STD_S = "0.2470,0.2435,0.2616"

SHAPES = [(5, 4, 3), (5, 4, 1), (28, 28, 1)]   # padding 0, 1, 2


def geometry(shape):
    per = int(np.prod(shape))
    return per, 4 * ((per + 2) // 3), (3 - per % 3) % 3


def record(strings, ws=b""):
    """{"instances":[{"b64":"..."},...]} with `ws` around every structural token."""
    elems = (ws + b",").join(ws + b"{" + ws + b'"b64"' + ws + b":" + ws + b'"' + s + b'"' + ws + b"}"
                             for s in strings)
    return ws + b"{" + ws + b'"instances"' + ws + b":" + ws + b"[" + elems + ws + b"]" + ws + \
        b"}" + ws


def strings_of(x_u8):
    return [base64.b64encode(np.ascontiguousarray(im).tobytes()) for im in x_u8]


def scan(rec, shape):
    return C.scan_instances_b64(rec, *shape)


def decode(rec, shape):
    return C.parse_instances_b64_host(rec, *shape)


def test_geometry_of_the_shapes():
    assert [geometry(s)[1:] for s in SHAPES] == [(80, 0), (28, 1), (1048, 2)]


# ---- 1. scanner and host decoder against base64.b64encode / numpy -------------------------------

@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("ws", [b"", b" \n\t\r "])
def test_scan_and_decode_match_numpy(shape, n, ws):
    rng = np.random.default_rng(hash((shape, n)) % 1000)
    x = rng.integers(0, 256, (n,) + shape, dtype=np.uint8)
    rec = record(strings_of(x), ws)
    st, off, ln, images = scan(rec, shape)
    assert (st, images) == (OK, n)
    arr = rec[off:off + ln]
    assert arr[:1] == b"[" and arr[-1:] == b"]" and rec[off + ln:].strip() == b"}"
    per, L, pad = geometry(shape)
    offs = C.b64_image_offsets(arr, *shape)
    assert len(offs) == n
    for i, o in enumerate(offs):
        assert arr[o:o + L] == strings_of(x)[i] and arr[o - 1:o] == b'"' and arr[o + L:o + L + 1] == b'"'
    st, got = decode(rec, shape)
    assert st == OK and got.dtype == np.float32 and got.shape == (n,) + shape
    assert np.array_equal(got.view(np.uint32), x.astype(np.float32).view(np.uint32))
    # the model input: identity prep, the CIFAR / scalar prep, and NCHW-ordered bytes
    Cc = shape[2]
    mean, std = (CIFAR_MEAN_S, CIFAR_STD_S) if Cc == 3 else ("0.1307", "0.3081")
    for prep in (InputPrep.build(Cc), InputPrep.build(Cc, 1 / 255, mean, std)):
        a4, b4 = prep.coeffs()
        y = C.apply_input_prep(got, *shape, False, a4, b4)
        assert np.array_equal(y.view(np.uint32),
                              prep.apply(x.astype(np.float32)).view(np.uint32))
    prep = InputPrep.build(Cc, 1 / 255, mean, std, "nchw")
    rec_t = record(strings_of(x.transpose(0, 3, 1, 2)), ws)
    st, got_t = decode(rec_t, shape)
    assert st == OK
    y = C.apply_input_prep(got_t, *shape, True, *prep.coeffs())
    assert np.array_equal(y.view(np.uint32), prep.apply(x.astype(np.float32)).view(np.uint32))
    # the same floats as the number-array decoder gives for the same pixels
    st, ref = C.parse_instances_host(json.dumps({"instances": x.tolist()}).encode(), *shape)
    assert st == OK and np.array_equal(ref.view(np.uint32), got.view(np.uint32))
    # the load generator's encoder writes the compact form of the same record
    assert encode_records_b64(x, n) == [record(strings_of(x))]
    assert encode_records_b64(x, n, "nchw") == [record(strings_of(x.transpose(0, 3, 1, 2)))]


# ---- 2. verdicts --------------------------------------------------------------------------------

SHAPE0 = SHAPES[0]
S0 = base64.b64encode(bytes(range(60)))

ENVELOPE_CASES = [
    (b"", BAD_ENVELOPE),
    (b"[" + S0 + b"]", BAD_ENVELOPE),                                   # not an object
    (b'"' + S0 + b'"', BAD_ENVELOPE),
    (b'{"instances" [{"b64":"' + S0 + b'"}]}', BAD_ENVELOPE),           # no ':'
    (b'{"instances":7}', BAD_ENVELOPE),                                 # no array
    (b'{"instances":[{"b64":"' + S0 + b'"} {"b64":"' + S0 + b'"}]}', BAD_ENVELOPE),
    (b'{"instances":[{"b64":"' + S0 + b'"};]}', BAD_ENVELOPE),
    (b'{"instances":[{"b64":"' + S0 + b'"},]}', BAD_ENVELOPE),          # a trailing comma
    (b'{"instances":[{"b64" "' + S0 + b'"}]}', BAD_ENVELOPE),
    (b'{"instances":[{"b64":"' + S0 + b'"]}', BAD_ENVELOPE),            # the element not closed
    (b'{"instances":[{"b64":"' + S0 + b'"}]} x', BAD_ENVELOPE),         # text after the document
    (b'{"instances":[{"b64":"' + S0 + b'"}]', BAD_ENVELOPE),
    (b'{"inputs":[{"b64":"' + S0 + b'"}]}', UNKNOWN_KEY),               # another top-level key
    (b'{"instances":[{"b64":"' + S0 + b'"}],"k":1}', UNKNOWN_KEY),
    (b'{"instances":[{"b65":"' + S0 + b'"}]}', UNKNOWN_KEY),            # another element key
    (b'{"instances":[{"B64":"' + S0 + b'"}]}', UNKNOWN_KEY),
    (b'{"instances":[{"b64":"' + S0 + b'","k":1}]}', UNKNOWN_KEY),      # a second key
    (b'{"instances":null}', NULL_INSTANCES),
    (b' { } ', NULL_INSTANCES),
    (b'{"instances":[]}', EMPTY),
    (b'{"instances": [ ] }', EMPTY),
    (b'{"instances":[[[[1,2,3]]]]}', BAD_SHAPE),                        # a numeric array
    (b'{"instances":["' + S0 + b'"]}', BAD_SHAPE),                      # a bare string
    (b'{"instances":[{"b64":"' + S0 + b'"},7]}', BAD_SHAPE),
    (b'{"instances":[{}]}', BAD_SHAPE),
    (b'{"instances":[{"b64":12}]}', BAD_SHAPE),                         # not a string
    (b'{"instances":[{"b64":["' + S0 + b'"]}]}', BAD_SHAPE),
    (b'{"instances":[{"b64":null}]}', BAD_SHAPE),
    (b'{"instances":[{"b64":"' + S0[:-1] + b'"}]}', BAD_SHAPE),         # one character short
    (b'{"instances":[{"b64":"' + S0 + b'A"}]}', BAD_SHAPE),             # one long
    (b'{"instances":[{"b64":"' + S0[:-4] + b'"}]}', BAD_SHAPE),         # one group short
    (b'{"instances":[{"b64":""}]}', BAD_SHAPE),
]


@pytest.mark.parametrize("i", range(len(ENVELOPE_CASES)))
def test_host_scan_verdicts(i):
    rec, want = ENVELOPE_CASES[i]
    st, off, ln, images = scan(rec, SHAPE0)
    assert st == want, (rec[:60], C.status_name(st))
    assert (off, ln, images) == (0, 0, 0)
    st, out = decode(rec, SHAPE0)
    assert st == want and out.shape[0] == 0


def test_truncated_values():
    x = np.arange(120, dtype=np.uint8).reshape(2, 5, 4, 3)
    rec = record(strings_of(x))
    first = rec.index(b'"b64":"') + 7
    second = rec.index(b'"b64":"', first) + 7
    for cut in (first, first + 1, first + 40, first + 79, first + 80,    # inside string 1
                second, second + 17, second + 80):                        # inside string 2
        assert scan(rec[:cut], SHAPE0)[0] == BAD_SHAPE, cut
        assert decode(rec[:cut], SHAPE0)[0] == BAD_SHAPE
    for cut in (0, 1, 5, 13, 14, 15, 16, 20, 21, first + 81, first + 82, first + 83,
                len(rec) - 2, len(rec) - 1):                              # inside the envelope
        assert scan(rec[:cut], SHAPE0)[0] == BAD_ENVELOPE, cut
        assert decode(rec[:cut], SHAPE0)[0] == BAD_ENVELOPE
    assert scan(rec, SHAPE0)[0] == OK
    # every prefix gets one of the table's verdicts, never OK
    for cut in range(len(rec)):
        assert scan(rec[:cut], SHAPE0)[0] in (BAD_ENVELOPE, BAD_SHAPE), cut


def plant(s: bytes, at: int, what: bytes) -> bytes:
    """`what` over the characters of s from `at` (same length)."""
    at = min(at, len(s) - len(what))
    return s[:at] + what + s[at + len(what):]


BAD_CHARS = [b"-", b"_", b" ", b"\n", b"=", b"\x80", b"\xff", b"\\/", b'"', b"\\", b"\t", b".",
             b"@", b"[", b"`", b"{"]


@pytest.mark.parametrize("shape", SHAPES)
def test_bad_characters_are_bad_number(shape):
    per, L, pad = geometry(shape)
    rng = np.random.default_rng(3)
    x = rng.integers(0, 256, (3,) + shape, dtype=np.uint8)
    ss = strings_of(x)
    data = L - pad
    for ch in BAD_CHARS:
        for at in (0, data // 2, data - len(ch)):        # first, a middle and the last data char
            for img in (0, 2):
                bad = list(ss)
                bad[img] = plant(ss[img], at, ch)
                assert len(bad[img]) == L and bad[img] != ss[img]
                rec = record(bad)
                assert scan(rec, shape)[:1] + scan(rec, shape)[3:] == (OK, 3), (ch, at)
                st, out = decode(rec, shape)
                assert st == BAD_NUMBER, (ch, at, img)
    # padding: one '=' too many (the last data character), one too few
    rec = record([plant(ss[0], data - 1, b"=")])
    assert scan(rec, shape)[0] == OK and decode(rec, shape)[0] == BAD_NUMBER
    for k in range(pad):
        rec = record([plant(ss[0], data + k, b"A")])
        assert scan(rec, shape)[0] == OK and decode(rec, shape)[0] == BAD_NUMBER
    # the URL-safe alphabet of the same bytes is rejected where it differs
    url = base64.urlsafe_b64encode(b"\xfb\xff\xfe" * (per // 3) + b"\xfb" * (per % 3))
    assert len(url) == L and (b"-" in url or b"_" in url)
    assert decode(record([url]), shape)[0] == BAD_NUMBER
    assert decode(record([url.replace(b"-", b"+").replace(b"_", b"/")]), shape)[0] == OK


@pytest.mark.parametrize("shape", SHAPES[1:])
def test_unused_trailing_bits_are_ignored(shape):
    per, L, pad = geometry(shape)
    alphabet = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
    x = np.random.default_rng(4).integers(0, 256, (1,) + shape, dtype=np.uint8)
    s = strings_of(x)[0]
    last = L - pad - 1
    v = alphabet.index(s[last:last + 1])
    unused = 2 * pad                       # bits: 2 with one '=', 4 with two
    assert v & ((1 << unused) - 1) == 0    # b64encode zeroes them
    for low in range(1, 1 << unused):
        t = plant(s, last, alphabet[v | low:(v | low) + 1])
        assert t != s
        st, out = decode(record([t]), shape)
        assert st == OK and np.array_equal(out[0], x[0].astype(np.float32))


def test_too_many_images_for_the_caller():
    x = np.zeros((3,) + SHAPE0, dtype=np.uint8)
    assert C.parse_instances_b64_host(record(strings_of(x)), *SHAPE0, 2)[0] == TOO_LARGE
    assert C.parse_instances_b64_host(record(strings_of(x)), *SHAPE0, 3)[0] == OK


# ---- 3. splitter --------------------------------------------------------------------------------

@pytest.mark.parametrize("ws", [b"", b" \n"])
def test_splitter_fragments(ws):
    shape, mb = SHAPES[1], 3
    x = np.random.default_rng(5).integers(0, 256, (7,) + shape, dtype=np.uint8)
    rec = record(strings_of(x), ws)
    st, off, ln, n = scan(rec, shape)
    assert (st, n) == (OK, 7)
    arr = rec[off:off + ln]
    spans = C.split_instances_b64(arr, *shape)
    assert len(spans) == 7
    for b, e in spans:
        assert arr[b:b + 1] == b"{" and arr[e - 1:e] == b"}"
    sizes, got = [], []
    for i0 in range(0, 7, mb):                       # (Engine::split_record's fragments)
        i1 = min(7, i0 + mb)
        frag = b'{"instances":[' + arr[spans[i0][0]:spans[i1 - 1][1]] + b"]}"
        st, _, _, k = scan(frag, shape)
        assert st == OK
        sizes.append(k)
        st, out = decode(frag, shape)
        assert st == OK
        got.append(out)
    assert sizes == [3, 3, 1]
    assert np.array_equal(np.concatenate(got), x.astype(np.float32))
    # a broken element list is refused
    assert C.split_instances_b64(arr[:-1], *shape) is None
    assert C.b64_image_offsets(arr[1:], *shape) is None
    assert C.split_instances_b64(b"[[[[1]]]]", *shape) is None


# ---- 4. stub engine end to end ------------------------------------------------------------------

H, W, CH, CLASSES = 4, 3, 3, 10


def stub_probs(x):
    """replica.cpp: logit k = (k + 1) * mean of channel k % C, then softmax (in double)."""
    means = x.reshape(x.shape[0], -1, x.shape[-1]).astype(np.float64).mean(axis=1)
    logits = np.stack([(k + 1) * means[:, k % x.shape[-1]] for k in range(CLASSES)], axis=1)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
def test_stub_engine_b64(layout):
    broker = K.Broker()
    broker.start()
    try:
        broker.create_topic("in", 1)
        broker.create_topic("out", 1)
        rng = np.random.default_rng(6)
        xs = {}
        for i, n in enumerate([1, 2, 3, 9, 1, 4, 2]):       # 9 > max_batch 4: served as fragments
            x = rng.integers(0, 256, (n, H, W, CH), dtype=np.uint8)
            key = f"r{i}".encode()
            xs[key] = x
            broker.append("in", 0, encode_records_b64(x, n, layout), [key])
        bad = strings_of(xs[b"r2"])
        bad[1] = plant(bad[1], 17, b"-")
        broker.append("in", 0, [record(bad)], [b"badchar"])
        broker.append("in", 0, encode_records_text(xs[b"r1"], 2), [b"numeric"])
        cfg = GaleConfig(topology_name="t", input_topic="in", output_topic="out",
                         bootstrap=f"127.0.0.1:{broker.port}", start_offset="earliest",
                         stub=True, max_batch=4, max_wait_us=500, output_key="input",
                         on_error="null", input_format="b64", input_scale=1 / 255,
                         input_mean=CIFAR_MEAN_S, input_std=CIFAR_STD_S,
                         input_layout=layout).validate()
        d = cfg.engine_dict(H, W, CH, CLASSES)
        assert d["input_format"] == "b64" and d["text_pack"] is False
        d["max_records"] = len(xs) + 2
        eng = C.Engine(d)
        eng.add_stub_replica(4, 0, True, -1)
        eng.start()
        assert eng.wait(30000), eng.stats()
        eng.stop()
        st = eng.stats()
        out = broker.read("out", 0)
    finally:
        broker.stop()
    assert len(out) == len(xs) + 2                          # ONE record per input record
    by_key = {r["key"]: r["value"] for r in out}
    assert set(by_key) == set(xs) | {b"badchar", b"numeric"}
    assert by_key[b"badchar"] is None and by_key[b"numeric"] is None
    prep = cfg.input_prep(CH)
    for k, x in xs.items():
        got = np.array(json.loads(by_key[k])["predictions"])
        want = stub_probs(prep.apply(x.astype(np.float32)))
        assert got.shape == want.shape == (x.shape[0], CLASSES), k
        np.testing.assert_allclose(got, want, atol=1e-6, err_msg=str(k))
        assert np.abs(got - stub_probs(x.astype(np.float32))).max() > 1e-3
    assert st["b64_records"] == len(xs) + 1                 # the good ones and the bad character
    assert st["errors"] == 2 and st["split_records"] == 1 and st["split_fragments"] == 3
    assert st["images_out"] == sum(x.shape[0] for x in xs.values())


def test_json_topology_rejects_b64_records():
    """The mode is exclusive: a b64 record in a json topology is an error record, as today."""
    x = np.zeros((1, H, W, CH), dtype=np.uint8)
    rec = encode_records_b64(x)[0]
    assert C.scan_instances(rec, H, W, CH)[0] != OK
    assert C.scan_instances_b64(encode_records_text(x)[0], H, W, CH)[0] == BAD_SHAPE


def test_gpu_ingest_is_refused_in_b64_mode():
    cfg = GaleConfig(topology_name="t", input_topic="in", output_topic="out",
                     input_format="b64").validate()
    eng = C.Engine(cfg.engine_dict(H, W, CH, CLASSES))
    with pytest.raises(ValueError):
        eng.enable_gpu_ingest(0, 1, 20)


# ---- 5. configuration ---------------------------------------------------------------------------

def test_config_sources(tmp_path):
    cli = parse_topology_args(["t", "in", "out", "--input-format", "b64"])
    env = from_sources(cli=dict(topology_name="t"), env={"GALE_INPUT_FORMAT": "b64"})
    toml = tmp_path / "g.toml"
    toml.write_text('[gale]\ninput-format = "b64"\n')
    tom = from_sources(cli=dict(topology_name="t"), env={}, toml_path=str(toml))
    for cfg in (cli, env, tom):
        assert cfg.input_format == "b64"
        assert cfg.engine_dict(32, 32, 3, 10)["input_format"] == "b64"
    mixed = from_sources(cli=dict(topology_name="t", input_format="json"),
                         env={"GALE_INPUT_FORMAT": "b64"}, toml_path=str(toml))
    assert mixed.input_format == "json"
    with pytest.raises(ValueError):
        GaleConfig(topology_name="t", input_format="base64").validate()
    with pytest.raises(ValueError):
        from_sources(cli=dict(topology_name="t"), env={"GALE_INPUT_FORMAT": "B64"})
    with pytest.raises(SystemExit):
        parse_topology_args(["t", "in", "out", "--input-format", "hex"])
    with pytest.raises(ValueError):
        C.Engine(dict(GaleConfig(topology_name="t", input_topic="in", output_topic="out")
                      .engine_dict(4, 3, 3, 10), input_format="hex"))


def test_default_engine_dict_gains_only_the_key():
    base = GaleConfig(topology_name="t").validate()
    d = base.engine_dict(32, 32, 3, 10)
    assert d["input_format"] == "json"
    b = GaleConfig(topology_name="t", input_format="b64").validate().engine_dict(32, 32, 3, 10)
    diff = {k for k in d if d[k] != b[k]}
    assert diff <= {"input_format", "text_pack"} and set(d) == set(b)
    assert b["text_pack"] is False
    # every other entry is what the defaults gave before the option existed
    assert d["text_pack"] == bool(base.gpu_ingest and base.text_pack and C.text_pack_fast())
    assert d["input_a"] == [1.0] * 4 and d["input_b"] == [0.0] * 4 and d["input_nchw"] is False


def test_produce_b64_needs_byte_pixels(capsys):
    with pytest.raises(SystemExit) as e:
        cmd_produce(["topic", "--encoding", "b64"])
    assert e.value.code == 2
    assert "--pixels byte" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cmd_produce(["topic", "--encoding", "hex", "--pixels", "byte"])
    with pytest.raises(ValueError):
        encode_records_b64(np.zeros((1, 2, 2, 3), dtype=np.float32))


# ---- 6. stand-alone sanitizer run ---------------------------------------------------------------

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None,
                    reason="needs ROCm clang++ and make")
def test_codec_under_address_and_ub_sanitizers():
    target = "build/asan/b64_scan_check"
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
