"""Top-k output (--top-k K) on the CPU: the two host encoders against the score-order rule written
in numpy, the configuration's three sources and refusals, and the stub engine end to end.

The oracle is the rule of csrc/codec/json_codec.h: key(v) = bits ^ (sign ? 0xffffffff :
0x80000000) as unsigned, entries descending by key, ties to the lower class index: a stable
argsort of the descending key. Score texts are C.format_float_java / format_float_java8 of the
selected values, so every comparison is byte equality."""

import json

import numpy as np
import pytest

from gale._native import native
from gale.config import GaleConfig, from_sources
from gale.engine import Engine

C = native()
K = C.kafka
H, W, CH, CLASSES = 32, 32, 3, 10


# ---- the oracle --------------------------------------------------------------------------------

def score_keys(x):
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return b ^ np.where(b >> 31 != 0, np.uint32(0xffffffff), np.uint32(0x80000000))


def topk_indices(x, k):
    """[rows, k] class indices in score order (stable argsort of the descending key)."""
    keys = score_keys(x).astype(np.int64)
    return np.argsort(-keys, axis=1, kind="stable")[:, :k].astype(np.int32)


def topk_document(x, k, json_string=False, java8=False):
    fmt = C.format_float_java8 if java8 else C.format_float_java
    x = np.ascontiguousarray(x, dtype=np.float32)
    items = []
    for row, sel in zip(x, topk_indices(x, k)):
        items.append('{"classes":[%s],"scores":[%s]}' % (
            ",".join(str(int(c)) for c in sel), ",".join(fmt(float(row[c])) for c in sel)))
    doc = '{"predictions":[%s]}' % ",".join(items)
    if json_string:
        doc = '"' + doc.replace('"', '\\"') + '"'
    return doc.encode()


def from_bits(words):
    return np.array(words, dtype=np.uint32).view(np.float32)


def softmax_rows(rows, classes, seed=1):
    z = np.random.default_rng(seed).normal(size=(rows, classes)).astype(np.float32) * 4
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def adversarial_rows(classes, k):
    """Rows on which a selection can go wrong: all equal; pairs of duplicates straddling the
    k-th place; both zeros; infinities and the NaNs at the ends of the key order; denormals."""
    rng = np.random.default_rng(classes * 131 + k)
    rows = [np.full(classes, 0.1, np.float32)]
    # values 0, 0, 1, 1, 2, 2, ... shuffled: whatever k is, a pair of equal values lies across
    # places k - 1 and k (k odd) or just before and after them (k even); and the same shifted
    for shift in (0, 1):
        v = ((np.arange(classes) + shift) // 2).astype(np.float32) / max(classes, 2)
        rows.append(rng.permutation(v))
    z = np.zeros(classes, np.float32)  # +0 and -0 alternate; -0 sorts below +0
    z[1::2] = -0.0
    rows.append(z)
    special = from_bits([0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7fffffff, 0xffffffff,
                         0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x00800000])
    s = rng.permutation(np.resize(special, classes))
    rows.append(s)
    d = from_bits(rng.integers(0, 0x00800000, classes))  # denormals (and maybe +0), duplicates
    d[: classes // 2] = d[classes - classes // 2:]
    rows.append(d)
    first = from_bits([0x7fffffff] + [0x3f000000] * (classes - 1))  # the largest key at class 0
    rows.append(first)
    return np.stack(rows).astype(np.float32)


def case_rows(classes, k):
    return np.concatenate([adversarial_rows(classes, k), softmax_rows(5, classes)])


CASES = [(10, 1), (10, 3), (10, 10), (1000, 5)]


def test_oracle_orders_by_the_bits():
    x = from_bits([[0x80000000, 0x00000000, 0x7f800000, 0x7fc00000, 0xff800000, 0xffc00000,
                    0x00000000, 0x3f800000]])
    # +NaN, +inf, 1.0, the two +0 (lower class first), -0, -inf, -NaN
    assert topk_indices(x, 8).tolist() == [[3, 2, 7, 1, 6, 0, 4, 5]]


# ---- the host codec ----------------------------------------------------------------------------

@pytest.mark.parametrize("classes,k", CASES)
def test_encode_topk_matches_the_oracle(classes, k):
    x = case_rows(classes, k)
    got = C.encode_predictions_topk(x, k)
    assert got == topk_document(x, k)
    doc = json.loads(got.replace(b"NaN", b"null").replace(b"-Infinity", b"null")
                     .replace(b"Infinity", b"null"))
    assert len(doc["predictions"]) == len(x)
    for item, sel in zip(doc["predictions"], topk_indices(x, k)):
        assert list(item) == ["classes", "scores"]
        assert item["classes"] == sel.tolist() and len(item["scores"]) == k
    assert C.encode_predictions_topk(x, k, False, True) == topk_document(x, k, java8=True)


@pytest.mark.parametrize("classes,k", CASES)
def test_encode_topk_json_string_is_doubly_encoded(classes, k):
    x = softmax_rows(3, classes, seed=5)  # finite values: the inner document is plain JSON
    got = C.encode_predictions_topk(x, k, True)
    assert got == topk_document(x, k, json_string=True)
    assert b'\\"classes\\"' in got and b'\\"scores\\"' in got
    inner = json.loads(got)
    assert isinstance(inner, str) and inner.encode() == C.encode_predictions_topk(x, k)
    doc = json.loads(inner)
    assert [p["classes"] for p in doc["predictions"]] == topk_indices(x, k).tolist()


def test_encode_topk_refuses_bad_k():
    x = softmax_rows(2, 10)
    for k in (0, -1, 11):
        with pytest.raises(ValueError):
            C.encode_predictions_topk(x, k)


def slots_of(x, sel):
    """Device-format slots of the selected values: characters from byte 0, length in byte 15."""
    out = bytearray()
    for row, idx in zip(x, sel):
        for c in idx:
            t = C.format_float_java(float(row[c])).encode()
            assert len(t) <= 15
            out += t + b"\0" * (15 - len(t)) + bytes([len(t)])
    return bytes(out)


@pytest.mark.parametrize("json_string", [False, True])
@pytest.mark.parametrize("classes,k", CASES)
def test_encode_topk_text_matches_the_float_encoder(classes, k, json_string):
    x = case_rows(classes, k)
    sel = topk_indices(x, k)
    got = C.encode_predictions_topk_text(slots_of(x, sel), sel, len(x), k, json_string)
    assert got == C.encode_predictions_topk(x, k, json_string)


def test_encode_topk_text_checks_its_sizes():
    x = softmax_rows(2, 10)
    sel = topk_indices(x, 3)
    with pytest.raises(ValueError):
        C.encode_predictions_topk_text(slots_of(x, sel)[:-16], sel, 2, 3, False)
    with pytest.raises(ValueError):
        C.encode_predictions_topk_text(slots_of(x, sel), sel[:1], 2, 3, False)


# ---- configuration -----------------------------------------------------------------------------

BASE = dict(topology_name="t", input_topic="in", output_topic="out")


def test_config_default_is_off():
    cfg = GaleConfig(**BASE).validate()
    assert cfg.top_k == 0
    assert cfg.engine_dict(H, W, CH, CLASSES)["top_k"] == 0
    assert from_sources(cli=dict(BASE, top_k=0), env={}).top_k == 0  # K = 0 is "off"


def test_config_three_sources(tmp_path):
    from gale.cli import parse_topology_args

    assert parse_topology_args(["t", "in", "out", "--top-k", "3"]).top_k == 3
    assert from_sources(cli=dict(BASE), env={"GALE_TOP_K": "4"}).top_k == 4
    toml = tmp_path / "gale.toml"
    toml.write_text('[gale]\ntop-k = 2\nmodel = "resnet50"\n')
    cfg = from_sources(cli=dict(BASE), env={}, toml_path=str(toml))
    assert cfg.top_k == 2 and cfg.model == "resnet50"
    # precedence: CLI > environment > TOML
    assert from_sources(cli=dict(BASE), env={"GALE_TOP_K": "4"}, toml_path=str(toml)).top_k == 4
    assert from_sources(cli=dict(BASE, top_k=5), env={"GALE_TOP_K": "4"},
                        toml_path=str(toml)).top_k == 5
    assert from_sources(cli=dict(BASE, top_k=3), env={}).engine_dict(
        H, W, CH, CLASSES)["top_k"] == 3


def test_config_help_names_the_option():
    from gale.cli import _topology_parser

    text = _topology_parser().format_help()
    assert "--top-k K" in text and "min(classes, 64)" in " ".join(text.split())


@pytest.mark.parametrize("model,k,upper", [("resnet20", -1, 10), ("resnet20", 11, 10),
                                           ("resnet50", 65, 64), ("lenet5", 64, 10)])
def test_config_refusals_name_both_bounds(model, k, upper):
    with pytest.raises(ValueError) as e:
        GaleConfig(model=model, top_k=k, **BASE).validate()
    assert "1 <= K" in str(e.value) and f"<= {upper}" in str(e.value)


def test_config_accepts_the_bounds():
    assert GaleConfig(model="resnet20", top_k=10, **BASE).validate().top_k == 10
    assert GaleConfig(model="resnet50", top_k=64, **BASE).validate().top_k == 64
    assert GaleConfig(model="resnet50", top_k=1, **BASE).validate().top_k == 1


def test_native_engine_refuses_bad_k():
    d = GaleConfig(**BASE).validate().engine_dict(H, W, CH, CLASSES)
    for k in (-1, 11, 65):
        with pytest.raises(ValueError):
            C.Engine(dict(d, top_k=k))


# ---- the stub engine, end to end ---------------------------------------------------------------

MAX_BATCH = 4
COUNTS = [1, 3, 2, 6, 1, 4, 2]  # the 6-image record is served as two fragments and joined


def serve(recs, **kw):
    broker = K.Broker()
    broker.start()
    try:
        broker.create_topic("in", 1)
        broker.create_topic("out", 1)
        for key, rec in recs:
            broker.append("in", 0, [rec], [key])
        cfg = GaleConfig(bootstrap=f"127.0.0.1:{broker.port}", start_offset="earliest",
                         stub=True, max_batch=MAX_BATCH, max_wait_us=500, queue_depth=64,
                         output_key="input", **BASE, **kw).validate()
        eng = Engine(cfg, max_records=len(recs))
        eng.start()
        assert eng.wait(30), eng.stats()
        eng.stop()
        out = broker.read("out", 0)
    finally:
        broker.stop()
    assert len(out) == len(recs)  # one output record per input record
    return eng.stats(), {r["key"]: r["value"] for r in out}


@pytest.fixture(scope="module")
def stub_records():
    rng = np.random.default_rng(3)
    recs = []
    for i, n in enumerate(COUNTS):
        x = rng.random((n, H, W, CH), dtype=np.float32)
        recs.append((f"r{i}".encode(), C.encode_instances(x)))
    recs.insert(2, (b"bad", b'{"instances": [[1,2]], "extra": 0}'))
    return recs


@pytest.fixture(scope="module")
def full_rows(stub_records):
    """The same records served with top_k = 0 (error-json): the rows the top-k runs select from."""
    st, by_key = serve(stub_records, on_error="error-json")
    assert st["errors"] == 1 and st["split_records"] == 1
    return by_key


def rows_of(value, json_string=False):
    doc = json.loads(value)
    if json_string:
        doc = json.loads(doc)
    return np.array(doc["predictions"], dtype=np.float32)


@pytest.mark.parametrize("kw", [dict(top_k=3), dict(top_k=1), dict(top_k=10),
                                dict(top_k=3, value_format="json-string"),
                                dict(top_k=3, float_format="java8")],
                         ids=["k3", "k1", "k10", "k3-json-string", "k3-java8"])
def test_stub_engine_outputs_are_the_topk_of_the_full_rows(stub_records, full_rows, kw):
    st, by_key = serve(stub_records, on_error="error-json", **kw)
    assert st["errors"] == 1 and st["split_records"] == 1
    assert st["images_out"] == sum(COUNTS)
    assert set(by_key) == set(full_rows)
    js = kw.get("value_format") == "json-string"
    for (key, _), n in zip([r for r in stub_records if r[0] != b"bad"], COUNTS):
        rows = rows_of(full_rows[key])  # (jdk19 text round-trips to the same binary32)
        assert rows.shape == (n, CLASSES)
        want = topk_document(rows, kw["top_k"], json_string=js,
                             java8=kw.get("float_format") == "java8")
        assert by_key[key] == want, key
    # the malformed record's output is what it is without top-k
    if js:
        assert json.loads(json.loads(by_key[b"bad"]))["error"] == "unknown_key"
    else:
        assert by_key[b"bad"] == full_rows[b"bad"]


def test_stub_engine_null_policy_unchanged(stub_records):
    _, by_key = serve(stub_records, on_error="null", top_k=3)
    assert by_key[b"bad"] is None
    assert sum(v is not None for v in by_key.values()) == len(COUNTS)
