"""Raw binary records (--input-format raw) on the host: scan, parser and splitter against the
oracles and the status table, the refusals, and a stub-replica run against b64 records."""

import numpy as np
import pytest

from gale._native import native
from gale.config import GaleConfig
from gale.data import encode_records_b64, encode_records_raw
from gale.engine import Engine
from gale.models.preprocess import ElemType, PixelUnpack

C = native()
OK, BAD_SHAPE, EMPTY, BAD_NUMBER = 0, 3, 4, 5
ELEMS = ("u8", "u16", "f16", "bf16", "f32")
PACKED = ("bgr24", "rgba", "bgra", "gray")
CIFAR = dict(input_scale=1 / 255, input_mean="0.4914,0.4822,0.4465",
             input_std="0.2470,0.2435,0.2616")


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def finite_wire(kind, shape, seed, n=3):
    """uint8 [n, B]: random images of the kind with the top exponent bit of every float element
    cleared (no Inf, no NaN); f32 images start with -0, the least subnormal, and the largest and
    smallest normals."""
    B = PixelUnpack(kind).frame_bytes(*shape[:2]) if kind in PACKED \
        else ElemType(kind).frame_bytes(*shape)
    wire = np.random.default_rng(seed).integers(0, 256, (n, B), dtype=np.uint8)
    if kind in ("f16", "bf16", "f32"):
        E = ElemType(kind).bytes_per_element
        wire.reshape(n, -1, E)[..., E - 1] &= 0xBF
    if kind == "f32":
        v = wire.view("<u4")
        v[:, :4] = np.array([0x80000000, 1, 0x7F7FFFFF, 0x00800000], "<u4")[:v.shape[1]]
    return wire


def oracle(kind, wire, HS, WS, CH, prep=None):
    if kind in PACKED:
        x = PixelUnpack(kind).apply(wire, HS, WS).astype(np.float32)
        return x if prep is None else prep.apply(x)
    return ElemType(kind).apply(wire, HS, WS, CH, prep)


@pytest.mark.parametrize("kind", ELEMS + PACKED)
def test_scan_parser_and_splitter(kind):
    """The oracle's bits, and the status table: empty, bad_shape, bad_number."""
    H, W, CH = 5, 7, 3
    wire = finite_wire(kind, (H, W, CH), 3)
    B, rec = wire.shape[1], wire.tobytes()
    kw = dict(format=kind) if kind in PACKED else dict(dtype=kind)
    assert C.scan_instances_raw(3 * B, B) == (OK, 0, 3 * B, 3)
    assert C.scan_instances_raw(0, B)[0] == EMPTY and C.scan_instances_raw(3 * B - 1, B)[0] == BAD_SHAPE
    assert C.split_instances_raw(3 * B, B, 2) == [(0, 2 * B), (2 * B, 3 * B)]
    st, got = C.parse_instances_raw_host(rec, H, W, CH, **kw)
    assert st == OK and np.array_equal(bits(got.reshape(3, H, W, CH)),
                                       bits(oracle(kind, wire, H, W, CH)))
    assert C.parse_instances_raw_host(b"", H, W, CH, **kw)[0] == EMPTY
    assert C.parse_instances_raw_host(rec[:-1], H, W, CH, **kw)[0] == BAD_SHAPE
    if kind in ("f16", "bf16", "f32"):          # Inf in the last element of the last image
        inf = {"f16": b"\x00\x7c", "bf16": b"\x80\x7f", "f32": b"\x00\x00\x80\x7f"}[kind]
        assert C.parse_instances_raw_host(rec[:-len(inf)] + inf, H, W, CH, **kw)[0] == BAD_NUMBER


def test_configuration_refusals_name_the_option():
    base = dict(topology_name="t", input_format="raw")
    for t in ELEMS:
        GaleConfig(input_dtype=t, input_layout="nchw", input_scale=0.5, **base).validate()
    for pf in PACKED:
        GaleConfig(input_pixel_format=pf, **base).validate()
    refused = [(dict(input_pixel_format="bgra", input_layout="nchw"), "--input-layout nchw"),
               (dict(input_pixel_format="gray", input_dtype="f16"),
                "--input-dtype f16.*--input-pixel-format rgb"),
               (dict(input_pixel_format="nv12"), "--input-pixel-format nv12.*--input-format raw"),
               (dict(b64_ingest=True), "--b64-ingest needs --input-format b64"),
               (dict(input_pixel_format="gray", model="lenet5"), "gray gives 3-channel RGB"),
               # the refusals with json keep their text
               (dict(input_format="json", input_dtype="f16"),
                "--input-dtype f16 needs --input-format b64"),
               (dict(input_format="json", input_pixel_format="rgba"),
                "--input-pixel-format rgba needs --input-format b64")]
    for kw, text in refused:
        with pytest.raises(ValueError, match=text):
            GaleConfig(**dict(base, **kw)).validate()


def test_native_engine_refuses_the_same_combinations():
    d = GaleConfig(topology_name="t", input_topic="in", output_topic="out",
                   input_format="raw").validate().engine_dict(4, 3, 3, 10)
    C.Engine(dict(d, input_dtype="f16"))
    C.Engine(dict(d, pixel_format="bgra"))
    refused = [(dict(input_format="bin"), "input_format: json, b64 or raw"),
               (dict(pixel_format="nv12"), "input_format raw: no pixel_format i420 / nv12"),
               (dict(b64_ingest=True), "b64_ingest needs input_format b64"),
               (dict(input_dtype="bf16", pixel_format="gray"), "needs pixel_format rgb"),
               (dict(C=1, pixel_format="gray"), "needs a 3-channel model"),
               (dict(pixel_format="rgba", input_nchw=True), "no nchw layout"),
               (dict(C=5, input_a=[0.5, 0.5, 0.5, 0.25], input_b=[0.0] * 4), "C <= 4")]
    for kw, text in refused:
        with pytest.raises(ValueError, match=text):
            C.Engine(dict(d, **kw))
    with pytest.raises(ValueError, match="enable_gpu_ingest: input_format raw"):
        C.Engine(d).enable_gpu_ingest(0)


def serve(recs, params=None, **kw):
    """(key -> output value, stats) of a topology fed recs [(key, value)]: stub replicas when
    params is None, else the GPU engine with those weights."""
    broker = C.kafka.Broker()
    broker.start()
    try:
        broker.create_topic("in", 1)
        broker.create_topic("out", 1)
        for key, rec in recs:
            broker.append("in", 0, [rec], [key])
        cfg = GaleConfig(topology_name="t", input_topic="in", output_topic="out",
                         bootstrap=f"127.0.0.1:{broker.port}", start_offset="earliest",
                         max_wait_us=500, output_key="input", stub=params is None, **kw)
        eng = Engine(cfg.validate(), devices=[0], max_records=len(recs), params=params)
        eng.start()
        assert eng.wait(120), eng.stats()
        eng.stop()
        out = broker.read("out", 0)
    finally:
        broker.stop()
    assert len(out) == len(recs)
    return {r["key"]: r["value"] for r in out}, eng.stats()


def pixel_sets(shape, counts, seed):
    rng = np.random.default_rng(seed)
    return {f"r{i}".encode(): rng.integers(0, 256, (n,) + tuple(shape), dtype=np.uint8)
            for i, n in enumerate(counts)}


def test_stub_engine_raw_equals_b64():
    """Predictions byte for byte those of the same pixels sent as b64 records; the record of 9
    images over --max-batch 4 joined into one output; a bad_shape record through error-json."""
    xs = pixel_sets((32, 32, 3), [1, 2, 3, 9, 1], 8)
    kw = dict(max_batch=4, on_error="error-json", **CIFAR)
    want, _ = serve([(k, encode_records_b64(x, x.shape[0])[0]) for k, x in xs.items()],
                    input_format="b64", **kw)
    raw = [(k, encode_records_raw(x, x.shape[0])[0]) for k, x in xs.items()]
    got, st = serve(raw + [(b"short", raw[2][1][:-1])], input_format="raw", **kw)
    assert b"bad_shape" in got.pop(b"short")
    assert got == want and got[b"r3"].count(b"],[") == 8
    assert (st["raw_records"], st["b64_records"], st["errors"], st["split_records"]) == \
        (len(xs), 0, 1, 1), st
