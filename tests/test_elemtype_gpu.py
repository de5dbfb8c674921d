"""Typed tensor records (--input-dtype u16 | f16 | bf16 | f32) on the GPU: the
b64_typed_instances kernel bit for bit against the numpy oracle
(gale.models.preprocess.ElemType) on every 16-bit pattern, on f32 patterns and on small shapes in
every launch form, its bounds, verdicts and launcher refusals, and the engine end to end on every
step launch site against a json topology fed the same values as text (f16, f32) and against the
u8 b64 topology (u16). Every comparison is on the bits; the data is finite except in the verdict
tests."""

import base64
import logging

import numpy as np
import pytest
import torch

from gale import ops
from gale._native import native
from gale.config import GaleConfig
from gale.data import encode_records, encode_records_b64, encode_records_typed
from gale.engine import Engine
from gale.models import get_model, init_params
from gale.models.preprocess import ElemType, InputPrep
from gale.models.reference import calibrate_bn

pytestmark = pytest.mark.gpu

C = native()
K = C.kafka
IMG = np.dtype([("off", "<i8"), ("slot", "<i4"), ("rec", "<i4")])
assert IMG.itemsize == C.B64_IMAGE_BYTES

CIFAR_MEAN_S = "0.4914,0.4822,0.4465"
CIFAR_STD_S = "0.2470,0.2435,0.2616"
# (the float32 after -7: no u16, f16 or bf16 value, and no prep here maps one onto it)
SENTINEL = float(np.float32(-7.0000005))
TYPED = ("u16", "f16", "bf16", "f32")
N = 16          # images per launch: image i starts at phase i modulo 16
CHUNK_CHARS = 4096
PREPS = {1: InputPrep.build(1, 1 / 255, "0.1307", "0.3081"),
         3: InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S),    # (differs per channel)
         5: InputPrep.build(5, 1 / 255, "0.5", "0.25")}               # (general C: uniform)
NONFINITE = {"f16": (0x7C00, 0xFC00, 0x7E00, 0x7C01), "bf16": (0x7F80, 0xFF80, 0x7FC0, 0x7F81),
             "f32": (0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001)}   # +Inf -Inf qNaN NaN(bit 0)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def all_u16_patterns(t):
    """The 65 536 patterns as wire bytes, the non-finite ones replaced with 0."""
    p = np.arange(65536, dtype="<u2")
    p[ElemType(t).nonfinite(p.view(np.uint8))] = 0
    return p.view(np.uint8)


def f32_patterns(n, seed):
    """n finite f32 patterns as wire bytes: random, then -0, the least subnormal, the largest."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype("<u4")
    p[(p & 0x7F800000) == 0x7F800000] &= 0xBFFFFFFF
    special = [0x80000000, 0x00000001, 0x7F7FFFFF, 0x807FFFFF]
    p[:4] = special[:len(p[:4])]
    p[-1] = 0x00000001 if n > 1 else p[-1]
    return p.view(np.uint8)


_wire = {}


def wire(t, shape, n=N):
    """n random finite images of the type, wire bytes uint8 [n, B]; computed once."""
    key = (t, shape, n)
    if key not in _wire:
        per = shape[0] * shape[1] * shape[2]
        seed = per * 31 + TYPED.index(t)
        if t == "f32":
            w = f32_patterns(n * per, seed).reshape(n, -1).copy()
        else:
            idx = np.random.default_rng(seed).integers(0, 65536, n * per)
            w = all_u16_patterns(t).reshape(-1, 2)[idx].reshape(n, -1).copy()
        w.setflags(write=False)
        _wire[key] = w
    return _wire[key]


_oracle = {}


def oracle(t, shape, prep=None, n=N):
    """float32 [n, HS, WS, C] model inputs of wire(t, shape, n); computed once per prep."""
    key = (t, shape, n, prep)
    if key not in _oracle:
        w = wire(t, shape, n)
        if prep is not None and prep.nchw:   # (the same elements, sent [C][H][W])
            w = nchw_wire(t, shape, n)
        _oracle[key] = ElemType(t).apply(w, *shape, prep)
        _oracle[key].setflags(write=False)
    return _oracle[key]


def nchw_wire(t, shape, n=N):
    HS, WS, CH = shape
    E = ElemType(t).bytes_per_element
    w = wire(t, shape, n).reshape(n, HS, WS, CH, E)
    return np.ascontiguousarray(w.transpose(0, 3, 1, 2, 4)).reshape(n, -1)


def stage(strings, phases):
    """The strings in one byte buffer, string i starting at phase phases[i] modulo 16, each
    followed by the text a record has there, and 16 bytes of slack at the end."""
    buf = bytearray(b'{"instances":[{"')
    offs = []
    for s, ph in zip(strings, phases):
        buf += b'"b64":"'
        while len(buf) % 16 != ph:
            buf += b" "
        offs.append(len(buf))
        buf += s + b'"},{'
    buf += b"\xee" * 16
    return np.frombuffer(bytes(buf), dtype=np.uint8), offs


def strings_of(w):
    return [base64.b64encode(im.tobytes()) for im in w]


class Staged:
    """Strings on the device with their descriptor table: string i -> slot slots[i], record
    recs[i]."""

    def __init__(self, strings, phases, slots, recs):
        raw, offs = stage(strings, phases)
        tab = np.zeros(len(strings), dtype=IMG)
        tab["off"], tab["slot"], tab["rec"] = offs, slots, recs
        self.raw = torch.from_numpy(raw.copy()).cuda()
        self.tab = torch.from_numpy(tab.view(np.int32).reshape(-1, 4).copy()).cuda()
        self.n = len(strings)


def run(st, shape, t, nslots, nrec, prep=None, header=None, misalign=False):
    """(floats [nslots, HS, WS, C], statuses [nrec]). header: the device-count form with that
    count. misalign: the output starts 4 bytes past a 16-byte boundary (the scalar store path of
    the 16-bit types). The guard floats before the first slot and after the last one are checked
    to be untouched."""
    per = shape[0] * shape[1] * shape[2]
    flat = torch.full((nslots * per + 8,), SENTINEL, device="cuda")
    lead = 5 if misalign else 4
    out = flat[lead:lead + nslots * per]
    assert out.data_ptr() % 16 == (4 if misalign else 0)
    status = torch.zeros(nrec, dtype=torch.int32, device="cuda")
    hdr = torch.tensor([header], dtype=torch.int32, device="cuda") if header is not None else None
    ops.b64_typed_instances(st.raw, st.tab, shape, out, status, ElemType(t), d_images=hdr,
                            prep=prep)
    torch.cuda.synchronize()
    f = flat.cpu().numpy()
    assert (f[:lead] == SENTINEL).all() and (f[lead + nslots * per:] == SENTINEL).all()
    return f[lead:lead + nslots * per].reshape(nslots, *shape), status.cpu().numpy()


ODD = [2 * i + 1 for i in range(N)]   # image i in slot 2 i + 1: the even slots stay sentinel


# ---- 1. every 16-bit pattern; f32 patterns ------------------------------------------------------

@pytest.mark.parametrize("t", ["u16", "f16", "bf16"])
def test_every_16_bit_pattern(t):
    """All 65 536 patterns (the non-finite ones zeroed) as 16 images of 64x64x1, image i at start
    phase i, without and with a prep: the oracle's bits. f16 subnormals convert exactly."""
    shape = (64, 64, 1)
    w = all_u16_patterns(t).reshape(N, -1)
    st = Staged(strings_of(w), range(N), ODD, [i // 4 for i in range(N)])
    for prep in (None, PREPS[1]):
        want = ElemType(t).apply(w, *shape, prep)
        got, status = run(st, shape, t, 2 * N + 1, 4, prep=prep)
        assert list(status) == [0] * 4, (t, prep is not None)
        assert np.array_equal(bits(got[1::2]), bits(want)), (t, prep is not None)
        assert (got[0::2] == SENTINEL).all()
    if t == "f16":
        sub = ElemType(t).apply(w, *shape).ravel()[1:0x400]
        assert (sub > 0).all() and sub[0] == 2.0 ** -24


@pytest.mark.parametrize("shape", [(32, 32, 3), (33, 31, 3)])
def test_f32_patterns(shape):
    """Random finite patterns with -0, subnormals and the largest finite value: 32x32x3 is exactly
    4 chunks, 33x31x3 leaves a partial last wave and chunk. Without a prep the bits are the
    string's; with the CIFAR prep the oracle's fma."""
    per = shape[0] * shape[1] * shape[2]
    L = 4 * ((4 * per + 2) // 3)
    if shape == (32, 32, 3):
        assert L == 4 * CHUNK_CHARS
    else:
        assert L % CHUNK_CHARS != 0 and -(-L // CHUNK_CHARS) == 4 and (L // 16) % 64 != 0
    w = wire("f32", shape)
    st = Staged(strings_of(w), range(N), ODD, [i // 4 for i in range(N)])
    for misalign in (False, True):
        got, status = run(st, shape, "f32", 2 * N + 1, 4, misalign=misalign)
        assert list(status) == [0] * 4
        assert np.array_equal(bits(got[1::2]).reshape(N, -1), w.view("<u4"))
        assert (got[0::2] == SENTINEL).all()
    got, status = run(st, shape, "f32", 2 * N + 1, 4, prep=PREPS[3])
    assert list(status) == [0] * 4
    assert np.array_equal(bits(got[1::2]), bits(oracle("f32", shape, PREPS[3])))


# ---- 2. small shapes, every launch form ---------------------------------------------------------

SHAPES = [(1, 1, 1), (1, 2, 1), (5, 7, 1), (5, 7, 3), (5, 7, 5), (32, 32, 3)]


@pytest.mark.parametrize("t", TYPED)
@pytest.mark.parametrize("shape", SHAPES)
def test_launch_forms(shape, t):
    """Image i at start phase i modulo 16 (all 16 phases) in slot 2 i + 1. Without and with the
    prep, on an aligned and on a 16-byte-misaligned output base (the scalar store path), with the
    nchw prep, and in the device-count form with a count below the images: the oracle's bits, the
    slots in between, the slots past the count and the guards around the tensor untouched."""
    CH = shape[2]
    w = wire(t, shape)
    st = Staged(strings_of(w), range(N), ODD, [i // 4 for i in range(N)])
    for prep in (None, PREPS[CH]):
        want = bits(oracle(t, shape, prep))
        for misalign in (False, True):
            for header in (None, N):
                got, status = run(st, shape, t, 2 * N + 1, 4, prep=prep, header=header,
                                  misalign=misalign)
                what = (shape, t, prep is not None, misalign, header)
                assert list(status) == [0] * 4, what
                assert np.array_equal(bits(got[1::2]), want), what
                assert (got[0::2] == SENTINEL).all(), what
    # [C][H][W]-ordered strings, transposed at the store
    a = PREPS[CH]
    nchw = InputPrep.build(CH, a.scale, [0.5] if CH > 4 else [0.1 * (c + 1) for c in range(CH)],
                           [0.25], layout="nchw")
    sn = Staged(strings_of(nchw_wire(t, shape)), range(N), ODD, [0] * N)
    for misalign in (False, True):
        got, status = run(sn, shape, t, 2 * N + 1, 1, prep=nchw, misalign=misalign)
        assert list(status) == [0]
        assert np.array_equal(bits(got[1::2]), bits(oracle(t, shape, nchw))), (shape, t, "nchw")
        assert (got[0::2] == SENTINEL).all()
    # a device count of N - 3: the last three descriptors' slots stay sentinel; 0 writes nothing
    want = bits(oracle(t, shape, PREPS[CH]))
    for misalign in (False, True):
        got, status = run(st, shape, t, 2 * N + 1, 4, prep=PREPS[CH], header=N - 3,
                          misalign=misalign)
        assert list(status) == [0] * 4
        assert np.array_equal(bits(got[1:2 * (N - 3):2]), want[:N - 3]), (shape, t, misalign)
        assert (got[0::2] == SENTINEL).all() and (got[2 * (N - 3) + 1:] == SENTINEL).all()
    got, status = run(st, shape, t, 2 * N + 1, 4, header=0)
    assert (got == SENTINEL).all() and list(status) == [0] * 4


# ---- 3. verdicts --------------------------------------------------------------------------------

def plant(s: bytes, at: int, what: bytes) -> bytes:
    return s[:at] + what + s[at + len(what):]


@pytest.mark.parametrize("header", [None, "count"])
@pytest.mark.parametrize("t", TYPED)
@pytest.mark.parametrize("shape", [(5, 7, 1), (32, 31, 1)])
def test_verdicts(shape, t, header):
    """Records of two images, one plant each; the first and the last record are clean. Characters:
    a bad byte and a '=' in the first, a middle and the last window of a string, and a data
    character in every '=' position (both shapes pad: 2 characters for E = 2, 1 for E = 4;
    32x31x1 as f32 has a second chunk). Elements: each non-finite class at the first and the last
    element of the first and the last image of a record. Every image is written, inside its own
    slot."""
    e = ElemType(t)
    E, per = e.bytes_per_element, shape[0] * shape[1] * shape[2]
    B = per * E
    L, pad = 4 * ((B + 2) // 3), (3 - B % 3) % 3
    assert pad == (2 if E == 2 else 1) and L > 5 * 16
    mid = 16 * (L // 32) + 5
    assert 16 <= mid < L - 16
    plants = [None]
    for at in (0, mid, L - pad - 1):
        plants += [("char", at, b"-"), ("char", at, b"=")]
    plants += [("char", L - 1 - k, b"A") for k in range(pad)]
    for pattern in NONFINITE.get(t, ()):
        for img in (0, 1):
            for el in (0, per - 1):
                plants.append(("elem", img, el, pattern))
    plants.append(None)
    nrec = len(plants)
    base = wire(t, shape, 2)
    images, want_status = [], []
    for p in plants:
        w = base.copy()
        strings = strings_of(w)
        if p is not None and p[0] == "char":
            strings[1] = plant(strings[1], p[1], p[2])
        elif p is not None:
            _, img, el, pattern = p
            w[img, el * E:(el + 1) * E] = np.frombuffer(int(pattern).to_bytes(E, "little"),
                                                        np.uint8)
            strings = strings_of(w)
        images += strings
        want_status.append(0 if p is None else 2)
    n = 2 * nrec
    st = Staged(images, [(7 * i + 1) % 16 for i in range(n)], [2 * i + 1 for i in range(n)],
                [i // 2 for i in range(n)])
    got, status = run(st, shape, t, 2 * n + 1, nrec, header=n if header else None)
    assert list(status) == want_status
    want = oracle(t, shape, None, 2)
    assert (got[0::2] == SENTINEL).all()          # every image stayed inside its own slot ...
    for r, p in enumerate(plants):
        a, b = got[4 * r + 1], got[4 * r + 3]
        if p is None or p[0] == "char":           # (the untouched first image of the record)
            assert np.array_equal(bits(a), bits(want[0])), r
        if p is None:
            assert np.array_equal(bits(b), bits(want[1])), r
        elif p[0] == "elem":                      # ... and was written: all but the planted one
            _, img, el, pattern = p
            both = np.stack([a, b]).reshape(2, -1)
            keep = np.ones((2, per), bool)
            keep[img, el] = False
            assert np.array_equal(bits(both)[keep], bits(want).reshape(2, -1)[keep]), r
            assert not np.isfinite(both[img, el]), r
        else:                                     # a bad character far from the first element
            if p[1] >= 16:
                assert bits(b).ravel()[0] == bits(want[1]).ravel()[0], r
            assert (np.isnan(b) | (b != SENTINEL)).all(), r


# ---- 4. launcher refusals -----------------------------------------------------------------------

def test_launcher_refusals():
    shape = (5, 7, 5)
    st = Staged(strings_of(wire("bf16", shape)), range(N), range(N), range(N))
    out = torch.full((N,) + shape, SENTINEL, device="cuda")
    status = torch.zeros(N, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def launch(images=N, imgs=None, raw=None, size=shape, o=None, s=None, dtype="bf16", **kw):
        return C.b64_typed_instances(images, st.tab.data_ptr() if imgs is None else imgs,
                                     st.raw.data_ptr() if raw is None else raw, size[0], size[1],
                                     size[2], out.data_ptr() if o is None else o,
                                     status.data_ptr() if s is None else s, stream, dtype=dtype,
                                     **kw)

    bad = C.HIP_ERROR_INVALID_VALUE
    assert launch(size=(0, 7, 5)) == bad and launch(size=(5, -2, 5)) == bad   # non-positive sizes
    assert launch(size=(5, 7, 0)) == bad
    assert launch(imgs=0) == bad and launch(raw=0) == bad and launch(o=0) == bad  # null pointers
    assert launch(s=0) == bad
    for d in ("u8", "f64", "F16", "half", ""):                                # an unknown type
        assert launch(dtype=d) == bad
    assert launch(images=65536) == bad
    assert launch(size=(16384, 16384, 5)) == bad                              # > 2^30 floats
    per_channel = dict(a=[0.5, 0.5, 0.5, 0.25], b=[0.0] * 4)
    assert launch(**per_channel) == bad                                       # C = 5, non-uniform
    assert launch(images=0) == 0 and launch(images=0, **per_channel) == bad
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item() and not status.any().item()         # nothing launched
    with pytest.raises(ValueError, match="refused"):
        ops.b64_typed_instances(st.raw, st.tab, (0, 7, 5), out, status, ElemType("bf16"))
    with pytest.raises(ValueError, match="refused"):
        ops.b64_typed_instances(st.raw, st.tab, shape, out, status, ElemType("u8"))
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item() and not status.any().item()
    assert launch(a=[0.5] * 4, b=[1.0] * 4) == 0                              # uniform: served
    torch.cuda.synchronize()
    want = ElemType("bf16").apply(wire("bf16", shape), *shape,
                                  InputPrep(5, (0.5,) * 5, (1.0,) * 5))
    assert np.array_equal(bits(out.cpu().numpy()), bits(want)) and not status.any().item()


# ---- 5. the engine ------------------------------------------------------------------------------

COUNTS = [1, 2, 1, 3, 4, 1]
PREP_KW = dict(input_scale=1 / 255, input_mean=CIFAR_MEAN_S, input_std=CIFAR_STD_S)
SITES = {"direct": {}, "plain": dict(graph_step=False), "graph": dict(step_launch="graph"),
         "graph-noencode": dict(step_launch="graph", gpu_encode=False)}


def serve(recs, params, model="resnet20", max_batch=32, **kw):
    broker = K.Broker()
    broker.start()
    try:
        broker.create_topic("in", 1)
        broker.create_topic("out", 1)
        for key, rec in recs:
            broker.append("in", 0, [rec], [key])
        cfg = GaleConfig(topology_name="g", input_topic="in", output_topic="out", model=model,
                         dtype="bf16", bootstrap=f"127.0.0.1:{broker.port}",
                         start_offset="earliest", max_batch=max_batch, max_wait_us=500,
                         output_key="input", on_error="null", **kw)
        eng = Engine(cfg.validate(), devices=[0], max_records=len(recs), params=params)
        eng.start()
        assert eng.wait(120), eng.stats()
        eng.stop()
        out = broker.read("out", 0)
    finally:
        broker.stop()
    assert len(out) == len(recs)
    return eng.stats(), {r["key"]: r["value"] for r in out}


def unit_scale_params(model, prep):
    net = get_model(model)
    params = init_params(net, seed=0, calibrate=False)
    rng = np.random.default_rng(77)
    x = rng.integers(0, 256, (16,) + tuple(net.input_shape)).astype(np.float32)
    calibrate_bn(net, params, torch.from_numpy(prep.apply(x)))
    return params


def value_sets(shape, seed):
    """key -> float32 [n, H, W, C]: pixels with three fraction bits, exact in f16, bf16 would not
    be."""
    rng = np.random.default_rng(seed)
    return {f"r{i}".encode(): (rng.integers(0, 2048, (n,) + tuple(shape)) / 8).astype(np.float32)
            for i, n in enumerate(COUNTS)}


def typed_records(sets, t, bad=True):
    """The sets as typed records, then a record with an Inf element and one with a bad
    character (u16: the bad character only)."""
    recs = [(k, encode_records_typed(x, t, x.shape[0])[0]) for k, x in sets.items()]
    extra = []
    if bad:
        rec = bytearray(recs[1][1])
        at = bytes(rec).rindex(b'"b64":"') + 7 + 100
        rec[at:at + 1] = b"-"
        extra.append((b"badchar", bytes(rec)))
        if t != "u16":
            e = ElemType(t)
            x = sets[b"r3"]
            w = e.to_wire(x).reshape(x.shape[0], -1).copy()
            inf = int(NONFINITE[t][0]).to_bytes(e.bytes_per_element, "little")
            w[-1, -e.bytes_per_element:] = np.frombuffer(inf, np.uint8)   # the very last element
            extra.append((b"inf", b'{"instances":[' + b",".join(
                b'{"b64":"' + base64.b64encode(im.tobytes()) + b'"}' for im in w) + b"]}"))
    return recs + extra


@pytest.fixture(scope="module")
def r20():
    """The weights, the value sets and the two reference runs, computed once: a json topology fed
    the values as text (exact: Float.toString round-trips), and the u8 b64 topology."""
    params = unit_scale_params("resnet20", PREPS[3])
    shape = get_model("resnet20").input_shape
    sets = value_sets(shape, 71)
    # (for f32 a 2^-12 fraction on top, which f16 cannot hold)
    f32sets = {k: (x + np.float32(2.0 ** -12)).astype(np.float32) for k, x in sets.items()}
    assert all((x != sets[k]).all() for k, x in f32sets.items())
    u8sets = {k: np.floor(x).astype(np.uint8) for k, x in sets.items()}

    def text(s):
        return [(k, encode_records(x, x.shape[0])[0]) for k, x in s.items()]

    ref = {}
    for name, s in (("f16", sets), ("f32", f32sets)):
        st, ref[name] = serve(text(s), params, input_format="json", gpu_ingest=False, **PREP_KW)
        assert st["errors"] == 0 and all(v is not None for v in ref[name].values())
    st, ref["u16"] = serve([(k, encode_records_b64(x, x.shape[0])[0]) for k, x in u8sets.items()],
                           params, input_format="b64", **PREP_KW)
    assert st["errors"] == 0 and st["typed_records"] == 0
    return dict(params=params, sets={"f16": sets, "f32": f32sets,
                                     "u16": {k: x.astype(np.float32) for k, x in u8sets.items()}},
                ref=ref)


def check_typed(got, stats, want, t, nsets=len(COUNTS)):
    nbad = 1 if t == "u16" else 2
    assert got.pop(b"badchar") is None
    if t != "u16":
        assert got.pop(b"inf") is None
    assert got == want
    assert stats["typed_records"] == nsets + nbad == stats["b64_records"], stats
    assert stats["yuv_records"] == 0 == stats["packed_records"], stats
    assert stats["errors"] == nbad and stats["images_out"] == sum(COUNTS), stats


@pytest.mark.parametrize("t", ["f16", "f32", "u16"])
@pytest.mark.parametrize("site", list(SITES))
def test_engine_every_step_site(r20, site, t):
    """Op by op, the direct launch and both captured graphs: f16 and f32 records give, key by
    key, the bytes of the json topology fed the same values as text; u16 records of 0..255 the
    bytes of the u8 b64 topology. The record with an Inf element and the one with a bad character
    are errors and their neighbours are served."""
    stats, got = serve(typed_records(r20["sets"][t], t), r20["params"], input_format="b64",
                       input_dtype=t, **PREP_KW, **SITES[site])
    check_typed(got, stats, r20["ref"][t], t)
    assert (stats["graph_step_batches"] > 0) == (site != "plain"), stats
    assert stats["ingested_records"] == 0, stats


def test_engine_with_input_resize(r20):
    """--input-size 40,36: the decode writes the resize's source tensor."""
    sets = value_sets((40, 36, 3), 72)
    kw = dict(PREP_KW, input_size="40,36", input_antialias=False)
    text = [(k, encode_records(x, x.shape[0])[0]) for k, x in sets.items()]
    _, want = serve(text, r20["params"], input_format="json", gpu_ingest=False, **kw)
    stats, got = serve(typed_records(sets, "f16"), r20["params"], input_format="b64",
                       input_dtype="f16", **kw)
    check_typed(got, stats, want, "f16")
    # (the two bad records went through the step too: their images are written)
    assert stats["resized_images"] == sum(COUNTS) + COUNTS[1] + COUNTS[3], stats


def test_engine_max_batch_smaller_than_a_record(r20):
    """--max-batch 3: the record of 4 images is split by the byte-count splitter and joined."""
    stats, got = serve(typed_records(r20["sets"]["f32"], "f32"), r20["params"], max_batch=3,
                       input_format="b64", input_dtype="f32", **PREP_KW)
    check_typed(got, stats, r20["ref"]["f32"], "f32")
    assert stats["split_records"] == COUNTS.count(4), stats


def test_engine_b64_ingest_is_crc_only(r20, caplog):
    with caplog.at_level(logging.INFO, logger="gale.engine"):
        stats, got = serve(typed_records(r20["sets"]["f16"], "f16"), r20["params"],
                           input_format="b64", input_dtype="f16", b64_ingest=True, **PREP_KW)
    lines = [r.getMessage() for r in caplog.records if "CRC-only" in r.getMessage()]
    assert len(lines) == 1 and "f16" in lines[0], caplog.text
    check_typed(got, stats, r20["ref"]["f16"], "f16")
    assert stats["ingested_records"] == len(COUNTS) + 2, stats
    assert stats["ingest_parsed_records"] == 0, stats


def test_engine_lenet5_f16():
    """C = 1: LeNet-5 is served with f16 records, the bytes of the json topology."""
    kw = dict(input_scale=1 / 255, input_mean="0.1307", input_std="0.3081")
    params = unit_scale_params("lenet5", PREPS[1])
    sets = value_sets(get_model("lenet5").input_shape, 73)
    text = [(k, encode_records(x, x.shape[0])[0]) for k, x in sets.items()]
    _, want = serve(text, params, model="lenet5", input_format="json", gpu_ingest=False, **kw)
    stats, got = serve(typed_records(sets, "f16"), params, model="lenet5", input_format="b64",
                       input_dtype="f16", **kw)
    check_typed(got, stats, want, "f16")
    assert all(v is not None for v in want.values())
