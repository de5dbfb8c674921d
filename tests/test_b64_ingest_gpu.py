"""Device ingest of base64 image records (--b64-ingest) on the GPU: the fused kernel
(ingest_crc_b64) bit for bit against numpy / InputPrep.apply at every start phase, its
per-workgroup verdicts, its CRC windows against crc32c_chunks and the host CRC32C, and the engine
end to end against the host-decode path of the same records."""

import base64
import json

import numpy as np
import pytest
import torch

from gale import ops
from gale._native import native
from gale.config import GaleConfig
from gale.data import encode_records_b64, encode_records_text
from gale.engine import Engine
from gale.models import fold_params, get_model, init_params
from gale.models.preprocess import InputPrep
from gale.models.reference import calibrate_bn, forward

pytestmark = pytest.mark.gpu

C = native()
K = C.kafka
IMG = np.dtype([("off", "<i8"), ("slot", "<i4"), ("rec", "<i4")])
WIN = np.dtype([("end", "<i8"), ("len", "<i4"), ("pad", "<i4")])
assert IMG.itemsize == C.B64_IMAGE_BYTES

CIFAR_MEAN_S = "0.4914,0.4822,0.4465"
CIFAR_STD_S = "0.2470,0.2435,0.2616"
SENTINEL = -7.0
CHUNK = C.B64_CHUNK_CHARS


def geometry(shape):
    per = int(np.prod(shape))
    return per, 4 * ((per + 2) // 3), (3 - per % 3) % 3


def chunks_of(shape):
    return -(-geometry(shape)[1] // CHUNK)


def b64_of(im) -> bytes:
    return base64.b64encode(np.ascontiguousarray(im).tobytes())


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


def dev_table(offs, slots):
    tab = np.zeros(len(offs), dtype=IMG)
    tab["off"], tab["slot"], tab["rec"] = offs, slots, -1     # (rec is not read)
    return torch.from_numpy(tab.view(np.int32).reshape(-1, 4).copy()).cuda()


def gpu_ingest(strings, phases, slots, shape, total, prep=None, bad_fill=7):
    """(arena [total, H, W, C] floats, wg_bad words): image i's string goes to slot slots[i]."""
    raw, offs = stage(strings, phases)
    arena = torch.full((total,) + tuple(shape), SENTINEL, device="cuda")
    wg_bad = torch.full((len(strings) * chunks_of(shape),), bad_fill, dtype=torch.int32,
                        device="cuda")
    ops.ingest_crc_b64(torch.from_numpy(raw.copy()).cuda(), shape, arena=arena,
                       table=dev_table(offs, slots), wg_bad=wg_bad, prep=prep)
    torch.cuda.synchronize()
    return arena.cpu().numpy(), wg_bad.cpu().numpy()


def prep_for(Cc, layout="nhwc"):
    if Cc == 3:
        return InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S, layout)
    return InputPrep.build(Cc, 1 / 255, "0.1307", "0.3081", layout)


def gapped_slots(n):
    """n distinct slots out of order, with gaps, in an arena of 2 n + 1 slots."""
    total = 2 * n + 1
    slots = [(7 * i + 3) % total for i in range(n)]
    assert len(set(slots)) == n and slots != sorted(slots)
    return slots, total


def check_arena(got, want_bits, slots, what):
    """Image i sits in slot slots[i], bit for bit; every other float is still the sentinel."""
    bits = got.view(np.uint32)
    for i, slot in enumerate(slots):
        bad = np.nonzero(bits[slot] != want_bits[i])
        assert bad[0].size == 0, (what, i, [(hex(bits[slot][j]), hex(want_bits[i][j]))
                                            for j in zip(*bad)][:4])
    rest = np.ones(got.shape[0], dtype=bool)
    rest[slots] = False
    assert (got[rest] == SENTINEL).all(), what


# ---- 1. the decode half against numpy -----------------------------------------------------------

SHAPES = [
    ((1, 1, 1), 16),       # L = 4, two '='
    ((1, 1, 3), 16),       # no padding, one lane
    ((28, 28, 1), 16),     # two '=', slot bases 16-byte aligned
    ((5, 5, 3), 16),       # 75 values: slot bases mostly not 16-byte aligned, per-lane stores
    ((32, 32, 3), 16),     # exactly one chunk
    ((33, 33, 3), 16),     # two chunks, the second with a 4-character last lane
    ((224, 224, 3), 2),    # 49 chunks
]


@pytest.fixture(scope="module")
def images():
    rng = np.random.default_rng(61)
    out = {}
    for shape, n in SHAPES:
        x = rng.integers(0, 256, (n,) + shape, dtype=np.uint8)
        x[0].flat[:4] = [0, 255, 1, 254][:x[0].size]
        out[shape] = x
    return out


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_decode_matches_numpy_at_every_phase(images, k):
    shape, n = SHAPES[k]
    per, L, pad = geometry(shape)
    x = images[shape]
    strings = [b64_of(im) for im in x]
    assert all(len(s) == L and s.count(b"=") == pad for s in strings)
    if shape == (33, 33, 3):
        assert chunks_of(shape) == 2 and (L - CHUNK) % 16 == 4
    if shape == (224, 224, 3):
        assert chunks_of(shape) == 49
    if shape == (32, 32, 3):
        assert L == CHUNK
    slots, total = gapped_slots(n)
    if shape == (28, 28, 1):
        assert all((s * per * 4) % 16 == 0 for s in slots)
    if shape == (5, 5, 3):
        assert any((s * per * 4) % 16 != 0 for s in slots)
    want = x.astype(np.float32).view(np.uint32)
    # n images per launch, image i at phase (first + i) % 16: all 16 phases over the launches
    for first in range(0, 16, n):
        phases = [(first + i) % 16 for i in range(n)]
        got, bad = gpu_ingest(strings, phases, slots, shape, total)
        assert (bad == 0).all(), (shape, first)
        check_arena(got, want, slots, (shape, first))


@pytest.mark.parametrize("variant", ["c3", "c1", "nchw"])
def test_decode_prep_variants(images, variant):
    shape = {"c3": (33, 33, 3), "c1": (28, 28, 1), "nchw": (5, 5, 3)}[variant]
    x = images[shape]
    n = x.shape[0]
    prep = prep_for(shape[2], "nchw" if variant == "nchw" else "nhwc")
    want = prep.apply(x.astype(np.float32)).view(np.uint32)      # (NHWC values either way)
    src = x.transpose(0, 3, 1, 2) if variant == "nchw" else x
    strings = [b64_of(im) for im in src]
    slots, total = gapped_slots(n)
    got, bad = gpu_ingest(strings, list(range(n)), slots, shape, total, prep=prep)
    assert (bad == 0).all()
    check_arena(got, want, slots, variant)
    assert not np.array_equal(want, x.astype(np.float32).view(np.uint32))


# ---- 2. verdicts: one word per decode workgroup, every one stored -------------------------------

def plant(s: bytes, at: int, what: bytes) -> bytes:
    return s[:at] + what + s[at + len(what):]


def test_verdict_words_two_chunks(images):
    shape = (33, 33, 3)
    x = images[shape][:4]
    s = [b64_of(im) for im in x]
    s[2] = plant(s[2], CHUNK + 100, b"-")                 # chunk 1 of image 2
    got, bad = gpu_ingest(s, [3, 8, 13, 0], [2, 0, 3, 1], shape, 5)
    want = [0] * 8
    want[2 * 2 + 1] = 2
    assert list(bad) == want                              # (prefilled with 7: all were stored)
    bits = got.view(np.uint32)
    ref = x.astype(np.float32).view(np.uint32)
    assert np.array_equal(bits[2], ref[0]) and np.array_equal(bits[0], ref[1])
    assert np.array_equal(bits[1], ref[3]) and (got[4] == SENTINEL).all()
    # '=' among the data characters of image 0's first chunk, a bad last character of image 3
    s = [b64_of(im) for im in x]
    s[0] = plant(s[0], 10, b"=")
    s[3] = plant(s[3], geometry(shape)[1] - 1, b"_")
    _, bad = gpu_ingest(s, [1, 6, 11, 15], [0, 1, 2, 3], shape, 4)
    assert list(bad) == [2, 0, 0, 0, 0, 0, 0, 2]


def test_verdict_words_padding(images):
    shape = (28, 28, 1)
    per, L, pad = geometry(shape)
    assert pad == 2
    x = images[shape][:5]
    s = [b64_of(im) for im in x]
    s[1] = plant(s[1], L - 1, b"A")                       # a non-'=' in the padding
    s[3] = plant(s[3], L // 2, b"=")                      # '=' in the data
    s[4] = plant(s[4], L - 2, b"\x00")
    got, bad = gpu_ingest(s, [0, 5, 10, 15, 7], [4, 3, 2, 1, 0], shape, 6)
    assert list(bad) == [0, 2, 0, 2, 2]
    bits = got.view(np.uint32)
    ref = x.astype(np.float32).view(np.uint32)
    assert np.array_equal(bits[4], ref[0]) and np.array_equal(bits[2], ref[2])
    assert (got[5] == SENTINEL).all()


# ---- 3. the CRC half ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def crc_tables():
    return torch.tensor(np.array(K.crc32c_device_tables(), dtype=np.uint32).view(np.int32),
                        device="cuda")


def dev_windows(wins):
    ch = np.zeros(len(wins), dtype=WIN)
    for i, (e, ln) in enumerate(wins):
        ch[i] = (e, ln, 0)
    return torch.from_numpy(ch.view(np.int32).reshape(-1, 4).copy()).cuda()


def windows_for(regions):
    wins, plan = [], []
    for s0, ln in regions:
        n = -(-ln // 4096)
        plan.append((s0, ln, len(wins), n))
        for k in range(n):
            wins.append((s0 + ln - 4096 * (n - 1 - k), ln - 4096 * (n - 1) if k == 0 else 4096))
    return wins, plan


def test_crc_windows_match_the_crc_kernel_and_the_host(crc_tables):
    rng = np.random.default_rng(62)
    buf = rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()
    d = torch.frombuffer(bytearray(buf + bytes(64)), dtype=torch.uint8).cuda()
    regions = [(3, 1), (70, 63), (201, 64), (333, 65), (1001, 4095), (6007, 4096), (11013, 9000)]
    wins, plan = windows_for(regions)
    assert [n for _, _, _, n in plan] == [1, 1, 1, 1, 1, 1, 3]
    assert any(e % 4 for e, _ in wins)
    dw = dev_windows(wins)
    out = torch.full((len(wins),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ops.ingest_crc_b64(d, (1, 1, 1), windows=dw, tables=crc_tables, crc_out=out)
    ref = torch.zeros(len(wins), dtype=torch.int32, device="cuda")
    C.crc32c_chunks(d.data_ptr(), dw.data_ptr(), len(wins), crc_tables.data_ptr(),
                    ref.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    raw_w = out.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(raw_w, ref.cpu().numpy().view(np.uint32))
    for s0, ln, first, n in plan:
        raw = 0
        for k in range(n):
            c = int(raw_w[first + k])
            raw = c if k == 0 else K.crc32c_shift(raw, 4096) ^ c
        std = raw ^ K.crc32c_shift(0xFFFFFFFF, ln) ^ 0xFFFFFFFF
        assert std == K.crc32c(buf[s0:s0 + ln]), (s0, ln)


def test_crc_window_loop_past_the_block_cap(crc_tables):
    """4100 windows: 1025 workgroups' worth, capped at 1024, so the window loop runs."""
    rng = np.random.default_rng(63)
    buf = rng.integers(0, 256, 4100 * 8 + 5, dtype=np.uint8).tobytes()
    d = torch.frombuffer(bytearray(buf + bytes(64)), dtype=torch.uint8).cuda()
    wins = [(5 + 8 * (i + 1), 8) for i in range(4100)]
    out = torch.zeros(len(wins), dtype=torch.int32, device="cuda")
    ops.ingest_crc_b64(d, (1, 1, 1), windows=dev_windows(wins), tables=crc_tables, crc_out=out)
    torch.cuda.synchronize()
    raw = out.cpu().numpy().view(np.uint32)
    for i in (0, 1, 2047, 4095, 4096, 4099):
        e, ln = wins[i]
        assert int(raw[i]) ^ K.crc32c_shift(0xFFFFFFFF, ln) ^ 0xFFFFFFFF == \
            K.crc32c(buf[e - ln:e]), i
    want = [K.crc32c(buf[e - ln:e]) ^ K.crc32c_shift(0xFFFFFFFF, 8) ^ 0xFFFFFFFF
            for e, ln in wins]
    np.testing.assert_array_equal(raw, np.array(want, dtype=np.uint32))


# ---- 4. launch combinations ---------------------------------------------------------------------

def test_both_halves_in_one_launch_and_each_alone(images, crc_tables):
    shape = (33, 33, 3)
    x = images[shape][:3]
    strings = [b64_of(im) for im in x]
    raw, offs = stage(strings, [2, 9, 12])
    buf = raw.tobytes()
    d = torch.from_numpy(raw.copy()).cuda()
    wins, plan = windows_for([(5, len(buf) - 16 - 5)])
    dw = dev_windows(wins)
    want = x.astype(np.float32).view(np.uint32)
    slots = [2, 0, 1]

    def run(with_crc, with_images):
        arena = torch.full((4,) + shape, SENTINEL, device="cuda")
        bad = torch.full((6,), 7, dtype=torch.int32, device="cuda")
        crc = torch.full((len(wins),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        kw = {}
        if with_images:
            kw.update(arena=arena, table=dev_table(offs, slots), wg_bad=bad)
        if with_crc:
            kw.update(windows=dw, tables=crc_tables, crc_out=crc)
        ops.ingest_crc_b64(d, shape, **kw)
        torch.cuda.synchronize()
        return arena.cpu().numpy(), bad.cpu().numpy(), crc.cpu().numpy().view(np.uint32)

    def joined(raw_w):
        s0, ln, first, n = plan[0]
        r = 0
        for k in range(n):
            r = int(raw_w[k]) if k == 0 else K.crc32c_shift(r, 4096) ^ int(raw_w[k])
        return r ^ K.crc32c_shift(0xFFFFFFFF, ln) ^ 0xFFFFFFFF

    std = K.crc32c(buf[5:len(buf) - 16])
    arena, bad, crc = run(True, True)
    check_arena(arena, want, slots, "both")
    assert list(bad) == [0] * 6 and joined(crc) == std
    arena, bad, crc = run(False, True)                   # nchunks = 0, images > 0
    check_arena(arena, want, slots, "images only")
    assert list(bad) == [0] * 6 and (crc == 0x5A5A5A5A).all()
    arena, bad, crc = run(True, False)                   # images = 0, nchunks > 0
    assert (arena == SENTINEL).all() and list(bad) == [7] * 6       # wg_bad is not touched
    assert joined(crc) == std
    arena, bad, crc = run(False, False)                  # both 0: returns without a launch
    assert (arena == SENTINEL).all() and list(bad) == [7] * 6 and (crc == 0x5A5A5A5A).all()


def test_rejected_launches():
    shape = (3, 3, 5)
    raw, offs = stage([b64_of(np.zeros(shape, dtype=np.uint8))], [0])
    d = torch.from_numpy(raw.copy()).cuda()
    arena = torch.zeros((1,) + shape, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    uneven = InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S)   # C = 5 > 4 coefficients
    with pytest.raises(RuntimeError):
        ops.ingest_crc_b64(d, shape, arena=arena, table=dev_table(offs, [0]), wg_bad=bad,
                           prep=uneven)
    with pytest.raises(RuntimeError):                    # no CPU fallback
        ops.ingest_crc_b64(torch.from_numpy(raw.copy()), shape, arena=arena,
                           table=dev_table(offs, [0]), wg_bad=bad)
    with pytest.raises(ValueError):                      # a word per decode workgroup
        ops.ingest_crc_b64(d, (33, 33, 3), arena=torch.zeros((1, 33, 33, 3), device="cuda"),
                           table=dev_table(offs, [0]), wg_bad=bad)


# ---- 5. engine end to end -----------------------------------------------------------------------

def centered_log(p):
    lp = np.log(np.maximum(np.asarray(p, dtype=np.float64), 1e-38))
    return lp - lp.mean(axis=-1, keepdims=True)


def unit_scale_params(net, prep, seed=0):
    """Seeded weights whose BatchNorm statistics come from preprocessed random pixels."""
    params = init_params(net, seed=seed, calibrate=False)
    rng = np.random.default_rng(77)
    x = rng.integers(0, 256, (16,) + tuple(net.input_shape)).astype(np.float32)
    calibrate_bn(net, params, torch.from_numpy(prep.apply(x)))
    return params


def serve(model, recs, params, max_batch=32, batches=None, partitions=1, on_error="null", **kw):
    """recs: (key, record) pairs appended one by one; batches: encoded record batches appended
    as they are (n_out then counts their records)."""
    broker = K.Broker()
    broker.start()
    try:
        broker.create_topic("in", partitions)
        broker.create_topic("out", 1)
        for key, rec in recs:
            broker.append("in", 0, [rec], [key])
        n = len(recs)
        for blob, nrec in batches or []:
            broker.append_batch_repeated("in", 0, blob, 1)
            n += nrec
        cfg = GaleConfig(topology_name="g", input_topic="in", output_topic="out", model=model,
                         bootstrap=f"127.0.0.1:{broker.port}", start_offset="earliest",
                         max_batch=max_batch, max_wait_us=500, output_key="input",
                         on_error=on_error, input_format="b64", **kw)
        eng = Engine(cfg.validate(), devices=[0], max_records=n, params=params)
        eng.start()
        assert eng.wait(120), eng.stats()
        eng.stop()
        out = broker.read("out", 0)
    finally:
        broker.stop()
    assert len(out) == n                                 # ONE output record per input record
    return eng, out


def by_key(out):
    return {r["key"]: r["value"] for r in out}


def compare(got_by_key, xs, refs):
    """tests/test_engine_gpu.py::test_gpu_engine_matches_oracle: centered log-softmax; per
    record argmax equal or rel < 1e-2; worst rel < 2e-2."""
    worst = 0.0
    for k in xs:
        assert got_by_key.get(k) is not None, k
        ref = centered_log(refs[k])
        got = centered_log(json.loads(got_by_key[k])["predictions"])
        assert got.shape == ref.shape, k
        rel = np.abs(got - ref).max() / max(np.abs(ref).max(), 1.0)
        worst = max(worst, rel)
        assert np.array_equal(got.argmax(-1), ref.argmax(-1)) or rel < 1e-2, (k, rel)
    assert worst < 2e-2, worst
    return worst


COUNTS = [1, 2, 1, 3, 1, 1, 4, 1, 2, 1, 3, 2]
PREPS = {
    "resnet20": dict(input_scale=1 / 255, input_mean=CIFAR_MEAN_S, input_std=CIFAR_STD_S),
    "lenet5": dict(input_scale=1 / 255, input_mean="0.1307", input_std="0.3081"),
}


def pixel_sets(shape, seed):
    rng = np.random.default_rng(seed)
    return {f"r{i}".encode(): rng.integers(0, 256, (n,) + tuple(shape), dtype=np.uint8)
            for i, n in enumerate(COUNTS)}


def b64_records(xs):
    return [(k, encode_records_b64(x, x.shape[0])[0]) for k, x in xs.items()]


def bad_records(xs):
    """A record with a bad character in its second image, and a numeric-array record."""
    x = xs[b"r1"]
    rec = encode_records_b64(x, 2)[0]
    at = rec.rindex(b'"b64":"') + 7 + 100
    bad = rec[:at] + b"-" + rec[at + 1:]
    return [(b"badchar", bad), (b"numeric", encode_records_text(x, 2)[0])]


@pytest.fixture(scope="module")
def r20():
    """ResNet-20, the fourteen records, and their host-decode run (b64_ingest off): the
    reference of every ingest run below."""
    net = get_model("resnet20")
    prep = InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S)
    params = unit_scale_params(net, prep)
    xs = pixel_sets(net.input_shape, 51)
    recs = b64_records(xs) + bad_records(xs)
    eng, out = serve("resnet20", recs, params, b64_ingest=False, **PREPS["resnet20"])
    st = eng.stats()
    assert st["ingested_records"] == 0 and st["errors"] == 2 and st["b64_records"] == 13, st
    base = by_key(out)
    assert base[b"badchar"] is None and base[b"numeric"] is None
    assert all(base[k] is not None for k in xs)
    return dict(net=net, params=params, xs=xs, recs=recs, base=base)


def test_engine_b64_ingest_matches_the_host_path(r20):
    """Decoded into the fetch's arena by the ingest launch, served by table steps: the input
    bits are those of the batch step's decoder and the fused forward works per image, so the
    prediction text is byte-identical."""
    eng, out = serve("resnet20", r20["recs"], r20["params"], b64_ingest=True,
                     **PREPS["resnet20"])
    assert by_key(out) == r20["base"]
    st = eng.stats()
    assert st["ingested_records"] == 14 and st["b64_records"] == 13, st
    assert st["ingest_parsed_records"] == 12 and st["preparsed_records"] == 12, st
    assert st["table_batches"] > 0 and st["errors"] == 2, st
    assert st["images_out"] == sum(COUNTS)
    assert st["ingest_plan_in_chunk"] > 0, st             # the plan rode the text's DMA


@pytest.mark.parametrize("site", ["plain", "graph"])
def test_engine_crc_only_ingest(r20, site):
    """No ingest parse on these launch sites: the ingest folds the CRCs and mirrors the text,
    the replica decodes from the resident mirror."""
    kw = {"plain": dict(graph_step=False), "graph": dict(step_launch="graph")}[site]
    eng, out = serve("resnet20", r20["recs"], r20["params"], b64_ingest=True,
                     **PREPS["resnet20"], **kw)
    assert by_key(out) == r20["base"]
    st = eng.stats()
    assert st["ingested_records"] == 14 and st["ingest_parsed_records"] == 0, st
    assert st["b64_records"] == 13 and st["errors"] == 2, st
    assert sum(r["resident_records"] for r in eng.replica_stats()) == 13


def test_engine_plan_in_its_own_copy(r20, monkeypatch):
    monkeypatch.setenv("GALE_INGEST_PLAN_SEPARATE", "1")
    eng, out = serve("resnet20", r20["recs"], r20["params"], b64_ingest=True,
                     **PREPS["resnet20"])
    assert by_key(out) == r20["base"]
    st = eng.stats()
    assert st["ingest_parsed_records"] == 12 and st["ingest_plan_in_chunk"] == 0, st


def test_engine_lenet5_b64_ingest():
    net = get_model("lenet5")
    prep = InputPrep.build(1, 1 / 255, "0.1307", "0.3081")
    params = unit_scale_params(net, prep)
    xs = pixel_sets(net.input_shape, 52)
    recs = b64_records(xs) + bad_records(xs)
    _, base = serve("lenet5", recs, params, b64_ingest=False, **PREPS["lenet5"])
    eng, out = serve("lenet5", recs, params, b64_ingest=True, **PREPS["lenet5"])
    assert by_key(out) == by_key(base)
    assert sum(v is not None for v in by_key(out).values()) == 12
    st = eng.stats()
    assert st["ingested_records"] == 14 and st["ingest_parsed_records"] == 12, st


def test_engine_corrupt_batch_stays_corrupt(r20):
    """Two batches of three records, one bit flipped inside a string of the second: the flipped
    character is outside the alphabet, so the device decode flags its record too - the verdict
    of all three is still the batch's."""
    rng = np.random.default_rng(55)
    shape = r20["net"].input_shape
    recs = [encode_records_b64(rng.integers(0, 256, (1,) + tuple(shape), dtype=np.uint8))[0]
            for _ in range(6)]
    good = K.encode_batch([(None, r, -1, None) for r in recs[:3]], 0, 0)
    bad = bytearray(K.encode_batch([(None, r, -1, None) for r in recs[3:]], 0, 0))
    at = bytes(bad).index(b'"b64":"', len(bad) // 2 - 2000) + 7 + 300
    assert bad[at] < 0x80
    bad[at] ^= 0x80
    eng, out = serve("resnet20", [], r20["params"], batches=[(good, 3), (bytes(bad), 3)],
                     on_error="error-json", b64_ingest=True, **PREPS["resnet20"])
    vals = [r["value"] for r in out]
    assert sum(b"predictions" in v for v in vals) == 3
    assert [json.loads(v)["error"] for v in vals if b"predictions" not in v] == ["corrupt"] * 3
    st = eng.stats()
    assert st["ingested_records"] == 6 and st["images_out"] == 3, st


def test_engine_splits_a_40_image_record():
    """max_batch 32: fragments of 32 and 8 behind the ingest, ONE 40-row output record. No
    preprocessing options, weights calibrated for raw pixels."""
    net = get_model("resnet20")
    prep = InputPrep.build(3)
    params = unit_scale_params(net, prep, seed=1)
    folded = fold_params(net, params)
    rng = np.random.default_rng(54)
    xs = {b"big": rng.integers(0, 256, (40,) + tuple(net.input_shape), dtype=np.uint8),
          b"small": rng.integers(0, 256, (3,) + tuple(net.input_shape), dtype=np.uint8)}
    refs = {k: forward(net, folded, torch.from_numpy(x.astype(np.float32))).numpy()
            for k, x in xs.items()}
    recs = [(k, encode_records_b64(x, x.shape[0])[0]) for k, x in xs.items()]
    eng, out = serve("resnet20", recs, params, b64_ingest=True)
    got = by_key(out)
    assert len(out) == 2 and len(json.loads(got[b"big"])["predictions"]) == 40
    compare(got, xs, refs)
    st = eng.stats()
    assert st["split_records"] == 1 and st["split_fragments"] == 2 and st["errors"] == 0, st
    assert st["b64_records"] == 2 and st["images_out"] == 43 and st["ingested_records"] == 2, st


def test_engine_locality_split(r20):
    """Two locality slots on one device: a record stolen by the other slot's replica is not
    resident there (its arena belongs to another locality) and goes down the span-copy path."""
    eng, out = serve("resnet20", r20["recs"], r20["params"], partitions=2, b64_ingest=True,
                     replicas=2, source_parallelism=2, locality_split=2, decode_threads=2,
                     **PREPS["resnet20"])
    assert by_key(out) == r20["base"]
    st = eng.stats()
    assert st["locality_slots"] == 2 and st["ingested_records"] == 14 and st["errors"] == 2, st
