"""YUV 4:2:0 frame records (--input-pixel-format i420 | nv12) on the GPU: the b64_yuv_instances
kernel bit for bit against the numpy oracle (gale.models.preprocess.YuvConvert) and against the
existing RGB decoder run on the oracle's bytes, its bounds, verdicts and launcher refusals, and the
engine end to end on every step launch site against the same engine fed RGB records of the
oracle's images. Every comparison is bit-exact."""

import base64
import logging

import numpy as np
import pytest
import torch

from gale import ops
from gale._native import native
from gale.config import GaleConfig
from gale.data import encode_records_b64, encode_records_yuv, pack_yuv420
from gale.engine import Engine
from gale.models import get_model, init_params
from gale.models.preprocess import InputPrep, YuvConvert
from gale.models.reference import calibrate_bn

pytestmark = pytest.mark.gpu

C = native()
K = C.kafka
IMG = np.dtype([("off", "<i8"), ("slot", "<i4"), ("rec", "<i4")])
assert IMG.itemsize == C.B64_IMAGE_BYTES

CIFAR_MEAN_S = "0.4914,0.4822,0.4465"
CIFAR_STD_S = "0.2470,0.2435,0.2616"
SENTINEL = -7.0
TABLES = [(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]
FORMATS = ("i420", "nv12")
EDGE = (0, 16, 128, 235, 240, 255)
N = 16          # frames per launch: frame i starts at phase i modulo 16
PREP = InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S)

# (HS, WS, pairs): pairs 0 = the launcher's choice.
#  2x2 .. 6x10: chroma planes at byte phase 1, 2 and 0 modulo 3, an odd chroma width;
#  2x4096: the widest strip of the issue, one row pair of 12 KB in LDS;
#  6x10 with 1 pair a block: 3 blocks, their luma ranges meet at bytes 20 and 40, inside quads;
#  24x512: the launcher's own split, 3 blocks of 4 pairs meeting at byte 4096 = 3 * 1365 + 1
CASES = [(2, 2, 0), (2, 4, 0), (4, 6, 0), (6, 10, 0), (32, 32, 0), (2, 4096, 0), (6, 10, 1),
         (24, 512, 0)]


def test_the_cases_are_what_their_comments_say():
    assert C.b64_yuv_pairs(32, 32) == 16 and C.b64_yuv_pairs(2, 4096) == 1
    assert C.b64_yuv_pairs(24, 512) == 4 and (2 * 4 * 512) % 3 == 1 and 24 // 2 // 4 == 3
    assert C.b64_yuv_pairs(224, 224) == 9
    assert C.b64_yuv_lds_bytes(4096, 1) <= C.YUV_LDS_BUDGET
    assert [(HS * WS) % 3 for HS, WS, _ in CASES[:4]] == [1, 2, 0, 0] and (10 // 2) % 2 == 1


_planes = {}


def planes(HS, WS):
    """N frames' planes: random, the first ones run through EDGE^3 so that both clamps fire."""
    if (HS, WS) not in _planes:
        rng = np.random.default_rng(HS * 10007 + WS)
        Y = rng.integers(0, 256, (N, HS, WS), dtype=np.uint8)
        U = rng.integers(0, 256, (N, HS // 2, WS // 2), dtype=np.uint8)
        V = rng.integers(0, 256, (N, HS // 2, WS // 2), dtype=np.uint8)
        e = np.array(EDGE, dtype=np.uint8)
        k = np.arange(N * (HS // 2) * (WS // 2)).reshape(U.shape)
        forced = k < 216
        U[forced], V[forced] = e[(k // 6) % 6][forced], e[k % 6][forced]
        up = lambda c: np.repeat(np.repeat(c, 2, axis=1), 2, axis=2)  # noqa: E731
        Y[up(forced)] = up(e[(k // 36) % 6])[up(forced)]
        _planes[(HS, WS)] = (Y, U, V)
    return _planes[(HS, WS)]


_oracle = {}


def oracle(HS, WS, matrix, range_):
    """uint8 [N, HS, WS, 3]: computed once per size and table (the format does not change it)."""
    key = (HS, WS, matrix, range_)
    if key not in _oracle:
        yc = YuvConvert("i420", matrix, range_)
        _oracle[key] = yc.apply(pack_yuv420(*planes(HS, WS), "i420"), HS, WS)
        _oracle[key].setflags(write=False)
    return _oracle[key]


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


def strings_of(HS, WS, fmt):
    return [base64.b64encode(f.tobytes()) for f in pack_yuv420(*planes(HS, WS), fmt)]


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


def run(st, size, yc, nslots, nrec, prep=None, header=None, pairs=0, misalign=False):
    """(floats [nslots, HS, WS, 3], statuses [nrec]). header: the device-count form with that
    count. misalign: the output starts 4 bytes past a 16-byte boundary (the scalar store path);
    the float before it and the one after the last slot are checked to be untouched."""
    HS, WS = size
    per = HS * WS * 3
    flat = torch.full((nslots * per + 8,), SENTINEL, device="cuda")
    lead = 5 if misalign else 4
    out = flat[lead:lead + nslots * per]
    assert out.data_ptr() % 16 == (4 if misalign else 0)
    status = torch.zeros(nrec, dtype=torch.int32, device="cuda")
    hdr = torch.tensor([header], dtype=torch.int32, device="cuda") if header is not None else None
    ops.b64_yuv_instances(st.raw, st.tab, size, out, status, yc, d_images=hdr, prep=prep,
                          pairs=pairs)
    torch.cuda.synchronize()
    f = flat.cpu().numpy()
    assert (f[:lead] == SENTINEL).all() and (f[lead + nslots * per:] == SENTINEL).all()
    return f[lead:lead + nslots * per].reshape(nslots, HS, WS, 3), status.cpu().numpy()


# ---- 1. bit-exactness ---------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("HS,WS,pairs", CASES)
def test_kernel_equals_the_oracle(HS, WS, pairs, fmt):
    """Frame i at start phase i modulo 16, in slot 2 i + 1 (the even slots stay sentinel); all
    four tables, with and without prep, both launch forms."""
    st = Staged(strings_of(HS, WS, fmt), range(N), [2 * i + 1 for i in range(N)],
                [i // 4 for i in range(N)])
    for matrix, range_ in TABLES:
        yc = YuvConvert(fmt, matrix, range_)
        rgb = oracle(HS, WS, matrix, range_).astype(np.float32)
        for prep, want in ((None, rgb), (PREP, PREP.apply(rgb))):
            for header in (None, N):
                got, status = run(st, (HS, WS), yc, 2 * N + 1, 4, prep=prep, header=header,
                                  pairs=pairs)
                what = (HS, WS, pairs, fmt, matrix, range_, prep is not None, header)
                assert list(status) == [0] * 4, what
                assert np.array_equal(got[1::2].view(np.uint32), want.view(np.uint32)), what
                assert (got[0::2] == SENTINEL).all(), what


@pytest.mark.parametrize("fmt", FORMATS)
def test_existing_rgb_decoder_is_the_yardstick(fmt):
    """The same bits as b64_decode_instances on the oracle's RGB bytes with the same prep."""
    for (HS, WS), prep in (((32, 32), PREP), ((6, 10), None), ((24, 512), PREP)):
        yc = YuvConvert(fmt, "bt601", "limited")
        rgb = oracle(HS, WS, "bt601", "limited")
        phases = [(5 * i + 3) % 16 for i in range(N)]
        got, status = run(Staged(strings_of(HS, WS, fmt), phases, range(N), range(N)), (HS, WS),
                          yc, N, N, prep=prep)
        rs = Staged([base64.b64encode(im.tobytes()) for im in rgb], phases, range(N), range(N))
        want = torch.full((N, HS, WS, 3), SENTINEL, device="cuda")
        wstatus = torch.zeros(N, dtype=torch.int32, device="cuda")
        ops.b64_decode_instances(rs.raw, rs.tab, (HS, WS, 3), want, wstatus, prep=prep)
        torch.cuda.synchronize()
        assert not status.any() and not wstatus.cpu().numpy().any()
        assert np.array_equal(got.view(np.uint32), want.cpu().numpy().view(np.uint32)), (HS, WS)


# ---- 2. bounds ----------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("HS,WS,pairs", [(6, 10, 0), (6, 10, 1), (32, 32, 0), (24, 512, 0)])
def test_bounds_and_the_scalar_store_path(HS, WS, pairs, fmt):
    """A device count of N - 3: the slots of the last three descriptors stay sentinel, like the
    slots between the frames and the floats around the tensor; then the same with a destination
    that is not 16-byte aligned (one store per float)."""
    yc = YuvConvert(fmt, "bt709", "limited")
    st = Staged(strings_of(HS, WS, fmt), range(N), [2 * i + 1 for i in range(N)], [0] * N)
    want = PREP.apply(oracle(HS, WS, "bt709", "limited").astype(np.float32)).view(np.uint32)
    for misalign in (False, True):
        got, status = run(st, (HS, WS), yc, 2 * N + 1, 1, prep=PREP, header=N - 3, pairs=pairs,
                          misalign=misalign)
        assert list(status) == [0]
        assert np.array_equal(got[1:2 * (N - 3):2].view(np.uint32), want[:N - 3]), misalign
        assert (got[0::2] == SENTINEL).all() and (got[2 * (N - 3) + 1:] == SENTINEL).all()
        got, _ = run(st, (HS, WS), yc, 2 * N + 1, 1, misalign=misalign, pairs=pairs)
        assert np.array_equal(got[1::2], oracle(HS, WS, "bt709", "limited").astype(np.float32))
        assert (got[0::2] == SENTINEL).all()
    # a count of 0 writes nothing at all
    got, status = run(st, (HS, WS), yc, 2 * N + 1, 1, header=0)
    assert (got == SENTINEL).all() and list(status) == [0]


# ---- 3. verdicts --------------------------------------------------------------------------------

def plant(s: bytes, at: int, what: bytes) -> bytes:
    return s[:at] + what + s[at + len(what):]


@pytest.mark.parametrize("header", [None, 8])
@pytest.mark.parametrize("fmt", FORMATS)
def test_verdicts(fmt, header):
    """32x32: L = 2048; luma bytes 0..1023 are quads 0..341, and quad 341 (characters 1364..1367)
    also holds the first chroma byte; I420's U is quads 341..426, its V 426..511 (NV12's UV:
    341..511). One bad character per record, records 1..6; records 0 and 7 are good."""
    HS, WS = 32, 32
    s = strings_of(HS, WS, fmt)[:8]
    L = len(s[0])
    assert L == 2048 and 1023 // 3 == 341 == 1024 // 3
    spots = [0, L - 1, 500, 4 * 380 + 2, 4 * 480 + 1, 1365]
    for rec, (at, ch) in enumerate(zip(spots, b"=-_ \\\x80"), start=1):
        s[rec] = plant(s[rec], at, bytes([ch]))
    st = Staged(s, [(7 * i + 1) % 16 for i in range(8)], [2 * i + 1 for i in range(8)], range(8))
    yc = YuvConvert(fmt, "bt601", "full")
    got, status = run(st, (HS, WS), yc, 17, 8, header=header)
    assert list(status) == [0, 2, 2, 2, 2, 2, 2, 0]
    want = oracle(HS, WS, "bt601", "full").astype(np.float32)
    assert np.array_equal(got[1], want[0]) and np.array_equal(got[15], want[7])
    assert (got[0::2] == SENTINEL).all()        # every frame stayed inside its own slot ...
    assert (got[1::2] != SENTINEL).all()        # ... and was written
    # a bad character far from a pixel leaves that pixel's value alone: record 3's is in luma
    # quad 125 (bytes 375..377), so its last row is the oracle's
    assert np.array_equal(got[7][HS - 1], want[3][HS - 1])


@pytest.mark.parametrize("fmt", FORMATS)
def test_verdict_in_a_quad_that_two_blocks_share(fmt):
    """24x512, 3 blocks of 4 row pairs: luma byte 4096 opens block 1 and lies in quad 1365 with
    the last two bytes of block 0. Either character of that quad is judged (by both blocks)."""
    HS, WS = 24, 512
    s = strings_of(HS, WS, fmt)[:4]
    s[1] = plant(s[1], 4 * 1365, b"!")
    s[2] = plant(s[2], 4 * 1365 + 3, b"~")
    st = Staged(s, [3, 9, 14, 0], range(4), range(4))
    got, status = run(st, (HS, WS), YuvConvert(fmt), 4, 4)
    assert list(status) == [0, 2, 2, 0]
    want = oracle(HS, WS, "bt601", "limited").astype(np.float32)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[3])


# ---- 4. launcher refusals -----------------------------------------------------------------------

def test_launcher_refusals():
    HS, WS = 6, 10
    st = Staged(strings_of(HS, WS, "i420"), range(N), range(N), range(N))
    out = torch.full((N, HS, WS, 3), SENTINEL, device="cuda")
    status = torch.zeros(N, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    kc = [*YuvConvert("i420").coeffs(), 16]

    def launch(images=N, imgs=None, raw=None, size=(HS, WS), Cc=3, o=None, s=None, **kw):
        return C.b64_yuv_instances(images, st.tab.data_ptr() if imgs is None else imgs,
                                   st.raw.data_ptr() if raw is None else raw, size[0], size[1],
                                   Cc, out.data_ptr() if o is None else o,
                                   status.data_ptr() if s is None else s, stream,
                                   coeffs=kc, **kw)

    bad = C.HIP_ERROR_INVALID_VALUE
    assert launch(size=(5, 10)) == bad and launch(size=(6, 9)) == bad       # odd
    assert launch(size=(0, 10)) == bad and launch(size=(6, -2)) == bad      # non-positive
    assert launch(Cc=1) == bad and launch(Cc=4) == bad
    assert launch(imgs=0) == bad and launch(raw=0) == bad and launch(o=0) == bad
    assert launch(s=0) == bad
    assert launch(images=65536) == bad
    assert launch(nchw=True) == bad
    assert launch(format="yuyv") == bad
    assert launch(pairs=4) == bad and launch(pairs=-1) == bad               # more than HS / 2
    # a row-pair block over the LDS budget: one pair of a 21 900-wide strip, 8 pairs of 4096
    assert C.b64_yuv_lds_bytes(21900, 1) > C.YUV_LDS_BUDGET
    assert launch(size=(2, 21900)) == bad and launch(size=(16, 4096), pairs=8) == bad
    assert launch(images=0) == 0
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item() and not status.any().item()       # nothing was launched
    with pytest.raises(ValueError, match="refused"):
        ops.b64_yuv_instances(st.raw, st.tab, (HS, WS), out, status, YuvConvert("i420"), pairs=4)
    assert launch() == 0                                                     # the same call, valid
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(),
                          oracle(HS, WS, "bt601", "limited").astype(np.float32))


# ---- 5. the engine ------------------------------------------------------------------------------

COUNTS = [1, 2, 1, 3, 1, 1, 4, 1, 2, 1, 3, 2]
PREP_KW = dict(input_scale=1 / 255, input_mean=CIFAR_MEAN_S, input_std=CIFAR_STD_S)
SITES = {"direct": {}, "plain": dict(graph_step=False), "graph": dict(step_launch="graph"),
         "graph-noencode": dict(step_launch="graph", gpu_encode=False)}


def serve(recs, params, max_batch=32, **kw):
    broker = K.Broker()
    broker.start()
    try:
        broker.create_topic("in", 1)
        broker.create_topic("out", 1)
        for key, rec in recs:
            broker.append("in", 0, [rec], [key])
        cfg = GaleConfig(topology_name="g", input_topic="in", output_topic="out",
                         model="resnet20", dtype="bf16", input_format="b64",
                         bootstrap=f"127.0.0.1:{broker.port}", start_offset="earliest",
                         max_batch=max_batch, max_wait_us=500, output_key="input",
                         on_error="null", **kw)
        eng = Engine(cfg.validate(), devices=[0], max_records=len(recs), params=params)
        eng.start()
        assert eng.wait(120), eng.stats()
        eng.stop()
        out = broker.read("out", 0)
    finally:
        broker.stop()
    assert len(out) == len(recs)
    return eng.stats(), {r["key"]: r["value"] for r in out}


@pytest.fixture(scope="module")
def r20():
    net = get_model("resnet20")
    params = init_params(net, seed=0, calibrate=False)
    rng = np.random.default_rng(77)
    x = rng.integers(0, 256, (16,) + tuple(net.input_shape)).astype(np.float32)
    calibrate_bn(net, params, torch.from_numpy(PREP.apply(x)))
    return params


def yuv_sets(HS, WS, seed):
    rng = np.random.default_rng(seed)
    return {f"r{i}".encode(): tuple(rng.integers(0, 256, (n, h, w), dtype=np.uint8)
                                    for h, w in ((HS, WS), (HS // 2, WS // 2), (HS // 2, WS // 2)))
            for i, n in enumerate(COUNTS)}


def yuv_records(sets, fmt):
    recs = [(k, encode_records_yuv(*p, fmt, p[0].shape[0])[0]) for k, p in sets.items()]
    bad = bytearray(recs[1][1])
    at = bytes(bad).rindex(b'"b64":"') + 7 + 100
    bad[at:at + 1] = b"-"
    return recs + [(b"badchar", bytes(bad))]


def rgb_records(sets, yc, HS, WS):
    return [(k, encode_records_b64(x, x.shape[0])[0])
            for k, x in ((k, yc.apply(pack_yuv420(*p, "i420"), HS, WS)) for k, p in sets.items())]


def check_against_rgb(got, stats, want, sets):
    assert got.pop(b"badchar") is None
    assert got == want and all(v is not None for v in want.values())
    assert stats["yuv_records"] == len(sets) + 1 == stats["b64_records"], stats
    assert stats["errors"] == 1 and stats["images_out"] == sum(COUNTS), stats


@pytest.mark.parametrize("site", list(SITES))
def test_engine_every_step_site(r20, site):
    """Op by op, the direct launch and both captured graphs: each YUV run gives, key by key, the
    text of the same engine fed RGB b64 records of the oracle's images."""
    sets = yuv_sets(32, 32, 61)
    kw = dict(PREP_KW, **SITES[site])
    wstats, want = serve(rgb_records(sets, YuvConvert("i420", "bt709", "full"), 32, 32), r20, **kw)
    assert wstats["yuv_records"] == 0 and wstats["errors"] == 0
    for fmt in FORMATS:
        stats, got = serve(yuv_records(sets, fmt), r20, input_pixel_format=fmt,
                           input_yuv_matrix="bt709", input_yuv_range="full", **kw)
        check_against_rgb(got, stats, want, sets)
        assert (stats["graph_step_batches"] > 0) == (site != "plain"), stats
        assert stats["ingested_records"] == 0, stats


def test_engine_lenet5_is_refused():
    with pytest.raises(ValueError, match="--input-pixel-format i420.*C = 1"):
        GaleConfig(topology_name="g", model="lenet5", input_format="b64",
                   input_pixel_format="i420").validate()


@pytest.mark.parametrize("fmt", FORMATS)
def test_engine_with_input_resize(r20, fmt):
    """--input-size 40,36, antialias off: the decode writes the resize's source tensor."""
    sets = yuv_sets(40, 36, 62)
    kw = dict(PREP_KW, input_size="40,36", input_antialias=False)
    _, want = serve(rgb_records(sets, YuvConvert("i420"), 40, 36), r20, **kw)
    stats, got = serve(yuv_records(sets, fmt), r20, input_pixel_format=fmt, **kw)
    check_against_rgb(got, stats, want, sets)
    # (the record with the bad character went through the step too: its two frames are written)
    assert stats["resized_images"] == sum(COUNTS) + COUNTS[1], stats


@pytest.mark.parametrize("fmt", FORMATS)
def test_engine_b64_ingest_is_crc_only(r20, fmt, caplog):
    sets = yuv_sets(32, 32, 63)
    _, want = serve(rgb_records(sets, YuvConvert("i420"), 32, 32), r20, **PREP_KW)
    with caplog.at_level(logging.INFO, logger="gale.engine"):
        stats, got = serve(yuv_records(sets, fmt), r20, input_pixel_format=fmt, b64_ingest=True,
                           **PREP_KW)
    lines = [r.getMessage() for r in caplog.records if "CRC-only" in r.getMessage()]
    assert len(lines) == 1 and fmt in lines[0], caplog.text
    check_against_rgb(got, stats, want, sets)
    assert stats["ingested_records"] == len(sets) + 1, stats
    assert stats["ingest_parsed_records"] == 0, stats
