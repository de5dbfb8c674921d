"""Packed-pixel records (--input-pixel-format bgr24 | rgba | bgra | gray) on the GPU: the
b64_packed_instances kernel bit for bit against the numpy oracle
(gale.models.preprocess.PixelUnpack) and against the existing RGB decoder run on the oracle's
bytes, its store paths, bounds, verdicts and launcher refusals, and the engine end to end on every
step launch site against the same engine fed RGB records of the oracle's images. Every comparison
is bit-exact."""

import base64
import logging

import numpy as np
import pytest
import torch

from gale import ops
from gale._native import native
from gale.config import GaleConfig
from gale.data import encode_records_b64, encode_records_packed
from gale.engine import Engine
from gale.models import get_model, init_params
from gale.models.preprocess import InputPrep, PixelUnpack
from gale.models.reference import calibrate_bn

pytestmark = pytest.mark.gpu

C = native()
K = C.kafka
IMG = np.dtype([("off", "<i8"), ("slot", "<i4"), ("rec", "<i4")])
assert IMG.itemsize == C.B64_IMAGE_BYTES

CIFAR_MEAN_S = "0.4914,0.4822,0.4465"
CIFAR_STD_S = "0.2470,0.2435,0.2616"
SENTINEL = -7.0
FORMATS = ("bgr24", "rgba", "bgra", "gray")
N = 16          # images per launch: image i starts at phase i modulo 16
PREP = InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S)   # (differs per channel)
WAVE_BYTES, CHUNK_BYTES, CHUNK_CHARS = 768, 3072, 4096

# (HS, WS) -> per format (B, '=' characters, chunks): what each case reaches.
#  1x1     one lane, one pixel
#  4x4     pad 2 for gray and rgba / bgra
#  5x7     pad 1 for gray and rgba / bgra; odd sizes
#  6x10    pad 0 for all four
#  16x17   gray: part of one wave; bgr24 and rgba / bgra: a whole wave and a partial one
#  32x32   bgr24: exactly one chunk; rgba / bgra: two chunks, pad 2; gray: two waves, pad 2
#  33x32   bgr24: two chunks, the second nearly empty
#  56x56   gray: two chunks, pad 2
TABLE = {
    (1, 1): {"gray": (1, 2, 1), "bgr24": (3, 0, 1), "rgba": (4, 2, 1)},
    (4, 4): {"gray": (16, 2, 1), "bgr24": (48, 0, 1), "rgba": (64, 2, 1)},
    (5, 7): {"gray": (35, 1, 1), "bgr24": (105, 0, 1), "rgba": (140, 1, 1)},
    (6, 10): {"gray": (60, 0, 1), "bgr24": (180, 0, 1), "rgba": (240, 0, 1)},
    (16, 17): {"gray": (272, 1, 1), "bgr24": (816, 0, 1), "rgba": (1088, 1, 1)},
    (32, 32): {"gray": (1024, 2, 1), "bgr24": (3072, 0, 1), "rgba": (4096, 2, 2)},
    (33, 32): {"gray": (1056, 0, 1), "bgr24": (3168, 0, 2), "rgba": (4224, 0, 2)},
    (56, 56): {"gray": (3136, 2, 2), "bgr24": (9408, 0, 4), "rgba": (12544, 2, 5)},
    (224, 224): {"gray": (50176, 2, 17), "bgr24": (150528, 0, 49), "rgba": (200704, 2, 66)},
}
CASES = [s for s in TABLE if s != (224, 224)]


def test_the_cases_are_what_the_table_says():
    """On the CPU: B, the padding and the chunk count of every case and format, and the wave and
    chunk boundaries the comments above name."""
    for (HS, WS), row in TABLE.items():
        for fmt in FORMATS:
            un = PixelUnpack(fmt)
            B = un.frame_bytes(HS, WS)
            L = 4 * ((B + 2) // 3)
            s = base64.b64encode(bytes(B))
            assert len(s) == L and C.packed_bpp(fmt) == un.bytes_per_pixel
            pad = len(s) - len(s.rstrip(b"="))
            chunks = -(-L // CHUNK_CHARS)
            assert (B, pad, chunks) == row["rgba" if fmt == "bgra" else fmt], (HS, WS, fmt)
    assert TABLE[(16, 17)]["gray"][0] < WAVE_BYTES < TABLE[(16, 17)]["bgr24"][0] < 2 * WAVE_BYTES
    assert WAVE_BYTES < TABLE[(16, 17)]["rgba"][0] < 2 * WAVE_BYTES
    assert TABLE[(32, 32)]["bgr24"][0] == CHUNK_BYTES
    assert WAVE_BYTES < TABLE[(32, 32)]["gray"][0] <= 2 * WAVE_BYTES
    assert 0 < TABLE[(33, 32)]["bgr24"][0] - CHUNK_BYTES < WAVE_BYTES // 4
    assert CHUNK_BYTES < TABLE[(56, 56)]["gray"][0] < 2 * CHUNK_BYTES


_packed = {}


def packed(HS, WS, fmt, n=N):
    """n random packed images, uint8 [n, B] (the alpha bytes random too)."""
    key = (HS, WS, fmt, n)
    if key not in _packed:
        rng = np.random.default_rng(HS * 10007 + WS * 31 + FORMATS.index(fmt))
        _packed[key] = rng.integers(0, 256, (n, PixelUnpack(fmt).frame_bytes(HS, WS)),
                                    dtype=np.uint8)
        _packed[key].setflags(write=False)
    return _packed[key]


_oracle = {}


def oracle(HS, WS, fmt, n=N):
    """uint8 [n, HS, WS, 3]: computed once per size and format."""
    key = (HS, WS, fmt, n)
    if key not in _oracle:
        _oracle[key] = PixelUnpack(fmt).apply(packed(HS, WS, fmt, n), HS, WS)
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


def strings_of(HS, WS, fmt, n=N):
    return [base64.b64encode(f.tobytes()) for f in packed(HS, WS, fmt, n)]


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


def run(st, size, fmt, nslots, nrec, prep=None, header=None, misalign=False):
    """(floats [nslots, HS, WS, 3], statuses [nrec]). header: the device-count form with that
    count. misalign: the output starts 4 bytes past a 16-byte boundary (the scalar store path).
    The guard floats before the first slot and after the last one are checked to be untouched."""
    HS, WS = size
    per = HS * WS * 3
    flat = torch.full((nslots * per + 8,), SENTINEL, device="cuda")
    lead = 5 if misalign else 4
    out = flat[lead:lead + nslots * per]
    assert out.data_ptr() % 16 == (4 if misalign else 0)
    status = torch.zeros(nrec, dtype=torch.int32, device="cuda")
    hdr = torch.tensor([header], dtype=torch.int32, device="cuda") if header is not None else None
    ops.b64_packed_instances(st.raw, st.tab, size, out, status, PixelUnpack(fmt), d_images=hdr,
                             prep=prep)
    torch.cuda.synchronize()
    f = flat.cpu().numpy()
    assert (f[:lead] == SENTINEL).all() and (f[lead + nslots * per:] == SENTINEL).all()
    return f[lead:lead + nslots * per].reshape(nslots, HS, WS, 3), status.cpu().numpy()


def rgb_decoder(rgb_u8, phases, prep):
    """What b64_decode_instances gives for the RGB strings of uint8 [n, HS, WS, 3] images."""
    n, HS, WS, _ = rgb_u8.shape
    rs = Staged([base64.b64encode(im.tobytes()) for im in rgb_u8], phases, range(n), range(n))
    want = torch.full((n, HS, WS, 3), SENTINEL, device="cuda")
    wstatus = torch.zeros(n, dtype=torch.int32, device="cuda")
    ops.b64_decode_instances(rs.raw, rs.tab, (HS, WS, 3), want, wstatus, prep=prep)
    torch.cuda.synchronize()
    assert not wstatus.cpu().numpy().any()
    return want.cpu().numpy()


# ---- 1. bit-exactness ---------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("HS,WS", CASES)
def test_kernel_equals_the_oracle_and_the_rgb_decoder(HS, WS, fmt):
    """Image i at start phase i modulo 16, in slot 2 i + 1 (the even slots stay sentinel), four
    records; without prep and with the CIFAR prep (per-channel: a coefficient indexed by wire
    order would show), both launch forms; and the bits of the RGB decoder on the oracle's bytes."""
    st = Staged(strings_of(HS, WS, fmt), range(N), [2 * i + 1 for i in range(N)],
                [i // 4 for i in range(N)])
    rgb = oracle(HS, WS, fmt).astype(np.float32)
    for prep, want in ((None, rgb), (PREP, PREP.apply(rgb))):
        yard = rgb_decoder(oracle(HS, WS, fmt), range(N), prep)
        assert np.array_equal(yard.view(np.uint32), want.view(np.uint32))
        for header in (None, N):
            got, status = run(st, (HS, WS), fmt, 2 * N + 1, 4, prep=prep, header=header)
            what = (HS, WS, fmt, prep is not None, header)
            assert list(status) == [0] * 4, what
            assert np.array_equal(got[1::2].view(np.uint32), want.view(np.uint32)), what
            assert (got[0::2] == SENTINEL).all(), what


@pytest.mark.parametrize("fmt", FORMATS)
def test_one_224x224_image(fmt):
    """Index range and many chunks: one image, phase 11, slot 1 of 3, with prep."""
    HS, WS = 224, 224
    st = Staged(strings_of(HS, WS, fmt, 1), [11], [1], [0])
    want = PREP.apply(oracle(HS, WS, fmt, 1).astype(np.float32))
    got, status = run(st, (HS, WS), fmt, 3, 1, prep=PREP)
    assert list(status) == [0]
    assert np.array_equal(got[1].view(np.uint32), want[0].view(np.uint32))
    assert (got[0] == SENTINEL).all() and (got[2] == SENTINEL).all()


# ---- 2. the scalar store path and the device count ----------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("HS,WS", CASES)
def test_scalar_store_path(HS, WS, fmt):
    """An output base one float past a 16-byte boundary: one float per lane and instruction, the
    same bits, the guards and the slots in between intact."""
    st = Staged(strings_of(HS, WS, fmt), range(N), [2 * i + 1 for i in range(N)], [0, 1] * (N // 2))
    rgb = oracle(HS, WS, fmt).astype(np.float32)
    for prep, want in ((None, rgb), (PREP, PREP.apply(rgb))):
        got, status = run(st, (HS, WS), fmt, 2 * N + 1, 2, prep=prep, misalign=True)
        assert list(status) == [0, 0]
        assert np.array_equal(got[1::2].view(np.uint32), want.view(np.uint32)), prep is not None
        assert (got[0::2] == SENTINEL).all()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("HS,WS", [(5, 7), (32, 32), (56, 56)])
def test_device_count_below_images(HS, WS, fmt):
    """A device count of N - 3: the slots of the last three descriptors stay sentinel, on both
    store paths; a count of 0 writes nothing at all."""
    st = Staged(strings_of(HS, WS, fmt), range(N), [2 * i + 1 for i in range(N)], [0] * N)
    want = PREP.apply(oracle(HS, WS, fmt).astype(np.float32)).view(np.uint32)
    for misalign in (False, True):
        got, status = run(st, (HS, WS), fmt, 2 * N + 1, 1, prep=PREP, header=N - 3,
                          misalign=misalign)
        assert list(status) == [0]
        assert np.array_equal(got[1:2 * (N - 3):2].view(np.uint32), want[:N - 3]), misalign
        assert (got[0::2] == SENTINEL).all() and (got[2 * (N - 3) + 1:] == SENTINEL).all()
    got, status = run(st, (HS, WS), fmt, 2 * N + 1, 1, header=0)
    assert (got == SENTINEL).all() and list(status) == [0]


# ---- 3. verdicts --------------------------------------------------------------------------------

def plant(s: bytes, at: int, what: bytes) -> bytes:
    return s[:at] + what + s[at + len(what):]


@pytest.mark.parametrize("header", [None, 7])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("HS,WS", [(56, 56), (5, 7)])
def test_verdicts(HS, WS, fmt, header):
    """One plant per record, records 1..5; records 0 and 6 are good. 56x56 has a second chunk in
    every format; 5x7 has one '=' (gray, rgba / bgra), 56x56 two. bgr24 strings have no '='
    position (B is a multiple of 3) and 5x7 no second chunk: those records stay good."""
    s = strings_of(HS, WS, fmt)[:7]
    L = len(s[0])
    pad = len(s[0]) - len(s[0].rstrip(b"="))
    two_chunks = L > CHUNK_CHARS
    s[1] = plant(s[1], 0, b"-")                      # a bad byte at the first character
    s[2] = plant(s[2], L - pad - 1, b"_")            # ... at the last data character
    if two_chunks:
        s[3] = plant(s[3], CHUNK_CHARS + 37, b"\x80")  # ... in the second chunk
    if pad:
        s[4] = plant(s[4], L - pad, b"A")            # a data character in a '=' position
    s[5] = plant(s[5], min(10, L - pad - 1), b"=")   # a '=' in a data position
    st = Staged(s, [(7 * i + 1) % 16 for i in range(7)], [2 * i + 1 for i in range(7)], range(7))
    got, status = run(st, (HS, WS), fmt, 15, 7, header=header)
    assert list(status) == [0, 2, 2, 2 if two_chunks else 0, 2 if pad else 0, 2, 0]
    want = oracle(HS, WS, fmt).astype(np.float32)
    for good in (0, 6) + (() if two_chunks else (3,)) + (() if pad else (4,)):
        assert np.array_equal(got[2 * good + 1], want[good]), good
    assert (got[0::2] == SENTINEL).all()        # every image stayed inside its own slot ...
    assert (got[1::2] != SENTINEL).all()        # ... and was written
    # a bad character far from a pixel leaves that pixel's value alone
    assert np.array_equal(got[3][HS - 1], want[1][HS - 1])


# ---- 4. launcher refusals -----------------------------------------------------------------------

def test_launcher_refusals():
    HS, WS = 6, 10
    st = Staged(strings_of(HS, WS, "bgra"), range(N), range(N), range(N))
    out = torch.full((N, HS, WS, 3), SENTINEL, device="cuda")
    status = torch.zeros(N, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def launch(images=N, imgs=None, raw=None, size=(HS, WS), Cc=3, o=None, s=None,
               format="bgra", **kw):
        return C.b64_packed_instances(images, st.tab.data_ptr() if imgs is None else imgs,
                                      st.raw.data_ptr() if raw is None else raw, size[0], size[1],
                                      Cc, out.data_ptr() if o is None else o,
                                      status.data_ptr() if s is None else s, stream,
                                      format=format, **kw)

    bad = C.HIP_ERROR_INVALID_VALUE
    assert launch(size=(0, 10)) == bad and launch(size=(6, -2)) == bad      # non-positive
    assert launch(Cc=1) == bad and launch(Cc=4) == bad
    assert launch(imgs=0) == bad and launch(raw=0) == bad and launch(o=0) == bad
    assert launch(s=0) == bad
    assert launch(images=65536) == bad
    assert launch(nchw=True) == bad
    for f in ("rgb", "bgr", "yuyv", "i420", "argb", ""):
        assert launch(format=f) == bad
    assert launch(size=(16384, 32768)) == bad                               # > 2^30 floats
    assert launch(images=0) == 0
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item() and not status.any().item()       # nothing was launched
    with pytest.raises(ValueError, match="refused"):
        ops.b64_packed_instances(st.raw, st.tab, (0, WS), out, status, PixelUnpack("bgra"))
    with pytest.raises(ValueError, match="refused"):
        ops.b64_packed_instances(st.raw, st.tab, (HS, WS), out, status, PixelUnpack("gray"),
                                 prep=InputPrep.build(3, 1 / 255, layout="nchw"))
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item() and not status.any().item()
    assert launch() == 0                                                     # the same call, valid
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), oracle(HS, WS, "bgra").astype(np.float32))


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


def packed_sets(HS, WS, fmt, seed):
    """key -> uint8 [n, B] packed images of one format."""
    rng = np.random.default_rng(seed)
    B = PixelUnpack(fmt).frame_bytes(HS, WS)
    return {f"r{i}".encode(): rng.integers(0, 256, (n, B), dtype=np.uint8)
            for i, n in enumerate(COUNTS)}


def b64_record(images):
    return b'{"instances":[' + b",".join(b'{"b64":"' + base64.b64encode(im.tobytes()) + b'"}'
                                         for im in images) + b"]}"


def packed_records(sets):
    recs = [(k, b64_record(p)) for k, p in sets.items()]
    bad = bytearray(recs[1][1])
    at = bytes(bad).rindex(b'"b64":"') + 7 + 100
    bad[at:at + 1] = b"-"
    return recs + [(b"badchar", bytes(bad))]


def rgb_records(sets, fmt, HS, WS):
    un = PixelUnpack(fmt)
    return [(k, encode_records_b64(un.apply(p, HS, WS), p.shape[0])[0]) for k, p in sets.items()]


def check_against_rgb(got, stats, want, sets):
    assert got.pop(b"badchar") is None
    assert got == want and all(v is not None for v in want.values())
    assert stats["packed_records"] == len(sets) + 1 == stats["b64_records"], stats
    assert stats["yuv_records"] == 0, stats
    assert stats["errors"] == 1 and stats["images_out"] == sum(COUNTS), stats


@pytest.mark.parametrize("site", list(SITES))
def test_engine_every_step_site(r20, site):
    """Op by op, the direct launch and both captured graphs: each packed run gives, key by key,
    the text of the same engine fed RGB b64 records of the oracle's images; the record with a bad
    character is one error and its neighbours are served."""
    kw = dict(PREP_KW, **SITES[site])
    for fmt in FORMATS:
        sets = packed_sets(32, 32, fmt, 61)
        wstats, want = serve(rgb_records(sets, fmt, 32, 32), r20, **kw)
        assert wstats["packed_records"] == 0 and wstats["errors"] == 0
        stats, got = serve(packed_records(sets), r20, input_pixel_format=fmt, **kw)
        check_against_rgb(got, stats, want, sets)
        assert (stats["graph_step_batches"] > 0) == (site != "plain"), stats
        assert stats["ingested_records"] == 0, stats


def test_engine_encode_records_packed_round_trip(r20):
    """gale.data.encode_records_packed of RGB images (with an alpha plane) is served as the RGB
    records of those images."""
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (6, 32, 32, 3), dtype=np.uint8)
    alpha = rng.integers(0, 256, (6, 32, 32), dtype=np.uint8)
    keys = [b"a", b"b", b"c"]
    _, want = serve(list(zip(keys, encode_records_b64(x, 2))), r20, **PREP_KW)
    stats, got = serve(list(zip(keys, encode_records_packed(x, "bgra", 2, alpha))), r20,
                       input_pixel_format="bgra", **PREP_KW)
    assert got == want and stats["packed_records"] == 3 and stats["errors"] == 0


def test_engine_lenet5_is_refused():
    with pytest.raises(ValueError, match="--input-pixel-format gray.*C = 1.*rgb already"):
        GaleConfig(topology_name="g", model="lenet5", input_format="b64",
                   input_pixel_format="gray").validate()
    with pytest.raises(ValueError, match="--input-pixel-format bgra.*C = 1"):
        GaleConfig(topology_name="g", model="lenet5", input_format="b64",
                   input_pixel_format="bgra").validate()


@pytest.mark.parametrize("fmt", ["rgba", "gray"])
def test_engine_with_input_resize(r20, fmt):
    """--input-size 40,36, antialias off: the decode writes the resize's source tensor."""
    sets = packed_sets(40, 36, fmt, 62)
    kw = dict(PREP_KW, input_size="40,36", input_antialias=False)
    _, want = serve(rgb_records(sets, fmt, 40, 36), r20, **kw)
    stats, got = serve(packed_records(sets), r20, input_pixel_format=fmt, **kw)
    check_against_rgb(got, stats, want, sets)
    # (the record with the bad character went through the step too: its two images are written)
    assert stats["resized_images"] == sum(COUNTS) + COUNTS[1], stats


@pytest.mark.parametrize("fmt", ["bgr24", "bgra"])
def test_engine_max_batch_smaller_than_a_record(r20, fmt):
    """--max-batch 3: the records of 4 images are split by the byte-count splitter and joined."""
    sets = packed_sets(32, 32, fmt, 64)
    _, want = serve(rgb_records(sets, fmt, 32, 32), r20, max_batch=3, **PREP_KW)
    stats, got = serve(packed_records(sets), r20, max_batch=3, input_pixel_format=fmt, **PREP_KW)
    check_against_rgb(got, stats, want, sets)
    assert stats["split_records"] == COUNTS.count(4), stats


@pytest.mark.parametrize("fmt", ["bgra", "gray"])
def test_engine_b64_ingest_is_crc_only(r20, fmt, caplog):
    sets = packed_sets(32, 32, fmt, 63)
    _, want = serve(rgb_records(sets, fmt, 32, 32), r20, **PREP_KW)
    with caplog.at_level(logging.INFO, logger="gale.engine"):
        stats, got = serve(packed_records(sets), r20, input_pixel_format=fmt, b64_ingest=True,
                           **PREP_KW)
    lines = [r.getMessage() for r in caplog.records if "CRC-only" in r.getMessage()]
    assert len(lines) == 1 and fmt in lines[0], caplog.text
    check_against_rgb(got, stats, want, sets)
    assert stats["ingested_records"] == len(sets) + 1, stats
    assert stats["ingest_parsed_records"] == 0, stats
