"""The host plan of the JSON device ingest (csrc/runtime/ingest_plan.h: plan_json_ingest +
fill_json_ingest) without a GPU: every count, offset and flag, and the filled plan bytes, against
an independent Python derivation of the layout; the edge cases of the tiling, the tile groups, the
arena, the count block, the in-chunk plan and the packed body; the contradictions the plan
refuses; and a stand-alone sanitizer run of the plan behind the real scanner."""

import os
import shutil
import subprocess

import numpy as np
import pytest

from gale._native import native
from gale.data import encode_records_text

C = native()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTR = C.BATCH_ATTR_OFFSET
G = C.GROUP_TILES
T = C.JSON_TILE_BYTES
SMALL = (2, 2, 1)              # per = 4, S = 8
RGB = (4, 4, 3)                # per = 48, S = 96
HEAD = len(b'{"instances":')   # where the array starts in a value
BIG = 1 << 20                  # a chunk with room for everything

CH = np.dtype([("end", "<i8"), ("len", "<i4"), ("pad", "<i4")])
REC = np.dtype([("off", "<i8"), ("len", "<i4"), ("slot", "<i4"), ("images", "<i4"),
                ("status", "<i4"), ("tile0", "<i4"), ("has_cnt", "<i4"), ("cnt_off", "<i8"),
                ("grp0", "<i8")])
assert REC.itemsize == 48 and CH.itemsize == 16


def a16(n):
    return (n + 15) & ~15


def a256(n):
    return (n + 255) & ~255


def tiles(off, ln):
    """2 KiB tiles of the text [off, off + ln), counted from its 16-byte-aligned start."""
    return 0 if ln <= 0 else -(-(off + ln - (off & ~15)) // T)


def fetch_of(arr_lens, status=None, lead=None):
    """Extents of a fetch with one batch per record: framing, then the value
    {"instances":<arr_len bytes>}. lead[i]: framing bytes before value i (default ATTR + 40).
    Returns (fetch size, batches, plan records (status, value_off, value_len, arr_off, arr_len))."""
    pos, batches, recs = 0, [], []
    for i, n in enumerate(arr_lens):
        b0 = pos
        pos += lead[i] if lead else ATTR + 40
        recs.append((status[i] if status else 0, pos, HEAD + n + 1, HEAD, n))
        pos += HEAD + n + 1
        batches.append((b0, pos - b0))
    return pos, batches, recs


def windows_of(batches):
    wins, per_batch = [], []
    for off, ln in batches:
        rs, re = off + ATTR, off + ln
        n = -(-(re - rs) // 4096)
        per_batch.append((len(wins), n))
        for k in range(n):
            wins.append((re - 4096 * (n - 1 - k), (re - rs) - 4096 * (n - 1) if k == 0 else 4096))
    return wins, per_batch


def derive(batches, recs, shape, arena_bytes, fetch_size, dev_cap, tap_result=-1,
           plan_separate=False, check_crcs=True):
    """The layout GpuIngest::run hands its kernels, re-derived; and the plan bytes."""
    per = shape[0] * shape[1] * shape[2]
    S = 2 * per
    wins, per_batch = windows_of(batches) if check_crcs else ([], [])
    rec_of = [i for i, r in enumerate(recs) if r[0] == 0]
    d = dict(windows=wins, batch_windows=per_batch, rec_of=rec_of, nc=len(wins), nr=len(rec_of))
    if not wins and not rec_of:
        return d, b""
    ext = [(recs[i][1] + recs[i][3], recs[i][4]) for i in rec_of]
    nts = [tiles(o, n) for o, n in ext]
    ngs = [-(-t // G) for t in nts]
    packed = tap_result >= 0
    lo = min([b[0] for b in batches] + [recs[i][1] for i in rec_of])
    hi = max([b[0] + b[1] for b in batches] + [recs[i][1] + recs[i][2] for i in rec_of])
    if packed:
        lo, hi = 0, fetch_size
    lo &= ~15
    span = hi - lo
    ng = -(-span // 2048) if packed else 0
    link = tap_result if packed else span
    c_lo = ((span + 63) & ~63) if packed else lo
    used = c_lo + link
    ntiles, ngroups = sum(nts), sum(ngs)
    cnt_base = -1
    if ntiles:
        cb = a256(4 * (ntiles + ngroups))
        if dev_cap > cb + 256 and ((dev_cap - cb) & ~255) >= a256(used + 64):
            cnt_base = (dev_cap - cb) & ~255
    pjs = []
    if arena_bytes > 0 and cnt_base >= 0:
        for j, (o, n) in enumerate(ext):
            slot, cap = -(-o // S), n // S
            if cap > 0 and (slot + cap) * per * 4 <= arena_bytes:
                pjs.append(j)
    ptiles = sum(nts[j] for j in pjs)
    nc, nr, npr = len(wins), len(rec_of), len(pjs)
    o_chunks = a16(8 * ng)
    o_groups = o_chunks + a16(16 * nc)
    o_recs = o_groups + a16(8 * ngroups)
    o_precs = o_recs + 48 * nr
    o_ptr = o_precs + 48 * npr
    o_gsum = o_ptr + a16(4 * ptiles)
    o_crc = o_gsum + a16(4 * ngroups)
    o_gbad = o_crc + a16(4 * nc)
    o_pbad = o_gbad + a16(4 * ngroups)
    plan_off = a256(max(fetch_size, used))
    lim = cnt_base if cnt_base >= 0 else dev_cap
    # (packed: the plan is written while the pack table still stands at 2 * c_lo in the chunk)
    on_tab = packed and plan_off < 2 * c_lo + 8 * ng and 2 * c_lo < plan_off + o_gsum
    d.update(pjs=pjs, np=npr, ntiles=ntiles, ngroups=ngroups, ptiles=ptiles, ng=ng, packed=packed,
             lo=lo, span=span, link=link, c_lo=c_lo, c_len=link, used=used, cnt_base=cnt_base,
             tab_off=2 * c_lo if packed else 0,
             o_chunks=o_chunks, o_groups=o_groups, o_recs=o_recs, o_precs=o_precs, o_ptr=o_ptr,
             o_gsum=o_gsum, prefix=o_gsum, o_crc=o_crc, o_gbad=o_gbad, o_pbad=o_pbad,
             io_bytes=o_pbad + a16(4 * ptiles), plan_off=plan_off,
             plan_in_chunk=(not plan_separate) and not on_tab and plan_off + o_gsum <= lim)
    # the plan bytes: windows, groups, count records, parse records, parse tile map
    plan = np.zeros(o_gsum, dtype=np.uint8)
    ch = np.zeros(nc, dtype=CH)
    for k, (e, n) in enumerate(wins):
        ch[k] = (e, n, 0)
    hr = np.zeros(nr, dtype=REC)
    groups = []
    tile0 = np.cumsum([0] + nts[:-1]) if nr else []
    grp0 = np.cumsum([0] + ngs[:-1]) if nr else []
    for j, (o, n) in enumerate(ext):
        hr[j] = (o, n, 0, 0, 0, tile0[j], 0, 0, grp0[j])
        groups += [(j, t0) for t0 in range(0, nts[j], G)]
    hp = np.zeros(npr, dtype=REC)
    tile_rec, pt = [], 0
    for k, j in enumerate(pjs):
        o, n = ext[j]
        hp[k] = (o, n, -(-o // S), -1, 0, pt, 1, cnt_base + 4 * (int(tile0[j]) + int(grp0[j])), 0)
        tile_rec += [k] * nts[j]
        pt += nts[j]
    for off, a in ((o_chunks, ch), (o_groups, np.array(groups, dtype="<i4").reshape(-1)),
                   (o_recs, hr), (o_precs, hp), (o_ptr, np.array(tile_rec, dtype="<i4"))):
        raw = np.frombuffer(a.tobytes(), dtype=np.uint8)
        plan[off:off + raw.size] = raw
    return d, plan.tobytes()


def plan_and_check(batches, recs, shape, arena_bytes, fetch_size, dev_cap, **kw):
    """The binding's plan, compared key by key and byte by byte with the derivation."""
    p = C.plan_json_ingest(batches, recs, *shape, arena_bytes=arena_bytes, fetch_size=fetch_size,
                           dev_cap=dev_cap, **kw)
    want, plan = derive(batches, recs, shape, arena_bytes, fetch_size, dev_cap, **kw)
    for k, v in want.items():
        got = [tuple(x) for x in p[k]] if k in ("windows", "batch_windows") else p[k]
        assert got == v, (k, got, v)
    assert p["plan"] == plan
    assert len(p["plan"]) == p["prefix"] == p["o_gsum"]
    return p


def sections(p):
    hr = np.frombuffer(p["plan"], dtype=REC, count=p["nr"], offset=p["o_recs"])
    hp = np.frombuffer(p["plan"], dtype=REC, count=p["np"], offset=p["o_precs"])
    hg = np.frombuffer(p["plan"], dtype="<i4", count=2 * p["ngroups"], offset=p["o_groups"])
    hpt = np.frombuffer(p["plan"], dtype="<i4", count=p["ptiles"], offset=p["o_ptr"])
    return hr, hp, [tuple(x) for x in hg.reshape(-1, 2)], list(hpt)


# ---- 1. tiles and groups ------------------------------------------------------------------------

def test_tiles_count_from_the_aligned_start():
    """An array that starts 5 bytes past a multiple of 16 and ends exactly on a tile boundary
    (counted from the aligned start) has 2 tiles; one byte more makes 3. The record behind it
    starts at the next tile."""
    lead = 16 * 9 + 5 - HEAD                       # array at 149 = 16 * 9 + 5
    for n, nt in ((2 * T - 5, 2), (2 * T - 4, 3), (2 * T - 5 - T, 1)):
        size, batches, recs = fetch_of([n, 200], lead=[lead, ATTR + 40])
        off = recs[0][1] + HEAD
        assert off == 149 and off % 16 == 5 and ((off + n - (off & ~15)) % T == 0) == (nt != 3)
        p = plan_and_check(batches, recs, SMALL, BIG, size, BIG)
        hr, hp, hg, hpt = sections(p)
        assert C.json_tile_count(off, n) == nt == tiles(off, n)
        assert list(hr["tile0"]) == [0, nt] and p["ntiles"] == nt + 1
        assert hpt == [0] * nt + [1]


def test_record_of_two_groups_and_the_record_behind_it():
    """A record of GROUP_TILES + 1 tiles: two groups, the last one short. The record behind it
    starts at tile0 = GROUP_TILES + 1, grp0 = 2, and its parse record finds its count block at
    cnt_base + (tile0 + grp0) * 4."""
    size, batches, recs = fetch_of([G * T + 100, 300, 40])
    p = plan_and_check(batches, recs, RGB, BIG, size, BIG)
    hr, hp, hg, hpt = sections(p)
    nt0 = tiles(recs[0][1] + HEAD, recs[0][4])
    assert nt0 == G + 1
    assert hg == [(0, 0), (0, G), (1, 0), (2, 0)] and p["ngroups"] == 4
    assert list(hr["tile0"]) == [0, G + 1, G + 2] and list(hr["grp0"]) == [0, 2, 3]
    assert p["cnt_base"] >= 0 and p["pjs"] == [0, 1]        # (40 bytes < S: record 2 not parsed)
    assert list(hp["cnt_off"]) == [p["cnt_base"], p["cnt_base"] + (G + 1 + 2) * 4]
    assert list(hp["tile0"]) == [0, G + 1] and hpt == [0] * (G + 1) + [1]
    assert list(hp["images"]) == [-1, -1] and list(hp["has_cnt"]) == [1, 1]
    assert list(hp["grp0"]) == [0, 0]
    S = 2 * 48
    assert list(hp["slot"]) == [-(-int(o) // S) for o in hp["off"]]


def test_bad_record_between_two_good_ones_is_skipped():
    size, batches, recs = fetch_of([100, 100, 100], status=[0, 3, 0])
    p = plan_and_check(batches, recs, SMALL, BIG, size, BIG)
    hr, hp, hg, hpt = sections(p)
    assert p["rec_of"] == [0, 2] and p["nr"] == 2 and p["pjs"] == [0, 1]
    assert list(hr["off"]) == [recs[0][1] + HEAD, recs[2][1] + HEAD]
    assert hg == [(0, 0), (1, 0)] and len(p["windows"]) == 3   # the bad record's batch is CRC'd


def test_scanned_records_plan_like_their_extents():
    """Records as the engine sees them: encoded text, scanned by the host scanner."""
    rng = np.random.default_rng(5)
    buf, batches, recs = bytearray(), [], []
    for n in (1, 3, 40):
        b0 = len(buf)
        buf += bytes(ATTR + 17 + n)
        v = encode_records_text(rng.integers(0, 256, (n,) + RGB, dtype=np.uint8), n)[0]
        st, arr_off, arr_len, images = C.scan_instances(v, *RGB)
        assert st == 0 and images == n and v[arr_off:arr_off + 1] == b"["
        recs.append((st, len(buf), len(v), arr_off, arr_len))
        buf += v
        batches.append((b0, len(buf) - b0))
    p = plan_and_check(batches, recs, RGB, BIG, len(buf), BIG)
    hr, hp, hg, hpt = sections(p)
    assert p["np"] == 3 and p["ngroups"] > 3               # the 40-image record: several groups
    for r in hr:
        assert buf[r["off"]:r["off"] + 1] == b"[" and buf[r["off"] + r["len"] - 1:][:1] == b"]"


# ---- 2. the arena -------------------------------------------------------------------------------

def test_arena_boundary_leaves_out_one_record_alone():
    """A record's slots are [ceil(off / S), + arr_len // S): with arena_bytes exactly at their end
    it is parsed, one byte less leaves it out - and it alone: a record that fits is parsed
    whether or not one before it in the list was. (The base64 plan cuts every later record too:
    its slots are a running count. Here they derive from text offsets, so in a fetch, where
    records ascend, a record behind one that did not fit cannot fit either; the list order of
    the plan's input is free, which is what pins the rule.)"""
    per, S = 4, 8
    size, batches, recs = fetch_of([64, 64, 64])
    ends = [(-(-(r[1] + HEAD) // S) + r[4] // S) * per * 4 for r in recs]
    assert ends == sorted(ends)
    for k in range(3):
        p = plan_and_check(batches, recs, SMALL, ends[k], size, BIG)
        assert p["pjs"] == list(range(k + 1))
        p = plan_and_check(batches, recs, SMALL, ends[k] - 1, size, BIG)
        assert p["pjs"] == list(range(k))
    # the last record of the fetch first in the list: it does not fit, the two behind it do
    turned = [recs[2], recs[0], recs[1]]
    p = plan_and_check(batches, turned, SMALL, ends[1], size, BIG)
    assert p["rec_of"] == [0, 1, 2] and p["pjs"] == [1, 2]
    hr, hp, hg, hpt = sections(p)
    assert list(hp["cnt_off"]) == [p["cnt_base"] + 4 * 2, p["cnt_base"] + 4 * 4]
    # an array shorter than one image's text takes no slots; the records around it are parsed
    size, batches, recs = fetch_of([64, 7, 64])
    p = plan_and_check(batches, recs, SMALL, BIG, size, BIG)
    assert p["nr"] == 3 and p["pjs"] == [0, 2] and p["ptiles"] == 2
    # no arena: counted, not parsed - and no parse sections
    p = plan_and_check(batches, recs, SMALL, 0, size, BIG)
    assert p["pjs"] == [] and p["o_precs"] == p["o_ptr"] == p["o_gsum"] and p["cnt_base"] >= 0


# ---- 3. the count block and the plan's place ----------------------------------------------------

def test_count_block_needs_room_behind_the_text():
    size, batches, recs = fetch_of([300, 300])
    ncnt = 2 + 2                                           # two tiles, two group sums
    cb = a256(4 * ncnt)
    need = a256(size + 64) + cb                            # the smallest aligned chunk with room
    p = plan_and_check(batches, recs, SMALL, BIG, size, need)
    assert p["cnt_base"] == need - cb == a256(size + 64) and p["np"] == 2
    assert p["cnt_base"] + 4 * ncnt <= need and p["cnt_base"] % 256 == 0
    assert p["cnt_base"] >= p["used"] + 64 and p["used"] == size
    p = plan_and_check(batches, recs, SMALL, BIG, size, need - 1)
    assert p["cnt_base"] == -1 and p["pjs"] == [] and p["np"] == 0 and p["ptiles"] == 0
    assert p["nr"] == 2 and p["ngroups"] == 2              # still counted (lane scratch)


def test_plan_rides_in_the_chunk_only_when_it_fits():
    size, _, _ = fetch_of([300, 300])
    pad = (100 - size) % 256                               # a fetch of 100 bytes past 256 * k
    size, batches, recs = fetch_of([300, 300], lead=[ATTR + 40 + pad, ATTR + 40])
    assert size % 256 == 100 and a256(size) == a256(size + 64)
    p = plan_and_check(batches, recs, SMALL, 0, size, BIG)
    assert p["plan_in_chunk"] and p["plan_off"] == a256(size)
    assert p["plan_off"] + p["prefix"] <= p["cnt_base"]
    # a chunk whose count block starts right behind the text: no room for the plan before it
    cb = a256(4 * 4)
    tight = a256(size + 64) + cb
    p = plan_and_check(batches, recs, SMALL, 0, size, tight)
    assert p["cnt_base"] >= 0 and not p["plan_in_chunk"]
    # exactly enough: the plan ends where the count block starts
    q = plan_and_check(batches, recs, SMALL, 0, size, BIG)
    exact = a256(size) + a256(q["prefix"]) + cb
    p = plan_and_check(batches, recs, SMALL, 0, size, exact)
    assert p["plan_in_chunk"] and p["cnt_base"] == exact - cb
    assert p["plan_off"] + p["prefix"] <= p["cnt_base"] < p["plan_off"] + p["prefix"] + 256
    p = plan_and_check(batches, recs, SMALL, 0, size, exact - 256)
    assert not p["plan_in_chunk"]
    # without a count block the limit is the chunk's end
    p = plan_and_check(batches, recs, SMALL, 0, size, size + 100)
    assert p["cnt_base"] == -1 and not p["plan_in_chunk"]
    # the switch gives the same result with all the room there is
    p = plan_and_check(batches, recs, SMALL, 0, size, BIG, plan_separate=True)
    assert not p["plan_in_chunk"] and p["cnt_base"] >= 0
    assert {k: v for k, v in p.items() if k != "plan_in_chunk"} == \
        {k: v for k, v in q.items() if k != "plan_in_chunk"}


def test_packed_body():
    """tap_result >= 0: the whole body crosses packed. lo = 0, the span is the body, one pack
    group per 2 KiB, the copy is the packed stream at pack_offset(span), and `used` - what the
    count block and the plan stay clear of - is the stream's end."""
    size, batches, recs = fetch_of([3000, 500], lead=[ATTR + 200, ATTR + 40])
    stream = size // 2 + 37
    p = plan_and_check(batches, recs, SMALL, BIG, size, BIG, tap_result=stream)
    po = (size + 63) & ~63
    assert p["packed"] and p["lo"] == 0 and p["span"] == size
    assert p["ng"] == -(-size // 2048) == 2 and p["link"] == stream
    assert (p["c_lo"], p["c_len"]) == (po, stream) and p["tab_off"] == 2 * po
    assert p["used"] == po + stream and p["plan_off"] == a256(po + stream)
    assert p["o_chunks"] == a16(8 * p["ng"]) == 16         # the pack table leads the plan
    assert p["plan"][:p["o_chunks"]] == bytes(16)          # (fill leaves it to the caller)
    assert p["cnt_base"] >= p["used"] + 64
    # raw, the same fetch: only the span of batches and records crosses
    q = plan_and_check(batches, recs, SMALL, BIG, size, BIG)
    assert not q["packed"] and q["ng"] == 0 and q["o_chunks"] == 0
    assert (q["c_lo"], q["c_len"], q["link"]) == (0, size, size) and q["used"] == size
    # a raw span starts at the first batch, rounded down to 16 bytes
    shifted = [(b0 + 1000, n) for b0, n in batches]
    srecs = [(s, vo + 1000, vl, ao, al) for s, vo, vl, ao, al in recs]
    q = plan_and_check(shifted, srecs, SMALL, BIG, size + 1000, BIG)
    assert q["lo"] == 1000 & ~15 and q["span"] == size + 1000 - q["lo"]


def test_packed_plan_stays_off_the_pack_table():
    """The plan is written while the packed body's group table still stands in the chunk (the
    caller moves it in front of the plan afterwards). A fetch of very many tiny records has a
    plan long enough to reach it from behind the stream: that plan takes the lane's buffer."""
    size, batches, recs = fetch_of([20] * 80, lead=[ATTR + 10] * 80)
    stream = size // 2 + 200
    p = plan_and_check(batches, recs, (1, 1, 1), BIG, size, BIG, tap_result=stream)
    assert p["plan_off"] < p["tab_off"] < p["plan_off"] + p["prefix"]
    assert p["plan_off"] + p["prefix"] <= p["cnt_base"] and not p["plan_in_chunk"]
    # the same stream with few records: the plan ends before the table and rides in the chunk
    size, batches, recs = fetch_of([2000, 2000])
    p = plan_and_check(batches, recs, (1, 1, 1), BIG, size, BIG, tap_result=size // 2 + 200)
    assert p["plan_off"] + p["prefix"] <= p["tab_off"] and p["plan_in_chunk"]


# ---- 4. degenerate fetches ----------------------------------------------------------------------

def test_without_crc_checks_no_windows_same_records():
    size, batches, recs = fetch_of([300, 5000])
    p = plan_and_check(batches, recs, SMALL, BIG, size, BIG)
    q = plan_and_check(batches, recs, SMALL, BIG, size, BIG, check_crcs=False)
    assert q["windows"] == [] and q["batch_windows"] == [] and q["nc"] == 0
    assert q["o_groups"] == q["o_chunks"] == 0
    for k in ("rec_of", "pjs", "ntiles", "ngroups", "ptiles", "lo", "span", "cnt_base"):
        assert q[k] == p[k], k
    assert q["plan"][q["o_recs"]:] == p["plan"][p["o_recs"]:]


def test_batches_only():
    size, batches, recs = fetch_of([100, 100], status=[1, 5])
    p = plan_and_check(batches, recs, SMALL, BIG, size, BIG)
    assert p["nc"] == 2 and p["nr"] == p["np"] == p["ntiles"] == p["ngroups"] == 0
    assert p["cnt_base"] == -1 and p["prefix"] == 32 and p["io_bytes"] == 48
    assert p["span"] == size and p["plan_in_chunk"]


def test_empty_fetch_is_the_empty_plan():
    for batches, recs, crcs in (([], [], True), ([(0, 200)], [(3, 70, 100, 13, 80)], False)):
        p = plan_and_check(batches, recs, SMALL, BIG, 200, BIG, check_crcs=crcs)
        assert p["nc"] == p["nr"] == p["np"] == 0 and p["plan"] == b""
        assert p["io_bytes"] == p["span"] == p["c_len"] == 0 and p["cnt_base"] == -1
        assert not p["plan_in_chunk"] and not p["packed"]


def test_contradictory_inputs_raise():
    size, batches, recs = fetch_of([100])
    st, vo, vl, ao, al = recs[0]
    ok = dict(arena_bytes=BIG, fetch_size=size, dev_cap=BIG)
    C.plan_json_ingest(batches, recs, *SMALL, **ok)

    def refused(b=batches, r=recs, shape=SMALL, **kw):
        with pytest.raises(ValueError):
            C.plan_json_ingest(b, r, *shape, **dict(ok, **kw))

    refused(b=[(0, size + 1)])                             # a batch past the fetch
    refused(b=[(-1, 10)])
    refused(b=[(0, -1)])
    refused(fetch_size=size - 1)                           # the value past the fetch
    refused(r=[(st, vo, vl, ao, al + 2)])                  # the array past its value
    refused(r=[(st, vo, vl, vl, 1)])
    refused(r=[(st, -1, vl, ao, al)])                      # negative extents
    refused(r=[(st, vo, -1, ao, al)])
    refused(r=[(st, vo, vl, -1, al)])
    refused(r=[(st, vo, vl, ao, -1)])
    refused(shape=(0, 2, 1))                               # H * W * C <= 0
    refused(shape=(2, -2, 1))
    refused(dev_cap=size - 1)                              # the copy past the mirror
    refused(tap_result=40, dev_cap=((size + 63) & ~63) + 39)
    # a record the scan refused is not looked at
    C.plan_json_ingest(batches, [(3, -1, -1, -1, -1)], *SMALL, **ok)


# ---- 5. stand-alone sanitizer run ---------------------------------------------------------------

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None,
                    reason="needs ROCm clang++ and make")
def test_plan_under_address_and_ub_sanitizers():
    target = "build/asan/json_plan_check"
    b = subprocess.run(["make", "-C", ROOT, target], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, target), "3000"], capture_output=True, text=True,
                       timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "all checks passed" in out
    assert "AddressSanitizer" not in out and "runtime error" not in out
