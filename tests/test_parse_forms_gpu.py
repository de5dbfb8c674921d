"""The serving forms of json_parse_instances at kernel level: the ingest form (the image count
from the group sums on the device, one plain-stored verdict per tile into host-mapped memory, no
count pass) and the captured step's form (tile count on the device, verdicts in a separate
status[] array, recs and the tile map only read from host-mapped memory), plus the preprocessing
instantiation in the ingest form.

The reference values are the float32 arrays the text was encoded from (C.encode_instances round
trips: bit equality), InputPrep.apply of them for the prep case, and the plain form's record
statuses (test_engine_gpu.gpu_parse) for the verdicts. The arena is prefilled with -7.0 and every
result array with a sentinel; staging comes from tests/test_engine_gpu.py."""

import json

import numpy as np
import pytest
import torch

from gale._native import native
from gale.models.preprocess import InputPrep
from test_engine_gpu import array_text, gpu_parse, host_tile_tokens, stage

pytestmark = pytest.mark.gpu

C = native()
G = C.GROUP_TILES
T = C.JSON_TILE_BYTES
CIFAR = (32, 32, 3)
FILL = -7.0
WORD_FILL = 0x5A5A5A5A
CIFAR_MEAN_S = "0.4914,0.4822,0.4465"
CIFAR_STD_S = "0.2470,0.2435,0.2616"


def stream():
    return torch.cuda.current_stream().cuda_stream


def record_tiles(r):
    return C.json_tile_count(int(r["off"]), int(r["len"]))


def tile_map(recs, n):
    """Owning record of every global tile; entries past the last record's tiles name record 0."""
    m = np.zeros(n, dtype=np.int32)
    for i, r in enumerate(recs):
        m[r["tile0"]:r["tile0"] + record_tiles(r)] = i
    return m


def mapped(parts):
    """The byte arrays of `parts` 16-byte aligned in ONE host-mapped buffer: (buffer, uint8 view,
    offsets)."""
    offs, o = [], 0
    for a in parts:
        offs.append(o)
        o += (a.nbytes + 15) & ~15
    mb = C.MappedBuffer(o + 16)
    v = mb.numpy()
    for a, off in zip(parts, offs):
        v[off:off + a.nbytes] = np.frombuffer(a.tobytes(), dtype=np.uint8)
    return mb, v, offs


def ingest_parse(arrays, dims, reserve, **prep_kw):
    """The ingest form over records `arrays` ((text, images) pairs): the counting launch
    (ingest_crc_count, no CRC windows) leaves every record's count block on the device, then ONE
    parse launch with images = -1, has_cnt = 1, no count pass, tile_bad / recs / tile map in one
    host-mapped buffer. Record i gets reserve[i] arena slots and one unowned slot behind them.
    Returns (arena [slots, H, W, C] float32, first slot per record, tile verdicts per record,
    the words behind the last tile's verdict)."""
    H, Wd, Cc = dims
    raw, recs, _, tiles = stage(arrays)
    slot0, s = [], 0
    for n in reserve:
        slot0.append(s)
        s += n + 1
    recs["slot"] = slot0
    groups, grp0 = [], []
    for i, r in enumerate(recs):
        grp0.append(len(groups))
        groups += [(i, t0) for t0 in range(0, record_tiles(r), G)]
    recs["pad"] = grp0  # JsonRecord::grp0
    d = torch.from_numpy(raw.copy()).cuda()
    drec = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    dgrp = torch.tensor(np.array(groups, dtype=np.int32).reshape(-1), device="cuda")
    cnt = torch.full((tiles + len(groups),), -1, dtype=torch.int32, device="cuda")
    gsum = torch.full((len(groups),), -1, dtype=torch.int32, device="cuda")
    C.ingest_crc_count(d.data_ptr(), 0, 0, 0, 0, len(recs), len(groups), drec.data_ptr(),
                       dgrp.data_ptr(), cnt.data_ptr(), gsum.data_ptr(), stream())
    recs2 = recs.copy()
    recs2["images"] = -1  # from the group sums, on the device
    recs2["has_cnt"] = 1
    recs2["cnt_off"] = [cnt.data_ptr() + 4 * (int(r["tile0"]) + grp0[i]) - d.data_ptr()
                        for i, r in enumerate(recs)]
    bad = np.full(tiles + 4, WORD_FILL, dtype=np.uint32)
    mb, v, (o_recs, o_map, o_bad) = mapped([recs2.view(np.uint8), tile_map(recs, tiles), bad])
    arena = torch.full((s, H, Wd, Cc), FILL, device="cuda")
    scratch = torch.full((tiles,), 123456, dtype=torch.int32, device="cuda")  # unused
    C.json_parse_instances(len(recs), tiles, mb.ptr + o_recs, mb.ptr + o_map, d.data_ptr(), H,
                           Wd, Cc, scratch.data_ptr(), arena.data_ptr(), stream(),
                           count_pass=False, tile_bad=mb.ptr + o_bad, **prep_kw)
    torch.cuda.synchronize()
    assert (scratch.cpu().numpy() == 123456).all()
    assert bytes(v[o_recs:o_recs + recs2.nbytes]) == recs2.tobytes()  # only read
    words = v[o_bad:o_bad + bad.nbytes].view(np.uint32).copy()
    per_rec = [words[r["tile0"]:r["tile0"] + record_tiles(r)] for r in recs]
    return arena.cpu().numpy(), slot0, per_rec, words[tiles:]


def check_arena(arena, slot0, xs):
    """Record i's images xs[i] bit exact at its slots (an int: that many slots are the record's
    to write, unchecked; None: nothing may be stored); every other float of the arena still the
    prefill."""
    owned = np.zeros(len(arena), dtype=bool)
    for s, x in zip(slot0, xs):
        if x is None:
            continue
        if isinstance(x, int):
            owned[s:s + x] = True
            continue
        owned[s:s + len(x)] = True
        np.testing.assert_array_equal(arena[s:s + len(x)].view(np.uint32), x.view(np.uint32))
    assert (arena[~owned] == FILL).all()


def float_records(rng, counts, dims, digits=None):
    """digits: the values rounded to that many decimals (short text: more images per tile)."""
    xs = [rng.random((n,) + dims, dtype=np.float32) for n in counts]
    if digits:
        xs = [np.round(x, digits).astype(np.float32) for x in xs]
    return xs, [array_text(C.encode_instances(x), *dims) for x in xs]


# ---- the ingest form ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["one_tile", "cifar", "cifar16"])
def test_ingest_form_good_records(case):
    rng = np.random.default_rng(31)
    if case == "one_tile":
        dims, counts = (5, 4, 3), (1, 3, 2)
    elif case == "cifar":
        dims, counts = CIFAR, (1, 3, 2)
    else:
        dims, counts = CIFAR, (16,)
    xs, arrays = float_records(rng, counts, dims, digits=4 if case == "one_tile" else None)
    nts = [C.json_tile_count(0, len(t)) for t, _ in arrays]
    if case == "one_tile":
        assert nts == [1, 1, 1]
    elif case == "cifar16":
        # the per-lane loops over the group sums (image count; a tile's element base) take a
        # second trip from group 64 on: a sum over min(groups, 64) groups comes out short here
        ngroups = -(-nts[0] // G)
        assert nts[0] >= 257 and ngroups > 64, (nts, ngroups)
        tok = host_tile_tokens(arrays[0][0], 0, len(arrays[0][0]))
        assert tok.sum() == xs[0].size and tok[:64 * G].sum() < tok.sum()
        assert tok[:64 * G].sum() % (32 * 32 * 3) != 0  # (the short sum: no whole images)
    arena, slot0, bad, tail = ingest_parse(arrays, dims, counts)
    check_arena(arena, slot0, xs)
    for b in bad:
        assert (b == 0).all(), b
    assert (tail == WORD_FILL).all()  # no verdict stored behind the last tile


def test_ingest_form_verdicts_are_localised():
    """good | malformed number | last number dropped | ragged nesting, right count | good."""
    rng = np.random.default_rng(32)
    (x0, _, _, x1), arrays = float_records(rng, (2, 1, 1, 1), CIFAR)
    good0, badnum, short, good1 = [t for t, _ in arrays]
    i = badnum.index(b",", 9000)  # a middle tile
    badnum = badnum[:i] + b".5.5" + badnum[i:]  # "0.123.5.5": a number with two points
    tok0 = max(badnum.rindex(b",", 0, i), badnum.rindex(b"[", 0, i)) + 1
    short = short[:short.rindex(b",")] + b"]]]]"  # 3071 elements
    x = rng.random((1,) + CIFAR, dtype=np.float32).tolist()
    x[0][0][1] = x[0][0][1] + [x[0][0][0].pop()]  # pixel (0, 0): 2 values, pixel (0, 1): 4
    ragged = json.dumps({"instances": x}).encode()
    ragged = ragged[ragged.index(b"["):ragged.rindex(b"]") + 1]
    arrays = [(good0, 2), (badnum, 1), (short, 1), (ragged, 1), (good1, 1)]
    _, plain = gpu_parse(arrays, *CIFAR)
    assert list(plain[[0, 2, 3, 4]]) == [0, 1, 3, 0] and plain[1] in (2, 3)

    arena, slot0, bad, tail = ingest_parse(arrays, CIFAR, (2, 1, 1, 1, 1))
    assert (tail == WORD_FILL).all()
    assert (bad[0] == 0).all() and (bad[4] == 0).all()
    # the malformed number: the plain form's verdict, on the tiles of the token or next to them
    nt = len(bad[1])
    t_lo, t_hi = tok0 // T, (i + 3) // T
    assert 0 < t_lo and t_hi < nt - 1
    assert bad[1].max() == plain[1]
    far = [t for t in range(nt) if t < t_lo - 1 or t > t_hi + 1]
    assert (bad[1][far] == 0).all(), bad[1]
    # the dropped number: no whole number of images, so nothing is expected and nothing stored;
    # only the record's last tile reports the count
    assert list(bad[2]) == [0] * (len(bad[2]) - 1) + [1]
    assert bad[3].max() == 3
    # the good records bit exact, the short record's slots and every unowned slot untouched; the
    # two bad records of the right count store only inside their own slots
    check_arena(arena, slot0, [x0, 1, None, 1, x1])


def test_ingest_form_prep_instantiation():
    """json_parse_prep_kernel in the ingest form: NCHW-nested records of 1, 3 and 2 CIFAR images
    with the CIFAR scale / mean / std, stored NHWC as InputPrep.apply of the source."""
    rng = np.random.default_rng(33)
    H, Wd, Cc = CIFAR
    prep = InputPrep.build(Cc, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S, "nchw")
    xs = [(rng.random((n,) + CIFAR, dtype=np.float32) * 255).astype(np.float32)
          for n in (1, 3, 2)]
    arrays = [array_text(C.encode_instances(np.ascontiguousarray(x.transpose(0, 3, 1, 2))),
                         Cc, H, Wd) for x in xs]
    arena, slot0, bad, tail = ingest_parse(arrays, CIFAR, (1, 3, 2), **prep.kernel_kwargs())
    check_arena(arena, slot0, [prep.apply(x) for x in xs])
    for b in bad:
        assert (b == 0).all(), b
    assert (tail == WORD_FILL).all()


def test_tile_verdicts_need_counted_records():
    rng = np.random.default_rng(34)
    _, arrays = float_records(rng, (1,), (5, 4, 3))
    raw, recs, total, tiles = stage(arrays)
    d = torch.from_numpy(raw.copy()).cuda()
    drec = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    dmap = torch.from_numpy(tile_map(recs, tiles)).cuda()
    cnt = torch.zeros(tiles, dtype=torch.int32, device="cuda")
    out = torch.full((total, 5, 4, 3), FILL, device="cuda")
    bad = torch.full((tiles + 1,), 77, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        C.json_parse_instances(1, tiles, drec.data_ptr(), dmap.data_ptr(), d.data_ptr(), 5, 4, 3,
                               cnt.data_ptr(), out.data_ptr(), stream(), count_pass=True,
                               tile_bad=bad.data_ptr())
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all() and (bad.cpu().numpy() == 77).all()


# ---- the captured step's form ------------------------------------------------------------------

@pytest.mark.parametrize("dev_tiles", ["all", "none"])
def test_step_graph_form(dev_tiles):
    """good | malformed number | last number dropped | good, host-given image counts, count pass
    on, the launch sized for twice the tiles the device count admits."""
    rng = np.random.default_rng(35)
    (x0, _, _, x1), arrays = float_records(rng, (2, 1, 1, 1), CIFAR)
    texts = [t for t, _ in arrays]
    i = texts[1].index(b",", 9000)
    texts[1] = texts[1][:i] + b".5.5" + texts[1][i:]
    texts[2] = texts[2][:texts[2].rindex(b",")] + b"]]]]"
    arrays = [(t, n) for t, (_, n) in zip(texts, arrays)]
    _, plain = gpu_parse(arrays, *CIFAR)
    assert plain[0] == 0 and plain[1] in (2, 3) and plain[2] == 1 and plain[3] == 0

    H, Wd, Cc = CIFAR
    raw, recs, total, tiles = stage(arrays)
    nrec = len(recs)
    mb, v, (o_recs, o_map) = mapped([recs.view(np.uint8), tile_map(recs, 2 * tiles)])
    before = bytes(v)
    d = torch.from_numpy(raw.copy()).cuda()
    real = tiles if dev_tiles == "all" else 0
    d_ntiles = torch.tensor([real], dtype=torch.int32, device="cuda")
    status0 = np.array([0] * nrec + [WORD_FILL] * 4, dtype=np.int32)
    status = torch.from_numpy(status0.copy()).cuda()
    counts = torch.full((2 * tiles,), 123456, dtype=torch.int32, device="cuda")
    arena = torch.full((total + 1, H, Wd, Cc), FILL, device="cuda")
    C.json_parse_instances(nrec, 2 * tiles, mb.ptr + o_recs, mb.ptr + o_map, d.data_ptr(), H, Wd,
                           Cc, counts.data_ptr(), arena.data_ptr(), stream(), count_pass=True,
                           d_ntiles=d_ntiles.data_ptr(), status=status.data_ptr())
    torch.cuda.synchronize()
    assert bytes(v) == before  # recs[].status and the tile map: only read
    st = status.cpu().numpy()
    got = arena.cpu().numpy()
    cn = counts.cpu().numpy()
    assert (st[nrec:] == WORD_FILL).all()
    assert (cn[real:] == 123456).all()  # no tile past the device count was counted
    if dev_tiles == "none":
        assert (st[:nrec] == 0).all() and (got == FILL).all()
        return
    assert list(st[:nrec]) == list(plain)
    for r, x in ((recs[0], x0), (recs[3], x1)):
        s = int(r["slot"])
        np.testing.assert_array_equal(got[s:s + len(x)].view(np.uint32), x.view(np.uint32))
    assert (got[total:] == FILL).all()
    # the short record stores its 3071 numbers and leaves the last float of its slot alone
    s = int(recs[2]["slot"])
    assert got[s].reshape(-1)[-1] == FILL and (got[s].reshape(-1)[:-1] != FILL).all()
