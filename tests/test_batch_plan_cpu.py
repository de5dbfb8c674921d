"""The host plan of a GPU replica's batch (csrc/runtime/batch_plan.h: MetaLayout, plan_batch +
fill_batch) without a GPU: the spans, the staged copies, the counts and every metadata byte against
an independent Python derivation written from the layout's description -

  [64-byte header: records, tiles, images, b64 descriptors]
  [JsonRecord (48 bytes) x max_batch][input pointer (8 bytes) x max_batch][tile -> record i32]
  b64: [B64Image (16 bytes) x max_batch][status i32 x max_batch] in the record table's place

- the tile boundaries, the staging's phases, resident and preparsed records, the b64 table, the
batch-size limit, the bytes each step form copies; and a stand-alone sanitizer run."""

import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from gale._native import native

C = native()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = C.JSON_TILE_BYTES
REC = np.dtype([("off", "<i8"), ("len", "<i4"), ("slot", "<i4"), ("images", "<i4"),
                ("status", "<i4"), ("tile0", "<i4"), ("has_cnt", "<i4"), ("cnt_off", "<i8"),
                ("grp0", "<i8")])
assert REC.itemsize == 48 == C.JSON_RECORD_BYTES
HDR, PTR, DESC = 64, 8, 16
FORMS = ("op-by-op", "captured", "kernels")
D_BYTES = 0x7F0000100000     # the slot's text buffer, a 256-byte-aligned device address
INPUT = 0x7F0000A00000       # the slot's input buffer
MIRROR = 0x7E0000000400      # a fetch mirror elsewhere in device memory (below the slot's buffer)
ARENA = 0x7D0000000000       # an ingest image arena
PER = 28 * 28                # elements per image


def a16(n):
    return (n + 15) & ~15


def tiles(phase, ln):
    """2 KiB tiles of a text of ln bytes that starts `phase` bytes into a 16-byte word."""
    return 0 if ln <= 0 else -(-((phase & 15) + ln) // T)


def pinned(buf, off, ln, images=1):
    return dict(buf=buf, arr_off=off, arr_len=ln, images=images, pinned=True)


def pageable(buf, off, ln, images=1):
    return dict(buf=buf, arr_off=off, arr_len=ln, images=images)


def resident(off, ln, images=1, counts=0, image=0, preparsed=False):
    return dict(arr_len=ln, images=images, resident=True, dev_text=MIRROR + off,
                dev_counts=counts, dev_image=image, preparsed=preparsed)


def used_bytes(form, mb, cap, nrec, ntiles, b64n, ptr_input, b64):
    """(offset, bytes) of the metadata a step copies: the size expressions of the replica before
    it had a plan (its submit() and step_for())."""
    rec_bytes = (48 + PTR) * mb
    if form == "op-by-op":     # from the record table on; b64: descriptors + status words
        return HDR, (DESC + 4) * mb if b64 else rec_bytes + 4 * ntiles
    if form == "captured":     # the whole allocation
        return 0, HDR + rec_bytes + 4 * cap
    if ntiles > 0:
        return 0, HDR + rec_bytes + 4 * ntiles
    if ptr_input:
        return 0, HDR + rec_bytes
    return 0, HDR + (DESC * b64n if b64 else 48 * nrec)


def derive(recs, mb, cap, form, ptr_input=False, b64=False):
    """Everything plan_batch + fill_batch produce, from the description."""
    spans, staged, cursor = [], [], 0
    for i, r in enumerate(recs):
        if r.get("resident"):
            continue
        lo, hi = r["arr_off"], r["arr_off"] + r["arr_len"]
        if not r.get("pinned"):
            host = cursor + lo % 16
            staged.append((i, host, r["arr_len"]))
            cursor = a16(host + r["arr_len"])
            continue
        for sp in spans:
            if sp[0] == r["buf"]:
                sp[1], sp[2] = min(sp[1], lo), max(sp[2], hi)
                break
        else:
            spans.append([r["buf"], lo, hi])
    placed, dev = [], 0
    for buf, lo, hi in spans:
        lo &= ~15
        placed.append((buf, lo, hi - lo, dev))
        dev += a16(hi - lo)
    staged_dev = dev
    host_of = {i: h for i, h, _ in staged}
    meta = bytearray(b"\xee" * (HDR + 56 * mb + 4 * cap))
    o_recs, o_xs, o_tiles = HDR, HDR + 48 * mb, HDR + 56 * mb
    o_status = HDR + DESC * mb
    parse_idx, nrec, ntiles, img, b64n, npre, nres, count_pass = [], 0, 0, 0, 0, 0, 0, False
    jrecs, descs, tile_map, xs = [], [], [], []
    for i, r in enumerate(recs):
        nres += bool(r.get("resident"))
        if r.get("preparsed"):
            parse_idx.append(-1)
            npre += 1
            xs += [r["dev_image"] + 4 * PER * k for k in range(r["images"])]
            img += r["images"]
            continue
        parse_idx.append(nrec)
        xs += [INPUT + 4 * PER * (img + k) for k in range(r["images"])]
        if r.get("resident"):
            off = r["dev_text"] - D_BYTES
        elif r.get("pinned"):
            buf, lo, _, d = next(p for p in placed if p[0] == r["buf"])
            off = d + r["arr_off"] - lo
        else:
            off = staged_dev + host_of[i]
        if b64:
            descs += [(off + o, img + k, nrec) for k, o in enumerate(r["b64_offs"])]
            b64n += r["images"]
        else:
            has = bool(r.get("resident") and r.get("dev_counts"))
            count_pass |= not has
            nt = tiles(off, r["arr_len"])
            jrecs.append((off, r["arr_len"], img, r["images"], 0, ntiles, int(has),
                          r["dev_counts"] - D_BYTES if has else 0, 0))
            tile_map += [nrec] * nt
            ntiles += nt
        nrec += 1
        img += r["images"]
    u_off, u_len = used_bytes(form, mb, cap, nrec, ntiles, b64n, ptr_input, b64)

    def put(off, data):  # (what lies outside the copied bytes is not written)
        n = max(0, min(len(data), u_off + u_len - off))
        meta[off:off + n] = data[:n]

    if form != "op-by-op":
        put(0, struct.pack("<4i", nrec, ntiles, img, b64n))
    if b64:
        put(HDR, b"".join(struct.pack("<qii", *d) for d in descs))
        put(o_status, bytes(4 * nrec))
    else:
        put(o_recs, np.array(jrecs, dtype=REC).tobytes())
        put(o_tiles, struct.pack(f"<{ntiles}i", *tile_map))
    if ptr_input:
        put(o_xs, struct.pack(f"<{img}Q", *xs))
    return dict(spans=placed, staged=staged, parse_idx=parse_idx, staged_bytes=cursor,
                staged_dev=staged_dev, dev_total=16 + staged_dev + cursor, nrec=nrec,
                ntiles=ntiles, img=img, b64n=b64n, npre=npre, resident=nres,
                count_pass=count_pass, used=(u_off, u_len), meta=bytes(meta),
                layout=dict(hdr=0, recs=o_recs, xs=o_xs, tiles=o_tiles, b64_table=HDR,
                            b64_status=o_status, total=len(meta)))


def check(recs, mb=8, cap=64, forms=FORMS, ptr_input=False, b64=False):
    """Plan and fill in every form; each must equal the derivation in every field and byte."""
    want = None
    for form in forms:
        got = C.plan_batch(recs, max_batch=mb, tiles_cap=cap, per=PER, form=form,
                           ptr_input=ptr_input, b64=b64, d_bytes=D_BYTES, input_base=INPUT)
        want = derive(recs, mb, cap, form, ptr_input, b64)
        for k, v in want.items():
            g = got[k]
            if k in ("spans", "staged"):
                g = [tuple(x) for x in g]
            assert g == v, (form, k, g if k != "meta" else "bytes differ")
    return want


def records(want, mb=8):
    return np.frombuffer(want["meta"], dtype=REC, count=mb, offset=HDR)


def test_one_pinned_record_phase_0_and_5():
    for phase in (0, 5):
        w = check([pinned(1, 4096 + phase, 300, images=2)])
        assert w["spans"] == [(1, 4096, 300 + phase, 0)] and not w["staged"]
        r = records(w)[0]
        assert (r["off"], r["len"], r["slot"], r["images"], r["tile0"]) == (phase, 300, 0, 2, 0)
        assert w["ntiles"] == 1 and w["count_pass"] and w["dev_total"] == 16 + a16(300 + phase)


@pytest.mark.parametrize("phase,ln,nt", [(0, 2048, 1), (0, 2049, 2), (15, 2034, 2), (7, 0, 0)])
def test_tile_boundaries(phase, ln, nt):
    w = check([pinned(1, 160 + phase, ln), pinned(1, 8192, 10)])
    assert w["ntiles"] == nt + 1
    assert list(records(w)["tile0"][:2]) == [0, nt]
    tile_map = np.frombuffer(w["meta"], "<i4", count=nt + 1, offset=w["layout"]["tiles"])
    assert list(tile_map) == [0] * nt + [1]


def test_two_fetch_buffers_interleaved():
    recs = [pinned(7, 1000, 100), pinned(9, 50, 20), pinned(7, 200, 40), pinned(9, 5000, 3000),
            pinned(7, 600, 10)]
    w = check(recs)
    # one span per buffer, from its lowest record (16-aligned down) to its highest end
    assert w["spans"] == [(7, 192, 1100 - 192, 0), (9, 48, 8000 - 48, a16(1100 - 192))]
    d9 = a16(1100 - 192)
    assert list(records(w)["off"][:5]) == [1000 - 192, d9 + 2, 8, d9 + 5000 - 48, 600 - 192]


def test_pageable_records_keep_their_phase():
    lens, phases = (1, 15, 16, 17, 16, 1), (0, 15, 1, 9, 0, 15)
    recs = [pageable(100 + i, 64 * i + p, n) for i, (n, p) in enumerate(zip(lens, phases))]
    w = check(recs)
    assert not w["spans"] and w["staged_dev"] == 0
    end = 0
    for (i, host, n), p in zip(w["staged"], phases):
        assert host % 16 == p and host >= end and n == lens[i]   # phase kept, no overlap
        end = host + n
    assert end <= w["staged_bytes"] == a16(end)
    # within what the replica once reserved up front, (len + 31) & ~15 per record
    assert w["staged_bytes"] <= sum((n + 31) & ~15 for n in lens)
    assert list(records(w)["off"][:6]) == [h for _, h, _ in w["staged"]]
    # behind a pinned span the staged bytes start at its 16-aligned end
    w = check([pinned(1, 37, 100)] + recs)
    assert w["staged_dev"] == a16(100 + 5) and records(w)["off"][1] == w["staged_dev"]


def test_resident_records_and_counts():
    recs = [resident(0x123, 5000, counts=MIRROR + 0x8000), resident(0x2345, 100),
            pinned(3, 16, 50)]
    w = check(recs)
    r = records(w)
    assert list(r["has_cnt"][:3]) == [1, 0, 0] and w["resident"] == 2
    assert r["off"][0] == MIRROR + 0x123 - D_BYTES < 0     # a signed distance
    assert r["cnt_off"][0] == MIRROR + 0x8000 - D_BYTES and r["cnt_off"][1] == 0
    assert list(r["tile0"][:3]) == [0, tiles(3, 5000), tiles(3, 5000) + 1]
    assert w["count_pass"] and w["spans"] == [(3, 16, 50, 0)]
    # no counting pass exactly when every parsed record brings its counts
    w = check([resident(0x123, 5000, counts=MIRROR + 0x8000),
               resident(0x4000, 9, image=ARENA, preparsed=True)], ptr_input=True,
              forms=("kernels",))
    assert not w["count_pass"] and w["dev_total"] == 16


def test_preparsed_and_parsed_mixed():
    recs = [resident(0, 10, images=2, image=ARENA + 4 * PER * 3, preparsed=True),
            pinned(1, 21, 3000, images=1),
            resident(64, 10, images=3, image=ARENA + 4 * PER * 40, preparsed=True),
            resident(0x77, 2100, images=2, counts=MIRROR + 0x9000)]
    w = check(recs, ptr_input=True, forms=("kernels",))
    assert w["parse_idx"] == [-1, 0, -1, 1] and (w["nrec"], w["npre"], w["img"]) == (2, 2, 8)
    xs = struct.unpack_from("<8Q", w["meta"], w["layout"]["xs"])
    one = 4 * PER
    assert xs == (ARENA + 3 * one, ARENA + 4 * one, INPUT + 2 * one, ARENA + 40 * one,
                  ARENA + 41 * one, ARENA + 42 * one, INPUT + 6 * one, INPUT + 7 * one)
    r = records(w)
    assert list(r["slot"][:2]) == [2, 6] and list(r["tile0"][:2]) == [0, 2]
    assert w["ntiles"] == 2 + tiles(7, 2100)


def test_all_preparsed_batch_the_table_step_refuses():
    # 17 arenas: the replica's one-launch table step takes 16, so the batch comes here
    recs = [resident(32 * i, 8, image=ARENA + (i << 32), preparsed=True) for i in range(17)]
    w = check(recs, mb=32, ptr_input=True, forms=("kernels",))
    assert (w["nrec"], w["ntiles"], w["img"], w["npre"]) == (0, 0, 17, 17)
    assert w["used"] == (0, HDR + 48 * 32 + 8 * 32) and not w["count_pass"]
    assert struct.unpack_from("<4i", w["meta"]) == (0, 0, 17, 0)


def test_b64_dense_table_beside_preparsed_records():
    L = 4 * ((PER + 2) // 3)
    frag = dict(pinned(5, 1003, 2 * (L + 12), images=2), b64_offs=[9, L + 21])
    recs = [resident(0, 10, images=3, image=ARENA, preparsed=True), frag,
            resident(64, 10, images=1, image=ARENA + 4 * PER * 9, preparsed=True),
            dict(pageable(6, 77, L + 12), b64_offs=[9])]
    w = check(recs, ptr_input=True, b64=True, forms=("kernels",))
    assert (w["nrec"], w["b64n"], w["img"], w["ntiles"]) == (2, 3, 7, 0)
    assert struct.unpack_from("<4i", w["meta"]) == (2, 0, 7, 3)   # its own descriptor count
    o = 1003 - 992
    descs = [struct.unpack_from("<qii", w["meta"], HDR + 16 * k) for k in range(3)]
    assert descs == [(o + 9, 3, 0), (o + L + 21, 4, 0), (w["staged_dev"] + 77 % 16 + 9, 6, 1)]
    status = w["layout"]["b64_status"]
    assert w["meta"][status:status + 12] == bytes(8) + b"\xee" * 4  # parsed records' words only
    # without the pointer table the steps copy descriptors only, or the table and its words
    pair = [frag, dict(pageable(6, 77, L + 12), b64_offs=[9])]
    assert check(pair, b64=True, forms=("op-by-op",))["used"] == (HDR, 20 * 8)
    w = check(pair, b64=True, forms=("captured", "kernels"))
    assert w["used"] == (0, HDR + 16 * 3)
    assert w["meta"][status:status + 8] == b"\xee" * 8    # (words that are not copied)
    # a record that does not match its scan
    with pytest.raises(Exception, match="does not match its scan"):
        C.plan_batch([dict(frag, b64_offs=[9])], max_batch=8, tiles_cap=4, per=PER,
                     form="kernels", b64=True)


def test_batch_size_limit():
    recs = [pinned(1, 100 * i, 50, images=n) for i, n in enumerate((3, 4, 1))]
    assert check(recs)["img"] == 8                         # exactly max_batch
    for extra in (pinned(1, 900, 50), resident(0, 9, image=ARENA, preparsed=True)):
        with pytest.raises(Exception, match="exceeds max_batch"):
            C.plan_batch(recs + [extra], max_batch=8, tiles_cap=64, per=PER, form="kernels",
                         ptr_input=True)


def test_used_bytes_of_every_form():
    mb, cap = 8, 64
    json_recs = [pinned(1, 5, 3000), pinned(1, 4000, 10)]
    L = 4 * ((PER + 2) // 3)
    b64_recs = [dict(pinned(1, 5, L + 12), b64_offs=[9])]
    lay = C.plan_batch(json_recs, max_batch=mb, tiles_cap=cap, per=PER, form="kernels")["layout"]
    assert lay == dict(hdr=0, recs=64, xs=64 + 48 * mb, tiles=64 + 56 * mb, b64_table=64,
                       b64_status=64 + 16 * mb, total=64 + 56 * mb + 4 * cap)

    def used(recs, form, **kw):
        return tuple(C.plan_batch(recs, max_batch=mb, tiles_cap=cap, per=PER, form=form,
                                  **kw)["used"])

    rec_bytes = 56 * mb
    # op by op: from the record table to the end of the batch's tile map; b64: table + words
    assert used(json_recs, "op-by-op") == (64, rec_bytes + 4 * 3)
    assert used(b64_recs, "op-by-op", b64=True) == (64, 20 * mb)
    # the captured step without the device formatter copies the whole allocation
    assert used(json_recs, "captured") == (0, 64 + rec_bytes + 4 * cap)
    assert used(b64_recs, "captured", b64=True) == (0, 64 + rec_bytes + 4 * cap)
    # the kernels-only step: header + records + pointers + tile map / ... + pointers / the
    # descriptors / the records
    assert used(json_recs, "kernels") == (0, 64 + rec_bytes + 4 * 3)
    assert used(json_recs, "kernels", ptr_input=True) == (0, 64 + rec_bytes + 4 * 3)
    assert used(b64_recs, "kernels", b64=True, ptr_input=True) == (0, 64 + rec_bytes)
    assert used(b64_recs, "kernels", b64=True) == (0, 64 + 16)
    empty = [pinned(1, 5, 0), pinned(1, 9, 0)]             # (no tiles at all)
    assert used(empty, "kernels") == (0, 64 + 48 * 2)
    assert used(empty, "kernels", ptr_input=True) == (0, 64 + rec_bytes)


# ---- stand-alone sanitizer run ------------------------------------------------------------------

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None,
                    reason="needs ROCm clang++ and make")
def test_plan_under_address_and_ub_sanitizers():
    target = "build/asan/batch_plan_check"
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
