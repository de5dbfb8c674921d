"""Device throughput of the GPU ingest kernels on their own (no other stream competing): the fused
CRC32C + token-count pass (ingest_crc_count) over a fetch-sized buffer and the JSON parse of its
records, for CIFAR (32x32x3, ~35 KB per image) and ImageNet (224x224x3, ~1.7 MB) records.

usage: python tools/bench_ingest.py [--iters 50]
Prints one JSON line per (shape, kernel): us per launch and GB/s of JSON text.

--encoding b64: the base64 ingest (ingest_crc_b64) over a fetch of one-image records, CRC windows
over the whole body included, against the same work as two launches on the same buffer
(crc32c_chunks + b64_decode_instances), alternating --rounds times in one process. One JSON line
per (case, round, contender); --out appends them to a file.
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gale._native import native  # noqa: E402

C = native()
K = C.kafka
REC = np.dtype([("off", "<i8"), ("len", "<i4"), ("slot", "<i4"), ("images", "<i4"),
                ("status", "<i4"), ("tile0", "<i4"), ("has_cnt", "<i4"), ("cnt_off", "<i8"),
                ("pad", "<i8")])


def build(shape, nrec, seed=0):
    rng = np.random.default_rng(seed)
    H, W, Cc = shape
    x = rng.random((1, H, W, Cc), dtype=np.float32)
    s, off, ln, n = C.scan_instances(C.encode_instances(x), H, W, Cc)
    txt = C.encode_instances(x)[off:off + ln]
    buf = bytearray()
    recs = np.zeros(nrec, dtype=REC)
    tiles = 0
    for i in range(nrec):
        recs[i] = (len(buf), len(txt), i, 1, 0, tiles, 0, 0, 0)
        tiles += C.json_tile_count(len(buf), len(txt))
        buf += txt + b" " * ((-len(txt)) % 16)
    buf += b" " * 64
    tile_rec = np.zeros(tiles, dtype=np.int32)
    groups = []
    for i, r in enumerate(recs):
        t = C.json_tile_count(int(r["off"]), int(r["len"]))
        tile_rec[r["tile0"]:r["tile0"] + t] = i
        recs[i]["pad"] = len(groups)  # JsonRecord::grp0
        groups += [(i, t0) for t0 in range(0, t, C.GROUP_TILES)]
    n = len(buf) - 64
    wins = [(n - 4096 * k, 4096) for k in range(n // 4096)][::-1]
    if n % 4096:
        wins = [(n - 4096 * len(wins), n % 4096)] + wins
    ch = np.zeros(len(wins), dtype=[("end", "<i8"), ("len", "<i4"), ("pad", "<i4")])
    for i, (e, w) in enumerate(wins):
        ch[i] = (e, w, 0)
    return bytes(buf), recs, tile_rec, tiles, ch, n, np.array(groups, dtype=np.int32)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


IMG = np.dtype([("off", "<i8"), ("slot", "<i4"), ("rec", "<i4")])
WIN = np.dtype([("end", "<i8"), ("len", "<i4"), ("pad", "<i4")])


def main_b64(a):
    from gale import ops
    from gale.data import encode_records_b64, synthetic_pixels
    from gale.models.preprocess import InputPrep

    s = torch.cuda.current_stream().cuda_stream
    tables = torch.tensor(np.array(K.crc32c_device_tables(), dtype=np.uint32).view(np.int32),
                          device="cuda")
    prep = InputPrep.build(3, 1 / 255, "0.4914,0.4822,0.4465", "0.2470,0.2435,0.2616")
    for name, shape, nimg in (("cifar_1024", (32, 32, 3), 1024),
                              ("imagenet_64", (224, 224, 3), 64)):
        H, W, Cc = shape
        recs = encode_records_b64(synthetic_pixels(nimg, shape, 0), 1)
        buf = bytearray()
        offs = []
        for r in recs:  # record values back to back behind a few framing bytes, as in a fetch
            buf += bytes(7)
            st, arr_off, arr_len, n = C.scan_instances_b64(r, H, W, Cc)
            assert st == 0 and n == 1
            offs.append(len(buf) + arr_off + C.b64_image_offsets(r[arr_off:arr_off + arr_len],
                                                                 H, W, Cc)[0])
            buf += r
        n = len(buf)
        nw = -(-n // 4096)
        ch = np.zeros(nw, dtype=WIN)
        for k in range(nw):
            ch[k] = (n - 4096 * (nw - 1 - k), n - 4096 * (nw - 1) if k == 0 else 4096, 0)
        tab = np.zeros(nimg, dtype=IMG)
        tab["off"], tab["slot"], tab["rec"] = offs, np.arange(nimg), np.arange(nimg)
        d = torch.frombuffer(bytearray(bytes(buf) + bytes(64)), dtype=torch.uint8).cuda()
        dch = torch.from_numpy(ch.view(np.int32).reshape(-1, 4).copy()).cuda()
        dtab = torch.from_numpy(tab.view(np.int32).reshape(-1, 4).copy()).cuda()
        cpi = -(-(4 * ((H * W * Cc + 2) // 3)) // C.B64_CHUNK_CHARS)
        crc = [torch.zeros(nw, dtype=torch.int32, device="cuda") for _ in range(2)]
        out = [torch.empty((nimg, H, W, Cc), device="cuda") for _ in range(2)]
        bad = torch.full((nimg * cpi,), 7, dtype=torch.int32, device="cuda")
        status = torch.zeros(nimg, dtype=torch.int32, device="cuda")

        def fused():
            ops.ingest_crc_b64(d, shape, arena=out[0], table=dtab, wg_bad=bad, windows=dch,
                               tables=tables, crc_out=crc[0], prep=prep)

        def pair():
            C.crc32c_chunks(d.data_ptr(), dch.data_ptr(), nw, tables.data_ptr(),
                            crc[1].data_ptr(), s)
            ops.b64_decode_instances(d, dtab, shape, out[1], status, prep=prep)

        for rnd in range(a.rounds):
            for kname, fn in (("fused", fused), ("crc;decode", pair)):
                us = timed(fn, a.iters)
                line = json.dumps(dict(tool="bench_ingest", encoding="b64", case=name, round=rnd,
                                       kernel=kname, images=nimg, windows=nw,
                                       text_mb=round(n / 1e6, 2), us=round(us, 1),
                                       gb_s=round(n / us / 1e3, 1)))
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
        # both forms computed the same thing
        assert torch.equal(crc[0], crc[1]) and torch.equal(out[0], out[1])
        assert (bad == 0).all() and (status == 0).all()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--encoding", default="json", choices=("json", "b64"))
    ap.add_argument("--rounds", type=int, default=5, help="--encoding b64: alternating rounds")
    ap.add_argument("--out", default="", help="--encoding b64: append the JSON lines to a file")
    a = ap.parse_args()
    if a.encoding == "b64":
        return main_b64(a)
    s = torch.cuda.current_stream().cuda_stream
    tables = torch.tensor(np.array(K.crc32c_device_tables(), dtype=np.uint32).view(np.int32),
                          device="cuda")
    for name, shape, nrec in (("cifar_fetch", (32, 32, 3), 64), ("cifar_batch", (32, 32, 3), 256),
                              ("imagenet_fetch", (224, 224, 3), 9),
                              ("imagenet_batch", (224, 224, 3), 256)):
        buf, recs, tile_rec, tiles, ch, n, groups = build(shape, nrec)
        dgrp = torch.from_numpy(groups.reshape(-1)).cuda()
        d = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
        dch = torch.from_numpy(ch.view(np.uint8).copy()).cuda()
        dmap = torch.from_numpy(tile_rec).cuda()
        drec = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
        crc = torch.zeros(len(ch), dtype=torch.int32, device="cuda")
        cnt = torch.zeros(tiles + len(groups), dtype=torch.int32, device="cuda")
        cnt_p = torch.zeros(tiles, dtype=torch.int32, device="cuda")  # the parse's own pass
        gsum = torch.zeros(max(1, len(groups)), dtype=torch.int32, device="cuda")
        H, W, Cc = shape
        out = torch.empty((nrec, H, W, Cc), device="cuda")

        def ingest():
            C.ingest_crc_count(d.data_ptr(), dch.data_ptr(), len(ch), tables.data_ptr(),
                               crc.data_ptr(), nrec, len(groups), drec.data_ptr(),
                               dgrp.data_ptr(), cnt.data_ptr(), gsum.data_ptr(), s)

        packed, tab = C.text_pack(buf[:n])
        dp = torch.frombuffer(bytearray(packed + bytes(64)), dtype=torch.uint8).cuda()
        dt = torch.from_numpy(tab.astype(np.int64)).to(torch.int32).cuda()
        text = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
        gbad = torch.zeros(max(1, len(groups)), dtype=torch.int32, device="cuda")

        def ingest_packed():  # the engine's form: the packed body, expansion folded in
            C.ingest_crc_count(d.data_ptr(), dch.data_ptr(), len(ch), tables.data_ptr(),
                               crc.data_ptr(), nrec, len(groups), drec.data_ptr(),
                               dgrp.data_ptr(), cnt.data_ptr(), gsum.data_ptr(), s,
                               gbad=gbad.data_ptr(), packed=dp.data_ptr(), tab=dt.data_ptr(),
                               text_out=text.data_ptr())

        def unpack_then_ingest():  # round 4: text_unpack pass, then crc+count on the text
            C.text_unpack(dp.data_ptr(), dt.data_ptr(), n, text.data_ptr(), s)
            C.ingest_crc_count(text.data_ptr(), dch.data_ptr(), len(ch), tables.data_ptr(),
                               crc.data_ptr(), nrec, len(groups), drec.data_ptr(),
                               dgrp.data_ptr(), cnt.data_ptr(), gsum.data_ptr(), s)

        def crc_only():
            C.ingest_crc_count(d.data_ptr(), dch.data_ptr(), len(ch), tables.data_ptr(),
                               crc.data_ptr(), 0, 0, drec.data_ptr(), dgrp.data_ptr(),
                               cnt.data_ptr(), gsum.data_ptr(), s)

        def parse():
            C.json_parse_instances(nrec, tiles, drec.data_ptr(), dmap.data_ptr(), d.data_ptr(), H,
                                   W, Cc, cnt_p.data_ptr(), out.data_ptr(), s, count_pass=True)

        # the replica's parse of ingested records: the ingest pass's count blocks, no count pass
        ingest()
        recs2 = recs.copy()
        recs2["has_cnt"] = 1
        recs2["cnt_off"] = [cnt.data_ptr() + 4 * (int(r["tile0"]) + int(r["pad"])) - d.data_ptr()
                            for r in recs]
        drec2 = torch.from_numpy(recs2.view(np.uint8).copy()).cuda()

        def parse_cnt():
            C.json_parse_instances(nrec, tiles, drec2.data_ptr(), dmap.data_ptr(), d.data_ptr(),
                                   H, W, Cc, cnt_p.data_ptr(), out.data_ptr(), s,
                                   count_pass=False)

        for kname, fn in (("crc+count", ingest), ("crc", crc_only),
                          ("crc+count+expand(packed)", ingest_packed),
                          ("unpack;crc+count (r4)", unpack_then_ingest),
                          ("count+parse", parse), ("parse(ingest counts)", parse_cnt)):
            us = timed(fn, a.iters)
            print(json.dumps(dict(case=name, kernel=kname, records=nrec, text_mb=round(n / 1e6, 2),
                                  us=round(us, 1), gb_s=round(n / us / 1e3, 1))), flush=True)
        for dr in (drec, drec2):
            st = dr.cpu().numpy().view(REC)["status"]
            assert (st == 0).all(), st


if __name__ == "__main__":
    main()
