"""GPU JSON parser throughput (json_count + json_parse kernels) on a batch of InstObj records.

The records are what bench.py streams: uniform [0,1) images in Java Float.toString format
(~35 KB of text per CIFAR image). Reports device time per batch and GB/s of JSON text.

--pixels byte: integer 0..255 pixels in Python's compact json.dumps text (what a client sends
when the GPU scales and normalises); --layout nchw: records nested [N][C][H][W]; --prep: the
parse applies the CIFAR scale / mean / std at its store (json_parse_prep_kernel;
implied by --layout nchw, whose transposing store belongs to it).

--encoding b64: the base64 decoder (b64_decode_instances) on the same byte pixels sent as
{"b64": ...} records, next to the parser (count + parse) on their byte-pixel text and a plain
device copy moving the decoder's bytes (in + out), alternating --rounds times in one process;
one line per batch with every round's time and the medians.
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
REC = np.dtype([("off", "<i8"), ("len", "<i4"), ("slot", "<i4"), ("images", "<i4"),
                ("status", "<i4"), ("tile0", "<i4"), ("has_cnt", "<i4"), ("cnt_off", "<i8"),
                ("pad", "<i8")])
assert REC.itemsize == C.JSON_RECORD_BYTES, "JsonRecord layout changed (gale/kernels.h)"



def staged_batch(batch, H, W, Cc, distinct=64, seed=0, pixels="unit", layout="nhwc"):
    from gale.data import encode_records_text

    rng = np.random.default_rng(seed)
    texts = []
    for _ in range(min(batch, distinct)):
        if pixels == "unit" and layout == "nhwc":
            rec = C.encode_instances(rng.random((1, H, W, Cc), dtype=np.float32))
        else:
            x = (rng.integers(0, 256, (1, H, W, Cc), dtype=np.uint8) if pixels == "byte"
                 else rng.random((1, H, W, Cc), dtype=np.float32))
            rec = encode_records_text(x, 1, layout)[0]
        # (the scan counts brackets: an NCHW record nests (C, H, W))
        s, off, ln, n = (C.scan_instances(rec, Cc, H, W) if layout == "nchw"
                         else C.scan_instances(rec, H, W, Cc))
        assert s == 0 and n == 1
        texts.append(rec[off:off + ln])
    buf = bytearray()
    recs = np.zeros(batch, dtype=REC)
    tiles = 0
    for i in range(batch):
        t = texts[i % len(texts)]
        recs[i] = (len(buf), len(t), i, 1, 0, tiles, 0, 0, 0)
        tiles += C.json_tile_count(len(buf), len(t))
        buf += t + b" " * ((-len(t)) % 16)
    buf += b" " * 16
    tile_rec = np.zeros(tiles, dtype=np.int32)
    for i, r in enumerate(recs):
        n = C.json_tile_count(int(r["off"]), int(r["len"]))
        tile_rec[r["tile0"]:r["tile0"] + n] = i
    return np.frombuffer(bytes(buf), dtype=np.uint8), recs, tile_rec, tiles


IMG = np.dtype([("off", "<i8"), ("slot", "<i4"), ("rec", "<i4")])


def staged_b64(batch, H, W, Cc, distinct=64, seed=0, layout="nhwc"):
    """The instances arrays of one-image b64 records of the pixels staged_batch(pixels="byte")
    draws, 16-byte aligned like its texts, and their image descriptor table."""
    from gale.data import encode_records_b64

    assert IMG.itemsize == C.B64_IMAGE_BYTES, "B64Image layout changed (gale/kernels.h)"
    rng = np.random.default_rng(seed)
    texts = []
    for _ in range(min(batch, distinct)):
        rec = encode_records_b64(rng.integers(0, 256, (1, H, W, Cc), dtype=np.uint8), 1,
                                 layout)[0]
        s, off, ln, n = C.scan_instances_b64(rec, H, W, Cc)
        assert s == 0 and n == 1
        arr = rec[off:off + ln]
        texts.append((arr, C.b64_image_offsets(arr, H, W, Cc)[0]))
    buf = bytearray()
    tab = np.zeros(batch, dtype=IMG)
    for i in range(batch):
        t, o = texts[i % len(texts)]
        tab[i] = (len(buf) + o, i, i)
        buf += t + b" " * ((-len(t)) % 16)
    buf += b" " * 16
    return np.frombuffer(bytes(buf), dtype=np.uint8), tab


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def bench_b64(a, H, W, Cc, kw):
    s = torch.cuda.current_stream()
    med = lambda v: float(np.median(v))  # noqa: E731
    for b in (int(v) for v in a.batches.split(",")):
        raw, tab = staged_b64(b, H, W, Cc, layout=a.layout)
        d_raw = torch.from_numpy(raw.copy()).cuda()
        d_tab = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
        d_status = torch.zeros(b, dtype=torch.int32, device="cuda")
        out = torch.empty((b, H, W, Cc), device="cuda")
        traw, recs, tile_rec, tiles = staged_batch(b, H, W, Cc, pixels="byte", layout=a.layout)
        t_raw = torch.from_numpy(traw.copy()).cuda()
        t_recs = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
        t_tile_rec = torch.from_numpy(tile_rec).cuda()
        t_counts = torch.zeros(tiles, dtype=torch.int32, device="cuda")
        t_out = torch.empty((b, H, W, Cc), device="cuda")
        # a copy that moves what the decoder moves: its text in plus its floats out
        moved = b * (4 * ((H * W * Cc + 2) // 3) + 4 * H * W * Cc)
        c_src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        c_dst = torch.empty_like(c_src)

        def decode():
            C.b64_decode_instances(b, d_tab.data_ptr(), d_raw.data_ptr(), H, W, Cc,
                                   out.data_ptr(), d_status.data_ptr(), s.cuda_stream, 0, **kw)

        def parse():
            C.json_parse_instances(b, tiles, t_recs.data_ptr(), t_tile_rec.data_ptr(),
                                   t_raw.data_ptr(), H, W, Cc, t_counts.data_ptr(),
                                   t_out.data_ptr(), s.cuda_stream, True, **kw)

        def copy():
            c_dst.copy_(c_src)

        for fn in (decode, parse, copy):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        assert (d_status.cpu().numpy() == 0).all()
        assert (t_recs.cpu().numpy().view(REC)["status"] == 0).all()
        assert torch.equal(out, t_out), "decoder and parser disagree on the same pixels"
        us = {"decode": [], "parse": [], "copy": []}
        for _ in range(a.rounds):
            for name, fn in (("decode", decode), ("parse", parse), ("copy", copy)):
                us[name].append(round(timed(fn, a.iters), 2))
        print(json.dumps(dict(
            kernel="b64_decode_instances", batch=b, shape=[H, W, Cc], layout=a.layout,
            prep=bool(kw), iters=a.iters, bytes_per_image=round(raw.size / b, 1),
            text_bytes_per_image=round(traw.size / b, 1), moved_bytes=moved,
            us=us["decode"], us_median=med(us["decode"]),
            parser_us=us["parse"], parser_us_median=med(us["parse"]),
            copy_us=us["copy"], copy_us_median=med(us["copy"]),
            gb_s=round(moved / med(us["decode"]) / 1e3, 1),
            copy_gb_s=round(moved / med(us["copy"]) / 1e3, 1),
            img_s=round(b / med(us["decode"]) * 1e6))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encoding", default="json", choices=("json", "b64"),
                    help="b64: the base64 decoder next to the parser on the same byte pixels")
    ap.add_argument("--rounds", type=int, default=3, help="--encoding b64: alternating rounds")
    ap.add_argument("--batches", default="1,64,256,1024")
    ap.add_argument("--shape", default="32,32,3")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--pixels", default="unit", choices=("unit", "byte"))
    ap.add_argument("--layout", default="nhwc", choices=("nhwc", "nchw"))
    ap.add_argument("--prep", action="store_true",
                    help="apply scale 1/255 (byte pixels) and the CIFAR mean / std in the parse")
    a = ap.parse_args()
    H, W, Cc = (int(v) for v in a.shape.split(","))
    kw = {}
    if a.prep or a.layout == "nchw":
        from gale.models.preprocess import InputPrep

        mean, std = ((0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616)) if Cc == 3 \
            else ((0.5,), (0.25,))
        kw = InputPrep.build(Cc, 1 / 255 if a.pixels == "byte" else 1.0, mean, std,
                             a.layout).kernel_kwargs()
    if a.encoding == "b64":
        if a.pixels != "byte":
            ap.error("--encoding b64 carries uint8 pixels: it needs --pixels byte")
        bench_b64(a, H, W, Cc, kw)
        return
    s = torch.cuda.current_stream()
    for b in (int(v) for v in a.batches.split(",")):
        raw, recs, tile_rec, tiles = staged_batch(b, H, W, Cc, pixels=a.pixels, layout=a.layout)
        d_raw = torch.from_numpy(raw.copy()).cuda()
        d_recs0 = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
        d_recs = d_recs0.clone()
        d_tile_rec = torch.from_numpy(tile_rec).cuda()
        d_counts = torch.zeros(tiles, dtype=torch.int32, device="cuda")
        out = torch.empty((b, H, W, Cc), device="cuda")

        def run(count_pass=True):
            C.json_parse_instances(b, tiles, d_recs.data_ptr(), d_tile_rec.data_ptr(),
                                   d_raw.data_ptr(), H, W, Cc, d_counts.data_ptr(),
                                   out.data_ptr(), s.cuda_stream, count_pass, **kw)

        for _ in range(3):
            run()
        torch.cuda.synchronize()
        st = d_recs.cpu().numpy().view(REC)["status"]
        assert (st == 0).all(), st
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / a.iters
        # the parse alone, from the counts (the serving step: the ingest pass counted them)
        e0.record()
        for _ in range(a.iters):
            run(False)
        e1.record()
        torch.cuda.synchronize()
        us_parse = e0.elapsed_time(e1) * 1e3 / a.iters
        print(json.dumps(dict(kernel="json_parse_instances", batch=b, tiles=tiles,
                              pixels=a.pixels, layout=a.layout, prep=bool(kw),
                              bytes=int(raw.size), bytes_per_image=round(raw.size / b, 1),
                              us=round(us, 2), parse_only_us=round(us_parse, 2),
                              gb_s=round(raw.size / us / 1e3, 1),
                              img_s=round(b / us * 1e6))), flush=True)


if __name__ == "__main__":
    main()
