"""The top-k selection + text kernel (topk_java) against the whole-row formatter
(format_floats_java) on the same softmax rows, both writing to host-mapped pinned memory as the
serving step does: the two ways one batch's output leaves the device, with --top-k and without.

Alternating rounds in one process (as tools/bench_json.py --encoding b64): per shape each round
times --iters back-to-back launches of one kernel between device events, then the other. Every
round is appended to --out (profiles/topk_ab.jsonl) and one summary line per shape is printed.
Bytes written per image are arithmetic: k * (16 + 4) for the selection, classes * 16 for the rows.
There is no pass mark.
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
SLOT = C.FLOAT_TEXT_SLOT


def softmax_rows(rows, classes, seed=0):
    z = np.random.default_rng(seed).normal(size=(rows, classes)).astype(np.float32) * 4
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def check(x, k, text, idx):
    """The selection's output against the rule (stable argsort of the descending key) and the
    host's Float.toString, before anything is timed."""
    b = x.view(np.uint32)
    keys = (b ^ np.where(b >> 31 != 0, np.uint32(0xffffffff), np.uint32(0x80000000)))
    want = np.argsort(-keys.astype(np.int64), axis=1, kind="stable")[:, :k]
    assert np.array_equal(idx.reshape(len(x), k), want), "selection differs from the rule"
    t = text.reshape(len(x), k, SLOT)
    for r in (0, len(x) - 1):
        for j in range(k):
            got = bytes(t[r, j, :t[r, j, SLOT - 1]]).decode()
            assert got == C.format_float_java(float(x[r, want[r, j]])), (r, j, got)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x10,256x1000", help="rows x classes, comma-separated")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join("profiles", "topk_ab.jsonl"))
    a = ap.parse_args()
    s = torch.cuda.current_stream().cuda_stream
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    dev = torch.cuda.get_device_name(0)
    with open(a.out, "a") as log:
        for shape in a.shapes.split(","):
            rows, classes = (int(v) for v in shape.split("x"))
            k = min(a.k, classes)
            x = softmax_rows(rows, classes)
            xd = torch.from_numpy(x).cuda()
            full = C.MappedBuffer(rows * classes * SLOT)
            sel = C.MappedBuffer(rows * k * (SLOT + 4))
            text_ptr, idx_ptr = sel.ptr, sel.ptr + rows * k * SLOT  # as GpuReplica lays them out

            def topk():
                C.topk_java(rows, classes, k, xd.data_ptr(), text_ptr, idx_ptr, s)

            def fmt():
                C.format_floats_java(rows * classes, xd.data_ptr(), full.ptr, s)

            for fn in (topk, fmt):
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            out = sel.numpy()
            check(x, k, out[:rows * k * SLOT], out[rows * k * SLOT:].view(np.int32))
            us = {"topk_java": [], "format_floats_java": []}
            for rnd in range(a.rounds):
                for name, fn in (("topk_java", topk), ("format_floats_java", fmt)):
                    t = round(timed(fn, a.iters), 3)
                    us[name].append(t)
                    log.write(json.dumps(dict(
                        kernel=name, round=rnd, rows=rows, classes=classes, k=k, iters=a.iters,
                        us_per_launch=t, device=dev,
                        bytes_per_image=k * (SLOT + 4) if name == "topk_java"
                        else classes * SLOT)) + "\n")
                    log.flush()
            med = {n: float(np.median(v)) for n, v in us.items()}
            print(json.dumps(dict(
                rows=rows, classes=classes, k=k, iters=a.iters, rounds=a.rounds,
                topk_us=us["topk_java"], topk_us_median=med["topk_java"],
                format_us=us["format_floats_java"], format_us_median=med["format_floats_java"],
                topk_bytes_per_image=k * (SLOT + 4), format_bytes_per_image=classes * SLOT,
                format_over_topk=round(med["format_floats_java"] / med["topk_java"], 2))),
                flush=True)


if __name__ == "__main__":
    main()
