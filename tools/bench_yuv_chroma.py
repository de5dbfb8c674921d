"""The linear-chroma 4:2:0 decoder (b64_yuv_linear_instances) next to its yardsticks, on the
protocol of ``bench_yuv10.py``: in one process, alternating --rounds times,

* ``lin_i420`` / ``lin_nv12``: the kernel on one-frame records of the same random planes,
* ``near_i420``: b64_yuv_instances (nearest chroma) on the i420 records - the same text in, the
  same count of floats out (other floats: not compared),
* ``rgb``: b64_decode_instances on RGB records of the same pixel count (the linear oracle's
  images, so it writes the floats of the linear kernels - checked),
* ``copy``: a plain device copy moving the linear kernel's bytes (its text in plus its floats out),

each timed with device events over --iters launches. The linear contenders and ``rgb`` are checked
against the numpy oracle on the bits before anything is timed. One JSON line per case and round
goes to --out (appended) and the medians with min-max to stdout. Cases: ``--cases
1024x32x32,64x224x224`` (batch x HS x WS), with and without the CIFAR prep.
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gale._native import native  # noqa: E402
from gale.data import (encode_records_b64, encode_records_yuv, pack_yuv420,  # noqa: E402
                       synthetic_yuv_planes)
from gale.models.preprocess import InputPrep, YuvLinearConvert  # noqa: E402
from tools.bench_yuv import staged, timed  # noqa: E402

C = native()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1024x32x32,64x224x224", help="batch x HS x WS, ...")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--distinct", type=int, default=64, help="distinct frames cycled in a batch")
    ap.add_argument("--out", default="profiles/yuv_chroma_ab.jsonl")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_yuv_chroma: no GPU (a timing needs one)")
    conv = {f: YuvLinearConvert(f) for f in ("i420", "nv12")}
    s = torch.cuda.current_stream().cuda_stream
    dev = lambda v: torch.from_numpy(v.copy()).cuda()  # noqa: E731
    cifar = InputPrep.build(3, 1 / 255, (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as log:
        for case in a.cases.split(","):
            b, HS, WS = (int(v) for v in case.split("x"))
            nd, hw = min(b, a.distinct), HS * WS
            B = hw * 3 // 2
            Y, U, V = synthetic_yuv_planes(nd, HS, WS, seed=0)
            rgb = conv["i420"].apply(pack_yuv420(Y, U, V, "i420"), HS, WS)
            assert np.array_equal(rgb, conv["nv12"].apply(pack_yuv420(Y, U, V, "nv12"), HS, WS))
            src = {f: staged(encode_records_yuv(Y, U, V, f, 1), B, b) for f in conv}
            src["rgb"] = staged(encode_records_b64(rgb, 1), 3 * hw, b)
            src = {k: (dev(r), dev(t.view(np.uint8))) for k, (r, t) in src.items()}
            names = ("lin_i420", "lin_nv12", "near_i420", "rgb")
            out = {k: torch.empty((b, HS, WS, 3), device="cuda") for k in names}
            status = torch.zeros(b, dtype=torch.int32, device="cuda")
            moved = b * (4 * B // 3 + 12 * hw)  # the linear kernel's text in and floats out
            cp = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
            cpd = torch.empty_like(cp)
            for prep in (False, True):
                kw = cifar.kernel_kwargs() if prep else {}

                def call(launcher, key, name, **extra):
                    raw, tab = src[key]
                    err = getattr(C, launcher)(b, tab.data_ptr(), raw.data_ptr(), HS, WS, 3,
                                               out[name].data_ptr(), status.data_ptr(), s, 0,
                                               **extra, **kw)
                    assert not err, (launcher, err)

                def yuv(launcher, fmt, name):
                    return lambda: call(launcher, fmt, name, **conv[fmt].kernel_kwargs())

                fns = [("lin_i420", yuv("b64_yuv_linear_instances", "i420", "lin_i420")),
                       ("lin_nv12", yuv("b64_yuv_linear_instances", "nv12", "lin_nv12")),
                       ("near_i420", yuv("b64_yuv_instances", "i420", "near_i420")),
                       ("rgb", lambda: call("b64_decode_instances", "rgb", "rgb")),
                       ("copy", lambda: cpd.copy_(cp))]
                for _, fn in fns:
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                assert not status.any().item()
                want = rgb.astype(np.float32)
                want = (cifar.apply(want) if prep else want)[np.arange(b) % nd]
                want = torch.from_numpy(want).cuda().view(torch.int32)
                for k in ("lin_i420", "lin_nv12", "rgb"):  # the oracle's floats, on the bits
                    assert torch.equal(out[k].view(torch.int32), want), k
                us = {name: [] for name, _ in fns}
                for rnd in range(a.rounds):
                    row = {name: round(timed(fn, a.iters), 2) for name, fn in fns}
                    for name, v in row.items():
                        us[name].append(v)
                    log.write(json.dumps(dict(batch=b, size=[HS, WS], prep=prep, round=rnd,
                                              iters=a.iters, moved_bytes=moved,
                                              pairs=C.b64_yuv_linear_pairs(HS, WS), us=row)) + "\n")
                    log.flush()
                med = {k: float(np.median(v)) for k, v in us.items()}
                print(json.dumps(dict(
                    batch=b, size=[HS, WS], prep=prep, rounds=a.rounds, iters=a.iters,
                    moved_bytes=moved,
                    us_median_min_max={k: [med[k], min(v), max(v)] for k, v in us.items()},
                    gb_s={k: round(moved / med[k] / 1e3, 1) for k in us},
                    vs_rgb={k: round(med[k] / med["rgb"], 3) for k in us})), flush=True)


if __name__ == "__main__":
    main()
