"""The edge-directed Bayer demosaic (raw_bayer_hamilton_instances) next to its yardsticks, on the
protocol of ``bench_bayer_malvar.py``: in one process, alternating --rounds times,

* ``hamilton``: the kernel on bayer_rggb8 frames staged at 16-byte boundaries, and
  ``hamilton_odd``: the same frames at byte phase 5 (every row realigned),
* ``malvar`` and ``bilinear``: raw_bayer_malvar_instances and raw_bayer_instances, unchanged, on
  the same frames,
* ``rawu8``: raw_instances u8 on RGB images of the same pixel count, 3 bytes a pixel (other
  floats: not compared),
* ``copy``: a plain device copy moving the kernel's bytes (1 byte a pixel in plus 12 out),

each timed with device events over --iters launches. The four Bayer contenders are checked against
their numpy oracles on the bits before anything is timed. One JSON line per case and round goes to
--out (appended) and the medians with min-max to stdout. Cases:
``--cases 1024x32x32,64x224x224`` (batch x HS x WS), with and without the CIFAR prep.
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gale._native import native  # noqa: E402
from gale.data import mosaic_bayer, synthetic_pixels  # noqa: E402
from gale.models.preprocess import BayerConvert, InputPrep  # noqa: E402
from tools.bench_yuv import timed  # noqa: E402
from tools.bench_yuv10 import ODD_PHASE, staged_raw  # noqa: E402

C = native()
LAUNCHER = {"hamilton": "raw_bayer_hamilton_instances", "hamilton_odd": "raw_bayer_hamilton_instances",
            "malvar": "raw_bayer_malvar_instances", "bilinear": "raw_bayer_instances"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1024x32x32,64x224x224", help="batch x HS x WS, ...")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--distinct", type=int, default=64, help="distinct frames cycled in a batch")
    ap.add_argument("--out", default="profiles/bayer_hamilton_ab.jsonl")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_bayer_hamilton: no GPU (a timing needs one)")
    order = "bayer_rggb8"
    oracle = {k: BayerConvert(order, k.split("_")[0]) for k in LAUNCHER}
    s = torch.cuda.current_stream().cuda_stream
    dev = lambda v: torch.from_numpy(v.copy()).cuda()  # noqa: E731
    cifar = InputPrep.build(3, 1 / 255, (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as log:
        for case in a.cases.split(","):
            b, HS, WS = (int(v) for v in case.split("x"))
            nd, hw = min(b, a.distinct), HS * WS
            px = synthetic_pixels(nd, (HS, WS, 3), 0)
            frames = mosaic_bayer(px, order).reshape(nd, -1)
            src = {"hamilton": staged_raw(frames, b),
                   "hamilton_odd": staged_raw(frames, b, ODD_PHASE),
                   "rawu8": staged_raw(px.reshape(nd, -1), b)}
            src = {k: (dev(r), dev(t.view(np.uint8))) for k, (r, t) in src.items()}
            src["malvar"] = src["bilinear"] = src["hamilton"]
            out = {k: torch.empty((b, HS, WS, 3), device="cuda") for k in src}
            status = torch.zeros(b, dtype=torch.int32, device="cuda")
            moved = b * 13 * hw  # bytes of the Bayer contenders: 1 a pixel in, 12 out
            cp = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
            cpd = torch.empty_like(cp)
            for prep in (False, True):
                kw = cifar.kernel_kwargs() if prep else {}

                def call(name, key, **extra):
                    raw, tab = src[key]
                    err = getattr(C, name)(b, tab.data_ptr(), raw.data_ptr(), HS, WS, 3,
                                           out[key].data_ptr(), status.data_ptr(), s, 0,
                                           **extra, **kw)
                    assert not err, (name, err)

                fns = [(k, lambda k=k: call(LAUNCHER[k], k, order=order)) for k in LAUNCHER]
                fns += [("rawu8", lambda: call("raw_instances", "rawu8")),
                        ("copy", lambda: cpd.copy_(cp))]
                for _, fn in fns:
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                for k, bc in oracle.items():  # the oracles' floats, on the bits
                    want = bc.to_float(bc.apply(frames, HS, WS), cifar if prep else None)
                    want = torch.from_numpy(want[np.arange(b) % nd]).cuda().view(torch.int32)
                    assert torch.equal(out[k].view(torch.int32), want), k
                us = {name: [] for name, _ in fns}
                for rnd in range(a.rounds):
                    row = {name: round(timed(fn, a.iters), 2) for name, fn in fns}
                    for name, v in row.items():
                        us[name].append(v)
                    log.write(json.dumps(dict(batch=b, size=[HS, WS], prep=prep, round=rnd,
                                              iters=a.iters, moved_bytes=moved, us=row)) + "\n")
                    log.flush()
                med = {k: float(np.median(v)) for k, v in us.items()}
                print(json.dumps(dict(
                    batch=b, size=[HS, WS], prep=prep, rounds=a.rounds, iters=a.iters,
                    moved_bytes=moved,
                    us_median_min_max={k: [med[k], min(v), max(v)] for k, v in us.items()},
                    gb_s={k: round(moved / med[k] / 1e3, 1) for k in us if k != "rawu8"},
                    vs_malvar={k: round(med[k] / med["malvar"], 3) for k in us},
                    vs_copy={k: round(med[k] / med["copy"], 3) for k in us})), flush=True)


if __name__ == "__main__":
    main()
