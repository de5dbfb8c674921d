"""The raw 10-bit 4:2:0 decoder (raw_yuv420p10_instances) next to its yardsticks, on the protocol
of ``bench_yuvp.py``: in one process, alternating --rounds times,

* ``p010`` / ``p10``: the kernel on p010le / yuv420p10le frames of the same random 10-bit samples,
  staged at 16-byte boundaries, and ``p010_odd`` / ``p10_odd``: the same frames at byte phase 5
  (the realigning dword loads),
* ``yuv444p``: raw_yuvp_instances on yuv444p frames - the same 3 bytes a pixel in, the same count
  of floats out (other floats: not compared),
* ``rawu8``: raw_instances u8 on RGB images of 3 bytes a pixel (other floats: not compared),
* ``copy``: a plain device copy moving the kernel's bytes (3 bytes a pixel in plus 12 out),

each timed with device events over --iters launches. The four 10-bit contenders are checked
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
from gale.data import (pack_yuv420p10, pack_yuvp, synthetic_pixels,  # noqa: E402
                       synthetic_yuv420p10_planes, synthetic_yuvp_planes)
from gale.models.preprocess import InputPrep, Yuv420HiConvert, YuvPlanarConvert  # noqa: E402
from tools.bench_yuv import IMG, timed  # noqa: E402

C = native()
ODD_PHASE = 5


def staged_raw(frames, batch, phase=0):
    """The frames cycled up to `batch`, each at byte `phase` of a 16-byte unit, and their
    descriptor table."""
    buf, tab = bytearray(), np.zeros(batch, dtype=IMG)
    for i in range(batch):
        buf += b"\0" * ((phase - len(buf)) % 16)
        tab[i] = (len(buf), i, i)
        buf += frames[i % len(frames)].tobytes()
    buf += b"\0" * 16
    return np.frombuffer(bytes(buf), dtype=np.uint8), tab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1024x32x32,64x224x224", help="batch x HS x WS, ...")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--distinct", type=int, default=64, help="distinct frames cycled in a batch")
    ap.add_argument("--out", default="profiles/yuv10_ab.jsonl")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_yuv10: no GPU (a timing needs one)")
    conv = {"p010": Yuv420HiConvert("p010le"), "p10": Yuv420HiConvert("yuv420p10le")}
    y444 = YuvPlanarConvert("yuv444p").kernel_kwargs()
    s = torch.cuda.current_stream().cuda_stream
    dev = lambda v: torch.from_numpy(v.copy()).cuda()  # noqa: E731
    cifar = InputPrep.build(3, 1 / 255, (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as log:
        for case in a.cases.split(","):
            b, HS, WS = (int(v) for v in case.split("x"))
            nd, hw = min(b, a.distinct), HS * WS
            planes = synthetic_yuv420p10_planes(nd, HS, WS, seed=0)
            frames = {k: pack_yuv420p10(*planes, c.format) for k, c in conv.items()}
            q = conv["p010"].apply(frames["p010"], HS, WS)
            assert np.array_equal(q, conv["p10"].apply(frames["p10"], HS, WS))
            src = {"yuv444p": staged_raw(pack_yuvp(*synthetic_yuvp_planes(nd, HS, WS, "yuv444p", 0),
                                                   "yuv444p"), b),
                   "rawu8": staged_raw(synthetic_pixels(nd, (HS, WS, 3), 0).reshape(nd, -1), b)}
            for k in conv:
                src[k] = staged_raw(frames[k], b)
                src[k + "_odd"] = staged_raw(frames[k], b, ODD_PHASE)
            src = {k: (dev(r), dev(t.view(np.uint8))) for k, (r, t) in src.items()}
            out = {k: torch.empty((b, HS, WS, 3), device="cuda") for k in src}
            status = torch.zeros(b, dtype=torch.int32, device="cuda")
            moved = b * 15 * hw  # bytes of every contender: 3 a pixel in, 12 out
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

                def hi(key):
                    kk = conv[key.split("_")[0]].kernel_kwargs()
                    return lambda: call("raw_yuv420p10_instances", key, **kk)

                fns = ([(k, hi(k)) for k in src if k.startswith("p")]
                       + [("yuv444p", lambda: call("raw_yuvp_instances", "yuv444p", **y444)),
                          ("rawu8", lambda: call("raw_instances", "rawu8")),
                          ("copy", lambda: cpd.copy_(cp))])
                for _, fn in fns:
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                want = conv["p010"].to_float(q, cifar if prep else None)
                want = torch.from_numpy(want[np.arange(b) % nd]).cuda().view(torch.int32)
                for k in src:  # the oracle's floats, on the bits
                    if k.startswith("p"):
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
                    gb_s={k: round(moved / med[k] / 1e3, 1) for k in us},
                    vs_yuv444p={k: round(med[k] / med["yuv444p"], 3) for k in us})), flush=True)


if __name__ == "__main__":
    main()
