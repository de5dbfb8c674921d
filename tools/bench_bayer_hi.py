"""The 10/12/16-bit Bayer demosaic (raw_bayer_hi_instances) next to its yardsticks, on the protocol
of ``bench_bayer_malvar.py``: in one process, alternating --rounds times,

* ``<form>`` for 10le, 16le, 10p, 12p (12le runs 10le's code with another mask): the kernel on
  bayer_rggb<form> frames staged at 16-byte boundaries, and ``10p_odd``: 10p frames at byte phase 5,
* ``u8``: the 8-bit kernel of the same demosaic (raw_bayer_instances / raw_bayer_malvar_instances)
  on bayer_rggb8 frames of the same size,
* ``copy``: a plain device copy of the output's bytes (12 a pixel read, 12 written),

each timed with device events over --iters launches, once with the bilinear and once with the
malvar demosaic. Every contender is checked against its numpy oracle on the bits before anything
is timed. One JSON line per case and round goes to --out (appended) and the medians with min-max
to stdout. Cases: ``--cases 64x224x224,8x1080x1920`` (batch x HS x WS), with the CIFAR prep.
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gale._native import native  # noqa: E402
from gale.data import pack_bayer_hi  # noqa: E402
from gale.models.preprocess import BayerConvert, BayerHiConvert, InputPrep  # noqa: E402
from tools.bench_yuv import timed  # noqa: E402
from tools.bench_yuv10 import ODD_PHASE, staged_raw  # noqa: E402

C = native()
FORMS = ("10le", "16le", "10p", "12p")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="64x224x224,8x1080x1920", help="batch x HS x WS, ...")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--distinct", type=int, default=2, help="distinct frames cycled in a batch")
    ap.add_argument("--out", default="profiles/bayer_hi_ab.jsonl")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_bayer_hi: no GPU (a timing needs one)")
    s = torch.cuda.current_stream().cuda_stream
    dev = lambda v: torch.from_numpy(v.copy()).cuda()  # noqa: E731
    cifar = InputPrep.build(3, 1 / 255, (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616))
    kw = cifar.kernel_kwargs()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as log:
        for case in a.cases.split(","):
            b, HS, WS = (int(v) for v in case.split("x"))
            nd, hw = min(b, a.distinct), HS * WS
            rng = np.random.default_rng(0)
            frames = {f: pack_bayer_hi(rng.integers(0, 1 << BayerHiConvert(f"bayer_rggb{f}").bits,
                                                    (nd, HS, WS)), f"bayer_rggb{f}")
                      for f in FORMS}
            frames["10p_odd"] = frames["10p"]
            frames["u8"] = rng.integers(0, 256, (nd, hw), dtype=np.uint8)
            src = {k: staged_raw(f, b, ODD_PHASE if k == "10p_odd" else 0)
                   for k, f in frames.items()}
            src = {k: (dev(r), dev(t.view(np.uint8))) for k, (r, t) in src.items()}
            out = torch.empty((b, HS, WS, 3), device="cuda")  # (one output: checked per contender)
            status = torch.zeros(b, dtype=torch.int32, device="cuda")
            cp = torch.empty(b * 12 * hw, dtype=torch.uint8, device="cuda")
            cpd = torch.empty_like(cp)
            for demosaic in ("bilinear", "malvar"):
                malvar = demosaic == "malvar"

                def call(key):
                    raw, tab = src[key]
                    if key == "u8":
                        name = "raw_bayer_malvar_instances" if malvar else "raw_bayer_instances"
                        extra = dict(order="bayer_rggb8")
                    else:
                        name = "raw_bayer_hi_instances"
                        extra = dict(format="bayer_rggb" + key.split("_")[0], malvar=malvar)
                    err = getattr(C, name)(b, tab.data_ptr(), raw.data_ptr(), HS, WS, 3,
                                           out.data_ptr(), status.data_ptr(), s, 0, **extra, **kw)
                    assert not err, (name, err)

                fns = [(k, (lambda k=k: call(k))) for k in src] + [("copy", lambda: cpd.copy_(cp))]
                for k in src:  # the oracles' floats, on the bits; this is the warm-up too
                    bc = BayerConvert("bayer_rggb8", demosaic) if k == "u8" \
                        else BayerHiConvert("bayer_rggb" + k.split("_")[0], demosaic)
                    for _ in range(3):
                        call(k)
                    torch.cuda.synchronize()
                    want = bc.to_float(bc.apply(frames[k], HS, WS), cifar)
                    want = torch.from_numpy(want[np.arange(b) % nd]).cuda().view(torch.int32)
                    assert torch.equal(out.view(torch.int32), want), k
                for _ in range(3):
                    cpd.copy_(cp)
                us = {name: [] for name, _ in fns}
                for rnd in range(a.rounds):
                    row = {name: round(timed(fn, a.iters), 2) for name, fn in fns}
                    for name, v in row.items():
                        us[name].append(v)
                    log.write(json.dumps(dict(batch=b, size=[HS, WS], demosaic=demosaic, round=rnd,
                                              iters=a.iters, us=row)) + "\n")
                    log.flush()
                med = {k: float(np.median(v)) for k, v in us.items()}
                print(json.dumps(dict(
                    batch=b, size=[HS, WS], demosaic=demosaic, rounds=a.rounds, iters=a.iters,
                    us_median_min_max={k: [med[k], min(v), max(v)] for k, v in us.items()},
                    out_gb_s={k: round(b * 12 * hw / med[k] / 1e3, 1) for k in us},
                    vs_u8={k: round(med[k] / med["u8"], 3) for k in us},
                    vs_copy={k: round(med[k] / med["copy"], 3) for k in us})), flush=True)


if __name__ == "__main__":
    main()
