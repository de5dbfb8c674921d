"""Planar YUV 4:2:2 / 4:4:4 decoders (b64_yuvp_instances, raw_yuvp_instances) next to their
yardsticks, on the protocol of ``bench_yuv422.py``: in one process, alternating --rounds times,

* ``b64_444`` / ``raw_444`` / ``b64_422`` / ``raw_422``: the planar kernels on one-frame records
  of random planes (the yuv444p frames are the yuv422p ones with every chroma column doubled),
* ``rgb``: b64_decode_instances on RGB records of the oracle's images of those frames (the same
  floats for every contender above and below but ``i420`` - checked on the bits before timing),
* ``rawu8``: raw_instances u8 on the same images' bytes,
* ``yuyv_b64`` / ``yuyv_raw``: the packed 4:2:2 kernels on the same planes packed as yuyv422,
* ``i420``: b64_yuv_instances on I420 frames of the same pixel count (other floats: not compared),
* ``copy_<planar kernel>``: a plain device copy moving that kernel's bytes (source in plus floats
  out),

each timed with device events over --iters launches. One JSON line per case and round goes to
--out (appended) and the medians with min-max to stdout. Cases: ``--cases
1024x32x32,64x224x224`` (batch x HS x WS), with and without the CIFAR prep. Every image starts at
a 16-byte boundary: the realigning raw loads and the per-lane store path are not timed.
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gale._native import native  # noqa: E402
from gale.data import (encode_records_b64, encode_records_yuv, encode_records_yuv422,  # noqa: E402
                       encode_records_yuvp, pack_yuv422, pack_yuvp, synthetic_yuv_planes,
                       synthetic_yuvp_planes)
from gale.models.preprocess import (InputPrep, Yuv422Convert, YuvConvert,  # noqa: E402
                                    YuvPlanarConvert)
from tools.bench_yuv import staged, timed  # noqa: E402
from tools.bench_yuv422 import staged_raw  # noqa: E402

C = native()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1024x32x32,64x224x224", help="batch x HS x WS, ...")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--distinct", type=int, default=64, help="distinct frames cycled in a batch")
    ap.add_argument("--out", default="profiles/yuvp_ab.jsonl")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_yuvp: no GPU (a timing needs one)")
    conv = {"444": YuvPlanarConvert("yuv444p"), "422": YuvPlanarConvert("yuv422p")}
    kws = {k: v.kernel_kwargs() for k, v in conv.items()}
    kws["yuyv"], kws["i420"] = (Yuv422Convert("yuyv422").kernel_kwargs(),
                                YuvConvert("i420").kernel_kwargs())
    s = torch.cuda.current_stream().cuda_stream
    dev = lambda v: torch.from_numpy(v.copy()).cuda()  # noqa: E731
    cifar = InputPrep.build(3, 1 / 255, (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as log:
        for case in a.cases.split(","):
            b, HS, WS = (int(v) for v in case.split("x"))
            nd, hw = min(b, a.distinct), HS * WS
            Y, U, V = synthetic_yuvp_planes(nd, HS, WS, "yuv422p", seed=0)
            planes = {"422": (Y, U, V), "444": (Y, np.repeat(U, 2, -1), np.repeat(V, 2, -1))}
            B = {"422": 2 * hw, "444": 3 * hw}
            frames = {k: pack_yuvp(*p, conv[k].format) for k, p in planes.items()}
            rgb = conv["422"].apply(frames["422"], HS, WS)
            assert np.array_equal(rgb, conv["444"].apply(frames["444"], HS, WS))
            src = {"rgb": staged(encode_records_b64(rgb, 1), 3 * hw, b),
                   "rawu8": staged_raw(rgb.reshape(nd, -1), b),
                   "yuyv_b64": staged(encode_records_yuv422(Y, U, V, "yuyv422", 1), 2 * hw, b),
                   "yuyv_raw": staged_raw(pack_yuv422(Y, U, V, "yuyv422"), b),
                   "i420": staged(encode_records_yuv(*synthetic_yuv_planes(nd, HS, WS, 0), "i420",
                                                     1), hw * 3 // 2, b)}
            moved = {}
            for k in conv:
                src["b64_" + k] = staged(encode_records_yuvp(*planes[k], conv[k].format, 1),
                                         B[k], b)
                src["raw_" + k] = staged_raw(frames[k], b)
                moved["b64_" + k] = b * (4 * ((B[k] + 2) // 3) + 12 * hw)
                moved["raw_" + k] = b * (B[k] + 12 * hw)
            src = {k: (dev(r), dev(t.view(np.uint8))) for k, (r, t) in src.items()}
            out = {k: torch.empty((b, HS, WS, 3), device="cuda") for k in src}
            status = torch.zeros(b, dtype=torch.int32, device="cuda")
            cp = {k: torch.empty(v // 2, dtype=torch.uint8, device="cuda")
                  for k, v in moved.items()}
            cpd = {k: torch.empty_like(v) for k, v in cp.items()}
            for prep in (False, True):
                kw = cifar.kernel_kwargs() if prep else {}

                def call(name, key, **extra):
                    raw, tab = src[key]
                    err = getattr(C, name)(b, tab.data_ptr(), raw.data_ptr(), HS, WS, 3,
                                           out[key].data_ptr(), status.data_ptr(), s, 0,
                                           **extra, **kw)
                    assert not err, (name, err)

                def planar(enc, k):
                    return lambda: call(enc + "_yuvp_instances", f"{enc}_{k}", **kws[k])

                def copy(k):
                    return lambda: cpd[k].copy_(cp[k])

                fns = ([(f"{enc}_{k}", planar(enc, k)) for k in conv for enc in ("b64", "raw")]
                       + [("rgb", lambda: call("b64_decode_instances", "rgb")),
                          ("rawu8", lambda: call("raw_instances", "rawu8")),
                          ("yuyv_b64", lambda: call("b64_yuv422_instances", "yuyv_b64",
                                                    **kws["yuyv"])),
                          ("yuyv_raw", lambda: call("raw_yuv422_instances", "yuyv_raw",
                                                    **kws["yuyv"])),
                          ("i420", lambda: call("b64_yuv_instances", "i420", **kws["i420"]))]
                       + [("copy_" + k, copy(k)) for k in moved])
                for _, fn in fns:
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                assert (status.cpu().numpy() == 0).all()
                for k in out:  # the same floats, on the bits
                    if k not in ("rgb", "i420"):
                        assert torch.equal(out[k].view(torch.int32),
                                           out["rgb"].view(torch.int32)), k
                us = {name: [] for name, _ in fns}
                for rnd in range(a.rounds):
                    row = {name: round(timed(fn, a.iters), 2) for name, fn in fns}
                    for name, v in row.items():
                        us[name].append(v)
                    log.write(json.dumps(dict(batch=b, size=[HS, WS], prep=prep, round=rnd,
                                              iters=a.iters, moved_bytes=moved, us=row)) + "\n")
                    log.flush()
                print(json.dumps(dict(
                    batch=b, size=[HS, WS], prep=prep, rounds=a.rounds, iters=a.iters,
                    moved_bytes=moved,
                    us_median_min_max={k: [float(np.median(v)), min(v), max(v)]
                                       for k, v in us.items()},
                    gb_s={k: round(moved[k] / float(np.median(us[k])) / 1e3, 1) for k in moved},
                    copy_gb_s={k: round(moved[k] / float(np.median(us["copy_" + k])) / 1e3, 1)
                               for k in moved})), flush=True)


if __name__ == "__main__":
    main()
