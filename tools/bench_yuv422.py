"""Packed YUV 4:2:2 decoders (b64_yuv422_instances, raw_yuv422_instances) next to their
yardsticks, on the protocol of ``bench_yuv.py``: in one process, alternating --rounds times,

* ``b64``:  b64_yuv422_instances on one-frame records of random planes (--pixel-format),
* ``raw``:  raw_yuv422_instances on the same frames' bytes,
* ``rgb``:  b64_decode_instances on RGB records of the same pixel count (the oracle's images of
  those frames: the same floats - checked on the bits before timing),
* ``rawu8``: raw_instances u8 on the same images' bytes,
* ``i420``: b64_yuv_instances on I420 frames of the same pixel count (other floats: not compared),
* ``copy_b64`` / ``copy_raw``: a plain device copy moving the bytes of either 4:2:2 kernel (its
  source in plus its floats out),

each timed with device events over --iters launches. One JSON line per case and round goes to
--out (appended) and the medians with min-max to stdout. Cases: ``--cases
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
from gale.data import (encode_records_b64, encode_records_yuv, encode_records_yuv422,  # noqa: E402
                       pack_yuv422, synthetic_yuv422_planes, synthetic_yuv_planes)
from gale.models.preprocess import InputPrep, Yuv422Convert, YuvConvert  # noqa: E402
from tools.bench_yuv import staged, timed  # noqa: E402

C = native()
IMG = np.dtype([("off", "<i8"), ("slot", "<i4"), ("rec", "<i4")])


def staged_raw(frames, batch):
    """The frames back to back (16-byte aligned: each is a multiple of 16 bytes or padded), cycled
    up to `batch`, and their descriptor table."""
    buf, tab = bytearray(), np.zeros(batch, dtype=IMG)
    for i in range(batch):
        tab[i] = (len(buf), i, i)
        fr = frames[i % len(frames)].tobytes()
        buf += fr + b"\0" * ((-len(fr)) % 16)
    buf += b"\0" * 16
    return np.frombuffer(bytes(buf), dtype=np.uint8), tab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1024x32x32,64x224x224", help="batch x HS x WS, ...")
    ap.add_argument("--pixel-format", default="yuyv422", choices=("yuyv422", "uyvy422"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--distinct", type=int, default=64, help="distinct frames cycled in a batch")
    ap.add_argument("--out", default="profiles/yuv422_ab.jsonl")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_yuv422: no GPU (a timing needs one)")
    yc, y420 = Yuv422Convert(a.pixel_format), YuvConvert("i420")
    ykw, y420kw = yc.kernel_kwargs(), y420.kernel_kwargs()
    s = torch.cuda.current_stream().cuda_stream
    dev = lambda v: torch.from_numpy(v.copy()).cuda()  # noqa: E731
    cifar = InputPrep.build(3, 1 / 255, (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as log:
        for case in a.cases.split(","):
            b, HS, WS = (int(v) for v in case.split("x"))
            nd = min(b, a.distinct)
            Y, U, V = synthetic_yuv422_planes(nd, HS, WS, seed=0)
            frames = pack_yuv422(Y, U, V, a.pixel_format)
            B, L = 2 * HS * WS, 4 * ((2 * HS * WS + 2) // 3)
            rgb = yc.apply(frames, HS, WS)
            src = {"b64": staged(encode_records_yuv422(Y, U, V, a.pixel_format, 1), B, b),
                   "raw": staged_raw(frames, b),
                   "rgb": staged(encode_records_b64(rgb, 1), HS * WS * 3, b),
                   "rawu8": staged_raw(rgb.reshape(nd, -1), b),
                   "i420": staged(encode_records_yuv(*synthetic_yuv_planes(nd, HS, WS, 0), "i420",
                                                     1), HS * WS * 3 // 2, b)}
            src = {k: (dev(r), dev(t.view(np.uint8))) for k, (r, t) in src.items()}
            out = {k: torch.empty((b, HS, WS, 3), device="cuda") for k in src}
            status = torch.zeros(b, dtype=torch.int32, device="cuda")
            moved = {"b64": b * (L + 12 * HS * WS), "raw": b * (B + 12 * HS * WS)}
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

                fns = (("b64", lambda: call("b64_yuv422_instances", "b64", **ykw)),
                       ("raw", lambda: call("raw_yuv422_instances", "raw", **ykw)),
                       ("rgb", lambda: call("b64_decode_instances", "rgb")),
                       ("rawu8", lambda: call("raw_instances", "rawu8")),
                       ("i420", lambda: call("b64_yuv_instances", "i420", **y420kw)),
                       ("copy_b64", lambda: cpd["b64"].copy_(cp["b64"])),
                       ("copy_raw", lambda: cpd["raw"].copy_(cp["raw"])))
                for _, fn in fns:
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                assert (status.cpu().numpy() == 0).all()
                for k in ("b64", "raw", "rawu8"):  # the same floats, on the bits
                    assert torch.equal(out[k].view(torch.int32), out["rgb"].view(torch.int32)), k
                us = {name: [] for name, _ in fns}
                for rnd in range(a.rounds):
                    row = {name: round(timed(fn, a.iters), 2) for name, fn in fns}
                    for name, v in row.items():
                        us[name].append(v)
                    log.write(json.dumps(dict(
                        pixel_format=a.pixel_format, batch=b, size=[HS, WS], prep=prep,
                        round=rnd, iters=a.iters, moved_bytes=moved, us=row)) + "\n")
                    log.flush()
                print(json.dumps(dict(
                    pixel_format=a.pixel_format, batch=b, size=[HS, WS], prep=prep,
                    rounds=a.rounds, iters=a.iters, moved_bytes=moved,
                    us_median_min_max={k: [float(np.median(v)), min(v), max(v)]
                                       for k, v in us.items()},
                    gb_s={k: round(moved[k] / float(np.median(us[k])) / 1e3, 1) for k in moved},
                    copy_gb_s={k: round(moved[k] / float(np.median(us["copy_" + k])) / 1e3, 1)
                               for k in moved})), flush=True)


if __name__ == "__main__":
    main()
