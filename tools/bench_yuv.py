"""YUV 4:2:0 frame decoder (b64_yuv_instances) next to the RGB b64 decoder and a device copy.

The protocol of ``bench_json.py --encoding b64``: in one process, alternating --rounds times,

* ``yuv``:  b64_yuv_instances on one-frame records of random planes (--pixel-format),
* ``rgb``:  b64_decode_instances on RGB records of the same pixel count (the oracle's images of
  those frames, so both write the same floats - checked before timing),
* ``copy``: a plain device copy moving the YUV decoder's bytes (its text in plus its floats out),

each timed with device events over --iters launches. One JSON line per case with every round's
time and the medians. Cases: ``--cases 1024x32x32,64x224x224`` (batch x HS x WS).
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
from gale.models.preprocess import InputPrep, YuvConvert  # noqa: E402

C = native()
IMG = np.dtype([("off", "<i8"), ("slot", "<i4"), ("rec", "<i4")])


def staged(records, nbytes, batch):
    """The instances arrays of one-image records, 16-byte aligned, cycled up to `batch`, and
    their image descriptor table."""
    assert IMG.itemsize == C.B64_IMAGE_BYTES, "B64Image layout changed (gale/kernels.h)"
    texts = []
    for rec in records:
        s, off, ln, n = C.scan_instances_b64_bytes(rec, nbytes)
        assert s == 0 and n == 1
        arr = rec[off:off + ln]
        texts.append((arr, C.b64_image_offsets_bytes(arr, nbytes)[0]))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1024x32x32,64x224x224", help="batch x HS x WS, ...")
    ap.add_argument("--pixel-format", default="i420", choices=("i420", "nv12"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--distinct", type=int, default=64, help="distinct frames cycled in a batch")
    ap.add_argument("--prep", action="store_true", help="the CIFAR scale / mean / std")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_yuv: no GPU (a timing needs one)")
    kw = {}
    if a.prep:
        kw = InputPrep.build(3, 1 / 255, (0.4914, 0.4822, 0.4465),
                             (0.2470, 0.2435, 0.2616)).kernel_kwargs()
    yc = YuvConvert(a.pixel_format)
    ykw = yc.kernel_kwargs()
    s = torch.cuda.current_stream()
    med = lambda v: float(np.median(v))  # noqa: E731
    for case in a.cases.split(","):
        b, HS, WS = (int(v) for v in case.split("x"))
        nd = min(b, a.distinct)
        Y, U, V = synthetic_yuv_planes(nd, HS, WS, seed=0)
        B = yc.frame_bytes(HS, WS)
        raw, tab = staged(encode_records_yuv(Y, U, V, a.pixel_format, 1), B, b)
        rgb = yc.apply(pack_yuv420(Y, U, V, a.pixel_format), HS, WS)
        rraw, rtab = staged(encode_records_b64(rgb, 1), HS * WS * 3, b)
        d_raw, d_tab = (torch.from_numpy(v.copy()).cuda() for v in (raw, tab.view(np.uint8)))
        r_raw, r_tab = (torch.from_numpy(v.copy()).cuda() for v in (rraw, rtab.view(np.uint8)))
        status = torch.zeros(b, dtype=torch.int32, device="cuda")
        out = torch.empty((b, HS, WS, 3), device="cuda")
        r_out = torch.empty((b, HS, WS, 3), device="cuda")
        moved = b * (4 * B // 3 + 4 * HS * WS * 3)
        c_src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        c_dst = torch.empty_like(c_src)

        def yuv():
            err = C.b64_yuv_instances(b, d_tab.data_ptr(), d_raw.data_ptr(), HS, WS, 3,
                                      out.data_ptr(), status.data_ptr(), s.cuda_stream, 0,
                                      **ykw, **kw)
            assert err == 0, err

        def rgb_decode():
            C.b64_decode_instances(b, r_tab.data_ptr(), r_raw.data_ptr(), HS, WS, 3,
                                   r_out.data_ptr(), status.data_ptr(), s.cuda_stream, 0, **kw)

        def copy():
            c_dst.copy_(c_src)

        fns = (("yuv", yuv), ("rgb", rgb_decode), ("copy", copy))
        for _, fn in fns:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == 0).all()
        assert torch.equal(out, r_out), "the YUV and the RGB decoder disagree on the same pixels"
        us = {name: [] for name, _ in fns}
        for _ in range(a.rounds):
            for name, fn in fns:
                us[name].append(round(timed(fn, a.iters), 2))
        print(json.dumps(dict(
            kernel="b64_yuv_instances", pixel_format=a.pixel_format, batch=b, size=[HS, WS],
            pairs=C.b64_yuv_pairs(HS, WS), prep=bool(kw), iters=a.iters,
            chars_per_image=4 * B // 3, rgb_chars_per_image=4 * HS * WS, moved_bytes=moved,
            us=us["yuv"], us_median=med(us["yuv"]),
            rgb_us=us["rgb"], rgb_us_median=med(us["rgb"]),
            copy_us=us["copy"], copy_us_median=med(us["copy"]),
            gb_s=round(moved / med(us["yuv"]) / 1e3, 1),
            copy_gb_s=round(moved / med(us["copy"]) / 1e3, 1),
            img_s=round(b / med(us["yuv"]) * 1e6))), flush=True)


if __name__ == "__main__":
    main()
