"""Packed-pixel decoder (b64_packed_instances) next to the RGB b64 decoder and a device copy.

The protocol of ``bench_yuv.py``: in one process, alternating --rounds times,

* ``bgr24`` / ``rgba`` / ``bgra`` / ``gray``: b64_packed_instances on one-image records of random
  bytes in that format,
* ``rgb``: b64_decode_instances on RGB records of the same pixel count (the oracle's images of the
  bgr24 records),
* ``copy_<format>``: a plain device copy moving that decoder's bytes (its text in plus its floats
  out; rgba and bgra share one),

each timed with device events over --iters launches. Before timing, every packed output is
compared with the RGB decoder's on the oracle's images of the same records. One JSON line per
case, prep and format with every round's time and the medians (and the rgb decoder's rounds of
the same session: bgr24 moves exactly its bytes, so its min-max is bgr24's yardstick). Cases:
``--cases 1024x32x32,64x224x224`` (batch x HS x WS), each without and with the CIFAR prep.
"""

import argparse
import base64
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gale._native import native  # noqa: E402
from gale.data import encode_records_b64  # noqa: E402
from gale.models.preprocess import PACKED_FORMATS, InputPrep, PixelUnpack  # noqa: E402

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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--distinct", type=int, default=64, help="distinct images cycled in a batch")
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pixfmt: no GPU (a timing needs one)")
    cifar = InputPrep.build(3, 1 / 255, (0.4914, 0.4822, 0.4465),
                            (0.2470, 0.2435, 0.2616)).kernel_kwargs()
    s = torch.cuda.current_stream()
    med = lambda v: float(np.median(v))  # noqa: E731
    for case in a.cases.split(","):
        b, HS, WS = (int(v) for v in case.split("x"))
        nd = min(b, a.distinct)
        rng = np.random.default_rng(0)
        dev = {}
        for fmt in PACKED_FORMATS:
            un = PixelUnpack(fmt)
            B = un.frame_bytes(HS, WS)
            px = rng.integers(0, 256, (nd, B), dtype=np.uint8)
            recs = [b'{"instances":[{"b64":"' + base64.b64encode(p.tobytes()) + b'"}]}'
                    for p in px]
            raw, tab = staged(recs, B, b)
            rraw, rtab = staged(encode_records_b64(un.apply(px, HS, WS), 1), HS * WS * 3, b)
            moved = b * (4 * ((B + 2) // 3) + 4 * HS * WS * 3)
            dev[fmt] = dict(
                B=B, moved=moved,
                raw=torch.from_numpy(raw.copy()).cuda(),
                tab=torch.from_numpy(tab.view(np.uint8).copy()).cuda(),
                rraw=torch.from_numpy(rraw.copy()).cuda(),
                rtab=torch.from_numpy(rtab.view(np.uint8).copy()).cuda(),
                c_src=torch.empty(moved // 2, dtype=torch.uint8, device="cuda"),
                c_dst=torch.empty(moved // 2, dtype=torch.uint8, device="cuda"))
        status = torch.zeros(b, dtype=torch.int32, device="cuda")
        out = torch.empty((b, HS, WS, 3), device="cuda")
        r_out = torch.empty((b, HS, WS, 3), device="cuda")
        for prep in (False, True):
            kw = cifar if prep else {}

            def packed(fmt):
                d = dev[fmt]

                def fn():
                    err = C.b64_packed_instances(b, d["tab"].data_ptr(), d["raw"].data_ptr(), HS,
                                                 WS, 3, out.data_ptr(), status.data_ptr(),
                                                 s.cuda_stream, 0, format=fmt, **kw)
                    assert err == 0, err
                return fn

            def rgb_decode(fmt):
                d = dev[fmt]

                def fn():
                    C.b64_decode_instances(b, d["rtab"].data_ptr(), d["rraw"].data_ptr(), HS, WS,
                                           3, r_out.data_ptr(), status.data_ptr(), s.cuda_stream,
                                           0, **kw)
                return fn

            def copy(fmt):
                d = dev[fmt]
                return lambda: d["c_dst"].copy_(d["c_src"])

            # the outputs first: every format against the rgb decoder on its oracle's images
            for fmt in PACKED_FORMATS:
                out.fill_(-1.0)
                r_out.fill_(-2.0)
                packed(fmt)()
                rgb_decode(fmt)()
                torch.cuda.synchronize()
                assert (status.cpu().numpy() == 0).all()
                assert torch.equal(out, r_out), f"{fmt}: the packed and the RGB decoder disagree"
            fns = [(fmt, packed(fmt)) for fmt in PACKED_FORMATS]
            fns += [("rgb", rgb_decode("bgr24"))]
            fns += [("copy_" + fmt, copy(fmt)) for fmt in ("bgr24", "rgba", "gray")]
            for _, fn in fns:
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            us = {name: [] for name, _ in fns}
            for _ in range(a.rounds):
                for name, fn in fns:
                    us[name].append(round(timed(fn, a.iters), 2))
            for fmt in PACKED_FORMATS:
                d = dev[fmt]
                cp = us["copy_" + ("rgba" if fmt == "bgra" else fmt)]
                line = json.dumps(dict(
                    kernel="b64_packed_instances", pixel_format=fmt, batch=b, size=[HS, WS],
                    prep=prep, iters=a.iters, chars_per_image=4 * ((d["B"] + 2) // 3),
                    rgb_chars_per_image=4 * HS * WS, moved_bytes=d["moved"],
                    us=us[fmt], us_median=med(us[fmt]),
                    rgb_us=us["rgb"], rgb_us_median=med(us["rgb"]),
                    rgb_us_min=min(us["rgb"]), rgb_us_max=max(us["rgb"]),
                    copy_us=cp, copy_us_median=med(cp),
                    gb_s=round(d["moved"] / med(us[fmt]) / 1e3, 1),
                    copy_gb_s=round(d["moved"] / med(cp) / 1e3, 1),
                    img_s=round(b / med(us[fmt]) * 1e6)))
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
