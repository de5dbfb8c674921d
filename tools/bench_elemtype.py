"""Typed-tensor decoder (b64_typed_instances) next to the u8 RGB b64 decoder and a device copy.

The protocol of ``bench_pixfmt.py``: in one process, alternating --rounds times,

* ``u16`` / ``f16`` / ``bf16`` / ``f32``: b64_typed_instances on one-image records of random
  finite elements of that type,
* ``u8``: b64_decode_instances on RGB records of the same element count,
* ``copy_<type>``: a plain device copy moving that decoder's bytes (its text in plus its floats
  out; the three 16-bit types share one),

each timed with device events over --iters launches. Before timing, every typed output is
compared with the numpy oracle (``gale.models.preprocess.ElemType.apply``) on the bits. One JSON
line per case, prep and type with every round's time and the medians (and the u8 decoder's rounds
of the same session). Cases: ``--cases 1024x32x32,64x224x224`` (batch x HS x WS, 3 channels), each
without and with the CIFAR prep.
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
from gale.models.preprocess import ELEM_TYPES, ElemType, InputPrep  # noqa: E402

C = native()
IMG = np.dtype([("off", "<i8"), ("slot", "<i4"), ("rec", "<i4")])
TYPES = ("u16", "f16", "bf16", "f32")


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


def random_wire(rng, t, n, per):
    """uint8 [n, per * E]: random finite elements of the type."""
    E = ELEM_TYPES[t][0]
    w = rng.integers(0, 256, (n, per, E), dtype=np.uint8)
    if t != "u16":
        w[..., E - 1] &= 0xBF   # (an exponent bit cleared: no Inf, no NaN)
    return w.reshape(n, -1)


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
        sys.exit("bench_elemtype: no GPU (a timing needs one)")
    cifar = InputPrep.build(3, 1 / 255, (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616))
    s = torch.cuda.current_stream()
    med = lambda v: float(np.median(v))  # noqa: E731
    for case in a.cases.split(","):
        b, HS, WS = (int(v) for v in case.split("x"))
        nd = min(b, a.distinct)
        per = HS * WS * 3
        rng = np.random.default_rng(0)
        dev = {}
        for t in TYPES + ("u8",):
            B = per * ELEM_TYPES[t][0]
            w = (rng.integers(0, 256, (nd, B), dtype=np.uint8) if t == "u8"
                 else random_wire(rng, t, nd, per))
            recs = [b'{"instances":[{"b64":"' + base64.b64encode(p.tobytes()) + b'"}]}'
                    for p in w]
            raw, tab = staged(recs, B, b)
            moved = b * (4 * ((B + 2) // 3) + 4 * per)
            dev[t] = dict(B=B, moved=moved, wire=w,
                          raw=torch.from_numpy(raw.copy()).cuda(),
                          tab=torch.from_numpy(tab.view(np.uint8).copy()).cuda(),
                          c_src=torch.empty(moved // 2, dtype=torch.uint8, device="cuda"),
                          c_dst=torch.empty(moved // 2, dtype=torch.uint8, device="cuda"))
        status = torch.zeros(b, dtype=torch.int32, device="cuda")
        out = torch.empty((b, HS, WS, 3), device="cuda")
        for prep in (False, True):
            kw = cifar.kernel_kwargs() if prep else {}

            def typed(t):
                d = dev[t]

                def fn():
                    err = C.b64_typed_instances(b, d["tab"].data_ptr(), d["raw"].data_ptr(), HS,
                                                WS, 3, out.data_ptr(), status.data_ptr(),
                                                s.cuda_stream, 0, dtype=t, **kw)
                    assert err == 0, err
                return fn

            def u8_decode():
                d = dev["u8"]
                return lambda: C.b64_decode_instances(b, d["tab"].data_ptr(), d["raw"].data_ptr(),
                                                      HS, WS, 3, out.data_ptr(),
                                                      status.data_ptr(), s.cuda_stream, 0, **kw)

            def copy(t):
                d = dev[t]
                return lambda: d["c_dst"].copy_(d["c_src"])

            # the outputs first: every type against the numpy oracle, on the bits
            for t in TYPES:
                out.fill_(-1.0)
                typed(t)()
                torch.cuda.synchronize()
                assert (status.cpu().numpy() == 0).all()
                want = ElemType(t).apply(dev[t]["wire"], HS, WS, 3, cifar if prep else None)
                got = out[:nd].cpu().numpy()
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
                    f"{t}: the kernel and the oracle disagree"
            fns = [(t, typed(t)) for t in TYPES] + [("u8", u8_decode())]
            fns += [("copy_" + t, copy(t)) for t in ("f16", "f32", "u8")]
            for _, fn in fns:
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            us = {name: [] for name, _ in fns}
            for _ in range(a.rounds):
                for name, fn in fns:
                    us[name].append(round(timed(fn, a.iters), 2))
            for t in TYPES + ("u8",):
                d = dev[t]
                cp = us["copy_" + ("f16" if t in ("u16", "bf16") else t)]
                line = json.dumps(dict(
                    kernel="b64_decode_instances" if t == "u8" else "b64_typed_instances",
                    input_dtype=t, batch=b, size=[HS, WS, 3], prep=prep, iters=a.iters,
                    chars_per_image=4 * ((d["B"] + 2) // 3), moved_bytes=d["moved"],
                    us=us[t], us_median=med(us[t]), us_min=min(us[t]), us_max=max(us[t]),
                    u8_us=us["u8"], u8_us_median=med(us["u8"]),
                    copy_us=cp, copy_us_median=med(cp), copy_us_min=min(cp), copy_us_max=max(cp),
                    vs_copy=round(med(us[t]) / med(cp), 2),
                    gb_s=round(d["moved"] / med(us[t]) / 1e3, 1),
                    copy_gb_s=round(d["moved"] / med(cp) / 1e3, 1),
                    img_s=round(b / med(us[t]) * 1e6)))
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
