"""Raw-record converter (raw_instances) next to the b64 decoder of the same pixels and a device copy.

The protocol of ``bench_elemtype.py``: in one process, alternating --rounds times, for each of
``u8`` / ``f16`` / ``f32`` / ``rgba``

* ``raw_<kind>``: raw_instances on images of random finite bytes of that kind, back to back,
* ``b64_<kind>``: the b64 decoder of the same bytes as one-image records (b64_decode_instances,
  b64_typed_instances or b64_packed_instances),
* ``copy_<kind>``: a plain device copy moving the raw kernel's bytes (its source in plus its
  floats out),

each timed with device events over --iters launches. Before timing, the raw output is compared
with the b64 decoder's on the bits. One JSON line per case, prep and kind with every round's time,
the medians and min-max. The copy and the b64 decoder are yardsticks, not thresholds. Cases:
``--cases 1024x32x32,64x224x224`` (batch x HS x WS, 3 channels), each without and with the CIFAR
prep.
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
from gale.models.preprocess import InputPrep  # noqa: E402

C = native()
IMG = np.dtype([("off", "<i8"), ("slot", "<i4"), ("rec", "<i4")])
KINDS = {"u8": 1, "f16": 2, "f32": 4, "rgba": None}   # bytes per element; rgba: 4 per pixel


def b64_staged(wire, batch):
    """One-image records' strings, 16-byte aligned, cycled up to `batch`, with their table."""
    buf = bytearray()
    tab = np.zeros(batch, dtype=IMG)
    strings = [base64.b64encode(w.tobytes()) for w in wire]
    for i in range(batch):
        s = strings[i % len(strings)]
        head = b'{"b64":"'
        tab[i] = (len(buf) + len(head), i, i)
        buf += head + s + b'"},'
        buf += b" " * ((-len(buf)) % 16)
    buf += b" " * 16
    return np.frombuffer(bytes(buf), dtype=np.uint8), tab


def raw_staged(wire, batch):
    """The images back to back (one record's value), cycled up to `batch`, with their table."""
    B = wire.shape[1]
    buf = np.concatenate([wire[i % len(wire)] for i in range(batch)] + [np.zeros(16, np.uint8)])
    tab = np.zeros(batch, dtype=IMG)
    tab["off"], tab["slot"], tab["rec"] = np.arange(batch) * B, np.arange(batch), np.arange(batch)
    return buf, tab


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
        sys.exit("bench_raw: no GPU (a timing needs one)")
    assert IMG.itemsize == C.B64_IMAGE_BYTES, "B64Image layout changed (gale/kernels.h)"
    cifar = InputPrep.build(3, 1 / 255, (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616))
    s = torch.cuda.current_stream()
    med = lambda v: float(np.median(v))  # noqa: E731
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    for case in a.cases.split(","):
        b, HS, WS = (int(v) for v in case.split("x"))
        nd, per = min(b, a.distinct), HS * WS * 3
        rng = np.random.default_rng(0)
        dev = {}
        for kind, E in KINDS.items():
            B = HS * WS * 4 if kind == "rgba" else per * E
            w = rng.integers(0, 256, (nd, B), dtype=np.uint8)
            if kind in ("f16", "f32"):
                w.reshape(nd, per, E)[..., E - 1] &= 0xBF   # (an exponent bit cleared: finite)
            rbuf, rtab = raw_staged(w, b)
            bbuf, btab = b64_staged(w, b)
            moved = b * (B + 4 * per)
            dev[kind] = dict(B=B, moved=moved, raw=cuda(rbuf), rtab=cuda(rtab.view(np.uint8)),
                             b64=cuda(bbuf), btab=cuda(btab.view(np.uint8)),
                             c_src=torch.empty(moved // 2, dtype=torch.uint8, device="cuda"),
                             c_dst=torch.empty(moved // 2, dtype=torch.uint8, device="cuda"))
        status = torch.zeros(b, dtype=torch.int32, device="cuda")
        out = torch.empty((b, HS, WS, 3), device="cuda")
        ref = torch.empty((b, HS, WS, 3), device="cuda")
        for prep in (False, True):
            kw = cifar.kernel_kwargs() if prep else {}

            def raw(kind, o=out):
                d = dev[kind]
                names = dict(format="rgba") if kind == "rgba" else dict(dtype=kind)

                def fn():
                    err = C.raw_instances(b, d["rtab"].data_ptr(), d["raw"].data_ptr(), HS, WS, 3,
                                          o.data_ptr(), status.data_ptr(), s.cuda_stream, 0,
                                          **names, **kw)
                    assert err == 0, err
                return fn

            def b64(kind, o=out):
                d = dev[kind]
                args = (b, d["btab"].data_ptr(), d["b64"].data_ptr(), HS, WS, 3, o.data_ptr(),
                        status.data_ptr(), s.cuda_stream, 0)
                if kind == "u8":
                    return lambda: C.b64_decode_instances(*args, **kw)
                if kind == "rgba":
                    return lambda: C.b64_packed_instances(*args, format="rgba", **kw)
                return lambda: C.b64_typed_instances(*args, dtype=kind, **kw)

            def copy(kind):
                d = dev[kind]
                return lambda: d["c_dst"].copy_(d["c_src"])

            # the outputs first: the raw converter against the b64 decoder, on the bits
            for kind in KINDS:
                out.fill_(-1.0)
                ref.fill_(-2.0)
                raw(kind)()
                b64(kind, ref)()
                torch.cuda.synchronize()
                assert (status.cpu().numpy() == 0).all()
                assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), \
                    f"{kind}: the raw converter and the b64 decoder disagree"
            fns = []
            for kind in KINDS:
                fns += [("raw_" + kind, raw(kind)), ("b64_" + kind, b64(kind)),
                        ("copy_" + kind, copy(kind))]
            for _, fn in fns:
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            us = {name: [] for name, _ in fns}
            for _ in range(a.rounds):
                for name, fn in fns:
                    us[name].append(round(timed(fn, a.iters), 2))
            for kind in KINDS:
                d = dev[kind]
                r, q, cp = us["raw_" + kind], us["b64_" + kind], us["copy_" + kind]
                line = json.dumps(dict(
                    kernel="raw_instances", kind=kind, batch=b, size=[HS, WS, 3], prep=prep,
                    iters=a.iters, bytes_per_image=d["B"], moved_bytes=d["moved"],
                    us=r, us_median=med(r), us_min=min(r), us_max=max(r),
                    b64_us=q, b64_us_median=med(q), b64_us_min=min(q), b64_us_max=max(q),
                    copy_us=cp, copy_us_median=med(cp), copy_us_min=min(cp), copy_us_max=max(cp),
                    vs_copy=round(med(r) / med(cp), 2), vs_b64=round(med(r) / med(q), 2),
                    gb_s=round(d["moved"] / med(r) / 1e3, 1),
                    copy_gb_s=round(d["moved"] / med(cp) / 1e3, 1),
                    img_s=round(b / med(r) * 1e6)))
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
