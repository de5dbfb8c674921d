"""The input resize kernel (resize_crop) against a plain device-to-device copy that moves the
same bytes: the whole source tensor read plus the destination written, as one hipMemcpyAsync of
half that total (it reads and writes each of its bytes once). The copy is the yardstick of a
memory-bound kernel, not a threshold.

Alternating rounds in one process (as tools/bench_topk.py): per case each round times --iters
back-to-back launches of the kernel between device events, then the copy. Every round is appended
to --out (profiles/resize_ab.jsonl) and one summary line per case is printed. Before anything is
timed the kernel's output is compared bit for bit with the host twin. There is no pass mark.

Cases: images x HSxWS -> HR,WR -> HxW (C = 3).

``--antialias`` measures the antialiased kernel (resize_crop_aa) instead: the same three cases
(the second is a pure crop, the first and third downscale) and the torchvision recipe
128 x 375x500 -> 256,341 -> 224x224; each round times resize_crop_aa, then resize_crop (not
antialiased) on the same shape, then the copy. Rounds go to profiles/resize_aa_ab.jsonl; the
output is first compared bit for bit with resize_crop_aa's host twin.
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gale import ops  # noqa: E402
from gale._native import native  # noqa: E402

C = native()
CASES = "256:40x40:32x32:32x32,128:256x256:256x256:224x224,128:300x260:256x240:224x224"
AA_CASES = CASES + ",128:375x500:256x341:224x224"


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
    ap.add_argument("--cases", default="")
    ap.add_argument("--antialias", action="store_true",
                    help="measure resize_crop_aa against resize_crop and the copy")
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=0, help="0 = about 64 GB of traffic per timing")
    ap.add_argument("--band", type=int, default=0,
                    help="--antialias: launch with this band height (1..8) instead of the host's "
                         "choice (rounds are logged with variant = band<N>)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    a.cases = a.cases or (AA_CASES if a.antialias else CASES)
    a.out = a.out or os.path.join("profiles",
                                  "resize_aa_ab.jsonl" if a.antialias else "resize_ab.jsonl")
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize: no GPU (nothing is measured without one)")
    s = torch.cuda.current_stream().cuda_stream
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    dev = torch.cuda.get_device_name(0)
    ch = a.channels
    with open(a.out, "a") as log:
        for case in a.cases.split(","):
            n, src, rs, dst = case.split(":")
            n = int(n)
            (HS, WS), (HR, WR), (H, W) = (tuple(int(v) for v in p.split("x")) for p in (src, rs, dst))
            x = np.random.default_rng(0).integers(0, 256, (n, HS, WS, ch)).astype(np.float32)
            xd = torch.from_numpy(x).cuda()
            out = torch.empty(n, H, W, ch, device="cuda")
            tables = ops.resize_tables(HS, WS, HR, WR, H, W, "cuda")
            ptrs = [t.data_ptr() for t in tables]
            total = (xd.numel() + out.numel()) * 4  # source read + destination written
            half = total // 2
            ca, cb = (torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(2))
            iters = a.iters or int(max(50, min(5000, 64e9 / total)))

            def kernel():
                C.resize_crop(n, HS, WS, H, W, ch, ptrs, xd.data_ptr(), out.data_ptr(), s)

            def copy():
                C.memcpy_async(cb.data_ptr(), ca.data_ptr(), half, s)

            if a.antialias:
                aa = ops.resize_aa_tables(HS, WS, HR, WR, H, W, "cuda")
                aa_out = torch.empty_like(out)
                dims, aptrs, fig = [HS, WS, HR, WR, H, W, ch], aa.ptrs(), list(aa.launch)
                variant = "chosen"
                if a.band:
                    ys, yn = (t.cpu().numpy() for t in aa.tensors[:2])
                    last = [min(y + a.band, H) - 1 for y in range(0, H, a.band)]
                    fig[2] = a.band
                    fig[3] = int(max(ys[l] + yn[l] - ys[y] for y, l in zip(range(0, H, a.band), last)))
                    variant = f"band{a.band}"

                def kernel_aa():
                    C.resize_crop_aa(n, dims, aptrs, fig, xd.data_ptr(), aa_out.data_ptr(), s)

                for _ in range(5):
                    kernel_aa()
                torch.cuda.synchronize()
                k = min(n, 4)
                for lo in (0, n - k):
                    want = C.resize_crop_aa_host(x[lo:lo + k], HR, WR, H, W)
                    got = aa_out[lo:lo + k].cpu().numpy()
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), case
                arms = (("resize_crop_aa", kernel_aa), ("resize_crop", kernel), ("copy", copy))
            else:
                arms = (("resize_crop", kernel), ("copy", copy))

            for fn in (kernel, copy):
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            k = min(n, 4)  # (the host twin on a few images: the first and the last ones)
            for lo in (0, n - k):
                want = C.resize_crop_host(x[lo:lo + k], HR, WR, H, W)
                got = out[lo:lo + k].cpu().numpy()
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), case
            us = {name: [] for name, _ in arms}
            for rnd in range(a.rounds):
                for name, fn in arms:
                    t = round(timed(fn, iters), 3)
                    us[name].append(t)
                    extra = dict(variant=variant, band=fig[2], band_rows=fig[3]) \
                        if name == "resize_crop_aa" else {}
                    log.write(json.dumps(dict(
                        kernel=name, round=rnd, case=case, channels=ch, iters=iters, **extra,
                        us_per_launch=t, bytes=total, gb_per_s=round(total / t * 1e-3, 1),
                        device=dev)) + "\n")
                    log.flush()
            med = {k_: float(np.median(v)) for k_, v in us.items()}
            if a.antialias:
                print(json.dumps(dict(
                    case=case, channels=ch, iters=iters, rounds=a.rounds, bytes=total,
                    taps=fig[:2], band=fig[2], band_rows=fig[3],
                    aa_us=us["resize_crop_aa"], aa_us_median=med["resize_crop_aa"],
                    resize_us=us["resize_crop"], resize_us_median=med["resize_crop"],
                    copy_us=us["copy"], copy_us_median=med["copy"],
                    aa_over_resize=round(med["resize_crop_aa"] / med["resize_crop"], 2),
                    aa_over_copy=round(med["resize_crop_aa"] / med["copy"], 2))), flush=True)
                continue
            print(json.dumps(dict(
                case=case, channels=ch, iters=iters, rounds=a.rounds, bytes=total,
                resize_us=us["resize_crop"], resize_us_median=med["resize_crop"],
                copy_us=us["copy"], copy_us_median=med["copy"],
                resize_gb_per_s=round(total / med["resize_crop"] * 1e-3, 1),
                copy_gb_per_s=round(total / med["copy"] * 1e-3, 1),
                resize_over_copy=round(med["resize_crop"] / med["copy"], 2))), flush=True)


if __name__ == "__main__":
    main()
