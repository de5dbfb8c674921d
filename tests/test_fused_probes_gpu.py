"""The whole-network kernels (csrc/kernels/resnet20_fused.hip, lenet5_fused.hip) and the layered
plans on the exact probe networks of tests/fused_probes.py.

A probe's reference logits are exact in any summation order (test_fused_probes_cpu.py asserts
the conditions), so a launch is held to D <= T, with D = max |centred float64 log of the kernel's
probabilities - centred reference logits| and T = 1e-5 worked out from the fp32 softmax alone
(fused_probes.T), while the smallest single-element error moves a logit by 20 T. Every form prints
its largest D.

One replica per plan is built over one packed device buffer; each probe's packed bytes are copied
over that buffer in place, so the plan's pointers stay valid and nothing is rebuilt or recaptured.

Limits, inherent to observing ten numbers: a pure permutation of the last stage's 64 pixels cannot
be seen through average pooling, and the carrier's gathers distinguish row parity (different
channel halves) but sum the two columns of a cell. Gross misplacements are what the random-weight
tests of test_models_gpu.py catch; the probes exist for the single wrong element.
"""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fused_probes as fp
from gale.runtime.replica import ModelReplica

pytestmark = pytest.mark.gpu

PERSISTENT = [(3, "relu"), (3, "open"), (16, "relu"), (16, "open")]  # (stage 1, stage 3)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def rig(kind):
    """(packed device buffer, fused replica, layered replica) of a model: `r20`, `r20_fp8` or
    `lenet5`. The fused ResNet-20 takes the persistent loop's batch."""
    if kind == "lenet5":
        net, first, big, wd = fp.lenet(), fp.lenet_packed(fp.LENET_SEEDS[0]), 257, "bf16"
    elif kind == "r20":
        net, first, big, wd = fp.r20(), fp.r20_packed(0, "relu"), 2 * cus() + 37, "bf16"
    else:
        net, first = fp.r20(), fp.r20_fp8_packed(fp.FP8_CONVS[0], "relu")
        big, wd = fp.N_IMAGES, "fp8"
    buf = first.to(torch.device("cuda", 0))
    fused = ModelReplica(net, buf, max_batch=big, slots=1, wdtype=wd, fused=True)
    layered = ModelReplica(net, buf, max_batch=min(big, 257), slots=1, wdtype=wd, fused=False)
    assert len(fused.ops) == 1 and len(layered.ops) > 1
    return buf, fused, layered


def load(kind, packed):
    """Overwrite the rig's packed buffer in place with another probe's bytes."""
    buf = rig(kind)[0]
    assert packed.shape == buf.shape
    torch.cuda.synchronize()
    buf.copy_(packed)
    torch.cuda.synchronize()


def check(name, probs, logits, failures):
    """D of one launch; a row that does not sum to 1 or a D above T is recorded."""
    probs = probs.cpu()
    d = (fp.centred_log(probs) - fp.centred(logits)).abs()
    D = d.max().item()
    rows = (probs.double().sum(1) - 1).abs().max().item()
    if not D <= fp.T or not rows <= 1e-5:
        img, cls = divmod(int(d.argmax()), d.shape[1])
        failures.append(f"{name}: D {D:.3e} at image {img} class {cls}, rows sum off by {rows:.1e}")
    return D


def report(form, Ds, failures):
    print(f"\n{form}: largest D {max(Ds):.3e} over {len(Ds)} launches (T {fp.T:.0e})")
    assert not failures, f"{form}:\n" + "\n".join(failures)


@pytest.mark.parametrize("form", ["four_waves", "layered"])
def test_resnet20_probes(form):
    """Every probe and variant at batch 32, eager: the 4-wave whole-network kernel, and the
    layered plan (conv_mfma's small-batch forms and head_pool_dense_softmax) on the same bytes."""
    assert os.environ.get("GALE_R20_WAVES") != "8"
    rep = rig("r20")[1 if form == "four_waves" else 2]
    Ds, failures = [], []
    for p in fp.r20_probes():
        load("r20", fp.r20_packed(p.conv, p.variant))
        Ds.append(check(p.name, rep.infer_eager(p.x), p.logits, failures))
    report(f"resnet20 {form}", Ds, failures)


def test_resnet20_probes_persistent_loop():
    """2 * CUs + 37 images, the 32 repeated cyclically: past the grid of 2 * CUs workgroups a
    workgroup's second and third images run over the LDS the previous image left behind (a stale
    border or shortcut cell shows here). Every row has the bits of its image's row among the
    first 32, and meets T."""
    _, rep, _ = rig("r20")
    B = 2 * cus() + 37
    Ds, failures = [], []
    for i, variant in PERSISTENT:
        p = fp.r20_probe(i, variant)
        load("r20", fp.r20_packed(i, variant))
        idx = torch.arange(B) % fp.N_IMAGES
        out = rep.infer_eager(p.x[idx]).cpu()
        Ds.append(check(p.name, out, p.logits[idx], failures))
        same = out.view(torch.int32) == out[: fp.N_IMAGES][idx].view(torch.int32)
        if not bool(same.all()):
            bad = (~same.all(1)).nonzero().flatten().tolist()
            failures.append(f"{p.name}: rows {bad[:8]} differ from their image's first row")
    report("resnet20 persistent loop", Ds, failures)


def eight_wave_rows():
    """Every probe at batch 32 on the fused kernel of this process (the child: 8 waves)."""
    rep = rig("r20")[1]
    rows = {}
    for p in fp.r20_probes():
        load("r20", fp.r20_packed(p.conv, p.variant))
        rows[f"{p.conv}_{p.variant}"] = rep.infer_eager(p.x).cpu().numpy()
    return rows


_WAVES_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from test_fused_probes_gpu import eight_wave_rows
np.savez(sys.argv[2], **eight_wave_rows())
print("PROBES_OK")
"""


def test_resnet20_probes_eight_waves(tmp_path):
    """One fresh child with GALE_R20_WAVES=8 (the selection is a per-process static; batch 32 is
    below the CU count) runs every probe once; the parent holds its rows to the same T."""
    assert os.environ.get("GALE_R20_WAVES") != "8" and fp.N_IMAGES <= cus()
    tests = os.path.dirname(os.path.abspath(__file__))
    path = str(tmp_path / "probes8.npz")
    env = dict(os.environ, GALE_R20_WAVES="8")
    r = subprocess.run([sys.executable, "-c", _WAVES_SCRIPT, tests, path], env=env,
                       cwd=os.path.dirname(tests), capture_output=True, text=True, timeout=100)
    assert r.returncode == 0 and "PROBES_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    rows = np.load(path)
    Ds, failures = [], []
    for p in fp.r20_probes():
        out = torch.from_numpy(rows[f"{p.conv}_{p.variant}"])
        Ds.append(check(p.name, out, p.logits, failures))
    report("resnet20 eight_waves", Ds, failures)


@pytest.mark.parametrize("form", ["fused", "layered"])
def test_resnet20_fp8_probes(form):
    """The fp8 probes against the e4m3 emulation: every value ahead of a rounding is exact, so
    kernel and emulation cannot differ by summation order and the logits meet the same T."""
    buf, fused, layered = rig("r20_fp8")
    rep = fused if form == "fused" else layered
    Ds, failures = [], []
    for i in fp.FP8_CONVS:
        for variant in fp.VARIANTS:
            p = fp.r20_fp8_probe(i, variant)
            assert rep.act_scales == p.scales  # (launch constants of the plan: the same for all)
            load("r20_fp8", fp.r20_fp8_packed(i, variant))
            Ds.append(check(p.name, rep.infer_eager(p.x), p.logits, failures))
    report(f"resnet20 fp8 {form}", Ds, failures)


@pytest.mark.parametrize("batch", fp.LENET_BATCHES)
@pytest.mark.parametrize("seed", fp.LENET_SEEDS)
@pytest.mark.parametrize("form", ["fused", "layered"])
def test_lenet5_probes(form, seed, batch):
    """LeNet-5 networks that are exact in all five layers, fused kernel (fp32 activations) and
    layered plan (bf16 activations: the probes' integers stay within 256), at the batches
    test_lenet5_fused_matches_layerwise_and_fp32 crosses."""
    rep = rig("lenet5")[1 if form == "fused" else 2]
    p = fp.lenet_probe(seed)
    load("lenet5", fp.lenet_packed(seed))
    failures = []
    D = check(f"{p.name} batch {batch}", rep.infer_eager(p.x[:batch]), p.logits[:batch], failures)
    report(f"lenet5 {form} seed {seed} batch {batch}", [D], failures)
