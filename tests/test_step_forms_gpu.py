"""The serving forms of the whole-network forwards and of the prediction formatter, at kernel
level: the InputTable passed by value (Executor.launch_table), the device pointer table `xs`,
the device batch count, the StepOut epilogue (prediction text, verdict hand-off), and
format_floats_java_dev / _step.

Reference: the same executor's plain form (infer_eager: contiguous input, host count, no
epilogue) on the same images. The forms differ only in addresses and counts, so every comparison
is bit identity. One case per model also checks the table form against the fp32 oracle with the
budgets of tests/test_models_gpu.py, so the file stands on its own. Images are scattered over
separately allocated arenas whose other floats are NaN; outputs are prefilled with -7.0, text with
0xEE and status_out with 0x5A bytes, and every "untouched" claim is checked against those. Every
code, pointer and count passed addresses memory the test allocated.

8-wave ResNet-20 (GALE_R20_WAVES=8) against the 4-wave kernel: the convolutions run the same MFMA
sequence per output, but the head's global average pool does not add in the same order (each of
the NW waves adds 64 / NW pixels, then NW partial sums are added), so the two forms can
legitimately differ in the last bit of the pooled fp32 sums. Measured on the MI355X: batch 1 is
bit identical, batch 37 is not (largest relative logit difference 9.9e-08). The 8-wave rows are
therefore held to the bounds tests/test_models_gpu.py applies to the fused kernel (against the
4-wave rows, the bf16 emulation and the fp32 oracle); what stays bit identical is asserted as
such: the table form against the plain form inside the 8-wave process, and the batch past the CU
count, which falls back to the 4-wave kernel.
"""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gale._native import native
from gale.models import fold_params, get_model, init_params
from gale.models.reference import forward
from gale.parallel.weights import materialize_weights
from gale.runtime.replica import ModelReplica
from test_models_gpu import rel_logit_err

pytestmark = pytest.mark.gpu

C = native()
SLOT = C.FLOAT_TEXT_SLOT
KEYS = ["resnet20", "resnet20_fp8", "lenet5"]
NAN = float("nan")
OUT_FILL, TEXT_FILL, STATUS_FILL = -7.0, 0xEE, 0x5A5A5A5A


# ---- models, replicas, buffers -----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def model(key):
    name, _, wd = key.partition("_")
    net = get_model(name)
    params = init_params(net, seed=11, calib_batch=16)
    packed = materialize_weights(net, torch.device("cuda", 0), params=params, wdtype=wd or "bf16")
    return net, params, packed


@functools.lru_cache(maxsize=None)
def replica(key, max_batch):
    net, _, packed = model(key)
    rep = ModelReplica(net, packed, max_batch=max_batch, slots=1,
                       wdtype="fp8" if key.endswith("fp8") else "bf16", fused=True)
    assert len(rep.ops) == 1 and rep.executor.step_out_ok
    return rep


def images(key, n, seed=99):
    net = model(key)[0]
    return torch.rand((n,) + tuple(net.input_shape), generator=torch.Generator().manual_seed(seed))


def stream():
    return torch.cuda.current_stream().cuda_stream


def put(ptr, t):
    """Copy the device tensor t to the raw device address ptr."""
    C.memcpy_async(ptr, t.data_ptr(), t.numel() * t.element_size(), stream())
    torch.cuda.synchronize()


def fill_out(ex):
    put(ex.output_ptr(0), torch.full((ex.max_batch, 10), OUT_FILL, device="cuda"))


def read_out(ex):
    torch.cuda.synchronize()
    out = torch.empty(ex.max_batch, 10, device="cuda")
    C.memcpy_async(out.data_ptr(), ex.output_ptr(0), out.numel() * 4, stream())
    torch.cuda.synchronize()
    return out.cpu()


def text_buffer(values):
    mb = C.MappedBuffer(values * SLOT)
    v = mb.numpy()
    v[:] = TEXT_FILL
    return mb, v.reshape(-1, SLOT)


def dev_int(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def same_bits(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                              b.contiguous().view(torch.int32))


def untouched(rows):
    return bool((rows == OUT_FILL).all())


def check_text(tv, values):
    """Slots [0, len(values)) are the host's Float.toString of the values (characters from byte
    0, length in byte 15); every later slot still holds the prefill."""
    flat = np.asarray(values, dtype=np.float32).reshape(-1)
    for i, v in enumerate(flat):
        got = bytes(tv[i, :tv[i, SLOT - 1]]).decode()
        assert got == C.format_float_java(float(v)), (i, float(v), got)
    assert (tv[len(flat):] == TEXT_FILL).all()


def scatter(x, places, nbases, slots):
    """Image k of x at slot places[k][1] of arena places[k][0]; every other float is NaN."""
    per = x[0].numel()
    arenas = [torch.full((slots * per,), NAN, device="cuda") for _ in range(nbases)]
    for img, (b, s) in zip(x, places):
        arenas[b][s * per:(s + 1) * per] = img.reshape(-1).cuda()
    return arenas


def table_code(base, slot):
    return (base << 24) | slot


# 36 distinct places over 16 bases of 4 slots: image i in base 7 i mod 16; a base's slots in
# the order it meets them are 2, 0, 3 (even bases) or 0, 3, 1 (odd ones): not monotonic
PLACES = [((7 * i) % 16, ((2, 0, 3), (0, 3, 1))[(7 * i) % 2][i // 16]) for i in range(36)]
# table position -> image: image 3 is referenced by positions 3 and 20
TABLE_IMG = list(range(20)) + [3] + list(range(20, 36))


def scattered_table(key):
    x = images(key, 36)
    arenas = scatter(x, PLACES, C.INPUT_TABLE_BASES, 4)
    codes = [table_code(*PLACES[k]) for k in TABLE_IMG]
    return x[TABLE_IMG], arenas, codes


def test_table_layout_is_the_intended_one():
    assert len(set(PLACES)) == 36 and len(TABLE_IMG) == 37
    assert (0, 0) in PLACES and max(b for b, _ in PLACES) == C.INPUT_TABLE_BASES - 1 == 15
    by_base = {}
    for k in TABLE_IMG:
        by_base.setdefault(PLACES[k][0], []).append(PLACES[k][1])
    seqs = [s for s in by_base.values() if len(s) >= 3]
    assert seqs and all(s != sorted(s) and s != sorted(s, reverse=True) for s in seqs)
    # the decode under test, and the image two mutations of it would serve instead
    codes = [table_code(*PLACES[k]) for k in TABLE_IMG]
    assert [(c >> 24, c & 0xffffff) for c in codes] == [PLACES[k] for k in TABLE_IMG]
    image_at = {p: k for k, p in enumerate(PLACES)}  # (no entry: that slot is NaN)
    # a shift of 23 doubles the base: of the positions whose doubled base is still a base of the
    # table, none gets its own image (a NaN slot or another image)
    moved = [(k, image_at.get((c >> 23, c & 0xffffff))) for k, c in zip(TABLE_IMG, codes)
             if 0 < (c >> 23) < C.INPUT_TABLE_BASES]
    assert len(moved) >= 10 and all(k != got for k, got in moved)
    # a 16-bit slot mask: the wide-slot case's first code then names its second image
    assert (table_code(0, 65537) & 0xffff) == (table_code(0, 1) & 0xffffff)


# ---- the InputTable form -----------------------------------------------------------------------

@pytest.mark.parametrize("key", KEYS)
def test_input_table_scattered(key):
    net, params, packed = model(key)
    rep = replica(key, 64)
    ex = rep.executor
    x, arenas, codes = scattered_table(key)
    ref = rep.infer_eager(x).cpu()
    text, tv = text_buffer(64 * 10)
    fill_out(ex)
    ex.launch_table(0, 37, [a.data_ptr() for a in arenas], codes, stream(), text=text.ptr)
    out = read_out(ex)
    assert same_bits(out[:37], ref)          # row i: the image at code i
    assert same_bits(out[3], out[20])        # one image behind two table positions
    assert untouched(out[37:])
    check_text(tv, out[:37].numpy())         # slots [0, 370) the text, [370, 640) the prefill
    # (launch_table passes no status / status_out / nrec at all: the table step has none)

    # the table form against the fp32 oracle, on its own
    folded = fold_params(net, params)
    want = forward(net, folded, x)
    if key.endswith("fp8"):
        from gale.models.graph import act_scales_from_packed

        emu = forward(net, folded, x, fp8_scales=act_scales_from_packed(net, packed))
        e_ref, budget = rel_logit_err(out[:37], want), rel_logit_err(emu, want)
        print(f"\n{key} table form vs fp32 mean {e_ref.mean().item():.2e} max "
              f"{e_ref.max().item():.2e} (quantisation budget mean {budget.mean().item():.2e})")
        assert e_ref.mean().item() < 1.25 * budget.mean().item() + 5e-3
    else:
        emu = forward(net, folded, x, bf16=True, bf16_acts=key != "lenet5")
        err = rel_logit_err(out[:37], want).max().item()
        budget = rel_logit_err(emu, want).max().item()
        print(f"\n{key} table form rel logit err vs fp32 {err:.2e} (bf16 emulation vs fp32 "
              f"{budget:.2e})")
        assert err < 1.5 * budget + 5e-3, f"{key}: relative logit error {err} (budget {budget})"


def test_input_table_slot_wider_than_16_bits():
    """LeNet-5 images at slots 65 537 and 1 of one arena: a 16-bit slot mask or a narrow multiply
    serves the image at slot 1 (or NaN) for the first."""
    key, per, hi = "lenet5", 784, 65537
    rep = replica(key, 64)
    ex = rep.executor
    x = images(key, 2)
    arena = torch.empty((hi + 1) * per, device="cuda")  # ~206 MB; NaN only around the images
    arena[:3 * per] = NAN
    arena[(hi - 2) * per:] = NAN
    arena[hi * per:(hi + 1) * per] = x[0].reshape(-1).cuda()
    arena[per:2 * per] = x[1].reshape(-1).cuda()
    ref = rep.infer_eager(x).cpu()
    assert not same_bits(ref[0], ref[1])
    text, tv = text_buffer(64 * 10)
    fill_out(ex)
    ex.launch_table(0, 2, [arena.data_ptr()], [table_code(0, hi), table_code(0, 1)], stream(),
                    text=text.ptr)
    out = read_out(ex)
    assert same_bits(out[:2], ref) and untouched(out[2:])
    check_text(tv, out[:2].numpy())


@pytest.mark.parametrize("key", KEYS)
def test_input_table_full(key):
    """batch = INPUT_TABLE_IMAGES with max_batch 512: every code of the table is used, and the
    ResNet-20 grid-stride loop runs with a table wherever 512 exceeds the resident workgroups."""
    n = C.INPUT_TABLE_IMAGES
    assert n == 512
    rep = replica(key, n)
    ex = rep.executor
    x = images(key, n)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(7)).tolist()
    places = [(p // 32, p % 32) for p in perm]
    arenas = scatter(x, places, 16, 32)
    ref = rep.infer_eager(x).cpu()
    text, tv = text_buffer(n * 10 + 8)
    fill_out(ex)
    ex.launch_table(0, n, [a.data_ptr() for a in arenas], [table_code(*p) for p in places],
                    stream(), text=text.ptr)
    out = read_out(ex)
    assert same_bits(out, ref)
    check_text(tv, out.numpy())


@pytest.mark.parametrize("key", KEYS)
def test_input_table_refusals_write_nothing(key):
    x, arenas, codes = scattered_table(key)
    bases = [a.data_ptr() for a in arenas]
    rep64, rep600 = replica(key, 64), replica(key, 600)
    # (512 codes for the launches that ask for more images than a 37-entry list names)
    codes512 = (codes * 14)[:512]
    cases = [(rep600, 513, bases, codes512),       # more than an InputTable holds
             (rep64, 65, bases, codes512),         # more than max_batch
             (rep64, 0, bases, codes),
             (rep64, 37, [0] + bases[1:], codes)]  # a null first base means "no table"
    for rep, batch, b, c in cases:
        ex = rep.executor
        fill_out(ex)
        with pytest.raises((ValueError, RuntimeError)):
            ex.launch_table(0, batch, b, c, stream())
        assert untouched(read_out(ex)), batch
    ex = rep64.executor
    fill_out(ex)
    with pytest.raises(ValueError):                # lists longer than the table: before any launch
        ex.launch_table(0, 37, bases + [bases[0]], codes, stream())
    with pytest.raises(ValueError):
        ex.launch_table(0, 37, bases, codes512 + [codes[0]], stream())
    assert untouched(read_out(ex))


def test_step_forms_refused_on_a_multi_kernel_plan():
    net = get_model("resnet50")
    params = init_params(net, seed=21, calib_batch=4)
    packed = materialize_weights(net, torch.device("cuda", 0), params=params)
    rep = ModelReplica(net, packed, max_batch=2, slots=1)
    ex = rep.executor
    assert len(rep.ops) > 1 and not ex.step_out_ok
    arena = torch.zeros(2 * 224 * 224 * 3, device="cuda")
    text, tv = text_buffer(2 * 1000)
    fill = torch.full((2, 1000), OUT_FILL, device="cuda")
    put(ex.output_ptr(0), fill)
    with pytest.raises(RuntimeError):
        ex.launch_table(0, 1, [arena.data_ptr()], [0], stream())
    with pytest.raises(RuntimeError):
        ex.launch_device_batch(0, dev_int(1).data_ptr(), stream(), text=text.ptr)
    torch.cuda.synchronize()
    got = torch.empty_like(fill)
    C.memcpy_async(got.data_ptr(), ex.output_ptr(0), got.numel() * 4, stream())
    torch.cuda.synchronize()
    assert untouched(got.cpu()) and (tv == TEXT_FILL).all()


# ---- the xs pointer table ----------------------------------------------------------------------

@pytest.mark.parametrize("key", KEYS)
def test_xs_pointer_table(key):
    rep = replica(key, 64)
    ex = rep.executor
    x = images(key, 36)
    per = x[0].numel()
    arenas = scatter(x, PLACES, 16, 4)
    order = torch.randperm(36, generator=torch.Generator().manual_seed(5)).tolist() + [3]
    ptrs = [arenas[PLACES[k][0]].data_ptr() + 4 * per * PLACES[k][1] for k in order]
    assert all(p % 16 == 0 for p in ptrs)
    xs = torch.tensor(ptrs, dtype=torch.int64, device="cuda")  # the table itself: device memory
    put(ex.input_ptr(0), torch.full((64 * per,), NAN, device="cuda"))  # must not be read
    ref = rep.infer_eager(x[order]).cpu()
    d_batch = dev_int(37)
    fill_out(ex)
    ex.launch_device_batch(0, d_batch.data_ptr(), stream(), xs=xs.data_ptr())
    out = read_out(ex)
    assert same_bits(out[:37], ref) and untouched(out[37:])


# ---- the device batch count and the epilogue ---------------------------------------------------

@pytest.mark.parametrize("count", [0, 1, 37, 64, 1000])
@pytest.mark.parametrize("key", KEYS)
def test_device_batch_count(key, count):
    rep = replica(key, 64)
    ex = rep.executor
    x = images(key, 64)
    ref = rep.infer_eager(x).cpu()
    put(ex.input_ptr(0), x.cuda())
    text, tv = text_buffer(64 * 10 + 8)
    d_batch = dev_int(count)
    fill_out(ex)
    ex.launch_device_batch(0, d_batch.data_ptr(), stream(), text=text.ptr)
    out = read_out(ex)
    n = min(count, 64)  # a count past max_batch serves max_batch images
    assert same_bits(out[:n], ref[:n]) and untouched(out[n:])
    check_text(tv, out[:n].numpy())


def handoff_arrays(n=640):
    pattern = (np.arange(n, dtype=np.int32) * 7) % 5 + 1  # non-zero everywhere
    status = torch.from_numpy(pattern.copy()).cuda()
    mb = C.MappedBuffer(4 * n)
    so = mb.numpy().view(np.int32)
    so[:] = STATUS_FILL
    return pattern, status, mb, so


def check_handoff(pattern, status, so, nrec):
    """status_out[i] = status[i], status[i] = 0 for i < nrec; both unchanged from nrec on. (A
    loop to nrec + 1 changes entry nrec of both; one to nrec - 1 leaves entry nrec - 1.)"""
    st = status.cpu().numpy()
    assert (so[:nrec] == pattern[:nrec]).all() and (st[:nrec] == 0).all()
    assert (so[nrec:] == STATUS_FILL).all() and (st[nrec:] == pattern[nrec:]).all()


@pytest.mark.parametrize("nrec,max_batch", [(0, 64), (1, 64), (257, 600), (600, 600)])
@pytest.mark.parametrize("key", KEYS)
def test_verdict_handoff(key, nrec, max_batch):
    """257 and 600 verdicts: the 256-thread stride loop of workgroup 0 wraps."""
    rep = replica(key, max_batch)
    ex = rep.executor
    x = images(key, 37)
    ref = rep.infer_eager(x).cpu()
    put(ex.input_ptr(0), x.cuda())
    d_nrec = dev_int(nrec)
    for count in (37, 0):  # no image at all: the hand-off still happens
        pattern, status, so_mb, so = handoff_arrays()
        text, tv = text_buffer(max_batch * 10)
        d_batch = dev_int(count)
        fill_out(ex)
        ex.launch_device_batch(0, d_batch.data_ptr(), stream(), text=text.ptr,
                               status=status.data_ptr(), status_out=so_mb.ptr,
                               nrec=d_nrec.data_ptr())
        out = read_out(ex)
        check_handoff(pattern, status, so, nrec)
        assert same_bits(out[:count], ref[:count]) and untouched(out[count:])
        check_text(tv, out[:count].numpy())


def test_verdict_handoff_needs_status_and_count():
    ex = replica("lenet5", 64).executor
    pattern, status, so_mb, so = handoff_arrays()
    d_batch = dev_int(1)
    fill_out(ex)
    with pytest.raises(ValueError):  # status_out without status / nrec: refused, nothing launched
        ex.launch_device_batch(0, d_batch.data_ptr(), stream(), status_out=so_mb.ptr)
    assert untouched(read_out(ex))
    check_handoff(pattern, status, so, 0)


# ---- format_floats_java_dev / _step ------------------------------------------------------------

def probs(n):
    """The "probs" generator of tests/test_format_gpu.py: softmax rows, n values."""
    rng = np.random.default_rng(1)
    z = rng.normal(size=(-(-n // 10), 10)).astype(np.float32) * 4
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32).ravel()[:n]


FORMAT_CASES = [(per, mx, count) for per, mx in ((10, 64), (1000, 4)) for count in (0, 3, mx)]


@pytest.mark.parametrize("per,mx,count", FORMAT_CASES)
def test_format_floats_java_dev(per, mx, count):
    max_n = per * mx
    x = probs(max_n)
    xd = torch.from_numpy(x).cuda()
    text, tv = text_buffer(max_n + 8)
    d_count = dev_int(count)
    C.format_floats_java_dev(max_n, d_count.data_ptr(), per, xd.data_ptr(), text.ptr, stream())
    torch.cuda.synchronize()
    check_text(tv, x[:count * per])


@pytest.mark.parametrize("per,mx,count", FORMAT_CASES)
def test_format_floats_java_step(per, mx, count):
    max_n = per * mx
    n = count * per
    x = probs(max_n)
    xd = torch.from_numpy(x).cuda()
    d_count = dev_int(count)
    # verdict counts below and above the value count, within the launch
    nrecs = sorted({n // 2, min(n + 259, max_n), max_n})
    assert any(r < n for r in nrecs) or n == 0
    assert any(r > n for r in nrecs) or n == max_n
    for nrec in nrecs:
        pattern, status, so_mb, so = handoff_arrays(max_n + 8)
        text, tv = text_buffer(max_n + 8)
        d_nrec = dev_int(nrec)
        C.format_floats_java_step(max_n, d_count.data_ptr(), per, xd.data_ptr(), text.ptr,
                                  d_nrec.data_ptr(), status.data_ptr(), so_mb.ptr, stream())
        torch.cuda.synchronize()
        check_text(tv, x[:n])
        check_handoff(pattern, status, so, nrec)


def test_format_floats_java_step_needs_the_verdict_count():
    x = torch.from_numpy(probs(30)).cuda()
    pattern, status, so_mb, so = handoff_arrays(64)
    text, tv = text_buffer(64)
    d_count = dev_int(3)
    with pytest.raises(RuntimeError):
        C.format_floats_java_step(30, d_count.data_ptr(), 10, x.data_ptr(), text.ptr, 0,
                                  status.data_ptr(), so_mb.ptr, stream())
    torch.cuda.synchronize()
    assert (tv == TEXT_FILL).all()
    check_handoff(pattern, status, so, 0)


# ---- the 8-wave ResNet-20 ----------------------------------------------------------------------

def waves_run():
    """The fused bf16 ResNet-20 at batches 1, 37, the CU count and one more (plain form), and the
    table form with text at 37: run by the child (8 waves up to the CU count) and the parent."""
    key = "resnet20"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rep = replica(key, cus + 1)
    ex = rep.executor
    x = images(key, cus + 1)
    res = {"cus": np.array(cus)}
    for b in (1, 37, cus, cus + 1):
        res[f"plain_{b}"] = rep.infer_eager(x[:b]).cpu().numpy()
    xt, arenas, codes = scattered_table(key)
    res["plain_table"] = rep.infer_eager(xt).cpu().numpy()
    text, tv = text_buffer(37 * 10 + 8)
    fill_out(ex)
    ex.launch_table(0, 37, [a.data_ptr() for a in arenas], codes, stream(), text=text.ptr)
    res["table_37"] = read_out(ex).numpy()
    res["text_37"] = tv.copy()
    return res


_WAVES_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from test_step_forms_gpu import waves_run
np.savez(sys.argv[2], **waves_run())
print("WAVES_OK")
"""


def test_resnet20_eight_waves(tmp_path):
    """One fresh child with GALE_R20_WAVES=8 (the selection is a per-process static)."""
    assert os.environ.get("GALE_R20_WAVES") != "8"  # this process runs the 4-wave kernel
    tests = os.path.dirname(os.path.abspath(__file__))
    path = str(tmp_path / "waves8.npz")
    env = dict(os.environ, GALE_R20_WAVES="8")
    r = subprocess.run([sys.executable, "-c", _WAVES_SCRIPT, tests, path], env=env,
                       cwd=os.path.dirname(tests), capture_output=True, text=True, timeout=100)
    assert r.returncode == 0 and "WAVES_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    w8 = np.load(path)
    w4 = waves_run()
    cus = int(w4["cus"])
    assert int(w8["cus"]) == cus
    # past one image per CU the child falls back to the 4-wave kernel: the same code
    assert same_bits(w8[f"plain_{cus + 1}"], w4[f"plain_{cus + 1}"])
    # the child's table form serves the image at code i and prints its own rows
    assert same_bits(w8["table_37"][:37], w8["plain_table"])
    assert same_bits(w8["table_37"][3], w8["table_37"][20])
    assert untouched(w8["table_37"][37:])
    check_text(w8["text_37"], w8["table_37"][:37])
    net, params, _ = model("resnet20")
    folded = fold_params(net, params)
    xt = scattered_table("resnet20")[0]
    cases = [(f"plain_{b}", images("resnet20", cus + 1)[:b]) for b in (1, 37, cus)]
    cases.append(("table_37", xt))
    for name, x in cases:
        a, b = torch.from_numpy(w8[name][:len(x)]), torch.from_numpy(w4[name][:len(x)])
        same = same_bits(a, b)
        ref, emu = forward(net, folded, x), forward(net, folded, x, bf16=True)
        e_ab, e_emu = rel_logit_err(a, b).max().item(), rel_logit_err(a, emu).max().item()
        e_ref, budget = rel_logit_err(a, ref).max().item(), rel_logit_err(emu, ref).max().item()
        print(f"\nresnet20 8 waves {name}: bit identical to 4 waves {same}; vs 4 waves "
              f"{e_ab:.2e}, vs bf16 emulation {e_emu:.2e}, vs fp32 {e_ref:.2e} "
              f"(budget {budget:.2e})")
        # (the bounds of test_resnet20_fused_matches_layerwise_and_fp32; the head's pooling order
        # differs between the two forms, see the module docstring)
        assert e_ab < 5e-3 and e_emu < 5e-3 and e_ref < 1.5 * budget + 5e-3, name
