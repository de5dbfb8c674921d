"""The executor against its own launchers: a small hand-built network run through
Executor.run_on equals, bit for bit, the same ops launched one at a time through the kernel
bindings with arguments taken from the ops' named fields - folded and unfolded BatchNorm, whole
batch and batch-chunked with a ragged last chunk. And a plan the executor refuses launches
nothing."""

import pytest
import torch

from gale._native import native
from gale.models import init_params
from gale.models.graph import (OP_AVGPOOL, OP_BN_ACT, OP_CONV, OP_HEAD, OP_MAXPOOL, AvgPool, Conv,
                               Head, MaxPool, Network)
from gale.parallel.weights import materialize_weights
from gale.runtime.replica import ModelReplica

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
B = 3
POOL = ("H", "W", "C", "k", "s", "pad", "Ho", "Wo")


def small_net():
    return Network("plan_probe", (8, 8, 3), 10, [
        Conv("c1", "input", "a", 3, 16, 3, pad=1),
        MaxPool("mp", "a", "b", 2, 2),
        Conv("c2", "b", "c", 16, 16, 3, pad=1, residual="b"),
        AvgPool("gp", "c", "g"),
        Head("fc", "g", 10)], dataset="probe")


def launch_one_by_one(ops, buf_bytes, x):
    """Every op through its own binding, over buffers of this function's own."""
    C = native()
    s = torch.cuda.current_stream().cuda_stream
    out = torch.full((B, 10), float("nan"), device=DEV)
    bufs = [x, out] + [torch.zeros(B * n, dtype=torch.uint8, device=DEV) for n in buf_bytes[2:]]
    at = [t.data_ptr() for t in bufs]
    for op in ops:
        xin, y = at[op["in"]], at[op["out"]]
        res = at[op["res"]] if op["res"] >= 0 else 0
        if op["kind"] == OP_CONV:
            C.conv2d(op["conv"], B, xin, op["w"], op["bias"], op["wscale"], res, y, s)
        elif op["kind"] == OP_MAXPOOL:
            C.maxpool2d(B, *(op[k] for k in POOL), xin, y, s, op["et"])
        elif op["kind"] == OP_AVGPOOL:
            C.avgpool_global(B, op["HW"], op["C"], xin, y, s, op["et"])
        elif op["kind"] == OP_HEAD:
            C.head_pool_dense_softmax(B, op["HW"], op["C"], op["N"], xin, op["w"], op["bias"], y,
                                      s, op["et"], op["in_scale"])
        else:
            assert op["kind"] == OP_BN_ACT and op["et"] == 0
            C.bn_act(B, op["HW"], op["Wo"], op["C"], xin, op["scale"], op["shift"], res,
                     op["res_H"], op["res_W"], op["res_C"], op["res_stride"], op["relu"], y, s)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("fold_bn", [True, False])
def test_executor_equals_its_launchers(fold_bn):
    net = small_net()
    params = init_params(net, seed=5, calib_batch=4)
    packed = materialize_weights(net, DEV, params=params, fold_bn=fold_bn)
    x = torch.rand((B,) + net.input_shape, generator=torch.Generator().manual_seed(2)).to(DEV)
    whole = ModelReplica(net, packed, max_batch=4, slots=2, fold_bn=fold_bn)
    kinds = [op["kind"] for op in whole.ops]
    bn = [] if fold_bn else [OP_BN_ACT]
    assert kinds == ([OP_CONV] + bn + [OP_MAXPOOL, OP_CONV] + bn + [OP_AVGPOOL, OP_HEAD])
    want = launch_one_by_one(whole.ops, whole.buf_bytes, x)
    assert torch.isfinite(want).all() and torch.allclose(want.sum(1), torch.ones(B, device=DEV))
    assert want.std(0).max().item() > 0  # (the images differ, so a misplaced row shows)
    got = whole.infer_eager(x)
    # the first two layers per chunk of 2 images: chunks of 2 and 1
    chunked = ModelReplica(net, packed, max_batch=4, slots=2, fold_bn=fold_bn, chunk=(2, 2))
    assert [op["layer"] < 2 for op in chunked.ops] == [k < len(bn) + 2 for k in range(len(kinds))]
    got_chunked = chunked.infer_eager(x)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(got_chunked, want)


def test_refused_plan_launches_nothing():
    C = native()
    net = small_net()
    packed = materialize_weights(net, DEV, params=init_params(net, seed=5, calib_batch=4))
    rep = ModelReplica(net, packed, max_batch=4, slots=1)
    sentinel = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    bad = [dict(op) for op in rep.ops]
    bad[0]["out"] = len(rep.buf_bytes)  # one past the buffer table
    with pytest.raises(ValueError, match="plan op 0 \\(conv\\): out is outside the buffer table"):
        C.Executor(0, bad, rep.buf_bytes, 4)
    torch.cuda.synchronize()
    assert bool((sentinel == 0x5A).all())
