"""Top-k output on the GPU: the selection + text kernel (csrc/kernels/topk.hip) in its three
forms, bit-exact against the score-order rule in numpy and the host's Float.toString
(tests/test_topk_cpu.py holds the oracle and the adversarial rows), and the engine with --top-k
on every site that launches the kernel.

Output buffers are host-mapped (as the replica's are) and prefilled with 0xEE bytes; every
"untouched" claim is checked against that fill.

Engine cases compare a --top-k run with a top_k = 0 run of the same keyed records: the class
indices must be the rule's selection from the full row, and every score text must be the very
string the full row holds for that class. ResNet-50's plan is not a whole-network kernel, so its
step is launched op by op and ends with topk_java (the form with the host's count) at 1000
classes; topk_java_step is launched by steps that take their counts from the device but have no
epilogue, which no plan of the zoo is today, and is covered here at kernel level. The ResNet-50
case serves one image per batch so that both runs give every convolution the same shape.
"""

import json

import numpy as np
import pytest
import torch

from gale import ops
from gale._native import native
from gale.config import GaleConfig
from gale.engine import Engine
from gale.models import get_model, init_params
from test_topk_cpu import case_rows, softmax_rows, topk_indices

pytestmark = pytest.mark.gpu

C = native()
K = C.kafka
SLOT = C.FLOAT_TEXT_SLOT
FILL, STATUS_FILL = 0xEE, 0x5A5A5A5A
PAD = 8  # entries behind the last one a launch may write


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev_int(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def out_buffers(entries):
    """Host-mapped text and index buffers of entries + PAD entries, prefilled."""
    text, idx = C.MappedBuffer((entries + PAD) * SLOT), C.MappedBuffer((entries + PAD) * 4)
    tv, iv = text.numpy(), idx.numpy()
    tv[:] = FILL
    iv[:] = FILL
    return text, tv.reshape(-1, SLOT), idx, iv


def check_entries(x, k, rows, tv, iv):
    """Entries [0, rows * k) are the rule's selection from x[:rows] and the host's text of the
    selected values; every byte behind them still holds the prefill."""
    n = rows * k
    want = topk_indices(x[:rows], k) if rows else np.zeros((0, k), np.int32)
    got = iv[:4 * n].view(np.int32).reshape(rows, k)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    for r in range(rows):
        for j in range(k):
            slot = tv[r * k + j]
            text = bytes(slot[:slot[SLOT - 1]]).decode()
            assert text == C.format_float_java(float(x[r, want[r, j]])), (r, j, text)
    assert (tv[n:] == FILL).all() and (iv[4 * n:] == FILL).all()


SHAPES = sorted({(c, k) for c in (1, 10, 63, 64, 65, 1000) for k in (1, min(5, c), min(64, c))})


def test_shapes_are_the_intended_ones():
    assert len(SHAPES) == 16 and (1, 1) in SHAPES and (1000, 64) in SHAPES and (65, 64) in SHAPES


@pytest.mark.parametrize("classes,k", SHAPES)
def test_topk_kernel_matches_the_rule(classes, k):
    """rows 1, 5 and 9 (none a multiple of the 4 rows per workgroup), as windows that between
    them cover every adversarial and softmax row."""
    x = case_rows(classes, k)
    xd = torch.from_numpy(x).cuda()
    assert len(x) == 12
    for rows, starts in ((1, range(12)), (5, (0, 5, 7)), (9, (0, 3))):
        for s0 in starts:
            text, tv, idx, iv = out_buffers(rows * k)
            C.topk_java(rows, classes, k, xd[s0:].data_ptr(), text.ptr, idx.ptr, stream())
            torch.cuda.synchronize()
            check_entries(x[s0:], k, rows, tv, iv)


def test_topk_largest_row():
    """classes = 4096, k = 64: the limits of the launchers (64 KiB of LDS per workgroup, 64
    strided entries per lane, a winner in every lane)."""
    x = softmax_rows(5, 4096, seed=3)
    x[1, 100:200] = x[1, 7]  # a hundred equal values among them
    xd = torch.from_numpy(x).cuda()
    text, tv, idx, iv = out_buffers(5 * 64)
    C.topk_java(5, 4096, 64, xd.data_ptr(), text.ptr, idx.ptr, stream())
    torch.cuda.synchronize()
    check_entries(x, 64, 5, tv, iv)


def test_topk_rows_end_at_the_allocation():
    """Nothing behind x[rows * classes] takes part: the values there are NaN, which would win
    every round of the last row (classes = 65: its last lane-strided pass is one entry wide)."""
    classes, k, rows = 65, 5, 5
    x = softmax_rows(rows, classes, seed=9)
    big = torch.full(((rows + 3) * classes,), float("nan"), device="cuda")
    big[:rows * classes] = torch.from_numpy(x).reshape(-1).cuda()
    text, tv, idx, iv = out_buffers(rows * k)
    C.topk_java(rows, classes, k, big.data_ptr(), text.ptr, idx.ptr, stream())
    torch.cuda.synchronize()
    check_entries(x, k, rows, tv, iv)


def test_ops_topk_wrapper():
    x = case_rows(63, 5)
    texts, indices = ops.topk(torch.from_numpy(x).cuda(), 5)
    assert texts.shape == (12, 5, SLOT) and texts.dtype == torch.uint8
    assert indices.shape == (12, 5) and indices.dtype == torch.int32
    tv = np.concatenate([texts.cpu().numpy().reshape(-1, SLOT),
                         np.full((PAD, SLOT), FILL, np.uint8)])
    iv = np.concatenate([indices.cpu().numpy().reshape(-1).view(np.uint8),
                         np.full(4 * PAD, FILL, np.uint8)])
    check_entries(x, 5, 12, tv, iv)
    with pytest.raises(RuntimeError):
        ops.topk(torch.from_numpy(x), 5)  # a CPU tensor: no fallback
    with pytest.raises(ValueError):
        ops.topk(torch.from_numpy(x).cuda(), 64)


@pytest.mark.parametrize("classes,k", [(10, 0), (10, -1), (10, 11), (100, 65), (4097, 5)])
def test_topk_refusals_launch_nothing(classes, k):
    xd = torch.zeros(2 * classes, device="cuda")
    text, tv, idx, iv = out_buffers(2 * 64)
    one = dev_int(2)
    status = torch.ones(8, dtype=torch.int32, device="cuda")
    so = C.MappedBuffer(32)
    so.numpy()[:] = FILL
    with pytest.raises(RuntimeError):
        C.topk_java(2, classes, k, xd.data_ptr(), text.ptr, idx.ptr, stream())
    with pytest.raises(RuntimeError):
        C.topk_java_dev(2, one.data_ptr(), classes, k, xd.data_ptr(), text.ptr, idx.ptr, stream())
    with pytest.raises(RuntimeError):
        C.topk_java_step(2, one.data_ptr(), classes, k, xd.data_ptr(), text.ptr, idx.ptr,
                         one.data_ptr(), status.data_ptr(), so.ptr, stream())
    torch.cuda.synchronize()
    assert (tv == FILL).all() and (iv == FILL).all() and (so.numpy() == FILL).all()
    assert (status.cpu().numpy() == 1).all()


# ---- the step's forms --------------------------------------------------------------------------

@pytest.mark.parametrize("count", [0, 1, 5, 9, 1000])
@pytest.mark.parametrize("classes,k", [(10, 3), (1000, 5)])
def test_topk_java_dev(classes, k, count):
    """max_rows 9 with the count on the device: rows past it keep the prefill (a count past
    max_rows serves max_rows)."""
    x = case_rows(classes, k)[:9]
    xd = torch.from_numpy(x).cuda()
    text, tv, idx, iv = out_buffers(9 * k)
    d_rows = dev_int(count)
    C.topk_java_dev(9, d_rows.data_ptr(), classes, k, xd.data_ptr(), text.ptr, idx.ptr, stream())
    torch.cuda.synchronize()
    check_entries(x, k, min(count, 9), tv, iv)


def handoff_arrays(n=640):
    pattern = (np.arange(n, dtype=np.int32) * 7) % 5 + 1  # non-zero everywhere
    status = torch.from_numpy(pattern.copy()).cuda()
    mb = C.MappedBuffer(4 * n)
    so = mb.numpy().view(np.int32)
    so[:] = STATUS_FILL
    return pattern, status, mb, so


def check_handoff(pattern, status, so, nrec):
    """status_out[i] = status[i], status[i] = 0 for i < nrec; both unchanged from nrec on."""
    st = status.cpu().numpy()
    assert (so[:nrec] == pattern[:nrec]).all() and (st[:nrec] == 0).all()
    assert (so[nrec:] == STATUS_FILL).all() and (st[nrec:] == pattern[nrec:]).all()


@pytest.mark.parametrize("count", [0, 5, 9])
@pytest.mark.parametrize("classes,k", [(10, 3), (1000, 5)])
def test_topk_java_step(classes, k, count):
    """Verdict counts below and above the row count, up to the launch's 64 threads per row of
    max_rows = 9 (576: the third workgroup's threads take part)."""
    x = case_rows(classes, k)[:9]
    xd = torch.from_numpy(x).cuda()
    d_rows = dev_int(count)
    for nrec in (0, 3, 9, 300, 576):
        pattern, status, so_mb, so = handoff_arrays()
        text, tv, idx, iv = out_buffers(9 * k)
        d_nrec = dev_int(nrec)
        C.topk_java_step(9, d_rows.data_ptr(), classes, k, xd.data_ptr(), text.ptr, idx.ptr,
                         d_nrec.data_ptr(), status.data_ptr(), so_mb.ptr, stream())
        torch.cuda.synchronize()
        check_entries(x, k, count, tv, iv)
        check_handoff(pattern, status, so, nrec)


def test_topk_java_step_needs_the_verdict_count():
    x = torch.from_numpy(softmax_rows(3, 10)).cuda()
    pattern, status, so_mb, so = handoff_arrays(64)
    text, tv, idx, iv = out_buffers(9)
    d_rows = dev_int(3)
    with pytest.raises(RuntimeError):
        C.topk_java_step(3, d_rows.data_ptr(), 10, 3, x.data_ptr(), text.ptr, idx.ptr, 0,
                         status.data_ptr(), so_mb.ptr, stream())
    with pytest.raises(RuntimeError):
        C.topk_java_dev(3, 0, 10, 3, x.data_ptr(), text.ptr, idx.ptr, stream())
    torch.cuda.synchronize()
    assert (tv == FILL).all() and (iv == FILL).all()
    check_handoff(pattern, status, so, 0)


# ---- the engine --------------------------------------------------------------------------------

def serve(model, recs, params, max_batch, **kw):
    broker = K.Broker()
    broker.start()
    try:
        broker.create_topic("in", 1)
        broker.create_topic("out", 1)
        for key, rec in recs:
            broker.append("in", 0, [rec], [key])
        cfg = GaleConfig(topology_name="g", input_topic="in", output_topic="out", model=model,
                         bootstrap=f"127.0.0.1:{broker.port}", start_offset="earliest",
                         max_batch=max_batch, max_wait_us=500, output_key="input",
                         on_error="error-json", **kw)
        eng = Engine(cfg.validate(), devices=[0], max_records=len(recs), params=params)
        eng.start()
        assert eng.wait(120), eng.stats()
        eng.stop()
        out = broker.read("out", 0)
    finally:
        broker.stop()
    assert len(out) == len(recs)  # one output record per input record
    return eng.stats(), {r["key"]: r["value"] for r in out}


def row_texts(value):
    """The full-row record's values as the strings it holds: [images][classes]."""
    doc = json.loads(value, parse_float=str)
    return doc["predictions"]


def check_against_full(full, got, k, classes):
    """Each top-k record against the full-row record of the same key."""
    assert set(got) == set(full)
    images = 0
    for key, value in full.items():
        if key == b"bad":  # still an error record (which stage judges it depends on the site)
            assert b"error" in got[key] and b"error" in value and b"classes" not in got[key]
            continue
        rows = row_texts(value)
        x = np.array([[float(t) for t in row] for row in rows], dtype=np.float32)
        assert x.shape[1] == classes
        want = topk_indices(x, k)
        doc = json.loads(got[key], parse_float=str)
        assert list(doc) == ["predictions"] and len(doc["predictions"]) == len(rows), key
        for item, row, sel in zip(doc["predictions"], rows, want):
            assert list(item) == ["classes", "scores"]
            assert item["classes"] == sel.tolist(), (key, item, sel)
            assert item["scores"] == [row[c] for c in sel], (key, item)
        images += len(rows)
    return images


R20_COUNTS = [1, 2, 4, 1, 3, 20, 2, 1, 4, 3, 1, 2]  # one record over max_batch = 16: fragments
SITES = {
    "table-step": dict(),                                # launch_table + topk_java
    "no-ingest-parse": dict(ingest_parse=False),         # direct step: epilogue + topk_java_dev
    "step-launch-graph": dict(step_launch="graph"),      # the same sequence, captured
    "no-graph-step": dict(graph_step=False),             # op by op: topk_java
    "no-gpu-encode": dict(gpu_encode=False),             # the rows come back, the host selects
}


@pytest.fixture(scope="module")
def r20():
    net = get_model("resnet20")
    params = init_params(net, seed=0, calib_batch=16)
    rng = np.random.default_rng(41)
    recs = []
    for i, n in enumerate(R20_COUNTS):
        x = rng.random((n,) + tuple(net.input_shape), dtype=np.float32)
        recs.append((f"r{i}".encode(), C.encode_instances(x)))
    recs.insert(4, (b"bad", b'{"instances": [[[[0.5, x]]]]}'))
    st, full = serve("resnet20", recs, params, 16)
    assert st["errors"] == 1 and st["split_records"] == 1 and st["table_batches"] > 0, st
    return dict(params=params, recs=recs, full=full)


@pytest.mark.parametrize("site", list(SITES))
def test_engine_resnet20_topk(r20, site):
    st, got = serve("resnet20", r20["recs"], r20["params"], 16, top_k=3, **SITES[site])
    assert st["errors"] == 1 and st["split_records"] == 1, st
    assert check_against_full(r20["full"], got, 3, 10) == sum(R20_COUNTS) == st["images_out"]
    assert (st["table_batches"] > 0) == (site == "table-step"), st
    assert (st["graph_step_batches"] > 0) == (site not in ("no-graph-step",)), st


def test_engine_resnet20_topk_json_string(r20):
    """--value-format json-string escapes the elements' quotes, in joined fragments too."""
    _, got = serve("resnet20", r20["recs"], r20["params"], 16, top_k=3,
                   value_format="json-string")
    inner = {}
    for k, v in got.items():
        assert b'"classes"' not in v.replace(b'\\"', b"")
        inner[k] = json.loads(v).encode()
    good = {k: v for k, v in r20["full"].items() if k != b"bad"}
    del inner[b"bad"]
    assert check_against_full(good, inner, 3, 10) == sum(R20_COUNTS)


def test_engine_resnet50_topk():
    net = get_model("resnet50")
    params = init_params(net, seed=3, calib_batch=4)
    rng = np.random.default_rng(4)
    recs = [(f"i{i}".encode(),
             C.encode_instances(rng.random((1,) + tuple(net.input_shape), dtype=np.float32)))
            for i in range(4)]
    kw = dict(gpu_ingest=True, text_pack=False)
    _, full = serve("resnet50", recs, params, 1, **kw)
    st, got = serve("resnet50", recs, params, 1, top_k=5, **kw)
    assert st["errors"] == 0, st
    assert check_against_full(full, got, 5, 1000) == 4
