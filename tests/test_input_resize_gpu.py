"""Input resize on the GPU: the resize_crop kernel (csrc/kernels/resize_crop.hip) in its two
forms, bit-exact against the numpy oracle ``InputResize.apply`` (tests/test_input_resize_cpu.py
checks the oracle itself against exact rational arithmetic), its bounds, its refusals, the
``gale.ops.resize_crop`` wrapper, and the engine with --input-size / --input-resize on every site
that emits the step.

Kernel cases place dst inside a larger device tensor filled with a sentinel bit pattern and src
at the very end of its tensor, behind NaNs; every "untouched" claim is checked against the
sentinel.

Engine cases compare run A - source-size records of raw pixels with the resize and preprocessing
options - with run B: the same images as ``apply(prep(x))`` written as float text, served with no
options and without the ingest parse. The outputs must be byte-equal per key. ResNet-50's plan
is not a whole-network kernel; its case serves one image per batch so that both runs give every
convolution the same shape."""

import numpy as np
import pytest
import torch

from gale import ops
from gale._native import native
from gale.config import GaleConfig
from gale.engine import Engine
from gale.models import get_model, init_params
from gale.models.preprocess import InputPrep, InputResize
from test_input_resize_cpu import (CIFAR_MEAN_S, CIFAR_STD_S, SHAPES, float_record,
                                   pixel_record, random_images, u32)

pytestmark = pytest.mark.gpu

C = native()
K = C.kafka
SENTINEL = np.uint32(0xEEEEEEEE)
PAD = 64  # sentinel floats before and after dst

# + a crop whose output row is 16 bytes, and an output row of 21 floats (per-float stores)
KERNEL_SHAPES = SHAPES + [(9, 6, 9, 6, 8, 4, 1), (7, 5, 9, 11, 6, 7, 3)]


def stream():
    return torch.cuda.current_stream().cuda_stream


def sentinel_tensor(n):
    return torch.full((n,), int(SENTINEL.view(np.int32)), dtype=torch.int32, device="cuda")


def place_src(x):
    """x at the very end of a device tensor, NaNs before it."""
    buf = torch.full((37 + x.size,), float("nan"), dtype=torch.float32, device="cuda")
    buf[37:] = torch.from_numpy(x.reshape(-1)).cuda()
    return buf, buf[37:].data_ptr()


def tables_for(dims):
    HS, WS, HR, WR, H, W, _ = dims
    return ops.resize_tables(HS, WS, HR, WR, H, W, "cuda")


def run_kernel(dims, x, n_launch, count=None, lead=PAD, tables=None):
    """Launch over n_launch images of x (count: the _dev form's device word); returns the whole
    dst tensor's words, the offset of dst in it, and the per-image float count."""
    HS, WS, HR, WR, H, W, Ch = dims
    tables = tables or tables_for(dims)
    per = H * W * Ch
    big = sentinel_tensor(lead + x.shape[0] * per + PAD)
    src_buf, src = place_src(x)
    dst = big[lead:].data_ptr()
    ptrs = [t.data_ptr() for t in tables]
    if count is None:
        C.resize_crop(n_launch, HS, WS, H, W, Ch, ptrs, src, dst, stream())
    else:
        d = torch.tensor([count], dtype=torch.int32, device="cuda")
        C.resize_crop_dev(n_launch, d.data_ptr(), HS, WS, H, W, Ch, ptrs, src, dst, stream())
    torch.cuda.synchronize()
    return big.cpu().numpy().view(np.uint32), lead, per


def check(words, lead, per, want, written):
    """Images [0, written) hold the oracle's bits; every other word holds the sentinel."""
    body = words[lead:lead + written * per]
    assert np.array_equal(body, u32(want[:written]).reshape(-1))
    assert (words[:lead] == SENTINEL).all()
    assert (words[lead + written * per:] == SENTINEL).all()


@pytest.fixture(scope="module")
def cases():
    """Per shape: 5 random images (both signs, several binades) and the oracle's output."""
    out = {}
    for dims in KERNEL_SHAPES:
        HS, WS, HR, WR, H, W, Ch = dims
        x = random_images(np.random.default_rng(HS * 1000 + WS), 5, HS, WS, Ch)
        out[dims] = (x, InputResize(HS, WS, HR, WR, H, W).apply(x))
    return out


@pytest.mark.parametrize("dims", KERNEL_SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_kernel_is_bit_exact_in_both_forms_and_stays_in_bounds(cases, dims):
    x, want = cases[dims]
    tables = tables_for(dims)
    for n in (1, 3, 5):
        check(*run_kernel(dims, x[:n], n, tables=tables), want, n)
        check(*run_kernel(dims, x[:n], n, count=n, tables=tables), want, n)


def test_kernel_dev_form_stops_at_the_device_count(cases):
    for dims in (KERNEL_SHAPES[1], KERNEL_SHAPES[4]):  # 16-byte stores / per-float stores
        x, want = cases[dims]
        for count in (0, 2, 5):
            check(*run_kernel(dims, x, 5, count=count), want, count)
        # a count above the launch size: the launch size holds
        check(*run_kernel(dims, x[:3], 3, count=9), want, 3)


def test_kernel_unaligned_dst_takes_the_per_float_path(cases):
    """A row of 96 floats with dst 4 bytes off a 16-byte boundary: same bits, same bounds."""
    dims = KERNEL_SHAPES[1]
    x, want = cases[dims]
    words, lead, per = run_kernel(dims, x[:3], 3, lead=PAD + 1)
    check(words, lead, per, want, 3)


def test_kernel_crop_copies_nan_and_max(cases):
    dims = (40, 36, 40, 36, 32, 32, 3)
    x = random_images(np.random.default_rng(8), 2, 40, 36, 3)
    x[0, 4, 2, 0], x[0, 4, 3, 0], x[0, 3, 2, 0] = 3.4e38, -3.4e38, np.nan
    x[1, 35, 33, 2], x[1, 36, 33, 2], x[1, 35, 34, 2] = np.nan, 3.4e38, -3.4e38
    words, lead, per = run_kernel(dims, x, 2)
    check(words, lead, per, np.ascontiguousarray(x[:, 4:36, 2:34]), 2)


def test_kernel_refusals_launch_nothing(cases):
    dims = KERNEL_SHAPES[1]
    HS, WS, HR, WR, H, W, Ch = dims
    x, _ = cases[dims]
    tables = tables_for(dims)
    ptrs = [t.data_ptr() for t in tables]
    big = sentinel_tensor(PAD + 5 * H * W * Ch + PAD)
    src_buf, src = place_src(x)
    dst = big[PAD:].data_ptr()
    one = torch.tensor([1], dtype=torch.int32, device="cuda")
    bad = [
        dict(src=0), dict(dst=0), dict(images=-1), dict(images=65536),
        dict(HS=0), dict(HS=4097), dict(WS=0), dict(WS=4097), dict(H=0), dict(H=4097),
        dict(W=0), dict(W=4097), dict(Ch=0), dict(Ch=-3),
    ] + [dict(null_table=i) for i in range(6)]
    for b in bad:
        a = dict(images=1, HS=HS, WS=WS, H=H, W=W, Ch=Ch, src=src, dst=dst)
        a.update({k: v for k, v in b.items() if k != "null_table"})
        p = list(ptrs)
        if "null_table" in b:
            p[b["null_table"]] = 0
        with pytest.raises(RuntimeError):
            C.resize_crop(a["images"], a["HS"], a["WS"], a["H"], a["W"], a["Ch"], p, a["src"],
                          a["dst"], stream())
        with pytest.raises(RuntimeError):
            C.resize_crop_dev(a["images"], one.data_ptr(), a["HS"], a["WS"], a["H"], a["W"],
                              a["Ch"], p, a["src"], a["dst"], stream())
    with pytest.raises(RuntimeError):  # the _dev form without its device word
        C.resize_crop_dev(1, 0, HS, WS, H, W, Ch, ptrs, src, dst, stream())
    with pytest.raises(RuntimeError):  # an image of 2^31 floats
        C.resize_crop(1, 4096, 4096, H, W, 128, ptrs, src, dst, stream())
    C.resize_crop(0, HS, WS, H, W, Ch, ptrs, src, dst, stream())  # no images: no launch, no error
    torch.cuda.synchronize()
    assert (big.cpu().numpy().view(np.uint32) == SENTINEL).all()


def test_ops_resize_crop_wrapper(cases):
    for dims in (KERNEL_SHAPES[0], KERNEL_SHAPES[4]):
        HS, WS, HR, WR, H, W, Ch = dims
        x, want = cases[dims]
        y = ops.resize_crop(torch.from_numpy(x).cuda(), (HR, WR), (H, W))
        assert y.shape == (5, H, W, Ch) and y.dtype == torch.float32 and y.is_cuda
        assert np.array_equal(u32(y.cpu().numpy()), u32(want))
        y2 = ops.resize_crop(torch.from_numpy(x).cuda(), (HR, WR), (H, W),
                             tables=tables_for(dims))
        assert torch.equal(y, y2)
    x, _ = cases[KERNEL_SHAPES[0]]
    with pytest.raises(RuntimeError):
        ops.resize_crop(torch.from_numpy(x), (32, 33), (32, 32))  # a CPU tensor: no fallback
    with pytest.raises(ValueError):
        ops.resize_crop(torch.from_numpy(x).cuda(), (31, 33), (32, 32))  # no padding
    with pytest.raises(ValueError):
        ops.resize_crop(torch.from_numpy(x).cuda(), (32, 33), (32, 32),
                        tables=tables_for(KERNEL_SHAPES[2]))
    assert ops.resize_crop(torch.from_numpy(x[:0]).cuda(), (32, 33), (32, 32)).shape == \
        (0, 32, 32, 3)


# ---- the engine --------------------------------------------------------------------------------

BAD = b"this is not an InstObj"


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


R20_COUNTS = [1, 2, 4, 1, 3, 20, 2, 1]  # one record over max_batch = 16: served as fragments
R20_OPTS = dict(input_size="40,36", input_resize="34,33", input_scale=1 / 255,
                input_mean=CIFAR_MEAN_S, input_std=CIFAR_STD_S)
SITES = {
    "default": dict(),                               # the direct step: resize_crop_dev
    "step-launch-graph": dict(step_launch="graph"),  # the same sequence, captured
    "no-graph-step": dict(graph_step=False),         # op by op: resize_crop
    "no-gpu-encode": dict(gpu_encode=False),         # the captured step with copies
}


@pytest.fixture(scope="module")
def r20():
    net = get_model("resnet20")
    params = init_params(net, seed=0, calib_batch=16)
    rng = np.random.default_rng(43)
    xs = {f"r{i}".encode(): rng.integers(0, 256, (n, 40, 36, 3), dtype=np.uint8)
          for i, n in enumerate(R20_COUNTS)}
    prep = InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S)
    rs = InputResize(40, 36, 34, 33, 32, 32)
    plain = [(k, float_record(rs.apply(prep.apply(x.astype(np.float32))))) for k, x in xs.items()]
    plain.insert(3, (b"bad", BAD))
    served = {}

    def run_b(site):
        """Run B on the same site: model-size float text, no options, no ingest parse."""
        if site not in served:
            st, out = serve("resnet20", plain, params, 16, ingest_parse=False, **SITES[site])
            assert st["errors"] == 1 and st["resized_images"] == 0, st
            served[site] = out
        return served[site]

    def records(fmt, layout):
        recs = [(k, pixel_record(x, fmt, layout)) for k, x in xs.items()]
        recs.insert(3, (b"bad", BAD))
        return recs

    return dict(params=params, run_b=run_b, records=records)


def check_r20(r20, site, fmt, layout):
    st, got = serve("resnet20", r20["records"](fmt, layout), r20["params"], 16, **R20_OPTS,
                    input_format=fmt, input_layout=layout, **SITES[site])
    want = r20["run_b"](site)
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], k
    assert b"error" in got[b"bad"]
    assert st["errors"] == 1 and st["split_records"] == 1, st
    assert st["images_out"] == sum(R20_COUNTS) == st["resized_images"], st
    assert st["table_batches"] == 0 and st["ingest_parsed_records"] == 0, st
    assert (st["graph_step_batches"] > 0) == (site != "no-graph-step"), st


@pytest.mark.parametrize("site", list(SITES))
def test_engine_resnet20_resize_on_every_site(r20, site):
    check_r20(r20, site, "json", "nhwc")


def test_engine_resnet20_resize_b64_input(r20):
    check_r20(r20, "default", "b64", "nhwc")


def test_engine_resnet20_resize_nchw_json_input(r20):
    check_r20(r20, "default", "json", "nchw")


def test_engine_lenet5_b64_resize():
    net = get_model("lenet5")
    params = init_params(net, seed=1, calib_batch=16)
    rng = np.random.default_rng(6)
    counts = [1, 3, 2, 18, 1]
    xs = {f"m{i}".encode(): rng.integers(0, 256, (n, 30, 33, 1), dtype=np.uint8)
          for i, n in enumerate(counts)}
    prep = InputPrep.build(1, 1 / 255, "0.1307", "0.3081")
    rs = InputResize(30, 33, 29, 31, 28, 28)
    plain = [(k, float_record(rs.apply(prep.apply(x.astype(np.float32))))) for k, x in xs.items()]
    _, want = serve("lenet5", plain, params, 16, ingest_parse=False)
    st, got = serve("lenet5", [(k, pixel_record(x, "b64", "nhwc")) for k, x in xs.items()], params,
                    16, input_format="b64", input_size="30,33", input_resize="29,31",
                    input_scale=1 / 255, input_mean="0.1307", input_std="0.3081")
    assert got == want
    assert st["errors"] == 0 and st["resized_images"] == sum(counts) == st["images_out"], st
    assert st["table_batches"] == 0 and st["graph_step_batches"] > 0, st


def test_engine_resnet50_b64_centre_crop():
    net = get_model("resnet50")
    params = init_params(net, seed=3, calib_batch=4)
    rng = np.random.default_rng(5)
    xs = {f"i{i}".encode(): rng.integers(0, 256, (1, 256, 256, 3), dtype=np.uint8)
          for i in range(3)}
    kw = dict(input_format="b64", text_pack=False)
    _, want = serve("resnet50", [(k, pixel_record(np.ascontiguousarray(x[:, 16:240, 16:240]),
                                                  "b64", "nhwc")) for k, x in xs.items()],
                    params, 1, **kw)
    st, got = serve("resnet50", [(k, pixel_record(x, "b64", "nhwc")) for k, x in xs.items()],
                    params, 1, input_size="256,256", input_resize="256,256", **kw)
    assert got == want
    assert st["errors"] == 0 and st["resized_images"] == 3 == st["images_out"], st
