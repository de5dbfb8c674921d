"""Antialiased input resize on the GPU: the resize_crop_aa kernel
(csrc/kernels/resize_crop_aa.hip) in its two forms, bit-exact against the numpy oracle
``InputResize(..., antialias=True).apply`` (tests/test_input_antialias_cpu.py checks the oracle
itself against exact rational arithmetic), its bounds, its refusals, the
``gale.ops.resize_crop_aa`` wrapper, and the engine with --input-antialias on every site that
emits the step.

Kernel cases place dst inside a larger device tensor filled with a sentinel bit pattern and src
at the very end of its tensor, behind NaNs; every "untouched" claim is checked against the
sentinel.

Engine cases compare run A - source-size records of raw pixels with the resize, antialias and
preprocessing options - with run B: the same images as ``apply(prep(x))`` written as float text,
served with no options and without the ingest parse. The outputs must be byte-equal per key.
ResNet-50's plan is not a whole-network kernel; its case serves one image per batch so that both
runs give every convolution the same shape."""

import numpy as np
import pytest
import torch

from gale import ops
from gale._native import native
from gale.config import GaleConfig
from gale.engine import Engine
from gale.models import get_model, init_params
from gale.models.preprocess import InputPrep, InputResize
from test_input_antialias_cpu import (CIFAR_MEAN_S, CIFAR_STD_S, KERNEL_SHAPES, float_record,
                                      pixel_record, random_images, u32)

pytestmark = pytest.mark.gpu

C = native()
K = C.kafka
SENTINEL = np.uint32(0xEEEEEEEE)
PAD = 64  # sentinel floats before and after dst

VEC_DIMS = KERNEL_SHAPES[1]    # rows of 96 floats: 16-byte stores
FLOAT_DIMS = KERNEL_SHAPES[6]  # rows of 21 floats: per-float stores
TILE_DIMS = KERNEL_SHAPES[8]   # two spans per row, four bands


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
    return ops.resize_aa_tables(*dims[:6], "cuda")


def run_kernel(dims, x, n_launch, count=None, lead=PAD, tables=None):
    """Launch over n_launch images of x (count: the _dev form's device word); returns the whole
    dst tensor's words, the offset of dst in it, and the per-image float count."""
    HS, WS, HR, WR, H, W, Ch = dims
    tables = tables or tables_for(dims)
    per = H * W * Ch
    big = sentinel_tensor(lead + x.shape[0] * per + PAD)
    src_buf, src = place_src(x)
    dst = big[lead:].data_ptr()
    if count is None:
        C.resize_crop_aa(n_launch, list(dims), tables.ptrs(), list(tables.launch), src, dst,
                         stream())
    else:
        d = torch.tensor([count], dtype=torch.int32, device="cuda")
        C.resize_crop_aa_dev(n_launch, d.data_ptr(), list(dims), tables.ptrs(),
                             list(tables.launch), src, dst, stream())
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
        out[dims] = (x, InputResize(HS, WS, HR, WR, H, W, antialias=True).apply(x))
    return out


def test_the_shapes_cross_the_tile_and_the_band_fallback():
    """What the shape table claims about the kernel's tile (256 floats of a row by `band` rows)."""
    t = tables_for(TILE_DIMS)
    assert TILE_DIMS[5] * TILE_DIMS[6] > 256 and TILE_DIMS[4] > t.launch[2] == 8
    ty, tx, band, rows = tables_for(KERNEL_SHAPES[7]).launch
    assert (ty, tx) == (16, 16) and band == 4 and rows + tx <= 64  # 8x: a lower band for the LDS
    assert tables_for(KERNEL_SHAPES[5]).launch[:2] == (1, 1)      # crop: single taps


@pytest.mark.parametrize("dims", KERNEL_SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_kernel_is_bit_exact_in_both_forms_and_stays_in_bounds(cases, dims):
    x, want = cases[dims]
    tables = tables_for(dims)
    for n in (1, 3, 5):
        check(*run_kernel(dims, x[:n], n, tables=tables), want, n)
        check(*run_kernel(dims, x[:n], n, count=n, tables=tables), want, n)


def test_kernel_dev_form_stops_at_the_device_count(cases):
    for dims in (VEC_DIMS, FLOAT_DIMS):
        x, want = cases[dims]
        for count in (0, 2, 5):
            check(*run_kernel(dims, x, 5, count=count), want, count)
        # a count above the launch size: the launch size holds
        check(*run_kernel(dims, x[:3], 3, count=9), want, 3)


@pytest.mark.parametrize("dims", [VEC_DIMS, TILE_DIMS], ids=lambda d: "x".join(map(str, d)))
def test_kernel_unaligned_dst_takes_the_per_float_path(cases, dims):
    """Rows of 96 / 288 floats with dst 4 bytes off a 16-byte boundary: same bits, same bounds."""
    x, want = cases[dims]
    words, lead, per = run_kernel(dims, x[:3], 3, lead=PAD + 1)
    check(words, lead, per, want, 3)


def test_kernel_crop_copies_nan_max_inf_and_negative_zero():
    dims = (40, 36, 40, 36, 32, 32, 3)
    x = random_images(np.random.default_rng(8), 2, 40, 36, 3)
    x[0, 4, 2, 0], x[0, 4, 3, 0], x[0, 3, 2, 0] = 3.4e38, -3.4e38, np.nan
    x[1, 35, 33, 2], x[1, 36, 33, 2], x[1, 35, 34, 2] = np.nan, 3.4e38, -3.4e38
    x[0, 9, 9, 1], x[0, 9, 10, 1], x[1, 9, 9, 1] = -0.0, np.inf, -np.inf
    x[1, 20, 20, 0] = np.array([0x7fa12345], np.uint32).view(np.float32)[0]  # a NaN payload
    for lead in (PAD, PAD + 1):  # both store paths
        words, lead, per = run_kernel(dims, x, 2, lead=lead)
        check(words, lead, per, np.ascontiguousarray(x[:, 4:36, 2:34]), 2)


def test_kernel_refusals_launch_nothing(cases):
    dims = VEC_DIMS
    HS, WS, HR, WR, H, W, Ch = dims
    x, _ = cases[dims]
    tables = tables_for(dims)
    ty, tx, band, rows = tables.launch
    big = sentinel_tensor(PAD + 5 * H * W * Ch + PAD)
    src_buf, src = place_src(x)
    dst = big[PAD:].data_ptr()
    one = torch.tensor([1], dtype=torch.int32, device="cuda")
    bad = [
        dict(src=0), dict(dst=0), dict(images=-1), dict(images=65536),
        dict(HS=0), dict(HS=4097), dict(WS=0), dict(WS=4097), dict(H=0), dict(H=4097),
        dict(W=0), dict(W=4097), dict(Ch=0), dict(Ch=-3),
        dict(HR=0), dict(HR=4097), dict(WR=0), dict(WR=4097), dict(HR=H - 1), dict(WR=W - 1),
        # a plan over the 8x limit, per axis (64 -> 7 rows, 48 -> 5 columns)
        dict(HR=7, H=7), dict(WR=5, W=5), dict(HS=8 * HR + 1), dict(WS=8 * WR + 1),
        # launch figures outside the kernel's tile
        dict(ty=0), dict(ty=18), dict(tx=0), dict(tx=18), dict(band=0), dict(band=9),
        dict(rows=0), dict(rows=65 - tx),
    ] + [dict(null_table=i) for i in range(6)]
    for b in bad:
        a = dict(images=1, HS=HS, WS=WS, HR=HR, WR=WR, H=H, W=W, Ch=Ch, src=src, dst=dst, ty=ty,
                 tx=tx, band=band, rows=rows)
        a.update({k: v for k, v in b.items() if k != "null_table"})
        p = tables.ptrs()
        if "null_table" in b:
            p[b["null_table"]] = 0
        d = [a[k] for k in ("HS", "WS", "HR", "WR", "H", "W", "Ch")]
        fig = [a[k] for k in ("ty", "tx", "band", "rows")]
        with pytest.raises(RuntimeError):
            C.resize_crop_aa(a["images"], d, p, fig, a["src"], a["dst"], stream())
        with pytest.raises(RuntimeError):
            C.resize_crop_aa_dev(a["images"], one.data_ptr(), d, p, fig, a["src"], a["dst"],
                                 stream())
    fig = list(tables.launch)
    with pytest.raises(RuntimeError):  # the _dev form without its device word
        C.resize_crop_aa_dev(1, 0, list(dims), tables.ptrs(), fig, src, dst, stream())
    with pytest.raises(RuntimeError):  # an image of 2^31 floats
        C.resize_crop_aa(1, [4096, 4096, 4096, 4096, H, W, 128], tables.ptrs(), fig, src, dst,
                         stream())
    # no images: no launch, no error
    C.resize_crop_aa(0, list(dims), tables.ptrs(), fig, src, dst, stream())
    torch.cuda.synchronize()
    assert (big.cpu().numpy().view(np.uint32) == SENTINEL).all()


def test_ops_resize_crop_aa_wrapper(cases):
    for dims in (KERNEL_SHAPES[0], FLOAT_DIMS):
        HS, WS, HR, WR, H, W, Ch = dims
        x, want = cases[dims]
        y = ops.resize_crop_aa(torch.from_numpy(x).cuda(), (HR, WR), (H, W))
        assert y.shape == (5, H, W, Ch) and y.dtype == torch.float32 and y.is_cuda
        assert np.array_equal(u32(y.cpu().numpy()), u32(want))
        y2 = ops.resize_crop_aa(torch.from_numpy(x).cuda(), (HR, WR), (H, W),
                                tables=tables_for(dims))
        assert torch.equal(y, y2)
    x, _ = cases[KERNEL_SHAPES[0]]
    with pytest.raises(RuntimeError):
        ops.resize_crop_aa(torch.from_numpy(x), (34, 33), (32, 32))  # a CPU tensor: no fallback
    with pytest.raises(TypeError):
        ops.resize_crop_aa(torch.from_numpy(x).cuda().double(), (34, 33), (32, 32))
    with pytest.raises(ValueError):
        ops.resize_crop_aa(torch.from_numpy(x).cuda()[0], (34, 33), (32, 32))  # not [N,HS,WS,C]
    with pytest.raises(ValueError):
        ops.resize_crop_aa(torch.from_numpy(x).cuda(), (31, 33), (32, 32))  # no padding
    with pytest.raises(ValueError):
        ops.resize_crop_aa(torch.from_numpy(x).cuda(), (4, 33), (4, 32))  # 40 -> 4: over 8x
    with pytest.raises(ValueError):
        ops.resize_crop_aa(torch.from_numpy(x).cuda(), (34, 33), (32, 32),
                           tables=tables_for(KERNEL_SHAPES[1]))
    with pytest.raises(ValueError):  # the other option's tables
        ops.resize_crop_aa(torch.from_numpy(x).cuda(), (34, 33), (32, 32),
                           tables=ops.resize_tables(40, 36, 34, 33, 32, 32, "cuda"))
    assert ops.resize_crop_aa(torch.from_numpy(x[:0]).cuda(), (34, 33), (32, 32)).shape == \
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
R20_OPTS = dict(input_size="40,36", input_resize="34,33", input_antialias=True,
                input_scale=1 / 255, input_mean=CIFAR_MEAN_S, input_std=CIFAR_STD_S)
SITES = {
    "default": dict(),                               # the direct step: resize_crop_aa_dev
    "step-launch-graph": dict(step_launch="graph"),  # the same sequence, captured
    "no-graph-step": dict(graph_step=False),         # op by op: resize_crop_aa
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
    rs = InputResize(40, 36, 34, 33, 32, 32, antialias=True)
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
def test_engine_resnet20_antialias_on_every_site(r20, site):
    check_r20(r20, site, "json", "nhwc")


def test_engine_resnet20_antialias_b64_input(r20):
    check_r20(r20, "default", "b64", "nhwc")


def test_engine_resnet20_antialias_nchw_json_input(r20):
    check_r20(r20, "default", "json", "nchw")


def test_engine_lenet5_b64_antialias():
    net = get_model("lenet5")
    params = init_params(net, seed=1, calib_batch=16)
    rng = np.random.default_rng(6)
    counts = [1, 3, 2, 18, 1]
    xs = {f"m{i}".encode(): rng.integers(0, 256, (n, 30, 33, 1), dtype=np.uint8)
          for i, n in enumerate(counts)}
    prep = InputPrep.build(1, 1 / 255, "0.1307", "0.3081")
    rs = InputResize(30, 33, 29, 31, 28, 28, antialias=True)
    plain = [(k, float_record(rs.apply(prep.apply(x.astype(np.float32))))) for k, x in xs.items()]
    _, want = serve("lenet5", plain, params, 16, ingest_parse=False)
    st, got = serve("lenet5", [(k, pixel_record(x, "b64", "nhwc")) for k, x in xs.items()], params,
                    16, input_format="b64", input_size="30,33", input_resize="29,31",
                    input_antialias=True, input_scale=1 / 255, input_mean="0.1307",
                    input_std="0.3081")
    assert got == want
    assert st["errors"] == 0 and st["resized_images"] == sum(counts) == st["images_out"], st
    assert st["table_batches"] == 0 and st["graph_step_batches"] > 0, st


def test_engine_resnet50_b64_resize_256_centre_crop():
    """Resize(256) of 288 x 320 records (-> 256 x 284) and the 224 crop: a true downscale. Run B
    is float text of the oracle's output; b64 cannot carry it, so B is JSON."""
    net = get_model("resnet50")
    params = init_params(net, seed=3, calib_batch=4)
    rng = np.random.default_rng(5)
    xs = {f"i{i}".encode(): rng.integers(0, 256, (1, 288, 320, 3), dtype=np.uint8)
          for i in range(3)}
    rs = InputResize.build(224, 224, "288,320", "256", antialias=True)
    assert (rs.HR, rs.WR) == (256, 284)
    plain = [(k, float_record(rs.apply(x.astype(np.float32)))) for k, x in xs.items()]
    _, want = serve("resnet50", plain, params, 1, ingest_parse=False)
    st, got = serve("resnet50", [(k, pixel_record(x, "b64", "nhwc")) for k, x in xs.items()],
                    params, 1, input_format="b64", text_pack=False, input_size="288,320",
                    input_resize="256", input_antialias=True)
    assert got == want
    assert st["errors"] == 0 and st["resized_images"] == 3 == st["images_out"], st
    assert st["table_batches"] == 0, st
