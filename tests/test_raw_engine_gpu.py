"""Raw binary records (--input-format raw) through the GPU engine: the prediction text of the same
pixels sent as b64 records on every step launch site, behind the input resize and for LeNet-5."""

import numpy as np
import pytest
import torch

from gale.config import GaleConfig
from gale.data import encode_records_b64, encode_records_raw, encode_records_typed
from gale.models import get_model, init_params
from gale.models.preprocess import InputPrep
from gale.models.reference import calibrate_bn
from test_input_raw_cpu import CIFAR, pixel_sets, serve

pytestmark = pytest.mark.gpu

COUNTS = [1, 2, 1, 3, 40, 1]      # (40 > --max-batch 32: split and joined)
MNIST = dict(input_scale=1 / 255, input_mean="0.1307", input_std="0.3081")
SITES = {"direct": {}, "plain": dict(graph_step=False), "graph": dict(step_launch="graph"),
         "graph-noencode": dict(step_launch="graph", gpu_encode=False)}


def params_for(model, prep_kw):
    net = get_model(model)
    params = init_params(net, seed=0, calibrate=False)
    prep = InputPrep.build(net.input_shape[2], prep_kw["input_scale"], prep_kw["input_mean"],
                           prep_kw["input_std"])
    x = np.random.default_rng(77).integers(0, 256, (16,) + tuple(net.input_shape))
    calibrate_bn(net, params, torch.from_numpy(prep.apply(x.astype(np.float32))))
    return params


def run(recs, params, **kw):
    return serve(recs, params=params, dtype="bf16", max_batch=32, on_error="null", **kw)


def b64_records(sets, dtype):
    enc = encode_records_b64 if dtype == "u8" else lambda x, n: encode_records_typed(x, dtype, n)
    return [(k, enc(x, x.shape[0])[0]) for k, x in sets.items()]


def raw_records(sets, dtype):
    """The sets, then a record one byte short and (f16) one whose last element is +Inf."""
    recs = [(k, encode_records_raw(x, x.shape[0], dtype)[0]) for k, x in sets.items()]
    recs.append((b"short", recs[3][1][:-1]))
    if dtype == "f16":
        recs.append((b"inf", recs[3][1][:-2] + b"\x00\x7c"))
    return recs


def check(got, stats, want, dtype):
    assert got.pop(b"short") is None
    if dtype == "f16":
        assert got.pop(b"inf") is None
    assert got == want and all(v is not None for v in want.values())
    nbad = 2 if dtype == "f16" else 1
    assert stats["raw_records"] == len(COUNTS) + nbad - 1 and stats["b64_records"] == 0, stats
    assert stats["errors"] == nbad and stats["images_out"] == sum(COUNTS), stats
    assert stats["split_records"] == 1 and stats["ingested_records"] == 0, stats


@pytest.fixture(scope="module")
def r20():
    """The weights, the pixels and the b64 reference runs, computed once."""
    params = params_for("resnet20", CIFAR)
    sets = pixel_sets(get_model("resnet20").input_shape, COUNTS, 71)
    ref = {}
    for dtype in ("u8", "f16"):
        ref[dtype], st = run(b64_records(sets, dtype), params, input_format="b64",
                             input_dtype=dtype, **CIFAR)
        assert st["errors"] == 0 and st["raw_records"] == 0
    return dict(params=params, sets=sets, ref=ref)


@pytest.mark.parametrize("dtype", ["u8", "f16"])
@pytest.mark.parametrize("site", list(SITES))
def test_engine_every_step_site(r20, site, dtype):
    got, stats = run(raw_records(r20["sets"], dtype), r20["params"], input_format="raw",
                     input_dtype=dtype, **CIFAR, **SITES[site])
    check(got, stats, r20["ref"][dtype], dtype)
    assert (stats["graph_step_batches"] > 0) == (site != "plain"), stats


def test_engine_with_input_resize(r20):
    """--input-size 40,36: the conversion writes the resize's source tensor."""
    sets = pixel_sets((40, 36, 3), COUNTS, 72)
    kw = dict(CIFAR, input_size="40,36", input_antialias=False)
    want, _ = run(b64_records(sets, "u8"), r20["params"], input_format="b64", **kw)
    got, stats = run(raw_records(sets, "u8"), r20["params"], input_format="raw", **kw)
    check(got, stats, want, "u8")
    assert stats["resized_images"] == sum(COUNTS), stats


def test_lenet5():
    """gray is refused at configuration as with b64; u8 rgb raw records (C = 1) are served."""
    with pytest.raises(ValueError, match="--input-pixel-format gray gives 3-channel RGB"):
        GaleConfig(topology_name="g", model="lenet5", input_format="raw",
                   input_pixel_format="gray").validate()
    params = params_for("lenet5", MNIST)
    sets = pixel_sets(get_model("lenet5").input_shape, COUNTS, 73)
    want, _ = run(b64_records(sets, "u8"), params, model="lenet5", input_format="b64", **MNIST)
    got, stats = run(raw_records(sets, "u8"), params, model="lenet5", input_format="raw", **MNIST)
    check(got, stats, want, "u8")
