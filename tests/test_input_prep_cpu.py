"""Input preprocessing (--input-scale / --input-mean / --input-std / --input-layout) without a
GPU: the coefficient definition and its validation, configuration precedence, the host helper's
single-rounding fma against exact rational arithmetic, the stub engine end to end on NCHW
records of raw integer pixels, and the fp8 calibration batch."""

import json
import os
import struct
from fractions import Fraction

import numpy as np
import pytest
import torch

from gale._native import native
from gale.cli import parse_topology_args
from gale.config import GaleConfig, from_sources
from gale.models import fold_params, get_model, init_params
from gale.models.preprocess import InputPrep, fma_f32
from gale.models.quant import E4M3_MAX, calibrate_act_scales

C = native()
K = C.kafka

CIFAR_MEAN = (0.4914, 0.4822, 0.4465)
CIFAR_STD = (0.2470, 0.2435, 0.2616)
CIFAR_MEAN_S = "0.4914,0.4822,0.4465"
CIFAR_STD_S = "0.2470,0.2435,0.2616"


def bits(v) -> int:
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def f32_round(x: Fraction) -> int:
    """Bits of the binary32 nearest to the rational x, ties to even (the approach of
    tests/test_json_float_exact.py::f32_correct, on a Fraction instead of a decimal text)."""
    sign = 0x80000000 if x < 0 else 0
    x = abs(x)
    if x == 0:
        return sign
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    if e < -126:
        return sign | round(x / Fraction(2) ** -149)
    m = round(x / Fraction(2) ** (e - 23))
    if m == 1 << 24:
        m >>= 1
        e += 1
    if e > 127:
        return sign | 0x7F800000
    return sign | ((e + 127) << 23) | (m & 0x7FFFFF)


def fma_exact_bits(x, a, b) -> int:
    """x * a + b in exact rational arithmetic, rounded once to binary32."""
    r = Fraction(float(x)) * Fraction(float(a)) + Fraction(float(b))
    if r == 0:  # (an exact zero sum of opposite signs is +0 in round-to-nearest)
        prod_neg = (np.signbit(x) != np.signbit(a))
        return 0x80000000 if (prod_neg and np.signbit(b)) else 0
    return f32_round(r)


def f32_of(v: float) -> float:
    """The double rounded once to binary32."""
    return float(np.float32(v))


# ---- 1. coefficients and validation ------------------------------------------------------------

def test_coefficients_cifar():
    p = InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S)
    for c in range(3):
        assert bits(p.a[c]) == f32_round(Fraction(1 / 255) / Fraction(CIFAR_STD[c]))
        assert bits(p.b[c]) == f32_round(-Fraction(CIFAR_MEAN[c]) / Fraction(CIFAR_STD[c]))
        # "computed in double and rounded once": the double quotient, then one narrowing
        assert bits(p.a[c]) == bits(f32_of((1 / 255) / CIFAR_STD[c]))
        assert bits(p.b[c]) == bits(f32_of(-CIFAR_MEAN[c] / CIFAR_STD[c]))
    assert not p.identity and not p.nchw
    a4, b4 = p.coeffs()
    assert len(a4) == len(b4) == 4 and a4[:3] == list(p.a) and b4[:3] == list(p.b)


def test_coefficients_scalar_and_identity():
    p = InputPrep.build(3, 1.0, "0.1307", "0.3081")
    assert len(p.a) == 3 and len(set(p.a)) == 1 and len(set(p.b)) == 1
    assert bits(p.a[0]) == bits(f32_of(1.0 / 0.3081))
    assert bits(p.b[0]) == bits(f32_of(-0.1307 / 0.3081))
    assert p.coeffs() == ([p.a[0]] * 4, [p.b[0]] * 4)
    q = InputPrep.build(3)
    assert q.identity and q.a == (1.0, 1.0, 1.0) and q.b == (0.0, 0.0, 0.0)
    assert all(bits(v) == 0 for v in q.b)  # +0.0, not -0.0
    d = GaleConfig(topology_name="t").validate().engine_dict(32, 32, 3, 10)
    assert d["input_a"] == [1.0] * 4 and d["input_b"] == [0.0] * 4 and d["input_nchw"] is False
    assert not InputPrep.build(3, layout="nchw").identity
    # a scalar on a model with more than four channels is fine (one value in every slot)
    assert InputPrep.build(8, 2.0, "1", "4").coeffs() == ([0.5] * 4, [-0.25] * 4)


@pytest.mark.parametrize("kw", [
    dict(input_std="0.25,0,0.25"),                     # a std of 0
    dict(input_std="0"),
    dict(input_mean="nan"),                            # non-finite values
    dict(input_std="inf"),
    dict(input_scale=float("inf")),
    dict(input_mean="0.1,0.2"),                        # neither 1 nor C values
    dict(input_std="1,1,1,1"),
    dict(input_mean="0.1,0.2,0.3", model="lenet5"),    # C = 1
    dict(input_layout="chwn"),                         # unknown layout
])
def test_validation_errors(kw):
    with pytest.raises(ValueError):
        GaleConfig(topology_name="t", **kw).validate()


def test_validation_per_channel_needs_c_le_4():
    with pytest.raises(ValueError):
        InputPrep.build(8, 1.0, ",".join(["0.5"] * 8), "1")
    with pytest.raises(ValueError):
        InputPrep.build(8, 1.0, "0", ",".join(["0.5"] * 8))
    InputPrep.build(4, 1.0, "0.1,0.2,0.3,0.4", "1,2,3,4")  # C = 4 per channel is allowed


# ---- 2. configuration precedence ---------------------------------------------------------------

def test_config_sources_agree(tmp_path):
    want = InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S, "nchw").engine_entries()
    cli = parse_topology_args(["t", "in", "out", "--input-scale", "0.00392156862745098",
                               "--input-mean", CIFAR_MEAN_S, "--input-std", CIFAR_STD_S,
                               "--input-layout", "nchw"])
    env = from_sources(cli=dict(topology_name="t"), env={
        "GALE_INPUT_SCALE": "0.00392156862745098", "GALE_INPUT_MEAN": CIFAR_MEAN_S,
        "GALE_INPUT_STD": CIFAR_STD_S, "GALE_INPUT_LAYOUT": "nchw"})
    toml = tmp_path / "g.toml"
    toml.write_text('[gale]\ninput-scale = 0.00392156862745098\n'
                    f'input-mean = "{CIFAR_MEAN_S}"\ninput_std = "{CIFAR_STD_S}"\n'
                    'input-layout = "nchw"\n')
    tom = from_sources(cli=dict(topology_name="t"), env={}, toml_path=str(toml))
    for cfg in (cli, env, tom):
        d = cfg.engine_dict(32, 32, 3, 10)
        assert {k: d[k] for k in want} == want
    assert want["input_nchw"] is True
    assert [bits(v) for v in want["input_a"][:3]] == \
        [bits(f32_of((1 / 255) / s)) for s in CIFAR_STD]
    # precedence: CLI > env > TOML
    mixed = from_sources(cli=dict(topology_name="t", input_mean="0.5"),
                         env={"GALE_INPUT_MEAN": "0.25", "GALE_INPUT_STD": "0.5"},
                         toml_path=str(toml))
    assert mixed.input_mean == "0.5" and mixed.input_std == "0.5" and mixed.input_layout == "nchw"


# ---- 3. host helper: one rounding --------------------------------------------------------------

def boundary_cases():
    """x, a, b with x * a within half an ulp of a rounding boundary of the sum: the exact
    product carries bits below the sum's last place that a rounded product loses."""
    one = np.float32(1.0)
    e = np.float32(2.0 ** -12)
    cases = [
        # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24: the 2^-24 is exactly half an ulp of 1; a rounded
        # product drops it (tie to even), fma keeps it and b tips the sum over the boundary
        (one + e, one + e, np.float32(2.0 ** -30)),
        (one + e, one + e, np.float32(-(2.0 ** -30))),
        (one + e, one + e, np.float32(0.0)),
        (one + e, -(one + e), np.float32(1.0) + np.float32(2.0 ** -11)),  # cancels to -2^-24
        (np.float32(3.0) * (one + e), one + e, np.float32(2.0 ** -28)),
        # product just below / above a midpoint of the sum's grid (sum in [2, 4): ulp 2^-22)
        (one + np.float32(2.0 ** -23), one + np.float32(2.0 ** -23), np.float32(1.0)),
        (one - np.float32(2.0 ** -24), one - np.float32(2.0 ** -24), np.float32(1.0)),
        (np.float32(255.0), np.float32(f32_of((1 / 255) / 0.2470)), np.float32(-1.9894737)),
        (np.float32(16777215.0), np.float32(16777215.0), np.float32(-2.8147494e14)),
    ]
    return cases


def test_host_helper_is_a_single_rounding_fma():
    rng = np.random.default_rng(11)
    n = 2000
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)).astype(np.float32)
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    # half of them with b near -x*a (cancellation: every product bit matters)
    prod = (x.astype(np.float64) * a.astype(np.float64))
    near = -(prod * (1 + rng.integers(-4, 5, n) * 2.0 ** -24)).astype(np.float32)
    b[::2] = near[::2]
    extra = boundary_cases()
    x = np.concatenate([x, np.array([c[0] for c in extra], np.float32)])
    a = np.concatenate([a, np.array([c[1] for c in extra], np.float32)])
    b = np.concatenate([b, np.array([c[2] for c in extra], np.float32)])
    want = np.array([fma_exact_bits(x[i], a[i], b[i]) for i in range(len(x))], dtype=np.uint32)
    # the helper takes per-channel coefficients: one 1x1x1 image per case
    got = np.array([C.apply_input_prep(x[i:i + 1], 1, 1, 1, False, [float(a[i])] * 4,
                                       [float(b[i])] * 4).view(np.uint32).ravel()[0]
                    for i in range(len(x))], dtype=np.uint32)
    bad = [(float(x[i]), float(a[i]), float(b[i]), hex(got[i]), hex(want[i]))
           for i in np.nonzero(got != want)[0][:10]]
    assert not bad, bad
    # the numpy definition used by the oracles agrees bit for bit
    assert np.array_equal(fma_f32(x, a, b).view(np.uint32), want)
    # and a multiply-then-add implementation does not: the check has teeth
    muladd = ((x * a).astype(np.float32) + b).astype(np.float32).view(np.uint32)
    assert (muladd != want).sum() > 100
    assert (muladd[-len(extra):] != want[-len(extra):]).sum() >= 3


def test_host_helper_channels_and_transposition():
    rng = np.random.default_rng(12)
    H, W, Cc = 5, 4, 3
    p = InputPrep.build(Cc, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S)
    a4, b4 = p.coeffs()
    x = rng.integers(0, 256, (3, H, W, Cc)).astype(np.float32)
    want = np.empty(x.shape, dtype=np.uint32)
    for idx in np.ndindex(*x.shape):
        want[idx] = fma_exact_bits(x[idx], np.float32(p.a[idx[3]]), np.float32(p.b[idx[3]]))
    got = C.apply_input_prep(x, H, W, Cc, False, a4, b4)
    assert got.shape == x.shape and np.array_equal(got.view(np.uint32), want)
    # the same images as parsed from an NCHW record: transposed back to NHWC
    got = C.apply_input_prep(np.ascontiguousarray(x.transpose(0, 3, 1, 2)), H, W, Cc, True, a4, b4)
    assert got.shape == x.shape and np.array_equal(got.view(np.uint32), want)
    assert np.array_equal(p.apply(x).view(np.uint32), want)
    # C = 4 uses every slot, C = 1 the first
    p4 = InputPrep.build(4, 0.5, "1,2,3,4", "2,4,8,16")
    x4 = rng.standard_normal((2, 3, 2, 4)).astype(np.float32)
    got = C.apply_input_prep(x4, 3, 2, 4, False, *p4.coeffs())
    assert np.array_equal(got.view(np.uint32), p4.apply(x4).view(np.uint32))
    assert np.array_equal(got, x4 * np.float32([.25, .125, .0625, .03125])
                          - np.float32([.5, .5, .375, .25]))  # (exact in binary32)


# ---- 4. stub engine end to end -----------------------------------------------------------------

H, W, CH, CLASSES = 4, 3, 3, 10


def stub_probs(x):
    """replica.cpp: logit k = (k + 1) * mean of channel k % C, then softmax (in double)."""
    means = x.reshape(x.shape[0], -1, x.shape[-1]).astype(np.float64).mean(axis=1)
    logits = np.stack([(k + 1) * means[:, k % x.shape[-1]] for k in range(CLASSES)], axis=1)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def nchw_record(x_nhwc) -> bytes:
    return json.dumps({"instances": x_nhwc.transpose(0, 3, 1, 2).tolist()},
                      separators=(",", ":")).encode()


def test_stub_engine_nchw_byte_pixels():
    broker = K.Broker()
    broker.start()
    try:
        broker.create_topic("in", 1)
        broker.create_topic("out", 1)
        rng = np.random.default_rng(5)
        xs = {}
        for i, n in enumerate([1, 2, 3, 1, 3, 2]):
            x = rng.integers(0, 256, (n, H, W, CH))
            xs[f"r{i}".encode()] = x
            broker.append("in", 0, [nchw_record(x)], [f"r{i}".encode()])
        assert b"." not in nchw_record(xs[b"r0"])  # integers, no decimal point
        # ragged: in one image the first row of channel 0 has W - 1 values, the second W + 1
        rag = xs[b"r1"].transpose(0, 3, 1, 2).tolist()
        rag[1][0][1].append(rag[1][0][0].pop())
        broker.append("in", 0, [json.dumps({"instances": rag}, separators=(",", ":")).encode()],
                      [b"ragged"])
        # an NHWC-nested record is the wrong shape for an NCHW topology
        broker.append("in", 0, [json.dumps({"instances": xs[b"r0"].tolist()}).encode()],
                      [b"nhwc"])
        cfg = GaleConfig(topology_name="t", input_topic="in", output_topic="out",
                         bootstrap=f"127.0.0.1:{broker.port}", start_offset="earliest",
                         stub=True, max_batch=4, max_wait_us=500, output_key="input",
                         on_error="null", input_scale=1 / 255, input_mean=CIFAR_MEAN_S,
                         input_std=CIFAR_STD_S, input_layout="nchw").validate()
        d = cfg.engine_dict(H, W, CH, CLASSES)
        d["max_records"] = len(xs) + 2
        eng = C.Engine(d)
        eng.add_stub_replica(4, 0, True, -1)
        eng.start()
        assert eng.wait(30000), eng.stats()
        eng.stop()
        out = broker.read("out", 0)
    finally:
        broker.stop()
    by_key = {r["key"]: r["value"] for r in out}
    assert set(by_key) == set(xs) | {b"ragged", b"nhwc"}
    assert by_key[b"ragged"] is None and by_key[b"nhwc"] is None
    prep = cfg.input_prep(CH)
    for k, x in xs.items():
        got = np.array(json.loads(by_key[k])["predictions"])
        want = stub_probs(prep.apply(x.astype(np.float32)))
        assert got.shape == want.shape, k
        np.testing.assert_allclose(got, want, atol=1e-6, err_msg=str(k))
        # and NOT what the raw pixels give: the options reached the replica
        assert np.abs(got - stub_probs(x.astype(np.float32))).max() > 1e-3


# ---- 5. fp8 calibration ------------------------------------------------------------------------

def test_fp8_calibration_covers_the_preprocessed_range():
    from gale.models.quant import CALIB_BATCH, CALIB_SEED

    net = get_model("resnet20")
    folded = fold_params(net, init_params(net, seed=0, calibrate=False))
    prep = InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S)
    base = calibrate_act_scales(net, folded)
    assert calibrate_act_scales(net, folded, None) == base  # bit-equal: today's values
    # today's input scale: the U[0,1) batch's amax with the margin (gale/models/quant.py)
    g = torch.Generator().manual_seed(CALIB_SEED)
    u = torch.rand((CALIB_BATCH,) + tuple(net.input_shape), generator=g)
    assert base["input"] == max(float(u.abs().max()) * 1.25, 1e-6) / E4M3_MAX
    sc = calibrate_act_scales(net, folded, prep)
    y = prep.apply((u.double() / prep.scale).float())
    # that batch is (u - mean) / std up to rounding
    ref = (u.double() - torch.tensor(CIFAR_MEAN, dtype=torch.float64)) / \
        torch.tensor(CIFAR_STD, dtype=torch.float64)
    assert float((y.double() - ref).abs().max()) < 1e-5
    ymax = float(y.abs().max())
    assert ymax > 1.9  # (0 - 0.4914) / 0.2470 = -1.99: outside U[0,1)'s range
    assert sc["input"] >= ymax / E4M3_MAX
    assert base["input"] < ymax / E4M3_MAX  # the unpreprocessed scale would saturate
    assert set(sc) == set(base)
