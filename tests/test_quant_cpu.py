"""fp8 (OCP e4m3fn) quantisation on the host: codes, per-row scales, activation calibration, the
fp8 emulation oracle's accuracy against fp32, and the packed fp8 layout / plan."""

import pytest
import torch

from gale.models import build_plan, fold_params, get_model, init_params, pack_params
from gale.models.graph import act_scales_from_packed, param_layout
from gale.models.quant import (E4M3_MAX, activation_tensors, calibrate_act_scales,
                               dequantize_rows_e4m3, e4m3_codes, e4m3_round, quantize_rows_e4m3)
from gale.models.reference import forward


def test_e4m3_is_ocp_not_fnuz():
    # OCP e4m3fn: 1.0 = 0x38, max 448 = 0x7e, -0.0 = 0x80 (fnuz would encode 1.0 as 0x40)
    codes = e4m3_codes(torch.tensor([1.0, 448.0, -2.0, 1000.0, 0.0]))
    assert codes.tolist() == [0x38, 0x7E, 0xC0, 0x7E, 0x00]
    assert e4m3_round(torch.tensor([0.3])).item() == pytest.approx(0.3125)


def test_row_quantisation_roundtrip():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(24, 100, generator=g) * torch.logspace(-3, 2, 24)[:, None]
    w[5] = 0
    q, s = quantize_rows_e4m3(w)
    assert q.dtype == torch.uint8 and s.shape == (24,)
    back = dequantize_rows_e4m3(q, s)
    assert back[5].abs().sum() == 0
    rel = ((back - w).abs() / w.abs().amax(1, keepdim=True).clamp_min(1e-30)).max()
    assert rel <= 2 ** -4 + 1e-6  # half an ulp of a 3-bit mantissa at the row max
    assert (back.abs().amax(1)[w.abs().amax(1) > 0] / w.abs().amax(1)[w.abs().amax(1) > 0]
            - 1).abs().max() < 1e-6  # the row max is exactly representable (448 * s)


def test_activation_scales_cover_calibration_range():
    net = get_model("resnet20")
    f = fold_params(net, init_params(net, seed=0))
    sc = calibrate_act_scales(net, f)
    assert set(sc) == set(activation_tensors(net))
    assert sc["input"] == pytest.approx(1.25 / E4M3_MAX, rel=0.01)  # U[0,1) inputs
    assert all(v > 0 for v in sc.values())
    assert sc == calibrate_act_scales(net, f)  # deterministic (seeded calibration batch)


@pytest.mark.parametrize("name", ["lenet5", "resnet20"])
def test_fp8_emulation_tracks_fp32(name):
    """The fp8 design (e4m3 weights per channel, e4m3 activations per tensor) is accurate enough
    to serve: softmax within a few 1e-2 and argmax agreement wherever the top-2 gap is clear."""
    net = get_model(name)
    f = fold_params(net, init_params(net, seed=5))
    sc = calibrate_act_scales(net, f)
    x = torch.rand((128,) + net.input_shape, generator=torch.Generator().manual_seed(9))
    ref = forward(net, f, x)
    emu = forward(net, f, x, fp8_scales=sc)
    err = (emu - ref).abs()
    assert err.max() < 0.15 and err.mean() < 0.015
    top2 = ref.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 0.1
    agree = (emu.argmax(1)[clear] == ref.argmax(1)[clear]).float().mean()
    assert agree >= 0.95


@pytest.mark.parametrize("name", ["lenet5", "resnet20", "resnet50"])
def test_fp8_packing_and_plan(name):
    net = get_model(name)
    layout, total = param_layout(net, "fp8")
    assert "act_scales" in layout
    if name == "resnet50":
        return  # the resnet50 fp32 calibration forward is slow on CPU; layout checked above
    f = fold_params(net, init_params(net, seed=1))
    buf = pack_params(net, f, "fp8")
    assert buf.numel() == total
    sc = act_scales_from_packed(net, buf)
    assert sc == pytest.approx(calibrate_act_scales(net, f))
    ops, buf_bytes = build_plan(net, 0, "fp8", sc, fused=False)
    convs = [op for op in ops if op["kind"] == 0]
    assert all(op["conv"]["fp8"] == 1 and op["conv"]["in_scale"] > 0 for op in convs)
    assert all("wscale" in op for op in convs)
    assert convs[0]["conv"]["in_scale"] == pytest.approx(sc["input"])
    # e4m3 activations: half the bytes of the bf16 plan's activation buffers
    _, bf16_bytes = build_plan(net, 0, "bf16", fused=False)
    assert sum(buf_bytes[2:]) * 2 == sum(bf16_bytes[2:])
    with pytest.raises(ValueError):
        build_plan(net, 0, "fp8")


def test_fp8_fused_resnet20_plan_carries_scales():
    from gale.models.graph import OP_RESNET20, Conv

    net = get_model("resnet20")
    f = fold_params(net, init_params(net, seed=1))
    sc = act_scales_from_packed(net, pack_params(net, f, "fp8"))
    ops, _ = build_plan(net, 4096, "fp8", sc)
    assert len(ops) == 1 and ops[0]["kind"] == OP_RESNET20 and ops[0]["fp8"] == 1
    # 59 pointers (19 weights, 19 biases, the classifier's two, 19 weight scales), 57 scales
    pointers = ops[0]["w"] + ops[0]["b"] + [ops[0]["fc_w"], ops[0]["fc_b"]] + ops[0]["ws"]
    assert [len(ops[0][k]) for k in ("w", "b", "ws")] == [19, 19, 19] and all(pointers)
    convs = [L for L in net.layers if isinstance(L, Conv)]
    s_in, s_out, s_res = (ops[0][k] for k in ("s_in", "s_out", "s_res"))
    assert len(s_in) == len(s_out) == len(s_res) == 19
    assert s_in[0] == pytest.approx(sc["input"])
    for i, L in enumerate(convs):
        assert s_in[i] == pytest.approx(sc[L.inp]) and s_out[i] == pytest.approx(sc[L.out])
        if L.residual:
            assert s_res[i] == pytest.approx(sc[L.residual])
