"""Host-side conv dispatch rules (no GPU needed): which layer shapes take the LDS halo-patch 3x3
kernel (conv_patch.hip) under each set_conv_patch mode, and which stay on the im2col GEMM; and
the launch plan of the MFMA conv (conv_mfma_plan): the batch-selected forms that
test_conv_forms_gpu.py launches, and the launches its 32-bit offsets make it refuse."""

import pytest
import torch

import conv_forms

from gale import ops
from gale._native import native


def _desc(H, Cin, Cout, k=3, stride=1, pad=1, res=False):
    w = torch.zeros(Cout, Cin, k, k)
    _, _, geom = ops.pack_conv(w, torch.zeros(Cout), device="cpu")
    Ho = (H + 2 * pad - k) // stride + 1
    d = dict(geom, H=H, W=H, Ho=Ho, Wo=Ho, stride=stride, pad=pad, relu=1, in_f32=0, out_f32=0)
    if res:
        d.update(has_res=1, res_H=Ho, res_W=Ho, res_C=geom["Cout"], res_stride=1)
    return d


def test_conv_patch_dispatch_rules():
    C = native()
    try:
        C.set_conv_patch(1)  # default: 128-channel tiles only
        assert C.conv_patch_supported(_desc(28, 128, 128), 256, False)
        assert C.conv_patch_supported(_desc(14, 256, 256), 256, False)
        assert C.conv_patch_supported(_desc(7, 512, 512), 3, False)      # two images per tile
        assert C.conv_patch_supported(_desc(28, 128, 128, res=True), 4, True)
        assert not C.conv_patch_supported(_desc(56, 64, 64), 256, False)  # 64-channel tile
        assert not C.conv_patch_supported(_desc(28, 128, 128, stride=2), 256, False)
        assert not C.conv_patch_supported(_desc(28, 128, 128, k=1, pad=0), 256, False)
        assert not C.conv_patch_supported(_desc(28, 96, 128), 256, False)  # Cin % 64
        C.set_conv_patch(2)  # + 64-channel tiles
        assert C.conv_patch_supported(_desc(56, 64, 64), 256, False)
        C.set_conv_patch(0)
        assert not C.conv_patch_supported(_desc(28, 128, 128), 256, False)
        C.set_conv_patch(1)
        C.set_conv_path(1)  # "never the GEMM paths" covers the patch kernel too
        assert not C.conv_patch_supported(_desc(28, 128, 128), 256, False)
    finally:
        C.set_conv_path(0)
        C.set_conv_patch(1)


# ---- conv_mfma_plan ------------------------------------------------------------------------


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("form", conv_forms.FORMS, ids=lambda f: f.name)
def test_conv_mfma_plan_of_the_gpu_forms(form, fp8):
    """Every case of test_conv_forms_gpu.py still selects the form it is there for: a moved
    threshold fails here instead of quietly un-testing an instantiation."""
    plan = native().conv_mfma_plan(conv_forms.desc(form, fp8), form.B, form.res is not None)
    conv_forms.check_plan(plan, form, fp8)


def test_conv_mfma_plan_forms_cover_the_batch_selected_instantiations():
    got = {(f.mode, f.nt, f.pr) for f in conv_forms.FORMS}
    for want in [("gather", 1, 4), ("fast", 1, 4), ("fast", 2, 2), ("fast", 4, 4), ("fast", 4, 2),
                 ("fast", 8, 2), ("1x1", 8, 2)]:
        assert want in got
    assert any(f.grid_m < f.m_tiles for f in conv_forms.FORMS)            # the tile walk
    assert any(f.nkc == (4, 2) and f.pr == 2 for f in conv_forms.FORMS)   # chunked at PR 2
    assert all(f.last_rows % (64 * f.pr) != 0 for f in conv_forms.FORMS)  # partial last tile


@pytest.mark.parametrize("B,H,Cin,Cout,k,pad,want", [
    # the shapes test_kernels_gpu.py runs: one pixel tile per wave, every tile has a workgroup
    (4, 32, 16, 16, 3, 1, dict(mode="fast", nt=1, pr=1, n_blocks=1, bk=160, nkc=1, m_tiles=64,
                               grid_m=64)),
    (5, 8, 64, 64, 3, 1, dict(mode="fast", nt=4, pr=1, n_blocks=1, bk=576, nkc=1, m_tiles=5,
                              grid_m=5)),
    (3, 14, 64, 256, 1, 0, dict(mode="1x1", nt=8, pr=1, n_blocks=2, bk=64, nkc=1, m_tiles=10,
                                grid_m=10)),
])
def test_conv_mfma_plan_small_shapes(B, H, Cin, Cout, k, pad, want):
    plan = native().conv_mfma_plan(_desc(H, Cin, Cout, k=k, pad=pad), B, False)
    assert plan["ok"]
    assert {key: plan[key] for key in want} == want


def test_conv_mfma_plan_refuses_what_it_always_refused():
    C = native()
    ok = _desc(8, 16, 16)
    assert C.conv_mfma_plan(ok, 2, False)["ok"]
    assert not C.conv_mfma_plan(dict(ok, Cout=18), 2, False)["ok"]       # Cout % 4
    assert not C.conv_mfma_plan(dict(ok, Kpad=144), 2, False)["ok"]      # Kpad % 32
    assert not C.conv_mfma_plan(dict(ok, Npad=24), 2, False)["ok"]       # Npad % (16 nt)
    assert not C.conv_mfma_plan(dict(ok, out_f32=1), 2, False)["ok"]     # fp32 out needs 1x1
    assert C.conv_mfma_plan(dict(_desc(8, 16, 16, k=1, pad=0), out_f32=1), 2, False)["ok"]


def test_conv_mfma_plan_32bit_limits():
    """The kernel indexes pixels, the input and the residual with 32-bit ints: a launch at or
    over 2^31 in any of the three is refused, the last one below it is planned."""
    C = native()
    # ResNet-50 56x56x256 -> 64 reduce, fp8 (which has no other kernel to go to): the input
    r = dict(_desc(56, 256, 64, k=1, pad=0), fp8=1)
    assert 2674 * 56 * 56 * 256 < 2 ** 31 <= 2675 * 56 * 56 * 256
    assert C.conv_mfma_plan(r, 2674, False)["ok"]
    assert not C.conv_mfma_plan(r, 2675, False)["ok"]
    assert not C.conv_mfma_plan(dict(r, fp8=0), 2675, False)["ok"]
    # 64 -> 256 expand with the identity residual: only the residual crosses
    e = dict(_desc(56, 64, 256, k=1, pad=0, res=True), fp8=1)
    assert 2675 * 56 * 56 * 64 < 2 ** 31 and 2675 * 56 * 56 < 2 ** 31
    assert C.conv_mfma_plan(e, 2674, True)["ok"]
    assert not C.conv_mfma_plan(e, 2675, True)["ok"]
    assert C.conv_mfma_plan(e, 2675, False)["ok"]   # the launch reads no residual
    # a padded 1x1 over a one-pixel, one-channel image has 9 output pixels per input element:
    # only M crosses. The last tile's pixels past M are indexed too, so M counts in whole tiles
    # (256 rows here).
    m = _desc(1, 1, 16, k=1, pad=1)
    assert (m["Ho"], m["Wo"]) == (3, 3)
    plan = C.conv_mfma_plan(m, 238609265, False)               # M = 2^31 - 263
    assert plan["ok"] and plan["pr"] == 4 and plan["m_tiles"] == 2 ** 23 - 1
    assert not C.conv_mfma_plan(m, 238609294, False)["ok"]     # M = 2^31 - 2: its last tile
    assert not C.conv_mfma_plan(m, 238609295, False)["ok"]     # M = 2^31 + 7
