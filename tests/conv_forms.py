"""The batch-selected launch forms of the MFMA conv (csrc/kernels/conv_mfma.hip) that the suite
pins: one table shared by test_conv_dispatch_cpu.py (the plan of every case, no launch) and
test_conv_forms_gpu.py (the launches themselves, bit-exact).

Each case is the smallest M = B*Ho*Wo that selects its form and never a multiple of the pixel
tile (64 * pr rows), so the last tile is partial and some 16-pixel sub-tiles lie wholly past M.
The plan columns are what conv_mfma_plan() must return for the case; where bf16 and fp8 differ
(the K chunk) the value is a (bf16, fp8) pair.
"""

from collections import namedtuple

from gale.models.graph import conv_n_tiles, round_up

Form = namedtuple("Form", "name B H W Cin Cout k stride pad in_f32 out_f32 res relu "
                          "mode nt pr n_blocks bk nkc m_tiles grid_m last_rows")

FORMS = [
    # NT1 PR4 gather, resident, 2054 tiles walked by 2048 workgroups; fp8: quantise while loading
    Form("stem3_walk", 547, 31, 31, 3, 16, 3, 1, 1, True, False, None, True,
         "gather", 1, 4, 1, 32, 1, 2054, 2048, 99),
    # NT1 PR4, 5 k-steps in groups of U = 2: an odd tail group
    Form("c16_pr4", 273, 31, 31, 16, 16, 3, 1, 1, False, False, None, False,
         "fast", 1, 4, 1, 160, 1, 1025, 1025, 209),
    # NT2 PR2, stride 2, option-A residual (the input itself, subsampled, channels zero-padded)
    Form("c32_s2_padres", 623, 29, 29, 16, 32, 3, 2, 1, False, False, "pad", True,
         "fast", 2, 2, 1, 160, 1, 1096, 1096, 15),
    # NT4 PR4, identity residual
    Form("c64_pr4_res", 1093, 15, 17, 32, 64, 3, 1, 1, False, False, "identity", False,
         "fast", 4, 4, 1, 288, 1, 1089, 1089, 187),
    # NT4 PR2
    Form("c64_pr2", 600, 15, 17, 32, 64, 3, 1, 1, False, False, None, True,
         "fast", 4, 2, 1, 288, 1, 1196, 1196, 40),
    # NT8 PR2 1x1, 16 n-blocks, 131 tiles walked by 128 workgroups
    Form("expand_walk", 341, 7, 7, 64, 2048, 1, 1, 0, False, False, None, False,
         "1x1", 8, 2, 16, 64, 1, 131, 128, 69),
    # the fc form: fp32 out, Npad 1024 > Cout 1000 (the c >= Cout guard of the last n-block)
    Form("fc_out_f32", 16300, 1, 1, 64, 1000, 1, 1, 0, False, True, None, False,
         "1x1", 8, 2, 8, 64, 1, 128, 128, 44),
    # NT8 PR2, K-chunked: bf16 4 chunks of 9 k-steps; fp8 19 + 17 k-steps
    Form("c2048_chunked_res", 167, 7, 7, 128, 2048, 3, 1, 1, False, False, "identity", True,
         "fast", 8, 2, 16, (288, 608), (4, 2), 64, 64, 119),
    # NT8 PR2 1x1 stride 2, K-chunked with a short last chunk: bf16 9,9,9,5 k-steps; fp8 19,13
    Form("proj_s2_chunked", 167, 13, 13, 1024, 2048, 1, 2, 0, False, False, None, False,
         "1x1", 8, 2, 16, (288, 608), (4, 2), 64, 64, 119),
    # LeNet conv1: NT1 PR4 gather, KW = 5
    Form("lenet_conv1", 340, 28, 28, 1, 8, 5, 1, 2, True, False, None, True,
         "gather", 1, 4, 1, 32, 1, 1042, 1042, 64),
    # K = 4608 at PR1: the K-chunked loop (bf16 16 chunks, fp8 8 with a short last one) on a
    # small shape
    Form("k4608_pr1", 2, 7, 7, 512, 512, 3, 1, 1, False, False, None, True,
         "fast", 8, 1, 4, (288, 608), (16, 8), 2, 2, 34),
    # The remaining (mode, NT, PR) instantiations the zoo plans launch at some batch up to 1024
    # (tests/golden/conv_routes.json): the PR1 forms of small launches ...
    Form("c16_pr1", 2, 9, 9, 16, 16, 3, 1, 1, False, False, None, True,
         "fast", 1, 1, 1, 160, 1, 3, 3, 34),
    Form("c32_pr1", 2, 9, 9, 16, 32, 3, 1, 1, False, False, "identity", True,
         "fast", 2, 1, 1, 160, 1, 3, 3, 34),
    Form("c64_pr1", 2, 9, 9, 32, 64, 3, 1, 1, False, False, None, True,
         "fast", 4, 1, 1, 288, 1, 3, 3, 34),
    Form("reduce_pr1", 2, 7, 7, 64, 64, 1, 1, 0, False, False, None, True,
         "1x1", 4, 1, 1, 64, 1, 2, 2, 34),
    Form("expand_pr1", 2, 7, 7, 64, 256, 1, 1, 0, False, False, "identity", True,
         "1x1", 8, 1, 2, 64, 1, 2, 2, 34),
    Form("fc_out_f32_pr1", 65, 1, 1, 64, 1000, 1, 1, 0, False, True, None, False,
         "1x1", 8, 1, 8, 64, 1, 2, 2, 1),
    Form("stem3_pr1", 2, 9, 9, 3, 16, 3, 1, 1, True, False, None, True,
         "gather", 1, 1, 1, 32, 1, 3, 3, 34),
    Form("stem7_pr1", 2, 29, 29, 3, 64, 7, 2, 3, True, False, None, True,
         "gather", 4, 1, 1, 160, 1, 8, 8, 2),
    # ... and the PR2 / PR4 forms at the smallest batch that selects them
    Form("c16_pr2", 137, 31, 31, 16, 16, 3, 1, 1, False, False, None, False,
         "fast", 1, 2, 1, 160, 1, 1029, 1029, 73),
    Form("c32_s2_pr4", 1164, 29, 29, 16, 32, 3, 2, 1, False, False, None, False,
         "fast", 2, 4, 1, 160, 1, 1024, 1024, 12),
    Form("reduce_pr2", 2673, 7, 7, 64, 64, 1, 1, 0, False, False, None, False,
         "1x1", 4, 2, 1, 64, 1, 1024, 1024, 33),
    Form("reduce_pr4", 5345, 7, 7, 64, 64, 1, 1, 0, False, False, "identity", True,
         "1x1", 4, 4, 1, 64, 1, 1024, 1024, 17),
    Form("stem3_pr2", 137, 31, 31, 3, 16, 3, 1, 1, True, False, None, False,
         "gather", 1, 2, 1, 32, 1, 1029, 1029, 73),
    Form("stem7_pr2", 582, 29, 29, 3, 64, 7, 2, 3, True, False, None, True,
         "gather", 4, 2, 1, 160, 1, 1024, 1024, 6),
    Form("stem7_pr4", 1164, 29, 29, 3, 64, 7, 2, 3, True, False, None, False,
         "gather", 4, 4, 1, 160, 1, 1024, 1024, 12),
]

PLAN_KEYS = ("mode", "nt", "pr", "n_blocks", "bk", "nkc", "m_tiles", "grid_m")


def out_size(f):
    return ((f.H + 2 * f.pad - f.k) // f.stride + 1, (f.W + 2 * f.pad - f.k) // f.stride + 1)


def geometry(f):
    """The packed-weight geometry ops.pack_conv / pack_conv_fp8 give for the case."""
    cout = round_up(f.Cout, 4)
    K = f.k * f.k * f.Cin
    return dict(Cin=f.Cin, Cout=cout, KH=f.k, KW=f.k, K=K, Kpad=round_up(K, 32),
                Npad=round_up(cout, conv_n_tiles(cout) * 16))


def desc(f, fp8, geom=None):
    """The ConvDesc dict of the case's launch (scales left at 1)."""
    Ho, Wo = out_size(f)
    d = dict(geom or geometry(f), H=f.H, W=f.W, Ho=Ho, Wo=Wo, stride=f.stride, pad=f.pad,
             relu=int(f.relu), in_f32=int(f.in_f32), out_f32=int(f.out_f32), fp8=int(fp8))
    if f.res == "identity":
        d.update(has_res=1, res_H=Ho, res_W=Wo, res_C=d["Cout"], res_stride=1)
    elif f.res == "pad":
        d.update(has_res=1, res_H=f.H, res_W=f.W, res_C=f.Cin, res_stride=2)
    return d


def expected_plan(f, fp8):
    pick = lambda v: v[int(fp8)] if isinstance(v, tuple) else v
    return {k: pick(getattr(f, k)) for k in PLAN_KEYS}


def check_plan(plan, f, fp8):
    """Assert that `plan` (conv_mfma_plan's dict) is the form the table claims for the case."""
    assert plan["ok"], f.name
    got = {k: plan[k] for k in PLAN_KEYS}
    assert got == expected_plan(f, fp8), f.name
    Ho, Wo = out_size(f)
    M = f.B * Ho * Wo
    bm = 64 * plan["pr"]
    assert M - (plan["m_tiles"] - 1) * bm == f.last_rows and f.last_rows < bm, f.name
    eb = 1 if fp8 else 2
    assert plan["lds_bytes"] == plan["nt"] * 16 * (plan["bk"] + 16) * eb <= 80 * 1024, f.name
