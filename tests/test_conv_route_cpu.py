"""The conv route (csrc/include/gale/conv_route.h) without a GPU: conv_route() makes, for every
conv of the 25 zoo plans and of the kernel tests, at every recorded batch and policy, the launch
the per-kernel code made before the route became one module (tests/golden/conv_routes.json,
recorded from that commit by a binding that called its functions in conv2d()'s order); the
predicates built on it agree with it; validate_plan refuses, by op index, kind and condition, a
plan with a conv no kernel takes; and a stand-alone sanitizer run over random and extreme descs."""

import copy
import json
import os
import shutil
import subprocess

import pytest

import conv_forms
import conv_routes as cr
from test_forward_plan_cpu import PLANNED, plan

from gale._native import native

C = native()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "conv_routes.json")) as _f:
    GOLDEN = json.load(_f)


class policy:
    """set_conv_path / set_conv_patch for a block, the defaults after it."""

    def __init__(self, path, patch):
        self.modes = (path, patch)

    def __enter__(self):
        C.set_conv_path(self.modes[0])
        C.set_conv_patch(self.modes[1])

    def __exit__(self, *exc):
        C.set_conv_path(0)
        C.set_conv_patch(1)


def zoo_entries():
    out = []
    for name in PLANNED:
        out += cr.plan_descs(name, plan(name)[0])
    return out


def current_descs():
    """{key: (desc, has_res, sources)} of the zoo plans and the kernel tests as they are today."""
    return cr.distinct(zoo_entries() + cr.suite_descs())


def test_golden_covers_the_zoo_and_the_kernel_tests():
    """The recorded descs (named by the hash of their canonical JSON) are exactly the distinct
    ones the zoo plans and the kernel tests make today: a new layer shape or test case needs its
    rows recorded."""
    got = [g[0] for g in GOLDEN["descs"]]
    assert got == [cr.key_digest(k) for k in current_descs()]
    assert GOLDEN["batches"] == list(cr.BATCHES) and GOLDEN["full_rows"] == list(cr.FULL_ROWS)
    assert [tuple(p) for p in GOLDEN["policies"]] == list(cr.POLICIES)
    assert len(got) == 270


def test_conv_route_reproduces_every_recorded_launch():
    """Per desc: the hash over every row (all policies and batches, every args scalar), and in
    full what the route decided at policy (0, 1), batches 1 / 64 / 256."""
    forms = set()
    for (d, has_res, sources), g in zip(current_descs().values(), GOLDEN["descs"]):
        rows, full = [], []
        for path, patch in cr.POLICIES:
            with policy(path, patch):
                for b in cr.BATCHES:
                    r = C.conv_route(d, b, has_res)
                    row = cr.canon(cr.row_of_route(d, b, has_res, r))
                    rows.append([path, patch, b, row])
                    forms.add(cr.form_of(row))
                    assert (r["kernel"] == "none") == (r["refusal"] is not None)
                    # the predicate and the MFMA plan built on the route
                    assert C.conv_patch_supported(d, b, has_res) == (r["kernel"] == "patch")
                    if r["kernel"] == "mfma":
                        plan_ = C.conv_mfma_plan(d, b, has_res)
                        assert plan_["ok"] and all(r[k] == v for k, v in plan_.items())
                    if (path, patch) == (0, 1) and b in cr.FULL_ROWS:
                        assert [k for k, _ in cr.decided(row)] == GOLDEN["row_keys"][r["kernel"]]
                        full.append([v for _, v in cr.decided(row)])
        assert full == g[2:], (sources[0], GOLDEN["row_keys"])
        assert cr.digest(rows) == g[1], sources[0]
    kernels = {f[0] for f in forms}
    assert kernels == {"f32", "gemm", "patch", "mfma"} and len(forms) == 54
    # every (kernel, template form) among them is launched by a GPU test that first asserts it
    # through conv_route: conv_forms.py (test_conv_forms_gpu.py), the GEMM / patch cases
    # (test_kernels_gpu.py), the packed stem (test_bottleneck_gpu.py), conv_f32 (one form)
    tested = {("f32",), ("gemm", ("BM", 128), ("BN", 64), ("NST", 2), ("STEM", 1))}

    def launched(d, batch, has_res):
        return cr.form_of(cr.row_of_route(d, batch, has_res, C.conv_route(d, batch, has_res)))

    with policy(1, 1):
        for f in conv_forms.FORMS:
            for fp8 in (False, True):
                tested.add(launched(conv_forms.desc(f, fp8), f.B, f.res is not None))
    with policy(2, 0):
        tested |= {launched(cr.gemm_desc(c), c[0], c[-1]) for c in cr.GEMM_CASES}
    with policy(0, 2):
        tested |= {launched(cr.patch_desc(c), c[0], c[-1]) for c in cr.PATCH_CASES}
    assert forms - {("none",)} <= tested, sorted(forms - tested, key=str)


def test_every_zoo_conv_has_a_kernel_at_every_batch():
    """What makes validating a plan at its largest batch sufficient: no zoo conv loses its kernel
    at a smaller one."""
    for d, has_res, sources in cr.distinct(zoo_entries()).values():
        for b in range(1, 257):
            r = C.conv_route(d, b, has_res)
            assert r["kernel"] != "none", (sources[0], b, r["refusal"])


def test_route_of_the_gpu_test_cases():
    """The GEMM / patch cases of test_kernels_gpu.py select, under the policy each test sets, the
    kernel and form they are there for."""
    assert len(cr.GEMM_FORMS) == len(cr.GEMM_CASES) and len(cr.PATCH_FORMS) == len(cr.PATCH_CASES)
    with policy(2, 0):
        for case, (bn, stages) in zip(cr.GEMM_CASES, cr.GEMM_FORMS):
            r = C.conv_route(cr.gemm_desc(case), case[0], case[-1])
            assert (r["kernel"], r["bn"], r["stages"]) == ("gemm", bn, stages), case
    with policy(2, 1):  # the default patch mode takes the 7x7x512 case away from conv_gemm
        got = [C.conv_route(cr.gemm_desc(c), c[0], c[-1])["kernel"] for c in cr.GEMM_CASES]
        assert got == ["gemm"] * 4 + ["patch", "gemm"]
    with policy(0, 2):
        for case, (bn, prr) in zip(cr.PATCH_CASES, cr.PATCH_FORMS):
            r = C.conv_route(cr.patch_desc(case), case[0], case[-1])
            assert (r["kernel"], r["bn"], r["prr"]) == ("patch", bn, prr), case
        assert C.conv_route(cr.patch_desc(cr.PATCH_CASES[4]), 3, True)["IMG"] == 2
    with policy(1, 2):
        for f in conv_forms.FORMS:
            r = C.conv_route(conv_forms.desc(f, False), f.B, f.res is not None)
            assert r["kernel"] == "mfma"
            conv_forms.check_plan(r, f, False)


# ---- validate_plan refuses a conv no kernel takes -------------------------------------------

def _find(name, pred):
    ops, bufs = plan(name)
    i = next(i for i, op in enumerate(ops) if pred(op))
    return ops, bufs, i


def _conv(name, pred=lambda c: True):
    return _find(name, lambda op: op["kind"] == 0 and pred(op["conv"]))


def _refused(ops, bufs, i, kind, word, max_batch=8, **conv):
    bad = copy.deepcopy(ops[i])
    bad["conv"].update(conv)
    with pytest.raises(ValueError) as e:
        C.validate_plan(ops[:i] + [bad] + ops[i + 1:], bufs, max_batch, 2)
    assert f"plan op {i} ({kind})" in str(e.value) and word in str(e.value), str(e.value)


def test_validate_plan_refuses_unroutable_convs():
    small = _conv("resnet20-bf16-layered", lambda c: c["KH"] == 3 and c["Cin"] == 16)
    _refused(*small, "conv", "Cout % 4", Cout=18)
    _refused(*small, "conv", "Kpad % 32", Kpad=144)
    _refused(*small, "conv", "Npad % (16 nt)", Npad=24)
    _refused(*small, "conv", "out_f32 outside a 1x1 conv", out_f32=1)
    fp8 = _conv("resnet20-fp8-layered", lambda c: c["KH"] == 3)
    _refused(*fp8, "conv", "in_scale / out_scale must be > 0", in_scale=0.0)
    stem = _conv("resnet50-bf16-layered", lambda c: c["stem"])
    _refused(*stem, "conv", "stem: stride != 2", stride=1)
    # max_batch raised until batch*H*W*Cin >= 2^31: 56x56x256 -> 64 of ResNet-50
    wide = _conv("resnet50-bf16-layered", lambda c: c["H"] == 56 and c["Cin"] == 256)
    ops, bufs, i = wide
    assert 2674 * 56 * 56 * 256 < 2 ** 31 <= 2675 * 56 * 56 * 256
    assert len(C.validate_plan(ops, bufs, 2674, 2)) == len(ops)
    with pytest.raises(ValueError) as e:
        C.validate_plan(ops, bufs, 2675, 2)
    assert "(conv)" in str(e.value) and "batch*H*W*Cin >= 2^31" in str(e.value)
    # ... unless the op is chunked: it is launched with chunk_images at most
    assert len(C.validate_plan(ops, bufs, 2675, 2, len(ops), 64)) == len(ops)


def test_validate_plan_refuses_unsupported_fused_ops():
    ops, bufs, i = _find("resnet50-bf16-fused", lambda op: op["kind"] == 9 and not op["down"])
    with pytest.raises(ValueError, match=f"plan op {i} \\(bottleneck\\): cin"):
        C.validate_plan(ops[:i] + [dict(ops[i], cin=128)] + ops[i + 1:], bufs, 8, 2)
    ops, bufs, i = _find("resnet50-bf16-fused", lambda op: op["kind"] == 10)
    with pytest.raises(ValueError, match=f"plan op {i} \\(stem_pool\\): unsupported geometry"):
        C.validate_plan(ops[:i] + [dict(ops[i], Ho=55)] + ops[i + 1:], bufs, 8, 2)
    ops, bufs, i = _find("resnet50-bf16-fused", lambda op: op["kind"] == 11)
    with pytest.raises(ValueError, match=f"plan op {i} \\(conv_proj\\): unsupported geometry"):
        C.validate_plan(ops[:i] + [dict(ops[i], Cin2=96)] + ops[i + 1:], bufs, 8, 2)


@pytest.mark.parametrize("name", PLANNED)
def test_every_zoo_plan_validates_at_the_default_batch(name):
    ops, bufs = plan(name)
    assert C.validate_plan(ops, bufs, 256, 2) == ops


# ---- stand-alone sanitizer run -----------------------------------------------------------------

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None,
                    reason="needs ROCm clang++ and make")
def test_route_under_address_and_ub_sanitizers():
    target = "build/asan/conv_route_check"
    b = subprocess.run(["make", "-C", ROOT, target], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, target), "300000"], capture_output=True, text=True,
                       timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "all checks passed" in out
    assert "AddressSanitizer" not in out and "runtime error" not in out
