"""The forward plan (csrc/include/gale/forward_plan.h) without a GPU: build_plan writes, for every
zoo model, dtype and plan variant, the ops it wrote before the ops became typed (hashes recorded
from the positional form, tests/golden/forward_plans.json); validate_plan - what Executor(...)
runs before its first HIP call - accepts them unchanged and refuses every broken one by op index
and kind; and a stand-alone sanitizer run over randomly corrupted plans."""

import copy
import hashlib
import json
import os
import shutil
import subprocess

import pytest

from gale._native import native
from gale.models import MODELS, get_model
from gale.models.graph import build_plan
from gale.models.quant import activation_tensors

C = native()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 1 << 20
KINDS = ("conv", "maxpool", "avgpool", "head", "softmax", "resnet20", "stem_pack", "bn_act",
         "lenet5", "bottleneck", "stem_pool", "conv_proj")
POOL = ("H", "W", "C", "k", "s", "pad", "Ho", "Wo")
VARIANTS = (("fused", {}), ("layered", dict(fused=False)), ("unfolded", dict(fold_bn=False)))


def configs():
    for model in sorted(MODELS):
        for wdtype in ("bf16", "fp8", "fp32"):
            for variant, kw in VARIANTS:
                yield f"{model}-{wdtype}-{variant}", model, wdtype, kw
    yield "resnet50-bf16-chunk11", "resnet50", "bf16", dict(chunk_layers=11)


CONFIGS = {name: rest for name, *rest in configs()}
# the unfolded-BN plan is bf16 / fp32 only: build_plan refuses these three
NO_PLAN = {f"{m}-fp8-unfolded" for m in MODELS}
PLANNED = sorted(set(CONFIGS) - NO_PLAN)
_plans = {}


def plan(name):
    """(ops, buf_bytes) of a configuration, built once; nobody changes it."""
    if name not in _plans:
        model, wdtype, kw = CONFIGS[name]
        net = get_model(model)
        sc = None
        if wdtype == "fp8":  # distinct scales, so that a swapped one shows
            sc = {t: 2.0 ** -(1 + i % 7) for i, t in enumerate(sorted(activation_tensors(net)))}
        _plans[name] = build_plan(net, BASE, wdtype, sc, **kw)
    return _plans[name]


# ---- the same plans as before the ops were typed ------------------------------------------------

def legacy_conv(d):
    """A ConvDesc dict as build_plan wrote it: the optional fields only where they applied."""
    d = dict(d)
    if not d["stem"]:
        del d["stem"]
    if not d["fp8"]:
        del d["in_scale"], d["out_scale"]
    if not d["has_res"]:
        for k in ("has_res", "res_H", "res_W", "res_C", "res_stride"):
            del d[k]
    if not (d["fp8"] and d.get("has_res")):
        del d["res_scale"]
    return d


def legacy_view(op):
    """The op in the positional dict form it had: `p` (up to eight ints whose meaning depended on
    the kind), `ptrs` / `scales` (flat lists decoded by index) and `et`. The written record of
    that layout; `res`, `bpi` and `layer` only where the old builder put them."""
    kind = KINDS[op["kind"]]
    io = {"kind": op["kind"], "in": op["in"], "out": op["out"]}
    rest = {"bpi": op["bpi"], "layer": op["layer"]}
    if kind == "conv":
        v = dict(io, **rest, res=op["res"], conv=legacy_conv(op["conv"]), w=op["w"],
                 bias=op["bias"])
        if op["conv"]["fp8"]:
            v["wscale"] = op["wscale"]
        return v
    if kind == "maxpool":
        return dict(io, **rest, p=[op[k] for k in POOL], et=op["et"])
    if kind == "avgpool":
        return dict(io, **rest, p=[op["HW"], op["C"]], et=op["et"])
    if kind == "head":
        return dict(io, **rest, p=[op["HW"], op["C"], op["N"]], w=op["w"], bias=op["bias"],
                    et=op["et"], scale=op["in_scale"])
    if kind == "softmax":
        return dict(io, **rest, p=[op["N"], op["ld"]])
    if kind == "stem_pack":
        return dict(io, **rest, p=[op[k] for k in ("H", "W", "C", "Wp", "lp")])
    if kind == "bn_act":  # w / bias carried the BN scale / shift
        return dict(io, **rest, res=op["res"], w=op["scale"], bias=op["shift"], et=op["et"],
                    p=[op[k] for k in ("HW", "Wo", "C", "relu", "res_H", "res_W", "res_C",
                                       "res_stride")])
    if kind == "resnet20":  # 19 w, 19 b, fc_w, fc_b (+ 19 wscale); 19 s_in, 19 s_out, 19 s_res
        v = dict(io, ptrs=op["w"] + op["b"] + [op["fc_w"], op["fc_b"]])
        if op["fp8"]:
            v.update(fp8=1, ptrs=v["ptrs"] + op["ws"],
                     scales=op["s_in"] + op["s_out"] + op["s_res"])
        return v
    if kind == "lenet5":
        return dict(io, ptrs=[op[f"{c}{i}"] for i in range(1, 6) for c in "wb"])
    if kind == "bottleneck":
        names = ("w1", "b1", "w2", "b2", "w3", "b3") + (("wd", "bd") if op["down"] else ())
        return dict(io, **rest, res=op["res"], p=[op["cin"], op["down"]],
                    ptrs=[op[k] for k in names])
    if kind == "stem_pool":
        return dict(io, **rest, res=op["res"], conv=legacy_conv(op["conv"]), w=op["w"],
                    bias=op["bias"], p=[op[k] for k in POOL])
    assert kind == "conv_proj"
    return dict(io, **rest, res=op["res"], conv=legacy_conv(op["conv"]),
                ptrs=[op["w"], op["bias"], op["wd"], op["bd"]],
                p=[op[k] for k in ("H2", "W2", "Cin2", "stride2", "Kpad2")])


def digest(op):
    return hashlib.sha256(json.dumps(op, sort_keys=True).encode()).hexdigest()[:16]


with open(os.path.join(ROOT, "tests", "golden", "forward_plans.json")) as _f:
    GOLDEN = json.load(_f)


def test_golden_covers_every_configuration():
    assert sorted(GOLDEN) == PLANNED and len(PLANNED) == 25
    sizes = [len(g["ops"]) for g in GOLDEN.values()]
    assert min(sizes) == 1 and max(sizes) == 111
    assert {k for g in GOLDEN.values() for k, _ in g["ops"]} == set(range(len(KINDS)))
    for name in sorted(NO_PLAN):
        with pytest.raises(ValueError):
            plan(name)


@pytest.mark.parametrize("name", PLANNED)
def test_same_plan_as_the_positional_form(name):
    ops, bufs = plan(name)
    want = GOLDEN[name]
    assert bufs == want["buf_bytes"]
    assert [op["kind"] for op in ops] == [k for k, _ in want["ops"]]
    for i, (op, (_, h)) in enumerate(zip(ops, want["ops"])):
        assert digest(legacy_view(op)) == h, (name, i, KINDS[op["kind"]], op)


# ---- validate_plan: the round trip and the refusals ---------------------------------------------

@pytest.mark.parametrize("name", PLANNED)
def test_validate_plan_returns_the_ops_unchanged(name):
    ops, bufs = plan(name)
    assert C.validate_plan(ops, bufs, 8, 2) == ops
    # every op chunked: build_plan gave each one the bytes per image of its operands
    if len(ops) > 1:
        assert C.validate_plan(ops, bufs, 8, 2, len(ops), 3) == ops


def one_of_each_kind():
    """{kind name: (ops, buf_bytes, index)}: a zoo plan holding an op of the kind, and where."""
    found = {}
    for name in PLANNED:
        ops, bufs = plan(name)
        for i, op in enumerate(ops):
            found.setdefault(KINDS[op["kind"]], (ops, bufs, i))
    assert sorted(found) == sorted(KINDS)
    return found


# the pointers each kind cannot run without (in a list: its first entry), and a list-valued key
POINTERS = dict(conv=("w", "bias"), head=("w", "bias"), bn_act=("scale", "shift"),
                resnet20=("w", "b", "fc_w", "fc_b"), lenet5=("w1", "b3", "w5", "b5"),
                bottleneck=("w1", "b2", "w3"), stem_pool=("w", "bias"),
                conv_proj=("w", "bias", "wd", "bd"), maxpool=(), avgpool=(), softmax=(),
                stem_pack=())
ET_KINDS = ("maxpool", "avgpool", "head", "bn_act")


def refusals(kind, op, nbuf):
    """(what, broken op) for every way of breaking `op` the contract names."""
    def broken(**kw):
        b = copy.deepcopy(op)
        b.update(kw)
        return b

    own = sorted(set(op) - {"kind", "in", "out", "res", "bpi", "layer"})
    for k in ["in", "out"] + own:
        b = copy.deepcopy(op)
        del b[k]
        yield f"no {k}", b
    yield "unknown key", broken(colour=1)
    if "conv" in op:
        yield "unknown conv key", broken(conv=dict(op["conv"], colour=1))
        yield "no conv H", broken(conv={k: v for k, v in op["conv"].items() if k != "H"})
    for k in ["bpi"] + [k for k in own if isinstance(op[k], list)]:
        yield f"{k} one short", broken(**{k: op[k][:-1]})
        yield f"{k} one long", broken(**{k: op[k] + op[k][-1:]})
    for k in POINTERS[kind]:
        v = op[k]
        yield f"null {k}", broken(**{k: [0] + v[1:] if isinstance(v, list) else 0})
    for k in ("in", "out", "res"):
        yield f"{k} past the table", broken(**{k: nbuf})
    yield "in negative", broken(**{"in": -1})
    yield "res below -1", broken(res=-2)
    if kind in ET_KINDS:
        yield "et 3", broken(et=3)
        yield "et -1", broken(et=-1)
    if kind == "conv_proj":
        yield "no res", {k: v for k, v in op.items() if k != "res"}


@pytest.mark.parametrize("kind", KINDS)
def test_validate_plan_refuses(kind):
    ops, bufs, i = one_of_each_kind()[kind]
    op = ops[i]
    assert C.validate_plan(ops, bufs, 8, 2) == ops
    cases = list(refusals(kind, op, len(bufs)))
    # bpi above its buffer, for each operand the op has
    for k, key in enumerate(("in", "out", "res")):
        if op[key] >= 0:
            bpi = list(op["bpi"])
            bpi[k] = bufs[op[key]] + 1
            cases.append((f"bpi[{k}] above its buffer", dict(op, bpi=bpi)))
    for what, bad in cases:
        plan_ = ops[:i] + [bad] + ops[i + 1:]
        with pytest.raises(ValueError) as e:
            C.validate_plan(plan_, bufs, 8, 2)
        assert f"plan op {i} ({kind})" in str(e.value), (what, str(e.value))
    # chunked without the bytes per image of an operand
    for k, key in enumerate(("in", "out", "res")):
        if op[key] >= 0:
            bpi = list(op["bpi"])
            bpi[k] = 0
            plan_ = ops[:i] + [dict(op, bpi=bpi)] + ops[i + 1:]
            assert len(C.validate_plan(plan_, bufs, 8, 2)) == len(ops)  # (unchunked: fine)
            with pytest.raises(ValueError) as e:
                C.validate_plan(plan_, bufs, 8, 2, i + 1, 3)
            assert f"plan op {i} ({kind})" in str(e.value) and "bpi" in str(e.value)
    no_bpi = ops[:i] + [{k: v for k, v in op.items() if k != "bpi"}] + ops[i + 1:]
    with pytest.raises(ValueError) as e:
        C.validate_plan(no_bpi, bufs, 8, 2, i + 1, 3)
    assert f"plan op {i} ({kind})" in str(e.value)


def test_validate_plan_names_the_field():
    ops, bufs, i = one_of_each_kind()["resnet20"]
    op = ops[i]
    for bad, word in ((dict(op, w=op["w"][:-1]), "'w' takes 19 entries, got 18"),
                      (dict(op, s_res=op["s_res"] + [1.0]), "'s_res' takes 19 entries, got 20"),
                      ({k: v for k, v in op.items() if k != "fc_b"}, "missing key 'fc_b'"),
                      (dict(op, scales=[]), "unknown key 'scales'"),
                      (dict(op, out=len(bufs)), "out is outside the buffer table"),
                      (dict(op, b=[0] + op["b"][1:]), "b[] is null")):
        with pytest.raises(ValueError, match="plan op 0 \\(resnet20\\)") as e:
            C.validate_plan([bad], bufs, 8, 2)
        assert word in str(e.value)
    # fp8: the weight scales are needed too
    ops8, bufs8 = plan("resnet20-fp8-fused")
    with pytest.raises(ValueError, match="ws\\[\\] is null"):
        C.validate_plan([dict(ops8[0], ws=ops8[0]["ws"][:-1] + [0])], bufs8, 8, 2)
    conv = next(op for op in plan("resnet50-fp8-layered")[0] if op["kind"] == 0)
    with pytest.raises(ValueError, match="plan op 0 \\(conv\\): wscale is null"):
        C.validate_plan([dict(conv, wscale=0)], plan("resnet50-fp8-layered")[1], 8, 2)
    with pytest.raises(ValueError, match="plan op 0: unknown kind 12"):
        C.validate_plan([dict(op, kind=12)], bufs, 8, 2)


def test_validate_plan_keeps_the_constructor_checks():
    ops, bufs = plan("resnet50-bf16-layered")
    for args in ((ops, bufs[:1], 8, 2), (ops, bufs, 0, 2), (ops, bufs, 8, 0),
                 (ops, bufs, 8, 2, -1, 0), (ops, bufs, 8, 2, len(ops) + 1, 0),
                 (ops, bufs, 8, 2, 0, -1)):
        with pytest.raises(ValueError):
            C.validate_plan(*args)
    # what may be left out defaults as before: res = -1, bpi = 0, the optional ConvDesc fields
    conv = next(op for op in ops if op["kind"] == 0 and op["res"] < 0)
    lean = {k: v for k, v in conv.items() if k not in ("res", "bpi", "layer")}
    lean["conv"] = legacy_conv(conv["conv"])
    assert C.validate_plan([lean], bufs, 8, 2) == [dict(conv, bpi=[0, 0, 0], layer=0)]


# ---- stand-alone sanitizer run ------------------------------------------------------------------

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None,
                    reason="needs ROCm clang++ and make")
def test_plan_under_address_and_ub_sanitizers():
    target = "build/asan/forward_plan_check"
    b = subprocess.run(["make", "-C", ROOT, target], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, target), "4000"], capture_output=True, text=True,
                       timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "all checks passed" in out
    assert "AddressSanitizer" not in out and "runtime error" not in out
