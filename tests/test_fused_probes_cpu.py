"""The probe networks of tests/fused_probes.py meet the conditions that make them exact and
observable (no GPU): what test_fused_probes_gpu.py asserts of the kernels rests on these.

Per probe the tests print the largest activation magnitude, the head shift s, the logit spread and
the two observability floors (run with -s to see them)."""

import pytest
import torch

import fused_probes as fp
from gale.models.graph import Conv, act_scales_from_packed
from gale.models.quant import quantize_rows_e4m3
from gale.models.reference import forward


def is_int(v, unit=1.0):
    return bool((v / unit == (v / unit).round()).all())


def spread(logits):
    return (logits.amax(1) - logits.amin(1)).max().item()


def check_logits_exact(p, last, name, unit=1.0):
    """The dense layer's fp32 sums are exact in any order: with the last activation `last` in
    multiples of `unit`, every partial sum of pooling and dense layer is an integer below 2^24
    in units of unit / (pixels * 2^s), and the bias of quarters lies on that grid too."""
    assert is_int(last, unit)
    w_int = (p.folded[f"{name}.weight"] * 2.0 ** p.shift).abs()
    sums = last.flatten(2).abs().sum(2) / unit
    bound = sums @ w_int.t() + p.folded[f"{name}.bias"].abs() * 2.0 ** p.shift / unit * 64
    assert bound.max().item() < 2 ** 24
    grid = unit * 2.0 ** -p.shift / last.flatten(2).shape[2]
    assert grid <= 0.25 and is_int(p.logits.double(), grid)


def check_head(folded, name):
    w = folded[f"{name}.weight"]
    assert bool(((w - w.mean(0)).abs().amax(0) > 0).all())  # no constant column
    assert is_int(folded[f"{name}.bias"], 0.25)


def check_round_trip(net, folded, buf):
    for L in net.layers:
        if isinstance(L, Conv):
            w, b = fp.unpack_conv(net, buf, L)
            assert torch.equal(w, folded[f"{L.name}.weight"]), L.name
            assert torch.equal(b, folded[f"{L.name}.bias"]), L.name


@pytest.mark.parametrize("case", ["bf16", "fp8", "lenet5"])
def test_walk_is_the_oracle(case):
    """fused_probes.walk (the forward with edit points) equals gale.models.reference.forward bit
    for bit, tensors and logits."""
    if case == "lenet5":
        net, p, scales = fp.lenet(), fp.lenet_probe(0), None
    elif case == "bf16":
        net, p, scales = fp.r20(), fp.r20_probe(8, "relu"), None
    else:
        net, p = fp.r20(), fp.r20_fp8_probe(8, "relu")
        scales = p.scales
    col, tensors = {}, {}
    forward(net, p.folded, p.x, collect=col, tensors=tensors, fp8_scales=scales)
    logits, t = fp.walk(net, p.folded, p.x, fp8_scales=scales)
    assert torch.equal(logits, col["logits"]) and torch.equal(logits, p.logits)
    assert set(t) == set(tensors) and all(torch.equal(t[k], tensors[k]) for k in t)


@pytest.mark.parametrize("i", range(fp.N_CONVS))
def test_resnet20_probe_conditions(i):
    net = fp.r20()
    L = fp.r20_convs()[i]
    act = wgt = None
    for variant in fp.VARIANTS:
        p = fp.r20_probe(i, variant)
        w, b = p.folded[f"{L.name}.weight"], p.folded[f"{L.name}.bias"]
        assert set(w.unique().tolist()) <= {-1.0, 0.0, 1.0} and is_int(b)
        if variant == "relu":
            assert b.abs().max() <= 1
        else:
            assert torch.equal(w, fp.r20_probe(i, "relu").folded[f"{L.name}.weight"])
        # 1. exactness: every activation is an integer that bf16 holds
        col, tensors = {}, {}
        forward(net, p.folded, p.x, collect=col, tensors=tensors)
        assert torch.equal(col["logits"], p.logits)
        amax = max(t.abs().max().item() for t in tensors.values())
        assert all(is_int(t) for t in tensors.values()) and amax <= fp.MAX_ACT
        assert all(torch.equal(t, t.bfloat16().float()) for t in tensors.values())
        check_logits_exact(p, tensors["l3.2.out"], "fc")
        check_head(p.folded, "fc")
        assert is_int(p.folded["fc.weight"] * 2.0 ** p.shift)
        assert (p.folded["fc.weight"] * 2.0 ** p.shift).abs().max() <= 8
        if variant == "open":  # every pre-activation of the probed conv is positive
            assert tensors[L.out].min() > 0
        # 2. spread
        assert spread(p.logits) <= fp.SPREAD
        # the packed buffer holds these integers
        check_round_trip(net, p.folded, fp.r20_packed(i, variant))
        # 3. observability, by autograd on the reference
        a, g = fp.r20_gains(p)
        act = a if act is None else torch.maximum(act, a)
        wgt = g if wgt is None else torch.maximum(wgt, g)
        print(f"\n{p.name}: largest activation {amax:.0f}, s {p.shift}, spread "
              f"{spread(p.logits):.2f}, floors so far: activations {act.min().item():.2e} "
              f"weights {wgt.min().item():.2e}")
    assert act.min().item() >= fp.FLOOR and wgt.min().item() >= fp.FLOOR
    # 4. carrier transparency: with the probed conv zero, X3 is the carrier's definition
    p = fp.r20_probe(i, "relu")
    zeroed = dict(p.folded)
    zeroed[f"{L.name}.weight"] = torch.zeros_like(p.folded[f"{L.name}.weight"])
    zeroed[f"{L.name}.bias"] = torch.zeros(L.cout)
    tensors = {}
    forward(net, zeroed, p.x, tensors=tensors)
    assert torch.equal(tensors["l3.2.out"], fp.carrier_x3(p.x, i))
    assert i == 0 or tensors["l3.2.out"].any()


def drop_corner_tap(probe):
    """The mistake "the centre tap of the probed conv is not read at the top-left pixel"."""
    def edit(L, y, inp):
        if L is probe.layer:
            w = probe.folded[f"{L.name}.weight"]
            y = y.clone()
            y[:, :, 0, 0] -= inp[:, :, 0, 0] @ w[:, :, 1, 1].t()
        return y
    return dict(edit_conv=edit)


def shift_shortcut(probe):
    """The mistake "block 2.1's shortcut is read one pixel off"."""
    def edit(L, r):
        return torch.roll(r, 1, dims=3) if L.name == "l2.0.conv2" else r
    return dict(edit_res=edit)


@pytest.mark.parametrize("mistake,convs", [(drop_corner_tap, range(0, 7)), (shift_shortcut, [8])])
def test_probes_notice_a_mistake_in_the_expectation(mistake, convs):
    """The probes are not vacuous: a one-line mistake applied to the expectation (not to a
    kernel) moves the reference logits of the probes that should notice by more than 20 T."""
    for i in convs:
        moved = 0.0
        for variant in fp.VARIANTS:
            p = fp.r20_probe(i, variant)
            wrong = fp.walk(fp.r20(), p.folded, p.x, **mistake(p))[0]
            moved = max(moved, (fp.centred(wrong) - fp.centred(p.logits)).abs().max().item())
        print(f"\n{mistake.__name__} conv {i}: logits move by {moved:.2e}")
        assert moved > fp.FLOOR, (mistake.__name__, i, moved)


@pytest.mark.parametrize("i", fp.FP8_CONVS)
def test_resnet20_fp8_probe_conditions(i):
    net = fp.r20()
    L = fp.r20_convs()[i]
    exps = fp.fp8_scale_exponents()
    blind = None
    for variant in fp.VARIANTS:
        p = fp.r20_fp8_probe(i, variant)
        w = p.folded[f"{L.name}.weight"]
        assert set(w.unique().tolist()) <= {-fp.FP8_W, 0.0, fp.FP8_W}
        assert bool(w.flatten(1).abs().amax(1).eq(fp.FP8_W).all())  # every row has a non-zero
        q, s = quantize_rows_e4m3(w.flatten(1))
        assert bool((s == 2.0 ** -9).all()) and set(q.unique().tolist()) <= {0, 0x7E, 0xFE}
        # the packed buffer carries the probes' scales
        assert act_scales_from_packed(net, fp.r20_fp8_packed(i, variant)) == p.scales
        assert all(p.scales[n] == 2.0 ** e for n, e in exps.items())
        # every value ahead of an e4m3 rounding is exact in fp32 in any order, and below saturation
        pre = {}
        logits, t = fp.walk(net, p.folded, p.x, fp8_scales=p.scales, pre=pre)
        assert torch.equal(logits, p.logits)
        for name, v in pre.items():
            assert is_int(v, fp.FP8_UNIT) and v.abs().max() < 2 ** 17, name
            assert v.abs().max().item() / p.scales[name] < 448, name
        assert is_int(p.x) and p.x.max().item() / p.scales["input"] < 448
        x3 = t["l3.2.out"]
        unit = max(2.0 ** -k for k in range(7) if is_int(x3, 2.0 ** -k))
        check_logits_exact(p, x3, "fc", unit)
        assert spread(p.logits) <= fp.SPREAD
        # every conv weight is 7 * 2^k or zero: power-of-two row scales, codes +-448, so the
        # kernels' acc * (wscale * s_in) is exact
        for Lc in fp.r20_convs():
            qc, sc = quantize_rows_e4m3(p.folded[f"{Lc.name}.weight"].flatten(1))
            assert set(qc.unique().tolist()) <= {0, 0x7E, 0xFE}, Lc.name
            assert bool((torch.log2(sc) == torch.log2(sc).round()).all()), Lc.name
        if variant == "open":
            assert t[L.out].min() > 0
        seen = fp.fp8_observed(p)
        blind = ~seen if blind is None else blind & ~seen
        print(f"\n{p.name}: s {p.shift}, spread {spread(p.logits):.2f}, largest code "
              f"{max(v.abs().max().item() / p.scales[n] for n, v in pre.items()):.1f}, "
              f"not observable alone {(~seen).float().mean().item():.3f}")
        if variant == "open" and i >= 13:
            assert bool(seen.all())
    share = blind.float().mean().item()
    print(f"fp8 conv {i}: not observable in either variant {share:.3f}")
    assert share <= 0.05


@pytest.mark.parametrize("seed", fp.LENET_SEEDS)
def test_lenet5_probe_conditions(seed):
    net = fp.lenet()
    p = fp.lenet_probe(seed)
    assert set(p.x.unique().tolist()) <= {0.0, 1.0, 2.0, 3.0} and len(p.x) == max(fp.LENET_BATCHES)
    col, tensors = {}, {}
    forward(net, p.folded, p.x, collect=col, tensors=tensors)
    assert torch.equal(col["logits"], p.logits)
    # order-independent fp32 sums: sum |w| |a| + |b| < 2^24 for every output of every layer
    report = []
    for L in net.layers:
        if not isinstance(L, Conv):
            continue
        w, b = p.folded[f"{L.name}.weight"], p.folded[f"{L.name}.bias"]
        assert is_int(w) and w.abs().max() <= 2 and is_int(b)
        assert torch.equal(w, w.bfloat16().float())
        bound = torch.nn.functional.conv2d(tensors[L.inp].abs(), w.abs(), b.abs(),
                                           stride=L.stride, padding=L.pad)
        assert bound.max() < 2 ** 24 and is_int(tensors[L.out])
        # (the layered plan stores bf16 activations: integers up to 256 are exact there too)
        assert tensors[L.out].max() <= fp.MAX_ACT
        assert torch.equal(tensors[L.out], tensors[L.out].bfloat16().float())
        report.append(f"{L.out} {tensors[L.out].max().item():.0f}")
    w3 = p.folded["fc3.weight"] * 2.0 ** p.shift
    assert is_int(w3) and w3.abs().max() <= 8
    check_logits_exact(p, tensors["f2"], "fc3")
    check_head(p.folded, "fc3")
    assert spread(p.logits) <= fp.SPREAD
    check_round_trip(net, p.folded, fp.lenet_packed(seed))
    gains = fp.lenet_gains(p)
    floors = {n: g.min().item() for n, g in gains.items()}
    print(f"\n{p.name}: largest activations {', '.join(report)}; s {p.shift}, spread "
          f"{spread(p.logits):.2f}, floors " + ", ".join(f"{n} {v:.2e}" for n, v in floors.items()))
    assert min(floors.values()) >= fp.FLOOR

