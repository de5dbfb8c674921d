"""Exact probe networks for the whole-network kernels (csrc/kernels/resnet20_fused.hip and
lenet5_fused.hip): one definition shared by test_fused_probes_cpu.py (the conditions that make a
probe exact and observable, no launch) and test_fused_probes_gpu.py (the launches).

All a test sees of a fused kernel is ten probabilities per image, so the probes are networks whose
arithmetic is exact: integer activations of at most 256 (exact in bf16), weights that are exact in
bf16 / e4m3, so every fp32 partial sum is a small integer and any summation order gives the same
logits. The only slack left between the reference logits and the kernel's output is the fp32
softmax, which is what the tolerance T is worked out from.

ResNet-20: one probe per convolution. Every other conv is a *carrier* that passes non-negative
integers through unchanged (zero blocks, centre-tap identities, and 2x2 gathers in the stride-2
convs so no pixel is dropped), so every output element of the probed conv reaches the head with a
known gain. Each probe has two variants: `relu` (weights in {-1, 0, 1}, bias in {-1, 0, 1}: the
ReLU and the negative range stay honest) and `open` (the same weights with the bias raised per
channel until every pre-activation is positive: every element's value is pinned).

The head is integers in [-8, 8] over 2^s with a bias of quarters, s the smallest shift that keeps
every image's logit spread within 12 (no probability underflows, the log inversion is well
conditioned). The fp8 probes use weights of 7 * 2^k only (power-of-two row scales, codes +-448)
and power-of-two activation scales, so every value ahead of an e4m3 rounding is exact and the
rounding a deterministic function of it; their expectation is the oracle's e4m3 emulation.
LeNet-5: networks that are exact in all five layers at once, with activations small enough for
the layered plan's bf16 storage too.

Limits, inherent to observing ten numbers: a pure permutation of the last stage's 64 pixels cannot
be seen through average pooling, and the gathers distinguish row parity (different channel halves)
but sum the two columns of a cell. Gross misplacements are what the random-weight tests of
test_models_gpu.py catch; the probes exist for the single wrong element.
"""

import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from gale.models import get_model
from gale.models.graph import Conv, Head, MaxPool, pack_params, param_layout
from gale.models.quant import activation_tensors, e4m3_round, fake_quant_weight

# The arithmetic between exact logits and the output: an fp32 exp of an argument of magnitude
# <= SPREAD (argument rounding ~ 12 * 2^-24 relative plus a few ulp for the function), a sum of
# ten terms and one division: under 2e-6 in the logit. T allows five times that.
T = 1e-5
FLOOR = 20 * T          # the smallest single-element error must move a centred logit by this much
SPREAD = 12.0           # largest logit spread (max - min over the classes) of any image
MAX_ACT = 256           # integers up to here are exact in bf16
N_IMAGES = 32
VARIANTS = ("relu", "open")
DENSITY = {3: 1.0, 16: 0.3, 32: 0.12, 64: 0.06}  # share of non-zero probed weights per Cin
FP8_CARRIER_W = (0.875, 1.75, 3.5, 7.0)
FP8_UNIT = 2.0 ** -6    # every value ahead of an e4m3 rounding is a multiple of this
FP8_W = 0.875           # |probed weight| of the fp8 probes: row scale 2^-9, codes +-448


def centred(v):
    v = v.double()
    return v - v.mean(dim=1, keepdim=True)


def centred_log(p):
    """The softmax inverted: centred float64 log-probabilities."""
    return centred(p.double().clamp_min(1e-300).log())


def deviation(probs, ref_logits):
    """D of a launch: max |centred log of the kernel's probabilities - centred reference logits|."""
    return (centred_log(probs) - centred(ref_logits)).abs().max().item()


# ---- a forward with edit points -------------------------------------------------------------------

def walk(net, params, x_nhwc, fp8_scales=None, edit_conv=None, edit_res=None, start=None,
         pre=None, stop=None):
    """gale.models.reference.forward for conv / pool / head networks, restated with edit points
    (the CPU test asserts that it equals the oracle bit for bit). `edit_conv(L, y, inp)` may
    replace a conv's raw output (bias included), `edit_res(L, r)` its residual. `start`
    (tensors, layer name): resume after that layer from the given tensors. `stop`: return after
    that layer. `pre` receives every conv output as it is before the e4m3 rounding. Returns
    (logits, tensors)."""
    def q(name, v):
        if fp8_scales is None:
            return v
        s = fp8_scales[name]
        return e4m3_round(v / s) * s

    if start is None:
        t = {"input": q("input", x_nhwc.float().permute(0, 3, 1, 2))}
        skip = None
    else:
        t, skip = dict(start[0]), start[1]
    logits = None
    for L in net.layers:
        if skip is not None:
            if L.name == skip:
                skip = None
            continue
        if isinstance(L, Conv):
            w = params[f"{L.name}.weight"]
            if fp8_scales is not None:
                w = fake_quant_weight(w)
            y = F.conv2d(t[L.inp], w, params[f"{L.name}.bias"], stride=L.stride, padding=L.pad)
            if edit_conv is not None:
                y = edit_conv(L, y, t[L.inp])
            if L.residual is not None:
                r = t[L.residual]
                if L.res_mode == "pad":
                    r = r[:, :, ::2, ::2]
                    r = F.pad(r, (0, 0, 0, 0, 0, L.cout - r.shape[1]))
                if edit_res is not None:
                    r = edit_res(L, r)
                y = y + r
            if L.relu:
                y = F.relu(y)
            if pre is not None:
                pre[L.out] = y
            t[L.out] = q(L.out, y)
        elif isinstance(L, MaxPool):
            t[L.out] = F.max_pool2d(t[L.inp], L.k, L.s, L.p)
        elif isinstance(L, Head):
            pooled = t[L.inp].mean(dim=(2, 3))
            logits = pooled @ params[f"{L.name}.weight"].t() + params[f"{L.name}.bias"]
        if L.name == stop:
            break
    return logits, t


# ---- ResNet-20 -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def r20():
    return get_model("resnet20")


def r20_convs():
    return [L for L in r20().layers if isinstance(L, Conv)]


N_CONVS = 19
# The convs that have an fp8 probe. Left out: 10, 12 and 14, for which no carrier weight of the
# family keeps every value ahead of an e4m3 rounding on the FP8_UNIT grid (the probed conv's own
# sums of 0.875 * rounded carrier values fall between its points), and 9 and 11, whose last
# activations are fine-grained and large at once: the bound on the dense layer's partial sums
# (test_fused_probes_cpu.check_logits_exact) passes 2^24, so their logits are not provably the
# same in every summation order.
FP8_CONVS = tuple(i for i in range(N_CONVS) if i not in (9, 10, 11, 12, 14))


def _centre(cout, cin, src):
    w = torch.zeros(cout, cin, 3, 3)
    for co in range(cout):
        w[co, src(co), 1, 1] = 1.0
    return w


def _gather(C):
    """Stride 2, pad 1, C -> 2C: out channel co sums the two columns of one row of its 2x2 cell
    (row 0 of the cell for co < C, row 1 for co >= C) of in channel co % C."""
    w = torch.zeros(2 * C, C, 3, 3)
    for co in range(2 * C):
        kh = 1 if co < C else 2
        w[co, co % C, kh, 1] = w[co, co % C, kh, 2] = 1.0
    return w


def carrier(probe):
    """Folded conv parameters with every conv but `probe` a carrier (`probe` itself: zero)."""
    convs = r20_convs()
    p = {}
    for i, L in enumerate(convs):
        partner = 0 if i == 0 else (i + 1 if i % 2 else i - 1)
        if i == probe:
            w = torch.zeros(L.cout, L.cin, 3, 3)
        elif i == 0:
            w = _centre(16, 3, lambda c: c % 3)
        elif L.stride == 2:
            w = _gather(L.cin)
        elif convs[i - 1].stride == 2 or partner == probe:
            w = _centre(L.cout, L.cin, lambda c: c)
        else:
            w = torch.zeros(L.cout, L.cin, 3, 3)
        p[f"{L.name}.weight"] = w
        p[f"{L.name}.bias"] = torch.zeros(L.cout)
    return p


def carrier_x3(x_nhwc, probe):
    """What the carrier makes of an image when conv `probe` is zero, from its definition: the
    stem copy, then per stride-2 block the row gathers (absent when the probed conv is one of that
    block's two) plus the option-A shortcut. [N, 64, 8, 8]."""
    img = x_nhwc.float().permute(0, 3, 1, 2)
    x = img[:, [c % 3 for c in range(16)]] * float(probe != 0)
    for down in (7, 13):
        pair = (x[:, :, :, 0::2] + x[:, :, :, 1::2]) * float(probe not in (down, down + 1))
        out = torch.cat([pair[:, :, 0::2], pair[:, :, 1::2]], dim=1)
        out[:, : x.shape[1]] += x[:, :, 0::2, 0::2]
        x = out
    return x


def unpack_conv(net, buf, L):
    """Read conv L's bf16 weights [cout, cin, k, k] and bias back out of a packed bf16 buffer;
    everything else of the two entries must be zero padding."""
    layout = param_layout(net, "bf16")[0]
    ew, eb = layout[f"{L.name}.w"], layout[f"{L.name}.b"]
    flat = buf[ew.offset: ew.offset + ew.nbytes].view(torch.bfloat16).float().view(ew.shape)
    cin_s = L.cin if L.inp == "input" else (L.cin + 7) // 8 * 8
    K = L.k * L.k * cin_s
    w = flat[: L.cout, :K].reshape(L.cout, L.k, L.k, cin_s)
    assert not flat[L.cout:].any() and not flat[:, K:].any() and not w[..., L.cin:].any()
    b = buf[eb.offset: eb.offset + eb.nbytes].view(torch.float32)
    assert not b[L.cout:].any()
    return w[..., : L.cin].permute(0, 3, 1, 2), b[: L.cout]


def probe_weights(i, seed=None):
    """Weights in {-1, 0, 1} (every row non-zero) and a bias in {-1, 0, 1} for conv i."""
    L = r20_convs()[i]
    g = torch.Generator().manual_seed(1000 + i if seed is None else seed)
    w = torch.randint(0, 2, (L.cout, L.cin, 3, 3), generator=g).float() * 2 - 1
    w = torch.where(torch.rand(w.shape, generator=g) < DENSITY[L.cin], w, torch.zeros(()))
    for co in range(L.cout):
        if not w[co].any():
            w[co, co % L.cin, 1, 1] = 1.0
    b = torch.randint(-1, 2, (L.cout,), generator=g).float()
    return w, b


def head_ints(seed, pooled, lo=4):
    """fc weight integers in [-8, 8] and a bias of quarters for a head over `pooled` [N, C].

    The logits must stay within SPREAD although the pooled values are large, and the shift that
    scales them down also scales every element's gain, so the head is built to cancel the part of
    the pooled vector that carries no information: channels are paired by their mean over the
    images (neighbours in sorted order), and a pair gets a random column and its negative. What
    reaches the logits is the difference of two channels of like mean. Every column's largest
    centred entry is >= lo (a constant column would vanish when the logits are centred)."""
    g = torch.Generator().manual_seed(seed)
    C = pooled.shape[1]
    order = torch.argsort(pooled.double().mean(0), stable=True).tolist()
    w = torch.zeros(10, C)
    for a, b in zip(order[0::2], order[1::2]):
        while True:
            col = torch.randint(-8, 9, (10,), generator=g).float()
            if (col - col.mean()).abs().max() >= lo:
                break
        w[:, a], w[:, b] = col, -col
    return w, torch.randint(-8, 9, (10,), generator=g).float() / 4


def attach_head(net, folded, x, seed, fp8_scales=None):
    """Add the head to `folded`: head_ints over the network's own pooled values, and the smallest
    shift s for which every image's logit spread is <= SPREAD. Returns (s, logits)."""
    H = net.layers[-1]
    cin = net.shapes[H.inp][2]
    folded[f"{H.name}.weight"], folded[f"{H.name}.bias"] = torch.zeros(10, cin), torch.zeros(10)
    _, t = walk(net, folded, x, fp8_scales=fp8_scales)
    hw, hb = head_ints(seed, t[H.inp].mean(dim=(2, 3)))
    folded[f"{H.name}.bias"] = hb
    for s in range(24):
        folded[f"{H.name}.weight"] = hw / 2.0 ** s
        logits = walk(net, folded, x, fp8_scales=fp8_scales, start=(t, net.layers[-2].name))[0]
        if (logits.amax(1) - logits.amin(1)).max().item() <= SPREAD:
            return s, logits
    raise AssertionError("no head shift keeps the logit spread in range")


def r20_images(i):
    g = torch.Generator().manual_seed(7000 + i)
    return torch.randint(0, 2, (N_IMAGES, 32, 32, 3), generator=g).float()


def _conv_only(L, w, t):
    return F.conv2d(t[L.inp], w, None, stride=L.stride, padding=L.pad)


@functools.lru_cache(maxsize=None)
def r20_probe(i, variant):
    """The bf16 probe of conv i: folded parameters, images, head shift and reference logits."""
    net, L = r20(), r20_convs()[i]
    x = r20_images(i)
    folded = carrier(i)
    w, b = probe_weights(i)
    if variant == "open":
        _, t = walk(net, dict(folded, **{"fc.weight": torch.zeros(10, 64),
                                          "fc.bias": torch.zeros(10)}), x)
        b = 1.0 - _conv_only(L, w, t).amin(dim=(0, 2, 3))
    folded[f"{L.name}.weight"], folded[f"{L.name}.bias"] = w, b
    s, logits = attach_head(net, folded, x, 9000 + i)
    return SimpleNamespace(conv=i, layer=L, variant=variant, folded=folded, x=x, shift=s,
                           logits=logits, name=f"conv{i}:{L.name}:{variant}")


def r20_probes():
    return [r20_probe(i, v) for i in range(N_CONVS) for v in VARIANTS]


@functools.lru_cache(maxsize=None)
def r20_packed(i, variant):
    return pack_params(r20(), r20_probe(i, variant).folded, "bf16")


# ---- ResNet-20, fp8 ---------------------------------------------------------------------------------

def fp8_scale_exponents():
    """One power-of-two scale per activation tensor, the same for every probe (the plan carries
    the scales as launch constants, so one replica serves all probes): neighbouring tensors get
    different exponents, so a scale taken from the wrong tensor shows; each is raised until no
    probe's activation comes within a factor two of the +-448 saturation."""
    return _fp8_scales()[0]


@functools.lru_cache(maxsize=None)
def _fp8_scales():
    net = r20()
    names = activation_tensors(net)
    amax = dict.fromkeys(names, 0.0)
    for i in range(N_CONVS):  # (all of them: the scales do not depend on which are left out)
        for v in VARIANTS:
            folded, x = _fp8_folded(i, v)
            _, t = walk(net, folded, x)
            for n in names:
                amax[n] = max(amax[n], float(t[n].abs().max()))
    exps = {}
    for j, n in enumerate(names):
        e = (0, -1, 1, -2)[j % 4]
        while amax[n] / 2.0 ** e >= 224.0:
            e += 1
        exps[n] = e
    return exps, {n: 2.0 ** e for n, e in exps.items()}


@functools.lru_cache(maxsize=None)
def _fp8_folded(i, variant):
    """Conv parameters of the fp8 probe of conv i (head still zero). The probed weights are
    +-0.875. A carrier weight of 1.0 would get the row scale fl(1/448), and 448 * fl(1/448) * n
    is not n in fp32, so every carrier weight is 7 * 2^k as well (row scale 2^(k-6), code 448):
    per carrier conv the smallest of 0.875, 1.75, 3.5, 7 for which every value ahead of the e4m3
    rounding is a multiple of FP8_UNIT. The carrier then scales what it carries and rounds it to
    e4m3, deterministically from exact values; the emulation is the expectation."""
    net, convs = r20(), r20_convs()
    x = r20_images(i)
    folded = carrier(i)
    folded["fc.weight"], folded["fc.bias"] = torch.zeros(10, 64), torch.zeros(10)
    ones = dict.fromkeys(activation_tensors(net), 1.0)  # (power-of-two scales: the same values)
    t, prev = {"input": x.permute(0, 3, 1, 2)}, None
    for j, L in enumerate(convs):
        name = f"{L.name}.weight"
        tries = [1.0]
        if j == i:
            w, b = probe_weights(i)
            w = w * FP8_W
            if variant == "open":
                b = torch.ceil(1.0 - _conv_only(L, w, t).amin(dim=(0, 2, 3)))
            folded[name], folded[f"{L.name}.bias"] = w, b
        elif folded[name].any():
            tries = FP8_CARRIER_W
        pattern = folded[name]
        for m in tries:
            folded[name] = pattern * m
            pre = {}
            start = None if prev is None else (t, prev)
            nxt = walk(net, folded, x, fp8_scales=ones, start=start, stop=L.name, pre=pre)[1]
            v = pre[L.out] / FP8_UNIT
            if bool((v == v.round()).all()):
                break
        t, prev = nxt, L.name
    return folded, x


@functools.lru_cache(maxsize=None)
def r20_fp8_probe(i, variant):
    net, L = r20(), r20_convs()[i]
    folded, x = _fp8_folded(i, variant)
    folded = dict(folded)
    scales = _fp8_scales()[1]
    s, logits = attach_head(net, folded, x, 9000 + i, fp8_scales=scales)
    return SimpleNamespace(conv=i, layer=L, variant=variant, folded=folded, x=x, shift=s,
                           logits=logits, scales=scales, name=f"fp8:conv{i}:{L.name}:{variant}")


@functools.lru_cache(maxsize=None)
def r20_fp8_packed(i, variant):
    """pack_params' fp8 buffer with the calibrated activation scales overwritten by the probes'
    powers of two."""
    net = r20()
    buf = pack_params(net, r20_fp8_probe(i, variant).folded, "fp8")
    e = param_layout(net, "fp8")[0]["act_scales"]
    sc = _fp8_scales()[1]
    raw = torch.tensor([sc[n] for n in activation_tensors(net)], dtype=torch.float32)
    buf[e.offset: e.offset + e.nbytes] = raw.view(torch.uint8)
    return buf


# ---- LeNet-5 -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def lenet():
    return get_model("lenet5")


LENET_SEEDS = (2, 3, 5)  # (of 0..7, the first three whose probes meet every CPU condition)
LENET_BATCHES = (1, 13, 257)
LENET_QUANTILE = {"conv1": 0.4, "conv2": 0.85, "fc1": 0.93, "fc2": 0.93}
LENET_DENSITY = {"conv1": 1.0, "conv2": 0.5, "fc1": 0.12, "fc2": 0.2}
LENET_PIXELS = (0.92, 0.06, 0.015, 0.005)  # share of image values 0, 1, 2, 3
LENET_POOL = (4000, 1500, 600, 257)  # images drawn, then kept round by round


@functools.lru_cache(maxsize=None)
def lenet_probe(seed):
    """A LeNet-5 that is exact in all five layers, in the fused kernel (fp32 activations) and in
    the layered plan (bf16 activations) alike: integer weights in [-2, 2] and integer biases for
    the convs and fc1 / fc2, fc3 integers over 2^s, images in {0..3}, and every activation an
    integer of at most 256, which bf16 holds.

    Weights of +-2 over fan-ins of 150 / 400 / 120 multiply the activations from layer to layer
    (uniform weights and images reach 10^5 at fc2: the layered plan would round them, and the
    head shift that absorbs them would push the last layer's gain below FLOOR). Four things keep
    them small: each channel's bias is the negated quantile of its own pre-activation over the
    images (most outputs are closed by the ReLU, the open ones are the tail above the quantile,
    and every element is still open in some image: the CPU test asserts it); conv2, fc1 and fc2
    keep a share of their weights (LENET_DENSITY); the images are mostly zero (LENET_PIXELS);
    and the 257 images are the calmest of a larger draw: round by round the images with the
    smallest peak activation are kept and the biases taken again (LENET_POOL)."""
    net = lenet()
    g = torch.Generator().manual_seed(300 + seed)
    u = torch.rand((LENET_POOL[0], 28, 28, 1), generator=g)
    x = (u[..., None] >= torch.tensor(LENET_PIXELS).cumsum(0)[:3]).sum(-1).float()
    weights = {}
    for L in net.layers:
        if isinstance(L, Conv):
            w = torch.randint(-2, 3, (L.cout, L.cin, L.k, L.k), generator=g).float()
            weights[L.name] = torch.where(
                torch.rand(w.shape, generator=g) < LENET_DENSITY[L.name], w, torch.zeros(()))
    for r in range(len(LENET_POOL)):
        folded = {}
        cur = x.permute(0, 3, 1, 2)
        peak = torch.zeros(len(x))
        for L in net.layers:
            if isinstance(L, Conv):
                w = weights[L.name]
                y = F.conv2d(cur, w, None, stride=L.stride, padding=L.pad)
                per_channel = y.transpose(0, 1).flatten(1)
                per_channel = per_channel[:, ::max(1, per_channel.shape[1] // 100000)]
                b = -torch.quantile(per_channel, LENET_QUANTILE[L.name], dim=1).floor()
                folded[f"{L.name}.weight"], folded[f"{L.name}.bias"] = w, b
                cur = F.relu(y + b.view(1, -1, 1, 1))
                peak = torch.maximum(peak, cur.flatten(1).amax(1))
            elif isinstance(L, MaxPool):
                cur = F.max_pool2d(cur, L.k, L.s, L.p)
        if r + 1 < len(LENET_POOL):
            x = x[peak.argsort(stable=True)[: LENET_POOL[r + 1]].sort().values]
    s, logits = attach_head(net, folded, x, 400 + seed)
    return SimpleNamespace(seed=seed, folded=folded, x=x, shift=s, logits=logits,
                           name=f"lenet5:seed{seed}")


@functools.lru_cache(maxsize=None)
def lenet_packed(seed):
    return pack_params(lenet(), lenet_probe(seed).folded, "bf16")


# ---- observability (autograd on the reference) -----------------------------------------------------

def r20_gains(p):
    """For the probed conv of a bf16 probe: (activation gains [Cout, Ho, Wo], weight gains
    [Cout, Cin, 3, 3]): the largest |d centred logit / d element| over the classes and over the
    images (for an output element: the images in which it is positive)."""
    net, L = r20(), p.layer
    params = dict(p.folded)
    w = params[f"{L.name}.weight"].clone().requires_grad_(True)
    params[f"{L.name}.weight"] = w
    logits, t = walk(net, params, p.x)
    cl = logits - logits.mean(dim=1, keepdim=True)
    out = t[L.out]
    is_open = (out > 0).float()
    # per-image weight gradients by the chain rule from the gradient at the conv's output (out =
    # relu(pre), d pre / d w = the input patch), checked against autograd's sum over the images
    patches = F.unfold(t[L.inp].detach(), 3, padding=1, stride=L.stride).transpose(1, 2)
    act = torch.zeros(out.shape[1:])
    wgt = torch.zeros(w.shape[0], w[0].numel())
    for k in range(10):
        g_out, g_w = torch.autograd.grad(cl[:, k].sum(), [out, w], retain_graph=True)
        g_pre = g_out * is_open
        act = torch.maximum(act, g_pre.abs().amax(0))
        per_image = torch.bmm(g_pre.flatten(2), patches)
        # (fp32 sums in another order: the centring by 1/10 leaves the dyadic numbers)
        assert (per_image.sum(0) - g_w.flatten(1)).abs().max() <= 1e-4 * g_w.abs().max()
        wgt = torch.maximum(wgt, per_image.abs().amax(0))
    return act, wgt.view_as(w)


def lenet_gains(p):
    """{layer: largest |d centred logit / d element| over the classes and the images in which
    the element is positive} for the output of every layer before the head."""
    net = lenet()
    x = p.x.clone().requires_grad_(True)  # (only to have a graph)
    logits, t = walk(net, p.folded, x)
    cl = logits - logits.mean(dim=1, keepdim=True)
    outs = [L.out for L in net.layers if isinstance(L, Conv)]
    gains = {n: torch.zeros(t[n].shape[1:]) for n in outs}
    for k in range(10):
        gs = torch.autograd.grad(cl[:, k].sum(), [t[n] for n in outs], retain_graph=True)
        for n, g in zip(outs, gs):
            gains[n] = torch.maximum(gains[n], (g.abs() * (t[n] > 0)).amax(0))
    return gains


def e4m3_step_up(v, scale):
    """The next e4m3 value above v >= 0 at `scale` (v is on the grid), minus v."""
    code = (v / scale).to(torch.float8_e4m3fn).view(torch.uint8)
    return (code + 1).view(torch.float8_e4m3fn).float() * scale - v


def fp8_observed(p, n_sample=256, rounds=(2, 10)):
    """For a fixed sample of the probed conv's output elements (the same for both variants):
    whether raising the element by one e4m3 step moves a centred logit of the emulation by
    FLOOR in some image. (The coarse grid lets some changes round away downstream, so for fp8
    observability is established on the emulation itself, by perturbation.) The images are tried
    in the order of the element's value, largest first: rounds[0] of them for every element, then
    rounds[1] more for the elements not seen yet."""
    net, L = r20(), p.layer
    logits, t = walk(net, p.folded, p.x, fp8_scales=p.scales)
    out = t[L.out].flatten(1)
    g = torch.Generator().manual_seed(5000 + p.conv)
    sample = torch.randperm(out.shape[1], generator=g)[:n_sample]
    ranked = out[:, sample].argsort(dim=0, descending=True, stable=True)  # [images, n]
    seen = torch.zeros(n_sample, dtype=torch.bool)
    first = 0
    for k in rounds:
        todo = (~seen).nonzero().flatten()
        if len(todo) == 0:
            break
        imgs = ranked[first: first + k, todo].t().reshape(-1)
        el = sample[todo].repeat_interleave(k)
        sub = {n: v[imgs] for n, v in t.items()}
        flat = sub[L.out].flatten(1).clone()
        rows = torch.arange(len(el))
        flat[rows, el] += e4m3_step_up(flat[rows, el], p.scales[L.out])
        sub[L.out] = flat.view_as(sub[L.out])
        moved = walk(net, p.folded, None, fp8_scales=p.scales, start=(sub, L.name))[0]
        hit = (centred(moved) - centred(logits[imgs])).abs().amax(1) >= FLOOR
        seen[todo] |= hit.view(-1, k).any(1)
        first += k
    return seen
