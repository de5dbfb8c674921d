"""Antialiased input resize (--input-antialias) without a GPU: the tap tables against an
independent derivation with rationals and against the native builder, the numpy oracle against
exact rational arithmetic with one rounding per stated operation, the host twin against the
oracle, a crop as a bit copy, a sanity bound against torch's antialiased bilinear interpolation,
configuration sources and refusals, the stub engine end to end, and the stand-alone sanitizer
driver."""

import base64
import json
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gale._native import native
from gale.cli import parse_topology_args
from gale.config import GaleConfig, from_sources
from gale.models.preprocess import InputPrep, InputResize

C = native()
K = C.kafka
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CIFAR_MEAN_S = "0.4914,0.4822,0.4465"
CIFAR_STD_S = "0.2470,0.2435,0.2616"

# (HS, WS, HR, WR, H, W, C): the kernel test's shapes (tests/test_input_antialias_gpu.py)
KERNEL_SHAPES = [
    (40, 36, 34, 33, 32, 32, 3),     # mild downscale, taps <= 3, 16-byte stores
    (64, 48, 36, 34, 32, 32, 3),     # taps 4 / 3
    (57, 45, 30, 29, 28, 28, 1),     # C = 1
    (20, 48, 32, 34, 32, 32, 3),     # up on rows, down on columns
    (5, 7, 32, 33, 32, 32, 3),       # upscale, edge entries of one tap
    (40, 36, 40, 36, 32, 32, 3),     # crop: a bit copy
    (23, 17, 9, 11, 6, 7, 3),        # 21-float rows, per-float stores
    (64, 40, 8, 5, 8, 4, 2),         # exactly 8x on both axes, 16-17 taps, C = 2
    (70, 150, 36, 100, 32, 96, 3),   # output row of 288 floats > one span, rows > one band
]
CROP = (40, 36, 40, 36, 32, 32, 3)


def f32_round(x: Fraction) -> np.float32:
    """The binary32 nearest to the rational x, ties to even."""
    if x == 0:
        return np.float32(0.0)
    sign = -1 if x < 0 else 1
    x = abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    if e < -126:
        m, e = round(x / Fraction(2) ** -149), -149
        return np.float32(sign * math.ldexp(m, e))
    m = round(x / Fraction(2) ** (e - 23))
    if e > 127 or (m == 1 << 24 and e == 127):
        return np.float32(sign * math.inf)
    return np.float32(sign * math.ldexp(m, e - 23))


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def random_images(rng, n, HS, WS, Ch):
    """fp32 values of both signs over several binades (so the roundings are not trivial)."""
    x = rng.standard_normal((n, HS, WS, Ch)) * 10.0 ** rng.integers(-2, 3, (n, HS, WS, Ch))
    return x.astype(np.float32)


# ---- 1. tables ---------------------------------------------------------------------------------

def axis_by_fractions(n_src, n_rs, n_out):
    """The triangle filter in source coordinates: output pixel i of the resized axis has its
    centre at (i + off + 1/2) * n_src / n_rs; with the support scale s = max(n_src / n_rs, 1)
    source pixel k (centre k + 1/2) has the weight 1 - |k + 1/2 - centre| / s where that is
    positive. u is that weight times 2 * max(n_src, n_rs), an integer (asserted against the
    rational), and the table's weight np.float32(u / U) on Python ints."""
    off = (n_rs - n_out) // 2
    scale = max(Fraction(n_src, n_rs), Fraction(1))
    S = max(n_src, n_rs)
    start, count, ws = [], [], []
    for i in range(n_out):
        centre = Fraction(2 * (i + off) + 1, 2) * Fraction(n_src, n_rs)
        tri = [1 - abs(Fraction(2 * k + 1, 2) - centre) / scale for k in range(n_src)]
        taps = [k for k in range(n_src) if tri[k] > 0]
        assert taps and taps == list(range(taps[0], taps[-1] + 1))
        # the definition's integer is the rational triangle times 2 S: checked, not assumed
        u = [2 * S - abs((2 * k + 1) * n_rs - (2 * (i + off) + 1) * n_src) for k in taps]
        assert all(Fraction(v, 2 * S) == tri[k] for v, k in zip(u, taps))
        U = sum(u)
        assert U <= 1 << 26
        start.append(taps[0]), count.append(len(taps))
        ws.extend(np.float32(v / U) for v in u)
    return np.array(start, np.int32), np.array(count, np.int32), np.array(ws, np.float32)


TABLE_DIMS = KERNEL_SHAPES + [(375, 500, 256, 341, 224, 224, 3), (4096, 4095, 512, 512, 1, 2, 1),
                              (1, 2, 4096, 4095, 4096, 4095, 1), (20, 24, 32, 32, 32, 32, 3)]


@pytest.mark.parametrize("dims", TABLE_DIMS, ids=lambda d: "x".join(map(str, d[:6])))
def test_tables_match_rational_derivation_and_native_builder(dims):
    HS, WS, HR, WR, H, W, _ = dims
    got = InputResize(HS, WS, HR, WR, H, W, antialias=True).aa_tables()
    want = axis_by_fractions(HS, HR, H) + axis_by_fractions(WS, WR, W)
    nat = C.build_resize_aa_tables(HS, WS, HR, WR, H, W)
    assert len(got) == len(nat) == 6
    for g, w, n in zip(got, want, nat):
        assert g.dtype == w.dtype == n.dtype and g.shape == w.shape == n.shape
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
        assert np.array_equal(g.view(np.uint32), n.view(np.uint32))
    for s, n, w, n_src, n_out in ((got[0], got[1], got[2], HS, H), (got[3], got[4], got[5], WS, W)):
        assert s.shape == n.shape == (n_out,) and w.shape == (n.sum(),)
        assert (s >= 0).all() and (s + n <= n_src).all() and (n >= 1).all() and (n <= 17).all()
        assert (w > 0).all() and (w <= 1).all()
        assert (np.diff(s) >= 0).all() and (np.diff(s + n) >= 0).all()
        # each entry's weights sum to 1 up to rounding
        offs = np.concatenate(([0], np.cumsum(n)[:-1]))
        sums = np.add.reduceat(w.astype(np.float64), offs)
        assert np.abs(sums - 1).max() <= 17 * 2.0 ** -24


def test_tables_non_shrinking_axis_has_the_lerp_forms_taps():
    """On an axis that does not shrink S = n_rs: the taps are the two pixels of the bilinear form
    (one at an edge) and the weights its 1 - w, w up to the rounding of the division."""
    for n_src, n_rs, n_out in ((5, 32, 32), (20, 32, 32), (7, 33, 32), (36, 36, 32)):
        rs = InputResize(n_src, n_src, n_rs, n_rs, n_out, n_out, antialias=True)
        s, n, w = rs.aa_tables()[:3]
        i0, i1, lw = InputResize(n_src, n_src, n_rs, n_rs, n_out, n_out).tables()[:3]
        o = 0
        for i in range(n_out):
            if n[i] == 1:
                assert lw[i] == 0 and s[i] == i0[i] and w[o] == 1
            else:
                assert n[i] == 2 and s[i] == i0[i] and s[i] + 1 == i1[i]
                assert abs(float(w[o + 1]) - float(lw[i])) <= 2.0 ** -24
            o += n[i]


# ---- 2. the oracle and the host twin -----------------------------------------------------------

def taps_exact(vals, ws):
    """One axis' tap sum: a single tap is the value itself; else one rounding for the multiply and
    one per fma, ascending."""
    if len(vals) == 1:
        return vals[0]
    acc = f32_round(Fraction(float(ws[0])) * Fraction(float(vals[0])))
    for v, w in zip(vals[1:], ws[1:]):
        acc = f32_round(Fraction(float(w)) * Fraction(float(v)) + Fraction(float(acc)))
    return acc


def apply_by_fractions(x, dims):
    HS, WS, HR, WR, H, W, Ch = dims
    ys, yn, wy = axis_by_fractions(HS, HR, H)
    xs, xn, wx = axis_by_fractions(WS, WR, W)
    xo = np.concatenate(([0], np.cumsum(xn)))
    yo = np.concatenate(([0], np.cumsum(yn)))
    t = np.zeros((HS, W, Ch), np.float32)  # the column stage, rounded to binary32
    for r in range(ys.min(), (ys + yn).max()):
        for xx in range(W):
            for c in range(Ch):
                t[r, xx, c] = taps_exact([x[r, xs[xx] + k, c] for k in range(xn[xx])],
                                         wx[xo[xx]:xo[xx + 1]])
    out = np.zeros((H, W, Ch), np.float32)
    for y in range(H):
        for xx in range(W):
            for c in range(Ch):
                out[y, xx, c] = taps_exact([t[ys[y] + k, xx, c] for k in range(yn[y])],
                                           wy[yo[y]:yo[y + 1]])
    return out


ORACLE_SHAPES = [(40, 36, 34, 33, 32, 32, 3), (57, 45, 30, 29, 28, 28, 1),
                 (20, 48, 32, 34, 32, 32, 3), (5, 7, 32, 33, 32, 32, 3),
                 (23, 17, 9, 11, 6, 7, 3), (64, 40, 8, 5, 8, 4, 2)]


@pytest.mark.parametrize("dims", ORACLE_SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_oracle_is_one_rounding_per_operation_and_host_twin_matches(dims):
    HS, WS, HR, WR, H, W, Ch = dims
    rs = InputResize(HS, WS, HR, WR, H, W, antialias=True)
    x = random_images(np.random.default_rng(HS * 100 + WS), 3, HS, WS, Ch)
    got = rs.apply(x)
    assert got.shape == (3, H, W, Ch) and got.dtype == np.float32
    want0 = apply_by_fractions(x[0], dims)
    assert np.array_equal(u32(got[0]), u32(want0))
    host = C.resize_crop_aa_host(x, HR, WR, H, W)
    assert host.shape == got.shape and np.array_equal(u32(host), u32(got))
    # torch tensors go through the same oracle
    assert np.array_equal(u32(rs.apply(torch.from_numpy(x)).numpy()), u32(got))
    # and it is another function than the option without antialiasing wherever an axis shrinks
    if HS > HR or WS > WR:
        assert not np.array_equal(u32(got), u32(InputResize(HS, WS, HR, WR, H, W).apply(x)))


@pytest.mark.parametrize("dims", [d for d in KERNEL_SHAPES if d not in ORACLE_SHAPES],
                         ids=lambda d: "x".join(map(str, d)))
def test_host_twin_matches_the_oracle_on_the_other_kernel_shapes(dims):
    HS, WS, HR, WR, H, W, Ch = dims
    x = random_images(np.random.default_rng(HS * 100 + WS), 2, HS, WS, Ch)
    got = InputResize(HS, WS, HR, WR, H, W, antialias=True).apply(x)
    assert np.array_equal(u32(C.resize_crop_aa_host(x, HR, WR, H, W)), u32(got))


def test_crop_is_a_bit_copy_also_next_to_max_nan_inf_and_negative_zero():
    HS, WS, HR, WR, H, W, Ch = CROP
    rs = InputResize(HS, WS, HR, WR, H, W, antialias=True)
    x = random_images(np.random.default_rng(3), 2, HS, WS, Ch)
    nan_payload = np.array([0x7fa12345], np.uint32).view(np.float32)[0]
    # inside the window (rows 4..35, columns 2..33) and right outside it
    for (i, y, xx, c, v) in [(0, 3, 5, 0, 3.4e38), (0, 4, 5, 0, -3.4e38), (0, 4, 6, 1, np.nan),
                             (0, 36, 7, 2, np.nan), (1, 10, 1, 0, 3.4e38), (1, 10, 2, 0, -3.4e38),
                             (1, 35, 34, 1, np.nan), (1, 35, 33, 1, -3.4e38),
                             (1, 20, 20, 2, np.inf), (1, 20, 21, 2, -np.inf), (0, 3, 9, 1, np.inf),
                             (0, 9, 9, 0, -0.0), (0, 9, 1, 0, -0.0), (1, 5, 5, 1, nan_payload)]:
        x[i, y, xx, c] = v
    want = x[:, 4:36, 2:34]
    assert np.array_equal(u32(rs.apply(x)), u32(want))
    assert np.array_equal(u32(C.resize_crop_aa_host(x, HR, WR, H, W)), u32(want))
    _, yn, wy, _, xn, wx = rs.aa_tables()
    assert (yn == 1).all() and (xn == 1).all() and (wy == 1).all() and (wx == 1).all()


TORCH_SHAPES = [(375, 500, 256, 341, 224, 224, 3), (40, 36, 32, 32, 32, 32, 3),
                (64, 48, 36, 34, 32, 32, 3), (57, 45, 30, 29, 28, 28, 1),
                (100, 13, 33, 35, 32, 32, 3), CROP, (512, 512, 256, 256, 224, 224, 3),
                (20, 24, 32, 32, 32, 32, 3)]
EXACT = {CROP, (512, 512, 256, 256, 224, 224, 3), (20, 24, 32, 32, 32, 32, 3)}


@pytest.mark.parametrize("dims", TORCH_SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_close_to_torch_antialiased_bilinear(dims):
    HS, WS, HR, WR, H, W, Ch = dims
    x = np.random.default_rng(11).integers(0, 256, (1, HS, WS, Ch)).astype(np.float32)
    got = InputResize(HS, WS, HR, WR, H, W, antialias=True).apply(x)
    t = F.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), size=(HR, WR), mode="bilinear",
                      align_corners=False, antialias=True).permute(0, 2, 3, 1).numpy()
    oy, ox = (HR - H) // 2, (WR - W) // 2
    err = float(np.abs(got - t[:, oy:oy + H, ox:ox + W]).max())
    bound = float(np.abs(x).max()) * max(HS, WS) * 2.0 ** -20
    print(f"{dims}: max |oracle - torch| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    if dims in EXACT:
        assert err == 0.0


def test_builders_refuse_over_the_limit_and_bad_dimensions():
    x = np.zeros((1, 5, 7, 3), np.float32)
    for hr, wr, h, w in [(3, 8, 4, 4), (8, 3, 4, 4), (4097, 8, 4, 4), (8, 8, 0, 4)]:
        with pytest.raises(ValueError):
            C.resize_crop_aa_host(x, hr, wr, h, w)
    with pytest.raises(ValueError):
        C.build_resize_aa_tables(0, 4, 4, 4, 4, 4)
    for dims in [(33, 4, 4, 4, 4, 4), (4, 33, 4, 4, 4, 4), (4096, 4096, 511, 512, 2, 2)]:
        with pytest.raises(ValueError):
            C.build_resize_aa_tables(*dims)
        with pytest.raises(ValueError):
            C.build_resize_aa_tables(*dims, device=True)
        with pytest.raises(ValueError, match="input_antialias"):
            InputResize(*dims, antialias=True).aa_tables()
    C.build_resize_aa_tables(32, 32, 4, 4, 4, 4)  # exactly 8x


def test_device_layout_of_the_tables():
    """The kernel's layout: weights with a fixed stride per axis, zero after the last tap, and the
    launch figures (largest tap counts, band height, LDS rows of a band)."""
    for dims in KERNEL_SHAPES:
        HS, WS, HR, WR, H, W, _ = dims
        ys, yn, wy, xs, xn, wx = C.build_resize_aa_tables(HS, WS, HR, WR, H, W)
        dys, dyn, dwy, dxs, dxn, dwx, ty, tx, band, rows = C.build_resize_aa_tables(
            HS, WS, HR, WR, H, W, device=True)
        assert np.array_equal(ys, dys) and np.array_equal(yn, dyn)
        assert np.array_equal(xs, dxs) and np.array_equal(xn, dxn)
        assert (ty, tx) == (yn.max(), xn.max())
        for n, w, dw, t in ((yn, wy, dwy, ty), (xn, wx, dwx, tx)):
            dw = dw.reshape(len(n), t)
            mask = np.arange(t)[None, :] < n[:, None]
            assert np.array_equal(dw[mask].view(np.uint32), w.view(np.uint32))
            assert (dw[~mask] == 0).all()
        assert band in (1, 2, 4, 8) and rows + tx <= 64
        need = max(ys[min(y + band, H) - 1] + yn[min(y + band, H) - 1] - ys[y]
                   for y in range(0, H, band))
        assert rows == need
    assert C.build_resize_aa_tables(64, 40, 8, 5, 8, 4, device=True)[8] == 4  # 8x: a lower band


# ---- 3. configuration --------------------------------------------------------------------------

def test_config_sources_and_precedence(tmp_path):
    cli = parse_topology_args(["t", "in", "out", "--input-size", "40,36", "--input-resize",
                               "34,33", "--input-antialias"])
    assert cli.input_antialias is True
    rs = cli.input_resize_plan()
    assert (rs.HS, rs.WS, rs.HR, rs.WR, rs.H, rs.W) == (40, 36, 34, 33, 32, 32)
    assert rs.active and rs.antialias
    off = parse_topology_args(["t", "in", "out", "--input-size", "40,36"])
    assert off.input_antialias is False and not off.input_resize_plan().antialias
    base = dict(topology_name="t", input_topic="in", output_topic="out")
    env = from_sources(cli=base, env={"GALE_INPUT_SIZE": "30,33", "GALE_INPUT_ANTIALIAS": "1",
                                      "GALE_MODEL": "lenet5"})
    assert env.input_antialias is True and env.input_resize_plan().antialias
    toml = tmp_path / "gale.toml"
    toml.write_text('[gale]\ninput-size = "48,40"\ninput-antialias = true\n')
    t = from_sources(cli=base, env={}, toml_path=str(toml))
    assert t.input_antialias is True and t.validate().input_resize_plan().antialias
    # CLI > env > TOML
    e = from_sources(cli=base, env={"GALE_INPUT_ANTIALIAS": "0"}, toml_path=str(toml))
    assert e.input_antialias is False
    c = from_sources(cli=dict(base, input_antialias=True), env={"GALE_INPUT_ANTIALIAS": "0"},
                     toml_path=str(toml))
    assert c.input_antialias is True
    d = cli.engine_dict(32, 32, 3, 10)
    assert (d["rec_H"], d["rec_W"], d["resize_H"], d["resize_W"]) == (40, 36, 34, 33)
    assert d["resize_antialias"] == 1
    assert "resize_antialias" not in off.engine_dict(32, 32, 3, 10)


def test_engine_entries():
    on = InputResize.build(32, 32, "40,36", "34,33", antialias=True)
    assert on.engine_entries() == dict(rec_H=40, rec_W=36, resize_H=34, resize_W=33,
                                       resize_antialias=1)
    off = InputResize.build(32, 32, "40,36", "34,33")
    assert off.antialias is False
    assert off.engine_entries() == dict(rec_H=40, rec_W=36, resize_H=34, resize_W=33)


@pytest.mark.parametrize("kw", [
    dict(),                                            # no resize at all
    dict(input_size="32,32", input_resize="32,32"),    # every size the model's: inactive
    dict(input_resize="32"),
    dict(input_size="264,36"),                         # 264 > 8 * 32 rows
    dict(input_size="40,300", input_resize="34,33"),   # 300 > 8 * 33 columns
])
def test_refusals_name_the_option(kw):
    with pytest.raises(ValueError, match="--input-antialias"):
        GaleConfig(topology_name="t", input_antialias=True, **kw).validate()
    GaleConfig(topology_name="t", **kw).validate()  # fine without the option
    with pytest.raises(ValueError, match="input_antialias"):
        InputResize.build(32, 32, kw.get("input_size", ""), kw.get("input_resize", ""),
                          antialias=True)


def test_exactly_eight_times_is_accepted():
    GaleConfig(topology_name="t", input_antialias=True, input_size="256,256").validate()
    # Resize(32) on 400 x 40 is 320 x 32: within the limit on both axes
    rs = GaleConfig(topology_name="t", input_antialias=True, input_size="400,40",
                    input_resize="32").validate().input_resize_plan()
    assert (rs.HR, rs.WR) == (320, 32) and rs.antialias


def test_native_engine_config_refuses_the_same():
    base = GaleConfig(topology_name="t", input_topic="in", output_topic="out", stub=True,
                      input_size="40,36").validate().engine_dict(32, 32, 3, 10)
    C.Engine(dict(base, resize_antialias=1))
    with pytest.raises(ValueError):
        C.Engine(dict(base, rec_H=264, resize_antialias=1))
    inactive = {k: v for k, v in base.items() if k not in ("rec_H", "rec_W", "resize_H",
                                                            "resize_W")}
    with pytest.raises(ValueError):
        C.Engine(dict(inactive, resize_antialias=1))


# ---- 4. stub engine end to end -----------------------------------------------------------------

CLASSES = 10
MAX_BATCH = 4
COUNTS = [1, 2, 6, 3, 1]  # (6 > max_batch: served as two fragments and joined)


def float_record(x) -> bytes:
    return C.encode_instances(np.ascontiguousarray(x, dtype=np.float32))


def pixel_record(x_u8, fmt, layout) -> bytes:
    v = x_u8.transpose(0, 3, 1, 2) if layout == "nchw" else x_u8
    if fmt == "b64":
        inst = [{"b64": base64.b64encode(np.ascontiguousarray(im).tobytes()).decode()} for im in v]
    else:
        inst = v.tolist()
    return json.dumps({"instances": inst}, separators=(",", ":")).encode()


def run_stub(records, model_hwc, **opts):
    broker = K.Broker()
    broker.start()
    try:
        broker.create_topic("in", 1)
        broker.create_topic("out", 1)
        for key, value in records:
            broker.append("in", 0, [value], [key])
        cfg = GaleConfig(topology_name="t", input_topic="in", output_topic="out",
                         bootstrap=f"127.0.0.1:{broker.port}", start_offset="earliest", stub=True,
                         max_batch=MAX_BATCH, max_wait_us=500, output_key="input",
                         on_error="null", **opts).validate()
        d = cfg.engine_dict(*model_hwc, CLASSES)
        d["max_records"] = len(records)
        eng = C.Engine(d)
        eng.add_stub_replica(MAX_BATCH, 0, True, -1)
        eng.start()
        assert eng.wait(30000), eng.stats()
        eng.stop()
        stats = dict(eng.stats())
        out = broker.read("out", 0)
    finally:
        broker.stop()
    return {r["key"]: r["value"] for r in out}, stats


@pytest.fixture(scope="module")
def stub_case():
    """Pixels at 40x36, and what the engine gives for apply(prep(x)) as float text, no options."""
    rng = np.random.default_rng(17)
    xs = {f"r{i}".encode(): rng.integers(0, 256, (n, 40, 36, 3), dtype=np.uint8)
          for i, n in enumerate(COUNTS)}
    prep = InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S)
    rs = InputResize(40, 36, 34, 33, 32, 32, antialias=True)
    recs = [(k, float_record(rs.apply(prep.apply(x.astype(np.float32))))) for k, x in xs.items()]
    recs.insert(2, (b"bad", b'{"instances": [[[1, 2'))
    want, stats = run_stub(recs, (32, 32, 3))
    assert stats["resized_images"] == 0
    assert want[b"bad"] is None and all(want[k] is not None for k in xs)
    return xs, want


@pytest.mark.parametrize("fmt", ["json", "b64"])
@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
def test_stub_engine_resizes_source_size_records(stub_case, fmt, layout):
    xs, want = stub_case
    recs = [(k, pixel_record(x, fmt, layout)) for k, x in xs.items()]
    recs.insert(2, (b"bad", b'{"instances": [[[1, 2'))
    opts = dict(input_size="40,36", input_resize="34,33", input_scale=1 / 255,
                input_mean=CIFAR_MEAN_S, input_std=CIFAR_STD_S, input_format=fmt,
                input_layout=layout)
    got, stats = run_stub(recs, (32, 32, 3), input_antialias=True, **opts)
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], k
    assert stats["resized_images"] == sum(COUNTS)
    assert len(json.loads(got[b"r2"])["predictions"]) == 6
    if (fmt, layout) == ("json", "nhwc"):  # the option is what makes the difference
        plain, _ = run_stub(recs, (32, 32, 3), **opts)
        assert any(plain[k] != want[k] for k in xs)


# ---- 5. stand-alone sanitizer run ---------------------------------------------------------------

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None,
                    reason="needs ROCm clang++ and make")
def test_resize_aa_under_address_and_ub_sanitizers():
    target = "build/asan/resize_aa_check"
    b = subprocess.run(["make", "-C", ROOT, target], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, target)], capture_output=True, text=True, timeout=300,
                       env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "resize_aa_check OK" in out
