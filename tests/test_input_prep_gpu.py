"""Input preprocessing on the GPU: the JSON parser's affine / NCHW store against an exact
rational fma oracle, unchanged verdicts, the identity launch, and the engine end to end on NCHW
records of raw integer pixels (bf16 ResNet-20 on every parse path, LeNet-5, fp8 ResNet-20)."""

import json
from fractions import Fraction

import numpy as np
import pytest
import torch

from gale._native import native
from gale.config import GaleConfig
from gale.engine import Engine
from gale.models import fold_params, get_model, init_params
from gale.models.preprocess import InputPrep
from gale.models.reference import calibrate_bn, forward

pytestmark = pytest.mark.gpu

C = native()
K = C.kafka
REC = np.dtype([("off", "<i8"), ("len", "<i4"), ("slot", "<i4"), ("images", "<i4"),
                ("status", "<i4"), ("tile0", "<i4"), ("has_cnt", "<i4"), ("cnt_off", "<i8"),
                ("pad", "<i8")])
assert REC.itemsize == C.JSON_RECORD_BYTES

CIFAR_MEAN_S = "0.4914,0.4822,0.4465"
CIFAR_STD_S = "0.2470,0.2435,0.2616"


# ---- staging (the approach of tests/test_engine_gpu.py::gpu_parse) -----------------------------

def stage(arrays):
    """Pack JSON array texts 16-byte aligned (+16 slack) and their JsonRecord table."""
    buf = bytearray()
    recs = np.zeros(len(arrays), dtype=REC)
    slot = tiles = 0
    for i, (txt, images) in enumerate(arrays):
        recs[i] = (len(buf), len(txt), slot, images, 0, tiles, 0, 0, 0)
        tiles += C.json_tile_count(len(buf), len(txt))
        buf += txt + b" " * ((-len(txt)) % 16)
        slot += images
    buf += b" " * 16
    return np.frombuffer(bytes(buf), dtype=np.uint8), recs, slot, tiles


def gpu_parse(arrays, H, Wd, Cc, **prep_kw):
    """(arena bits [images, H, W, C] uint32, per-record statuses); prep_kw: the binding's
    a / b / nchw arguments (none: the launch without an InputPrep)."""
    raw, recs, total, tiles = stage(arrays)
    tile_rec = np.zeros(max(tiles, 1), dtype=np.int32)
    for i, r in enumerate(recs):
        n = C.json_tile_count(int(r["off"]), int(r["len"]))
        tile_rec[r["tile0"]:r["tile0"] + n] = i
    d_raw = torch.from_numpy(raw.copy()).cuda()
    d_recs = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    d_tile_rec = torch.from_numpy(tile_rec).cuda()
    d_tiles = torch.zeros(max(tiles, 1), dtype=torch.int32, device="cuda")
    out = torch.full((max(total, 1), H, Wd, Cc), -7.0, device="cuda")
    C.json_parse_instances(len(arrays), tiles, d_recs.data_ptr(), d_tile_rec.data_ptr(),
                           d_raw.data_ptr(), H, Wd, Cc, d_tiles.data_ptr(), out.data_ptr(),
                           torch.cuda.current_stream().cuda_stream, **prep_kw)
    torch.cuda.synchronize()
    st = d_recs.cpu().numpy().view(REC)["status"]
    return out.cpu().numpy().view(np.uint32), st


def array_text(record: bytes, dims):
    """The instances array of a record nested by `dims` (the scan only counts brackets)."""
    s, off, ln, n = C.scan_instances(record, *dims)
    assert s == 0
    return record[off:off + ln], n


# ---- the oracle: exact rational arithmetic, rounded once ---------------------------------------

def f32_round(x: Fraction) -> int:
    """Bits of the binary32 nearest to x, ties to even (tests/test_json_float_exact.py's
    f32_correct, on a Fraction)."""
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


def oracle_bits(x_nhwc: np.ndarray, prep: InputPrep) -> np.ndarray:
    """fma(x, a[c], b[c]) of binary32 values x [..., C], exact and rounded once."""
    fa = [Fraction(v) for v in prep.a]
    fb = [Fraction(v) for v in prep.b]
    flat = x_nhwc.reshape(-1, x_nhwc.shape[-1])
    out = np.empty(flat.shape, dtype=np.uint32)
    for i in range(flat.shape[0]):
        for c in range(flat.shape[1]):
            r = Fraction(float(flat[i, c])) * fa[c] + fb[c]
            assert r != 0  # (no exact cancellation in these inputs: the sign of zero is moot)
            out[i, c] = f32_round(r)
    return out.reshape(x_nhwc.shape)


def wide_values(rng, shape):
    """Both signs, magnitudes 1e-8 .. 1e8."""
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-8, 9, shape)).astype(np.float32)


def records_of(xs, layout):
    """Java Float.toString records of NHWC arrays, nested NHWC or NCHW."""
    out = []
    for x in xs:
        n, H, Wd, Cc = x.shape
        if layout == "nchw":
            rec = C.encode_instances(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))
            out.append(array_text(rec, (Cc, H, Wd)))
        else:
            out.append(array_text(C.encode_instances(x), (H, Wd, Cc)))
    return out


SHAPES = [
    ((5, 4, 3), dict(mean="0.25,-3,100", std="0.5,3,0.001", scale=0.75)),     # per channel
    ((7, 6, 1), dict(mean="0.1307", std="0.3081", scale=1 / 255)),            # C = 1, scalar
    ((3, 5, 4), dict(mean="1,-2,3,-4", std="2,0.3,7,0.011", scale=1.5)),      # C = 4
]


@pytest.fixture(scope="module")
def cases():
    """Per shape: the prep, the NHWC arrays of records of 1, 3 and 2 images, their oracle."""
    rng = np.random.default_rng(21)
    out = []
    for (H, Wd, Cc), kw in SHAPES:
        prep = InputPrep.build(Cc, kw["scale"], kw["mean"], kw["std"])
        xs = [wide_values(rng, (n, H, Wd, Cc)) for n in (1, 3, 2)]
        want = oracle_bits(np.concatenate(xs), prep)
        out.append(((H, Wd, Cc), prep, xs, want))
    return out


# ---- 1. / 2. kernel ----------------------------------------------------------------------------

def test_kernel_nhwc_affine(cases):
    for (H, Wd, Cc), prep, xs, want in cases:
        a, b = prep.coeffs()
        got, st = gpu_parse(records_of(xs, "nhwc"), H, Wd, Cc, a=a, b=b)
        assert list(st) == [0, 0, 0], (H, Wd, Cc)
        bad = np.nonzero(got != want)
        assert got.shape == want.shape and bad[0].size == 0, \
            ((H, Wd, Cc), [(hex(got[i]), hex(want[i])) for i in zip(*bad)][:5])
    # the oracle differs from mul-then-add on these inputs, so bit equality means a fused op
    _, prep, xs, want = cases[0]
    x = np.concatenate(xs)
    muladd = (x * np.float32(prep.a) + np.float32(prep.b)).astype(np.float32).view(np.uint32)
    assert (muladd != want).any()


def test_kernel_nchw(cases):
    for (H, Wd, Cc), prep, xs, want in cases:
        a, b = prep.coeffs()
        got, st = gpu_parse(records_of(xs, "nchw"), H, Wd, Cc, a=a, b=b, nchw=True)
        assert list(st) == [0, 0, 0], (H, Wd, Cc)
        assert np.array_equal(got, want), (H, Wd, Cc)
        # transposition alone (identity coefficients): the parsed values, moved
        got, st = gpu_parse(records_of(xs, "nchw"), H, Wd, Cc, nchw=True)
        assert list(st) == [0, 0, 0]
        assert np.array_equal(got, np.concatenate(xs).view(np.uint32)), (H, Wd, Cc)


def test_kernel_nchw_multi_tile():
    """32x32x3 records: one of wide-range values spanning many 2 KiB tiles (token indices carry
    across tiles), and one of two images whose pixels are all single digits, compact - the
    densest text the feature makes realistic (a token every 2 bytes)."""
    rng = np.random.default_rng(22)
    H, Wd, Cc = 32, 32, 3
    prep = InputPrep.build(Cc, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S, "nchw")
    x1 = wide_values(rng, (1, H, Wd, Cc))
    x2 = rng.integers(0, 10, (2, H, Wd, Cc))
    dense = json.dumps(x2.transpose(0, 3, 1, 2).tolist(), separators=(",", ":")).encode()
    assert b" " not in dense and len(dense) < 2.2 * x2.size and len(dense) > 4 * 2048
    recs = records_of([x1], "nchw") + [(dense, 2)]
    assert len(recs[0][0]) > 10 * 2048
    got, st = gpu_parse(recs, H, Wd, Cc, **prep.kernel_kwargs())
    assert list(st) == [0, 0]
    want = oracle_bits(np.concatenate([x1, x2.astype(np.float32)]), prep)
    assert np.array_equal(got, want)


# ---- 3. verdicts -------------------------------------------------------------------------------

# H, W, C = 2, 2, 3 nested NCHW: [1][3][2][2]
GOOD = b"[[[[1,2],[3,4]],[[5,6],[7,8]],[[9,10],[11,12]]]]"
VERDICTS = [
    (GOOD, 0),
    (b"[[[[1,2],[3,4]],[[5,6,7],[8]],[[9,10],[11,12]]]]", 3),       # a ragged row
    (b"[[[1,2],[3,4]],[[5,6],[7,8]],[[9,10],[11,12]]]", 3),          # wrong rank
    (b"[[[[1,2],[3,4]],[[5,6],[7,8]],[[9,10],[11]]]]", 1),           # count off by one number
    (b"[[[[1,2],[3,4]],[[5,6],[7,8x]],[[9,10],[11,12]]]]", 2),       # a malformed number
    # One number too MANY cannot end in the count verdict: the 12th number is then not followed
    # by the closing brackets, which is a structure verdict, and a record's status is the worst
    # of its flags. The parser without an InputPrep says 3 for this text too (measured on the
    # MI355X, as for an extra number after any bracket level); the rule that holds is "the same
    # verdict as the unmodified path", asserted below.
    (b"[[[[1,2],[3,4]],[[5,6],[7,8]],[[9,10],[11,12,13]]]]", 3),
]


def test_nchw_verdicts_match_the_unmodified_path():
    H, Wd, Cc = 2, 2, 3
    prep = InputPrep.build(Cc, 0.5, "1,2,3", "4,5,6", "nchw")
    recs = [(t, 1) for t, _ in VERDICTS]
    _, st = gpu_parse(recs, H, Wd, Cc, **prep.kernel_kwargs())
    assert list(st) == [s for _, s in VERDICTS]
    # the same text is a [1][3][2][2] NHWC record to the path without an InputPrep
    _, st0 = gpu_parse(recs, Cc, H, Wd)
    assert list(st0) == list(st)
    # NHWC affine: the verdicts of the plain parse on NHWC-nested text
    nhwc = [(b"[[[[1,2,3],[4,5,6]],[[1,2,3],[4,5,6]]]]", 0),
            (b"[[[[1,2,3],[4,5,6]],[[1,2,3,4],[5,6]]]]", 3),
            (b"[[[[1,2,3],[4,5,6]],[[1,2,3],[4,5]]]]", 1),
            (b"[[[[1,2,3],[4,5,06]],[[1,2,3],[4,5,6]]]]", 2)]
    a, b = prep.coeffs()
    _, st = gpu_parse([(t, 1) for t, _ in nhwc], H, Wd, Cc, a=a, b=b)
    assert list(st) == [s for _, s in nhwc]


# ---- 4. identity -------------------------------------------------------------------------------

def test_identity_prep_is_the_plain_launch(cases):
    for (H, Wd, Cc), _, xs, _ in cases:
        recs = records_of(xs, "nhwc")
        plain, st0 = gpu_parse(recs, H, Wd, Cc)
        ident, st1 = gpu_parse(recs, H, Wd, Cc, a=[1.0] * 4, b=[0.0] * 4, nchw=False)
        assert list(st0) == list(st1) == [0, 0, 0]
        assert np.array_equal(plain, ident)
        assert np.array_equal(plain, np.concatenate(xs).view(np.uint32))


# ---- 5. - 7. engine end to end -----------------------------------------------------------------

def centered_log(p):
    lp = np.log(np.maximum(np.asarray(p, dtype=np.float64), 1e-38))
    return lp - lp.mean(axis=-1, keepdims=True)


MAX_BATCH = 4
COUNTS = [1, 2, 4, 1, 3, 6, 2, 1, 4, 3, 1, 2]  # one record with more images than MAX_BATCH


def pixel_records(shape, layout, seed=31):
    """Keyed records of integer 0..255 pixels (compact json.dumps) and their NHWC arrays."""
    rng = np.random.default_rng(seed)
    xs, recs = {}, []
    for i, n in enumerate(COUNTS):
        x = rng.integers(0, 256, (n,) + tuple(shape))
        key = f"r{i}".encode()
        xs[key] = x.astype(np.float32)
        nested = x.transpose(0, 3, 1, 2) if layout == "nchw" else x
        recs.append((key, json.dumps({"instances": nested.tolist()},
                                     separators=(",", ":")).encode()))
    return xs, recs


def unit_scale_params(net, prep, seed=0):
    """Seeded weights whose BatchNorm statistics come from preprocessed random pixels, so the
    activations stay at unit scale."""
    params = init_params(net, seed=seed, calibrate=False)
    rng = np.random.default_rng(77)
    x = rng.integers(0, 256, (16,) + tuple(net.input_shape)).astype(np.float32)
    calibrate_bn(net, params, torch.from_numpy(prep.apply(x)))
    return params


def serve(model, recs, params, **kw):
    """Run the records through an engine on GPU 0; (engine, {key: value bytes})."""
    broker = K.Broker()
    broker.start()
    try:
        broker.create_topic("in", 1)
        broker.create_topic("out", 1)
        for key, rec in recs:
            broker.append("in", 0, [rec], [key])
        cfg = GaleConfig(topology_name="g", input_topic="in", output_topic="out", model=model,
                         bootstrap=f"127.0.0.1:{broker.port}", start_offset="earliest",
                         max_batch=MAX_BATCH, max_wait_us=500, output_key="input", **kw)
        eng = Engine(cfg.validate(), devices=[0], max_records=len(recs), params=params)
        eng.start()
        assert eng.wait(120), eng.stats()
        eng.stop()
        out = broker.read("out", 0)
    finally:
        broker.stop()
    assert len(out) == len(recs)
    return eng, {r["key"]: r["value"] for r in out}


def compare(by_key, xs, ref_of):
    """The metric and bounds of tests/test_engine_gpu.py::test_gpu_engine_matches_oracle:
    centered log-softmax; per record argmax equal or rel < 1e-2; worst rel < 2e-2. Returns
    (passed, worst)."""
    worst, ok = 0.0, True
    for k, x in xs.items():
        if by_key.get(k) is None:
            return False, float("inf")
        ref = centered_log(ref_of(x))
        got = centered_log(json.loads(by_key[k])["predictions"])
        if got.shape != ref.shape:
            return False, float("inf")
        rel = np.abs(got - ref).max() / max(np.abs(ref).max(), 1.0)
        worst = max(worst, rel)
        ok &= bool(np.array_equal(got.argmax(-1), ref.argmax(-1)) or rel < 1e-2)
    return ok and worst < 2e-2, worst


PREP_KW = dict(input_scale=1 / 255, input_mean=CIFAR_MEAN_S, input_std=CIFAR_STD_S,
               input_layout="nchw")
MODES = {
    "ingest-parse": dict(gpu_ingest=True, text_pack=False, ingest_parse=True),
    "step-parse": dict(gpu_ingest=True, text_pack=False, ingest_parse=False),
    "host": dict(gpu_ingest=False, text_pack=False),
    "pack": dict(gpu_ingest=True, text_pack=True, ingest_parse=True),
}


@pytest.fixture(scope="module")
def r20():
    net = get_model("resnet20")
    prep = InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S, "nchw")
    params = unit_scale_params(net, prep)
    folded = fold_params(net, params)
    xs, recs = pixel_records(net.input_shape, "nchw")
    refs = {k: forward(net, folded, torch.from_numpy(prep.apply(x))).numpy()
            for k, x in xs.items()}
    served = {}

    def run(mode):
        if mode not in served:
            eng, by_key = serve("resnet20", recs, params, **PREP_KW, **MODES[mode])
            served[mode] = (eng.stats(), by_key)
        return served[mode]

    return dict(net=net, prep=prep, params=params, folded=folded, xs=xs, recs=recs, refs=refs,
                run=run)


def ref_lookup(r20):
    by_id = {id(x): r20["refs"][k] for k, x in r20["xs"].items()}
    return lambda x: by_id[id(x)]


@pytest.mark.parametrize("mode", list(MODES))
def test_engine_resnet20_bf16(r20, mode):
    if mode == "pack" and not C.text_pack_fast():
        pytest.skip("no AVX-512 VBMI on this host")
    st, by_key = r20["run"](mode)
    assert set(by_key) == set(r20["xs"])
    ok, worst = compare(by_key, r20["xs"], ref_lookup(r20))
    print(f"\n{mode}: worst relative logit error {worst:.4f}")
    assert ok, worst
    assert st["errors"] == 0 and st["images_out"] == sum(COUNTS)
    assert st["split_records"] == 1  # the 6-image record, served as fragments of <= 4
    assert (st["ingested_records"] > 0) == (mode != "host")
    # the ingest parse produced the inputs of every record it could (the split record's
    # fragments are host copies, parsed in the step)
    if mode in ("ingest-parse", "pack"):
        assert st["ingest_parsed_records"] >= len(COUNTS) - 1, st
    else:
        assert st["ingest_parsed_records"] == 0 and st["preparsed_records"] == 0, st


def test_engine_ingest_and_step_parse_are_byte_identical(r20):
    _, a = r20["run"]("ingest-parse")
    _, b = r20["run"]("step-parse")
    assert a == b
    _, c = r20["run"]("host")
    assert a == c  # (the host-staged step parse too: same kernel, same rounding)


def test_engine_default_options_fail_the_comparison(r20):
    """The positive tests cannot pass vacuously: the same records served with the options at
    their defaults miss the comparison (NCHW text is the wrong shape for an NHWC topology), and
    so do they with the layout alone (raw 0..255 pixels into unit-scale weights)."""
    _, by_key = serve("resnet20", r20["recs"], r20["params"], on_error="null")
    ok, _ = compare(by_key, r20["xs"], ref_lookup(r20))
    assert not ok
    assert all(v is None for v in by_key.values())
    _, by_key = serve("resnet20", r20["recs"], r20["params"], input_layout="nchw")
    assert all(v is not None for v in by_key.values())
    ok, worst = compare(by_key, r20["xs"], ref_lookup(r20))
    assert not ok and worst > 2e-2


def test_engine_lenet5_scalar_nhwc():
    net = get_model("lenet5")
    kw = dict(input_scale=1 / 255, input_mean="0.1307", input_std="0.3081")
    prep = InputPrep.build(1, 1 / 255, "0.1307", "0.3081")
    params = unit_scale_params(net, prep)
    folded = fold_params(net, params)
    xs, recs = pixel_records(net.input_shape, "nhwc", seed=32)
    eng, by_key = serve("lenet5", recs, params, gpu_ingest=True, text_pack=False,
                        ingest_parse=True, **kw)
    ok, worst = compare(
        by_key, xs, lambda x: forward(net, folded, torch.from_numpy(prep.apply(x))).numpy())
    assert ok, worst
    st = eng.stats()
    assert st["errors"] == 0 and st["ingest_parsed_records"] >= len(COUNTS) - 1, st
    # without the options the same records miss it
    _, by_key = serve("lenet5", recs, params, gpu_ingest=True, text_pack=False)
    ok, _ = compare(
        by_key, xs, lambda x: forward(net, folded, torch.from_numpy(prep.apply(x))).numpy())
    assert not ok


def rel_logit_err(p: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """tests/test_models_gpu.py: per-row max |dlogit| / max(|ref logit|, 1)."""
    def logits(q):
        lp = q.double().clamp_min(1e-300).log()
        return lp - lp.mean(dim=1, keepdim=True)
    a, b = logits(p), logits(ref)
    return (a - b).abs().amax(1) / b.abs().amax(1).clamp_min(1.0)


def test_engine_resnet20_fp8(r20):
    """Served fp8 outputs against the fp8 emulation oracle on the preprocessed inputs, with the
    tolerance of tests/test_models_gpu.py::test_fp8_model_matches_emulation_and_fp32 for that
    comparison: mean relative logit error < max(1e-2, 0.5 * budget), budget = the mean error of
    the emulation against fp32 (what e4m3 quantisation alone costs)."""
    from gale.models.graph import act_scales_from_packed
    from gale.models.quant import E4M3_MAX

    net, prep, folded = r20["net"], r20["prep"], r20["folded"]
    eng, by_key = serve("resnet20", r20["recs"], r20["params"], dtype="fp8", **PREP_KW,
                        **MODES["ingest-parse"])
    scales = act_scales_from_packed(net, eng.model_replicas[0].packed)
    keys = list(r20["xs"])
    y = torch.from_numpy(np.concatenate([prep.apply(r20["xs"][k]) for k in keys]))
    # the input tensor's scale was calibrated on preprocessed values: it does not saturate
    assert scales["input"] * E4M3_MAX >= 2.0
    emu = forward(net, folded, y, fp8_scales=scales)
    ref = forward(net, folded, y)
    got = torch.tensor(np.concatenate([json.loads(by_key[k])["predictions"] for k in keys]))
    assert got.shape == emu.shape
    e_emu = rel_logit_err(got, emu)
    budget = rel_logit_err(emu, ref)
    print(f"\nfp8 served vs emulation mean {e_emu.mean().item():.2e} max "
          f"{e_emu.max().item():.2e} (budget mean {budget.mean().item():.2e})")
    assert e_emu.mean().item() < max(1e-2, 0.5 * budget.mean().item())
