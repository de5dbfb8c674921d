"""Base64 uint8 image records (--input-format b64) on the GPU: the decode kernel bit for bit
against numpy / the exact-rational fma oracle at every start phase, its verdicts in both launch
forms, and the engine end to end on every step launch site (ResNet-20, LeNet-5, ResNet-50)."""

import base64
import json
from fractions import Fraction

import numpy as np
import pytest
import torch

from gale._native import native
from gale.config import GaleConfig
from gale.data import encode_records_b64, encode_records_text
from gale.engine import Engine
from gale.models import fold_params, get_model, init_params
from gale.models.preprocess import InputPrep
from gale.models.reference import calibrate_bn, forward

pytestmark = pytest.mark.gpu

C = native()
K = C.kafka
IMG = np.dtype([("off", "<i8"), ("slot", "<i4"), ("rec", "<i4")])
assert IMG.itemsize == C.B64_IMAGE_BYTES

CIFAR_MEAN_S = "0.4914,0.4822,0.4465"
CIFAR_STD_S = "0.2470,0.2435,0.2616"
SENTINEL = -7.0


def geometry(shape):
    per = int(np.prod(shape))
    return per, 4 * ((per + 2) // 3), (3 - per % 3) % 3


def b64_of(im) -> bytes:
    return base64.b64encode(np.ascontiguousarray(im).tobytes())


def stage(strings, phases):
    """The strings in one byte buffer, string i starting at phase phases[i] modulo 16, each
    followed by the text a record has there, and 16 bytes of slack at the end."""
    buf = bytearray(b'{"instances":[{"')
    offs = []
    for s, ph in zip(strings, phases):
        buf += b'"b64":"'
        while len(buf) % 16 != ph:
            buf += b" "
        offs.append(len(buf))
        buf += s + b'"},{'
    buf += b"\xee" * 16
    return np.frombuffer(bytes(buf), dtype=np.uint8), offs


def gpu_decode(strings, phases, slots, recs, nrec, shape, total, header=None, **prep_kw):
    """(out bits [total + 1, H, W, C] uint32 view of floats, statuses[nrec]): image i's string
    goes to slot slots[i] and belongs to record recs[i]. header: the device-header launch form
    with that image count (the launch stays sized for every descriptor)."""
    raw, offs = stage(strings, phases)
    tab = np.zeros(len(strings), dtype=IMG)
    tab["off"], tab["slot"], tab["rec"] = offs, slots, recs
    d_raw = torch.from_numpy(raw.copy()).cuda()
    d_tab = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
    d_status = torch.zeros(nrec, dtype=torch.int32, device="cuda")
    out = torch.full((total + 1,) + tuple(shape), SENTINEL, device="cuda")
    d_hdr = torch.tensor([header], dtype=torch.int32, device="cuda") if header is not None \
        else None
    C.b64_decode_instances(len(strings), d_tab.data_ptr(), d_raw.data_ptr(), *shape,
                           out.data_ptr(), d_status.data_ptr(),
                           torch.cuda.current_stream().cuda_stream,
                           d_hdr.data_ptr() if d_hdr is not None else 0, **prep_kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), d_status.cpu().numpy()


# ---- the exact oracle (tests/test_input_prep_gpu.py) --------------------------------------------

def f32_round(x: Fraction) -> int:
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
            assert r != 0
            out[i, c] = f32_round(r)
    return out.reshape(x_nhwc.shape)


# ---- 1. kernel against the oracle ---------------------------------------------------------------

SHAPES = [
    ((5, 4, 3), range(16)),      # 80 characters, no padding: every start phase
    ((5, 4, 1), [0, 7]),         # one '='
    ((28, 28, 1), [0, 13]),      # 1048 characters, "==", a partial last wave
    ((32, 32, 3), [0, 9]),       # exactly one workgroup
    ((40, 40, 3), range(16)),    # 6400 characters: a full chunk and a partial one
    ((3, 5, 4), [3]),            # C = 4 (general channel pattern), 80 characters
    ((7, 3, 5), [11]),           # C = 5: lanes do not start on a pixel
]
SLOTS = [4, 5, 0, 1, 2, 3]                # slots out of record order
RECS = [0, 0, 1, 2, 2, 2]                 # records of 2, 1 and 3 images


def prep_for(Cc, layout="nhwc"):
    if Cc == 3:
        return InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S, layout)
    if Cc == 4:
        return InputPrep.build(4, 0.5, "1,-2,3,-4", "2,0.3,7,0.011", layout)
    return InputPrep.build(Cc, 1 / 255, "0.1307", "0.3081", layout)


@pytest.fixture(scope="module")
def images():
    rng = np.random.default_rng(41)
    out = {}
    for shape, _ in SHAPES:
        x = rng.integers(0, 256, (len(SLOTS),) + shape, dtype=np.uint8)
        x[0].flat[:4] = [0, 255, 1, 254]
        out[shape] = x
    return out


def check(got, want_bits, x, what):
    """Image i of x sits in slot SLOTS[i]; the slot after the last one is untouched."""
    bits = got.view(np.uint32)
    for i, slot in enumerate(SLOTS):
        bad = np.nonzero(bits[slot] != want_bits[i])
        assert bad[0].size == 0, (what, i, [(hex(bits[slot][j]), hex(want_bits[i][j]))
                                            for j in zip(*bad)][:4])
    assert (got[len(SLOTS)] == SENTINEL).all(), what


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_kernel_matches_the_oracle(images, k):
    shape, phases = SHAPES[k]
    x = images[shape]
    xf = x.astype(np.float32)
    n = len(SLOTS)
    prep = prep_for(shape[2])
    want_prep = prep.apply(xf).view(np.uint32)
    if k == 0:   # the exact-rational fma on a sample: InputPrep.apply is that fma
        assert np.array_equal(want_prep, oracle_bits(xf, prep))
    strings = [b64_of(im) for im in x]
    strings_t = [b64_of(im.transpose(2, 0, 1)) for im in x]
    per, L, pad = geometry(shape)
    assert all(len(s) == L and s.count(b"=") == pad for s in strings)
    for ph in phases:
        ps = [(ph + 5 * i) % 16 for i in range(n)]
        got, st = gpu_decode(strings, ps, SLOTS, RECS, 3, shape, n)
        assert list(st) == [0, 0, 0], (shape, ph)
        check(got, xf.view(np.uint32), x, (shape, ph, "no prep"))
        got, st = gpu_decode(strings, ps, SLOTS, RECS, 3, shape, n, **prep.kernel_kwargs())
        assert list(st) == [0, 0, 0]
        check(got, want_prep, x, (shape, ph, "prep"))
        # NCHW-ordered bytes: the same tensor, with and without coefficients
        nchw = prep_for(shape[2], "nchw")
        got, st = gpu_decode(strings_t, ps, SLOTS, RECS, 3, shape, n, **nchw.kernel_kwargs())
        assert list(st) == [0, 0, 0]
        check(got, want_prep, x, (shape, ph, "nchw prep"))
        got, st = gpu_decode(strings_t, ps, SLOTS, RECS, 3, shape, n, nchw=True)
        assert list(st) == [0, 0, 0]
        check(got, xf.view(np.uint32), x, (shape, ph, "nchw"))


def test_op_wrapper(images):
    from gale import ops

    shape = (32, 32, 3)
    x = images[shape][:2]
    raw, offs = stage([b64_of(im) for im in x], [5, 14])
    tab = np.zeros(2, dtype=IMG)
    tab["off"], tab["slot"], tab["rec"] = offs, [1, 0], [0, 0]
    prep = prep_for(3)
    out = torch.full((2,) + shape, SENTINEL, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.b64_decode_instances(torch.from_numpy(raw.copy()).cuda(),
                             torch.from_numpy(tab.view(np.int32).reshape(2, 4).copy()).cuda(),
                             shape, out, status, prep=prep)
    torch.cuda.synchronize()
    assert status.item() == 0
    assert np.array_equal(out.cpu().numpy()[[1, 0]].view(np.uint32),
                          prep.apply(x.astype(np.float32)).view(np.uint32))
    with pytest.raises(RuntimeError):
        ops.b64_decode_instances(torch.from_numpy(raw.copy()), torch.zeros(2, 4, dtype=torch.int32),
                                 shape, out, status)


# ---- 2. verdicts --------------------------------------------------------------------------------

def plant(s: bytes, at: int, what: bytes) -> bytes:
    return s[:at] + what + s[at + len(what):]


@pytest.mark.parametrize("header", [None, 4])
def test_kernel_verdicts(images, header):
    """Five records: good, a bad character in the first lane, one in the second chunk's last
    lane, wrong padding ('=' where the shape has none), good (two images). header: the
    device-header form with a count of 4 of the 6 descriptors - the last record's images are
    past it and are not written."""
    shape = (40, 40, 3)
    per, L, pad = geometry(shape)
    assert (L, pad) == (6400, 0)
    x = images[shape]
    s = [b64_of(im) for im in x]
    s[1] = plant(s[1], 3, b"-")
    s[2] = plant(s[2], L - 2, b"\\/")          # characters 6398, 6399: lane 399 = chunk 1's last
    s[3] = plant(s[3], L - 1, b"=")
    slots, recs = [2, 0, 1, 3, 4, 5], [0, 1, 2, 3, 4, 4]
    got, st = gpu_decode(s, [1, 6, 11, 15, 0, 8], slots, recs, 5, shape, 6, header=header)
    assert list(st) == [0, 2, 2, 2, 0]
    bits = got.view(np.uint32)
    want = x.astype(np.float32).view(np.uint32)
    assert np.array_equal(bits[2], want[0])
    if header is None:
        assert np.array_equal(bits[4], want[4]) and np.array_equal(bits[5], want[5])
    else:
        assert (got[4] == SENTINEL).all() and (got[5] == SENTINEL).all()
    assert (got[6] == SENTINEL).all()
    # a bad record's images stay inside their own slots: everything else of them is the pixels
    assert np.array_equal(bits[0].ravel()[3:], want[1].ravel()[3:])


def test_kernel_every_byte_value(images):
    """Each of the 256 byte values planted in a record of its own (at a moving position): the
    status is 2 exactly for the values outside the alphabet, where the host decoder says
    BAD_NUMBER, and the others decode to what base64.b64decode gives."""
    shape = (5, 4, 3)
    alphabet = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
    base = b64_of(images[shape][1])
    strings = [plant(base, (7 * v) % 80, bytes([v])) for v in range(256)]
    got, st = gpu_decode(strings, [(3 * v) % 16 for v in range(256)], range(256), range(256),
                         256, shape, 256)
    for v in range(256):
        ok = bytes([v]) in [alphabet[i:i + 1] for i in range(64)]
        assert st[v] == (0 if ok else 2), v
        rec = b'{"instances":[{"b64":"' + strings[v] + b'"}]}'
        assert C.parse_instances_b64_host(rec, *shape)[0] == (0 if ok else 5), v
        if ok:
            want = np.frombuffer(base64.b64decode(strings[v]), dtype=np.uint8)
            assert np.array_equal(got[v].ravel(), want.astype(np.float32)), v
    assert (got[256] == SENTINEL).all()


def test_kernel_padding_verdicts(images):
    """(28, 28, 1), two '=': one too few, one too many, '=' in the middle, a bad character in the
    partial last lane; the good records around them are bit-exact."""
    shape = (28, 28, 1)
    per, L, pad = geometry(shape)
    x = images[shape][:6]
    s = [b64_of(im) for im in x]
    s[1] = plant(s[1], L - 2, b"A")
    s[2] = plant(s[2], L - 3, b"=")
    s[3] = plant(s[3], L // 2, b"=")
    s[4] = plant(s[4], L - 4, b"_")
    got, st = gpu_decode(s, [0, 3, 6, 9, 12, 15], range(6), range(6), 6, shape, 6)
    assert list(st) == [0, 2, 2, 2, 2, 0]
    bits = got.view(np.uint32)
    want = x.astype(np.float32).view(np.uint32)
    assert np.array_equal(bits[0], want[0]) and np.array_equal(bits[5], want[5])
    assert (got[6] == SENTINEL).all()
    # non-zero unused bits in the last data character are accepted
    alphabet = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
    v = alphabet.index(s[0][L - 3:L - 2])
    t = plant(s[0], L - 3, alphabet[v | 5:(v | 5) + 1])
    assert t != s[0]
    got, st = gpu_decode([t], [2], [0], [0], 1, shape, 1)
    assert list(st) == [0] and np.array_equal(got.view(np.uint32)[0], want[0])


# ---- 3. - 5. engine end to end ------------------------------------------------------------------

def centered_log(p):
    lp = np.log(np.maximum(np.asarray(p, dtype=np.float64), 1e-38))
    return lp - lp.mean(axis=-1, keepdims=True)


def unit_scale_params(net, prep, seed=0):
    """Seeded weights whose BatchNorm statistics come from preprocessed random pixels."""
    params = init_params(net, seed=seed, calibrate=False)
    rng = np.random.default_rng(77)
    x = rng.integers(0, 256, (16,) + tuple(net.input_shape)).astype(np.float32)
    calibrate_bn(net, params, torch.from_numpy(prep.apply(x)))
    return params


def serve(model, recs, params, max_batch=32, **kw):
    broker = K.Broker()
    broker.start()
    try:
        broker.create_topic("in", 1)
        broker.create_topic("out", 1)
        for key, rec in recs:
            broker.append("in", 0, [rec], [key])
        cfg = GaleConfig(topology_name="g", input_topic="in", output_topic="out", model=model,
                         bootstrap=f"127.0.0.1:{broker.port}", start_offset="earliest",
                         max_batch=max_batch, max_wait_us=500, output_key="input",
                         on_error="null", **kw)
        eng = Engine(cfg.validate(), devices=[0], max_records=len(recs), params=params)
        eng.start()
        assert eng.wait(120), eng.stats()
        eng.stop()
        out = broker.read("out", 0)
    finally:
        broker.stop()
    assert len(out) == len(recs)                     # ONE output record per input record
    return eng, {r["key"]: r["value"] for r in out}


def compare(by_key, xs, refs):
    """tests/test_engine_gpu.py::test_gpu_engine_matches_oracle: centered log-softmax; per
    record argmax equal or rel < 1e-2; worst rel < 2e-2."""
    worst = 0.0
    for k in xs:
        assert by_key.get(k) is not None, k
        ref = centered_log(refs[k])
        got = centered_log(json.loads(by_key[k])["predictions"])
        assert got.shape == ref.shape, k
        rel = np.abs(got - ref).max() / max(np.abs(ref).max(), 1.0)
        worst = max(worst, rel)
        assert np.array_equal(got.argmax(-1), ref.argmax(-1)) or rel < 1e-2, (k, rel)
    assert worst < 2e-2, worst
    return worst


COUNTS = [1, 2, 1, 3, 1, 1, 4, 1, 2, 1, 3, 2]
PREPS = {
    "resnet20": dict(input_scale=1 / 255, input_mean=CIFAR_MEAN_S, input_std=CIFAR_STD_S),
    "lenet5": dict(input_scale=1 / 255, input_mean="0.1307", input_std="0.3081"),
}


def pixel_sets(shape, seed):
    rng = np.random.default_rng(seed)
    return {f"r{i}".encode(): rng.integers(0, 256, (n,) + tuple(shape), dtype=np.uint8)
            for i, n in enumerate(COUNTS)}


def b64_records(xs, layout="nhwc"):
    return [(k, encode_records_b64(x, x.shape[0], layout)[0]) for k, x in xs.items()]


def bad_records(xs):
    """A record with a bad character in its second image, and a numeric-array record."""
    x = xs[b"r1"]
    rec = encode_records_b64(x, 2)[0]
    at = rec.rindex(b'"b64":"') + 7 + 100
    bad = rec[:at] + b"-" + rec[at + 1:]
    return [(b"badchar", bad), (b"numeric", encode_records_text(x, 2)[0])]


@pytest.fixture(scope="module")
def r20():
    net = get_model("resnet20")
    prep = InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S)
    params = unit_scale_params(net, prep)
    folded = fold_params(net, params)
    xs = pixel_sets(net.input_shape, 51)
    refs = {k: forward(net, folded, torch.from_numpy(prep.apply(x.astype(np.float32)))).numpy()
            for k, x in xs.items()}
    return dict(net=net, prep=prep, params=params, xs=xs, refs=refs)


def check_b64_run(eng, by_key, xs, refs):
    assert set(by_key) == set(xs) | {b"badchar", b"numeric"}
    assert by_key[b"badchar"] is None and by_key[b"numeric"] is None
    worst = compare(by_key, xs, refs)
    st = eng.stats()
    assert st["b64_records"] == len(xs) + 1, st     # the good records and the bad character
    assert st["ingested_records"] == 0 and st["errors"] == 2, st
    assert st["images_out"] == sum(x.shape[0] for x in xs.values())
    return worst


def test_engine_resnet20_b64_and_text_agree(r20):
    xs = r20["xs"]
    eng, by_key = serve("resnet20", b64_records(xs) + bad_records(xs), r20["params"],
                        input_format="b64", **PREPS["resnet20"])
    worst = check_b64_run(eng, by_key, xs, r20["refs"])
    print(f"\nresnet20 b64: worst relative logit error {worst:.4f}")
    # the same pixels as byte-pixel text through the host-decode JSON path: the input tensors
    # are bit-identical and the fused forward works per image, so the prediction text is too
    text = [(k, encode_records_text(x, x.shape[0])[0]) for k, x in xs.items()]
    _, by_text = serve("resnet20", text, r20["params"], input_format="json", gpu_ingest=False,
                       **PREPS["resnet20"])
    assert {k: by_key[k] for k in xs} == by_text


def test_engine_lenet5_b64():
    net = get_model("lenet5")
    prep = InputPrep.build(1, 1 / 255, "0.1307", "0.3081")
    params = unit_scale_params(net, prep)
    folded = fold_params(net, params)
    xs = pixel_sets(net.input_shape, 52)
    assert geometry(net.input_shape)[2] == 2
    refs = {k: forward(net, folded, torch.from_numpy(prep.apply(x.astype(np.float32)))).numpy()
            for k, x in xs.items()}
    eng, by_key = serve("lenet5", b64_records(xs) + bad_records(xs), params,
                        input_format="b64", **PREPS["lenet5"])
    check_b64_run(eng, by_key, xs, refs)


@pytest.mark.parametrize("site", ["plain", "graph", "graph-noencode", "nchw"])
def test_engine_resnet20_other_launch_sites(r20, site):
    """graph_step=False: the op-by-op step; step_launch=graph: the captured kernels-only step;
    with gpu_encode off: the captured step with copy nodes; nchw: [C][H][W]-ordered strings
    through the default direct-launch step."""
    kw = {"plain": dict(graph_step=False), "graph": dict(step_launch="graph"),
          "graph-noencode": dict(step_launch="graph", gpu_encode=False),
          "nchw": dict(input_layout="nchw")}[site]
    xs = r20["xs"]
    recs = b64_records(xs, "nchw" if site == "nchw" else "nhwc")
    eng, by_key = serve("resnet20", recs + bad_records(xs), r20["params"], input_format="b64",
                        **PREPS["resnet20"], **kw)
    if site == "nchw":   # (the bad-character record is NHWC-ordered: still a bad character)
        assert by_key[b"badchar"] is None
    check_b64_run(eng, by_key, xs, r20["refs"])
    st = eng.stats()
    assert (st["graph_step_batches"] > 0) == (site != "plain"), st


def test_engine_resnet50_b64():
    """224x224x3: 49 chunks per image, the op-by-op step of a plan that is not one network
    kernel; bf16. The tolerance of test_gpu_engine_resnet50_imagenet_records: the same replica's
    forward of the same input tensors."""
    from gale.parallel.weights import materialize_weights
    from gale.runtime.replica import ModelReplica

    net = get_model("resnet50")
    params = init_params(net, seed=3, calib_batch=4)
    prep = InputPrep.build(3, 1 / 255)
    rng = np.random.default_rng(53)
    xs = {f"i{i}".encode(): rng.integers(0, 256, (n,) + tuple(net.input_shape), dtype=np.uint8)
          for i, n in enumerate([1, 2])}
    eng, by_key = serve("resnet50", b64_records(xs), params, max_batch=8, input_format="b64",
                        input_scale=1 / 255, dtype="bf16")
    st = eng.stats()
    assert st["errors"] == 0 and st["b64_records"] == 2 and st["ingested_records"] == 0, st
    rep = ModelReplica(net, materialize_weights(net, torch.device("cuda", 0), params=params),
                       max_batch=8, slots=1)
    for k, x in xs.items():
        want = rep.infer_eager(torch.from_numpy(prep.apply(x.astype(np.float32)))).cpu().numpy()
        got = np.array(json.loads(by_key[k])["predictions"], dtype=np.float32)
        assert got.shape == want.shape, k
        np.testing.assert_allclose(got, want, rtol=2e-3, atol=1e-6, err_msg=k.decode())


def test_engine_splits_a_40_image_record():
    """max_batch 32: fragments of 32 and 8, ONE 40-row output record. No preprocessing options:
    the decode without an InputPrep, on weights calibrated for raw pixels."""
    net = get_model("resnet20")
    prep = InputPrep.build(3)
    params = unit_scale_params(net, prep, seed=1)
    folded = fold_params(net, params)
    rng = np.random.default_rng(54)
    xs = {b"big": rng.integers(0, 256, (40,) + tuple(net.input_shape), dtype=np.uint8),
          b"small": rng.integers(0, 256, (3,) + tuple(net.input_shape), dtype=np.uint8)}
    refs = {k: forward(net, folded, torch.from_numpy(x.astype(np.float32))).numpy()
            for k, x in xs.items()}
    eng, by_key = serve("resnet20", b64_records(xs), params, input_format="b64")
    assert len(json.loads(by_key[b"big"])["predictions"]) == 40
    compare(by_key, xs, refs)
    st = eng.stats()
    assert st["split_records"] == 1 and st["split_fragments"] == 2 and st["errors"] == 0, st
    assert st["b64_records"] == 2 and st["images_out"] == 43, st
