"""Raw 10-bit YUV 4:2:0 frame records (--input-pixel-format p010le | yuv420p10le) on the host: the
coefficient tables, the twin and the parser against the oracle, configuration, verdicts and the
stub engine. Every comparison of outputs is on the bits."""

import itertools
from fractions import Fraction as F

import numpy as np
import pytest

from gale._native import native
from gale.config import GaleConfig
from gale.data import encode_records_yuv420p10, pack_yuv420p10
from gale.models.preprocess import InputPrep, Yuv420HiConvert
from test_input_raw_cpu import BAD_SHAPE, CIFAR, EMPTY, OK, serve

C = native()
TABLES = [(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]
FORMATS = ("p010le", "yuv420p10le")
SIZES = [(2, 2), (2, 10), (4, 8), (6, 18), (32, 32), (2, 1040), (34, 130)]  # the GPU test's
PREP = InputPrep.build(3, CIFAR["input_scale"], CIFAR["input_mean"], CIFAR["input_std"])
CORNERS = np.array(list(itertools.product((0, 1023), repeat=3)))


def planes(n, HS, WS, seed):
    """10-bit Y [n, HS, WS], U, V [n, HS/2, WS/2]: the 8 cube corners first (as far as the frame
    has quads), then seeded noise; and junk for the six ignored bits of every word."""
    rng = np.random.default_rng(seed)
    Y, U, V = (rng.integers(0, 1024, (n, h, w), dtype=np.uint16)
               for h, w in ((HS, WS), (HS // 2, WS // 2), (HS // 2, WS // 2)))
    m = min(8, U[0].size)
    U.reshape(n, -1)[:, :m], V.reshape(n, -1)[:, :m] = CORNERS[:m, 1], CORNERS[:m, 2]
    Y[:, :2, :2 * min(m, WS // 2)] = np.repeat(CORNERS[:min(m, WS // 2), 0], 2)
    return (Y, U, V), rng.integers(0, 65536, (n, 3 * HS * WS // 2), dtype=np.uint16)


@pytest.mark.parametrize("matrix,range_", TABLES)
def test_coefficient_tables(matrix, range_):
    """The literals are the rounded rationals; the accumulator stays below 2^31 at the corners
    (it is affine); the unclamped result stays within 0.5 + 2047 * 2^-19 quarter steps of the
    float64 matrix."""
    yc = Yuv420HiConvert("p010le", matrix, range_)
    kr, kb = {"bt601": (F(299, 1000), F(114, 1000)), "bt709": (F(2126, 10000), F(722, 10000))}[matrix]
    sy, sc = (F(255, 219), F(255, 224)) if range_ == "limited" else (F(1020, 1023),) * 2
    real = (sy, 2 * (1 - kr) * sc, -2 * kb * (1 - kb) / (1 - kr - kb) * sc,
            -2 * kr * (1 - kr) / (1 - kr - kb) * sc, 2 * (1 - kb) * sc)
    want = tuple(int(round(q * (1 << 18))) for q in real)  # (round(): half to even, exact)
    assert C.yuv10_coeffs(matrix, range_) == (*want, 64 if range_ == "limited" else 0)
    assert yc.coeffs() == want
    worst = max(int(np.abs(a).max()) for a in yc.accumulators(*CORNERS.T))
    print(f"{matrix} {range_}: largest corner accumulator {worst}")
    assert worst <= 575820179 < 1 << 31
    rng = np.random.default_rng(10)
    grey = np.stack([np.arange(1024), np.full(1024, 512), np.full(1024, 512)], axis=1)
    yuv = np.concatenate([CORNERS, grey, rng.integers(0, 1024, (100000, 3))])
    y, u, v = (yuv[:, 0] - yc.yo).astype(np.float64), yuv[:, 1] - 512.0, yuv[:, 2] - 512.0
    r = [float(q) for q in real]
    exact = np.stack([r[0] * y + r[1] * v, r[0] * y + r[2] * u + r[3] * v, r[0] * y + r[4] * u], 1)
    got = np.stack([a >> 18 for a in yc.accumulators(*yuv.T)], axis=1)
    dist = float(np.abs(got - exact).max())
    print(f"{matrix} {range_}: largest distance {dist} quarter steps")
    assert dist <= 0.5 + 2047 * 2.0 ** -19


@pytest.mark.parametrize("HS,WS", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("fmt", FORMATS)
def test_host_twin_and_parser_equal_the_oracle(fmt, HS, WS):
    matrix, range_ = TABLES[(HS + WS // 2) % 4]
    yc = Yuv420HiConvert(fmt, matrix, range_)
    p, junk = planes(2, HS, WS, HS * 100 + WS)
    frames, clean = pack_yuv420p10(*p, fmt, junk), pack_yuv420p10(*p, fmt)
    B = 3 * HS * WS
    assert frames.shape == (2, B) and yc.frame_bytes(HS, WS) == B == C.yuv420p10_bytes(HS, WS)
    assert not np.array_equal(frames, clean)
    q = yc.apply(frames, HS, WS)
    assert q.max() <= 1020 and np.array_equal(q, yc.apply(clean, HS, WS))
    k, (a, b) = [*yc.coeffs(), yc.yo], PREP.coeffs()
    for i, fr in enumerate(frames):
        qh, f32 = C.yuv420p10_to_rgb_host(fr.tobytes(), HS, WS, fmt, k)
        assert np.array_equal(qh, q[i]) and np.array_equal(f32, yc.to_float(q[i]))
        _, f32p = C.yuv420p10_to_rgb_host(fr.tobytes(), HS, WS, fmt, k, a=a, b=b)
        assert np.array_equal(f32p.view(np.uint32), yc.to_float(q[i], PREP).view(np.uint32))
    rec = encode_records_yuv420p10(*p, fmt, 2, junk)[0]
    assert rec == frames.tobytes()
    st, out = C.parse_instances_raw_yuv420p10_host(rec, HS, WS, fmt, k)
    assert st == OK and np.array_equal(out, yc.to_float(q))
    # verdicts: records of 0, B - 1, B + 1 and 2 B bytes
    for n, want in ((0, EMPTY), (B - 1, BAD_SHAPE), (B + 1, BAD_SHAPE), (2 * B, OK)):
        assert C.parse_instances_raw_yuv420p10_host(rec[:n], HS, WS, fmt, k)[0] == want, n
    assert C.parse_instances_raw_yuv420p10_host(rec, HS + 1, WS, fmt, k)[0] == BAD_SHAPE
    assert C.parse_instances_raw_yuv420p10_host(rec, HS, WS, "nv12", k)[0] == BAD_SHAPE


# ---- configuration ------------------------------------------------------------------------------

def cfg(**kw):
    return GaleConfig(topology_name="t", input_topic="in", output_topic="out", **kw).validate()


REFUSED = [
    (dict(input_format="json"), "--input-format raw", dict(input_format="json")),
    (dict(input_format="b64"), "--input-format raw", dict(input_format="b64")),
    (dict(input_layout="nchw"), "--input-layout nchw", dict(input_nchw=True)),
    (dict(model="lenet5"), "C = 1", dict(C=1)),
    (dict(input_size="33,32", input_resize="32,32"), "--input-size.*even", dict(rec_H=33)),
    (dict(input_size="32,33", input_resize="32,32"), "--input-size.*even", dict(rec_W=33)),
    (dict(input_dtype="f16"), "--input-dtype f16", dict(input_dtype="f16")),
    (dict(b64_ingest=True), "--b64-ingest", dict(b64_ingest=True)),
]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("kw,match,engine_kw", REFUSED,
                         ids=["json", "b64", "nchw", "C=1", "odd-HS", "odd-WS", "dtype", "ingest"])
def test_refusals_name_their_option(fmt, kw, match, engine_kw):
    with pytest.raises(ValueError, match=match):
        cfg(**{"input_format": "raw", "input_pixel_format": fmt, **kw})
    # the native engine refuses the same combination in a dict built by hand
    d = cfg(input_format="raw", input_pixel_format=fmt, input_yuv_matrix="bt709")
    d = d.engine_dict(32, 32, 3, 10)
    C.Engine(d)
    with pytest.raises(ValueError):
        C.Engine(dict(d, **engine_kw))


# ---- the stub engine ----------------------------------------------------------------------------

def test_stub_engine_splits_on_frame_boundaries():
    """The predictions of the frames sent one image a record; the record of 9 images over
    --max-batch 4 is split on frame boundaries and joined into one output."""
    counts, fmt = [1, 2, 9, 1], "yuv420p10le"
    sets = {f"r{i}".encode(): planes(n, 32, 32, 40 + i) for i, n in enumerate(counts)}
    kw = dict(max_batch=4, on_error="null", input_format="raw", input_pixel_format=fmt, **CIFAR)
    recs = [(k, encode_records_yuv420p10(*p, fmt, p[0].shape[0], j)[0])
            for k, (p, j) in sets.items()]
    got, st = serve(recs + [(b"short", recs[2][1][:-2])], **kw)
    assert got.pop(b"short") is None
    assert (st["yuv_records"], st["raw_records"], st["errors"], st["split_records"]) == \
        (len(counts), len(counts), 1, 1), st
    singles = [(k + b"/%d" % i, r) for k, (p, j) in sets.items()
               for i, r in enumerate(encode_records_yuv420p10(*p, fmt, 1, j))]
    one, _ = serve(singles, **kw)
    for k, (p, _) in sets.items():
        rows = [one[k + b"/%d" % i] for i in range(p[0].shape[0])]
        pre = b'{"predictions":['
        assert got[k] == pre + b",".join(r[len(pre):-2] for r in rows) + b"]}", k
