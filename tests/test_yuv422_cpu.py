"""Packed YUV 4:2:2 frame records (--input-pixel-format yuyv422 | uyvy422) on the host: twin
against oracle, the tie to 4:2:0, the distance from the real matrix, configuration, stub engine.
Every comparison is on the bits."""

import numpy as np
import pytest

from gale._native import native
from gale.config import GaleConfig
from gale.data import encode_records_b64, encode_records_yuv422, pack_yuv420, pack_yuv422
from gale.models.preprocess import InputPrep, Yuv422Convert, YuvConvert

C = native()
K = C.kafka
TABLES = [(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]
FORMATS = ("yuyv422", "uyvy422")
SIZES = [(1, 2), (3, 2), (5, 6), (7, 10)]
EDGE = (0, 16, 128, 235, 240, 255)
CIFAR_MEAN_S = "0.4914,0.4822,0.4465"
CIFAR_STD_S = "0.2470,0.2435,0.2616"
PREP = InputPrep.build(3, 1 / 255, CIFAR_MEAN_S, CIFAR_STD_S)


def planes(n, HS, WS, seed):
    """Y [n, HS, WS], U, V [n, HS, WS/2]: half of the samples from EDGE (both clamps fire)."""
    rng = np.random.default_rng(seed)

    def draw(shape):
        return np.where(rng.random(shape) < 0.5, rng.choice(EDGE, shape),
                        rng.integers(0, 256, shape)).astype(np.uint8)

    return draw((n, HS, WS)), draw((n, HS, WS // 2)), draw((n, HS, WS // 2))


@pytest.mark.parametrize("HS,WS", SIZES)
@pytest.mark.parametrize("matrix,range_", TABLES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_host_twin_equals_the_oracle(fmt, matrix, range_, HS, WS):
    yc = Yuv422Convert(fmt, matrix, range_)
    Y, U, V = planes(4, HS, WS, HS * 100 + WS)
    frames = pack_yuv422(Y, U, V, fmt)
    assert frames.shape == (4, Yuv422Convert.frame_bytes(HS, WS)) == (4, 2 * HS * WS)
    want = yc.apply(frames, HS, WS)
    k, (a, b) = [*yc.coeffs(), yc.yo], PREP.coeffs()
    for i, fr in enumerate(frames):
        rgb, f32 = C.yuv422_to_rgb_host(fr.tobytes(), HS, WS, fmt, k)
        assert np.array_equal(rgb, want[i]) and np.array_equal(f32, want[i].astype(np.float32))
        _, f32p = C.yuv422_to_rgb_host(fr.tobytes(), HS, WS, fmt, k, a=a, b=b)
        assert np.array_equal(f32p.view(np.uint32),
                              PREP.apply(want[i].astype(np.float32)).view(np.uint32))
    for enc in ("b64", "raw"):  # ... and the record parsers of either encoding
        st, out = C.parse_instances_yuv422_host(encode_records_yuv422(Y, U, V, fmt, 4, enc)[0],
                                                HS, WS, fmt, k, raw=enc == "raw")
        assert st == 0 and np.array_equal(out, want.astype(np.float32)), enc


@pytest.mark.parametrize("fmt", FORMATS)
def test_repeated_chroma_rows_give_the_420_result(fmt):
    """A 4:2:2 frame whose odd rows repeat the chroma of the row above is the 4:2:0 frame."""
    HS, WS = 6, 10
    Y, U, V = planes(3, HS, WS, 5)
    U, V = U[:, ::2], V[:, ::2]                                    # [3, HS/2, WS/2]
    got = Yuv422Convert(fmt, "bt709", "limited").apply(
        pack_yuv422(Y, np.repeat(U, 2, axis=1), np.repeat(V, 2, axis=1), fmt), HS, WS)
    want = YuvConvert("i420", "bt709", "limited").apply(pack_yuv420(Y, U, V, "i420"), HS, WS)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("matrix,range_", TABLES)
def test_distance_from_the_real_valued_matrix(matrix, range_):
    """A seeded sample: the unclamped result within 0.5 + 3 * 255 * 2^-21 of the real matrix."""
    yc = Yuv422Convert("uyvy422", matrix, range_)
    Y, U, V = planes(1, 64, 64, 11)
    Y, U, V = Y[0], np.repeat(U[0], 2, axis=-1), np.repeat(V[0], 2, axis=-1)
    sy, crv, cgu, cgv, cbu = (float(q) for q in yc.rationals())
    yy, u, v = sy * (Y.astype(np.float64) - yc.yo), U - 128.0, V - 128.0
    real = (yy + crv * v, yy + cgu * u + cgv * v, yy + cbu * u)
    worst = max(float(np.abs((a >> 20) - r).max()) for a, r in zip(yc.accumulators(Y, U, V), real))
    assert worst <= 0.5 + 3 * 255 * 2.0 ** -21


# ---- configuration ------------------------------------------------------------------------------

def cfg(**kw):
    return GaleConfig(topology_name="t", input_topic="in", output_topic="out", **kw).validate()


REFUSED = [
    (dict(input_format="json"), "--input-format b64 or raw", dict(input_format="json")),
    (dict(input_format="b64", input_layout="nchw"), "--input-layout nchw", dict(input_nchw=True)),
    (dict(input_format="raw", model="lenet5"), "C = 1", dict(C=1)),
    (dict(input_format="b64", input_size="32,33", input_resize="32,32"), "--input-size.*even WS",
     dict(rec_H=32, rec_W=33)),
    (dict(input_format="raw", input_dtype="f16"), "--input-dtype f16", dict(input_dtype="f16")),
    (dict(input_format="raw", b64_ingest=True), "--b64-ingest", dict(b64_ingest=True)),
    (dict(input_format="b64", input_pixel_format="yuyv"), "input_pixel_format",     # no "422"
     dict(pixel_format="yuyv")),
]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("kw,match,engine_kw", REFUSED, ids=[r[1] for r in REFUSED])
def test_refusals_name_their_option(fmt, kw, match, engine_kw):
    with pytest.raises(ValueError, match=match):
        cfg(**{"input_pixel_format": fmt, **kw})
    # the native engine refuses the same combination in a dict built by hand
    d = cfg(input_format="raw", input_pixel_format=fmt).engine_dict(32, 32, 3, 10)
    with pytest.raises(ValueError):
        C.Engine(dict(d, **engine_kw))


# ---- the stub engine end to end -----------------------------------------------------------------

MAX_BATCH, CLASSES = 4, 10
COUNTS = [1, 2, 1, 6, 3]        # r3: one record over max_batch (fragments of 4 and 2)


def run_stub(records, input_format, **opts):
    broker = K.Broker()
    broker.start()
    try:
        broker.create_topic("in", 1)
        broker.create_topic("out", 1)
        for key, value in records:
            broker.append("in", 0, [value], [key])
        c = cfg(bootstrap=f"127.0.0.1:{broker.port}", start_offset="earliest", stub=True,
                max_batch=MAX_BATCH, max_wait_us=500, output_key="input", on_error="null",
                input_format=input_format, input_scale=1 / 255, input_mean=CIFAR_MEAN_S,
                input_std=CIFAR_STD_S, **opts)
        d = c.engine_dict(32, 32, 3, CLASSES)
        d["max_records"] = len(records)
        eng = C.Engine(d)
        eng.add_stub_replica(MAX_BATCH, 0, True, -1)
        eng.start()
        assert eng.wait(30000), eng.stats()
        eng.stop()
        out = broker.read("out", 0)
    finally:
        broker.stop()
    assert len(out) == len(records)
    return {r["key"]: r["value"] for r in out}, dict(eng.stats())


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("enc", ["b64", "raw"])
def test_stub_engine_equals_rgb_records_of_the_oracle(enc, fmt):
    HS, WS = 32, 32
    sets = {f"r{i}".encode(): planes(n, HS, WS, 23 + i) for i, n in enumerate(COUNTS)}
    yc = Yuv422Convert(fmt, "bt709", "limited")
    rgb = {k: yc.apply(pack_yuv422(*p, fmt), HS, WS) for k, p in sets.items()}
    want, wstats = run_stub([(k, encode_records_b64(x, x.shape[0])[0]) for k, x in rgb.items()],
                            "b64")
    assert wstats["yuv_records"] == 0
    recs = [(k, encode_records_yuv422(*p, fmt, p[0].shape[0], enc)[0]) for k, p in sets.items()]
    recs.insert(2, (b"short", recs[0][1][:-4]))                     # bad_shape in either encoding
    got, stats = run_stub(recs, enc, input_pixel_format=fmt, input_yuv_matrix="bt709")  # accepted
    assert got.pop(b"short") is None
    assert got == want and all(v is not None for v in want.values())
    assert stats["yuv_records"] == len(COUNTS), stats
    assert stats["split_records"] == 1 and stats["errors"] == 1, stats
