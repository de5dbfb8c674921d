"""Triangle-filter chroma for b64 i420 / nv12 records (--input-yuv-chroma linear) on the host: the
oracle (YuvLinearConvert) against the nearest oracle, against a loop-form upsampler through the
yuv444p oracle and against the host twin, the stub engine, the refusals and the default. Every
comparison of outputs is on the bits."""

import numpy as np
import pytest

from gale._native import native
from gale.cli import parse_topology_args
from gale.config import GaleConfig, from_sources
from gale.data import encode_records_b64, encode_records_yuv, pack_yuv420
from gale.models.preprocess import InputPrep, YuvConvert, YuvLinearConvert, YuvPlanarConvert
from test_input_raw_cpu import CIFAR, OK, serve

C = native()
FORMATS = ("i420", "nv12")
TABLES = [(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]
SIZES = [(2, 2), (2, 4), (4, 2), (6, 18), (32, 32)]
PREP = InputPrep.build(3, CIFAR["input_scale"], CIFAR["input_mean"], CIFAR["input_std"])


def planes(n, HS, WS, seed):
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(0, 256, (n, h, w), dtype=np.uint8)
                 for h, w in ((HS, WS), (HS // 2, WS // 2), (HS // 2, WS // 2)))


def fancy(C):
    """libjpeg's h2v2_fancy_upsample loop on one plane [ch, cw]: every column takes 3 of its own
    sum and 1 of the last / next one, which at the first / last column is its own (4 s)."""
    C = C.astype(np.int64)
    out = np.empty((2 * C.shape[0], 2 * C.shape[1]), np.int64)
    for y in range(out.shape[0]):
        s = 3 * C[y >> 1] + C[min(max((y >> 1) + (1 if y & 1 else -1), 0), C.shape[0] - 1)]
        last, nxt = np.r_[s[0], s[:-1]], np.r_[s[1:], s[-1]]
        out[y, 0::2], out[y, 1::2] = (3 * s + last + 8) >> 4, (3 * s + nxt + 7) >> 4
    return out


@pytest.mark.parametrize("fmt", FORMATS)
def test_constant_chroma_equals_nearest(fmt):
    Y, U, V = planes(4, 6, 10, 1)
    U[:], V[:] = U[:, :1, :1], V[:, :1, :1]
    frames = pack_yuv420(Y, U, V, fmt)
    assert np.array_equal(YuvLinearConvert(fmt, "bt709", "full").apply(frames, 6, 10),
                          YuvConvert(fmt, "bt709", "full").apply(frames, 6, 10))


@pytest.mark.parametrize("HS,WS", SIZES, ids=str)
@pytest.mark.parametrize("fmt", FORMATS)
def test_oracle_is_yuv444p_of_the_loop_upsampler_and_the_host_twin(fmt, HS, WS):
    matrix, range_ = TABLES[(HS + WS // 2) % 4]
    yc = YuvLinearConvert(fmt, matrix, range_)
    Y, U, V = planes(2, HS, WS, HS * 100 + WS)
    frames = pack_yuv420(Y, U, V, fmt)
    want = yc.apply(frames, HS, WS)
    up = [np.stack([fancy(c) for c in P]).astype(np.uint8) for P in (U, V)]
    assert all(u.shape == Y.shape for u in up)
    f444 = np.concatenate([P.reshape(2, -1) for P in (Y, *up)], axis=1)
    assert np.array_equal(want, YuvPlanarConvert("yuv444p", matrix, range_).apply(f444, HS, WS))
    assert not np.array_equal(want, YuvConvert(fmt, matrix, range_).apply(frames, HS, WS)) \
        or (HS, WS) == (2, 2)
    k, (a, b) = [*yc.coeffs(), yc.yo], PREP.coeffs()
    for i, fr in enumerate(frames):
        rgb, f32 = C.yuv420_linear_to_rgb_host(fr.tobytes(), HS, WS, fmt, k)
        assert np.array_equal(rgb, want[i]) and np.array_equal(f32, want[i].astype(np.float32))
        _, f32p = C.yuv420_linear_to_rgb_host(fr.tobytes(), HS, WS, fmt, k, a=a, b=b)
        assert np.array_equal(f32p.view(np.uint32),
                              PREP.apply(want[i].astype(np.float32)).view(np.uint32))
    st, out = C.parse_instances_yuv_host(encode_records_yuv(Y, U, V, fmt, 2)[0], HS, WS, fmt, k,
                                         linear=True)
    assert st == OK and np.array_equal(out, want.astype(np.float32))


def test_stub_topology_equals_rgb_records_of_the_oracle():
    """One record of 5 images over --max-batch 4; the same images sent as rgb b64 records."""
    yc = YuvLinearConvert("nv12", "bt601", "full")
    sets = {f"r{i}".encode(): planes(n, 32, 32, 20 + i) for i, n in enumerate([1, 2, 5])}
    kw = dict(max_batch=4, on_error="null", input_format="b64", **CIFAR)
    want, _ = serve([(k, encode_records_b64(x, x.shape[0])[0]) for k, x in
                     ((k, yc.apply(pack_yuv420(*p, "nv12"), 32, 32)) for k, p in sets.items())],
                    **kw)
    recs = [(k, encode_records_yuv(*p, "nv12", p[0].shape[0])[0]) for k, p in sets.items()]
    yuv = dict(input_pixel_format="nv12", input_yuv_range="full")
    got, st = serve(recs, input_yuv_chroma="linear", **yuv, **kw)
    assert got == want and all(v is not None for v in got.values())
    assert (st["yuv_records"], st["errors"], st["split_records"]) == (3, 0, 1), st
    nearest, _ = serve(recs, **yuv, **kw)
    assert nearest != got


def cfg(**kw):
    return GaleConfig(topology_name="t", input_topic="in", output_topic="out", **kw).validate()


REFUSED = [dict(input_format="b64"), dict(input_format="json"),
           dict(input_format="b64", input_pixel_format="yuv444p"),
           dict(input_format="raw", input_pixel_format="yuyv422"),
           dict(input_format="b64", input_pixel_format="bgr24"),
           dict(input_format="raw", input_pixel_format="p010le")]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda d: "-".join(d.values()))
def test_refusals_name_the_option(kw):
    cfg(**kw, input_yuv_chroma="nearest")  # (naming the default is always allowed)
    with pytest.raises(ValueError, match="--input-yuv-chroma linear"):
        cfg(**kw, input_yuv_chroma="linear")
    with pytest.raises(ValueError, match="yuv_chroma"):  # a dict built by hand
        C.Engine(dict(cfg(**kw).engine_dict(32, 32, 3, 10), yuv_chroma="linear"))


def test_the_engine_dict_and_the_width_bound():
    ok = dict(input_format="b64", input_pixel_format="i420")
    d = cfg(**ok, input_yuv_chroma="linear").engine_dict(32, 32, 3, 10)
    assert d["yuv_chroma"] == "linear"
    C.Engine(d)
    C.Engine(dict(d, H=2, W=C.YUV_LINEAR_MAX_WS))
    for bad in (dict(H=2, W=C.YUV_LINEAR_MAX_WS + 2), dict(yuv_chroma="bilinear")):
        with pytest.raises(ValueError, match="yuv_chroma"):
            C.Engine(dict(d, **bad))
    assert C.b64_yuv_linear_lds_bytes(C.YUV_LINEAR_MAX_WS, 1) <= C.YUV_LDS_BUDGET \
        < C.b64_yuv_linear_lds_bytes(C.YUV_LINEAR_MAX_WS + 2, 1)
    # nearest, named or defaulted: the engine dict of today
    assert cfg(**ok, input_yuv_chroma="nearest").engine_dict(32, 32, 3, 10) == \
        cfg(**ok).engine_dict(32, 32, 3, 10)
    assert "yuv_chroma" not in cfg(**ok).engine_dict(32, 32, 3, 10)
    assert type(cfg(**ok).input_yuv()) is YuvConvert


def test_three_sources_and_their_precedence(tmp_path):
    toml = tmp_path / "g.toml"
    toml.write_text('[gale]\ninput-format = "b64"\ninput-pixel-format = "i420"\n'
                    'input-yuv-chroma = "linear"\n')
    base = dict(cli=dict(topology_name="t"), toml_path=str(toml))
    assert from_sources(env={}, **base).input_yuv() == YuvLinearConvert("i420")
    env = {"GALE_INPUT_YUV_CHROMA": "nearest"}
    assert from_sources(env=env, **base).input_yuv_chroma == "nearest"
    c = parse_topology_args(["t", "in", "out", "--config", str(toml), "--input-yuv-chroma",
                             "linear", "--input-pixel-format", "nv12"])
    assert c.input_yuv() == YuvLinearConvert("nv12")
