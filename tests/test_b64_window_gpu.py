"""The lane window of the four b64 entry points (csrc/kernels/b64_decode.cuh: load_window,
window_bad, and b64_packed.hip's copy of them), pinned at every character position:
b64_decode_instances, b64_packed_instances, b64_yuv_instances and ingest_crc_b64, each at the
smallest strings that have every padding case.

Per case ONE launch of L + 1 one-image records of the same image: image i starts at phase
i mod 16; image i < L has character i replaced by '*' - or, where character i is a '=' of the
padding, by 'A' -; image L is clean. The verdicts must be those of the format's host parser on
the same records - 2 exactly where the host says BAD_NUMBER, at every position, none skipped -,
the clean image the oracle's bits, and the floats around the output untouched."""

import base64

import numpy as np
import pytest
import torch

from gale import ops
from gale._native import native
from gale.models.preprocess import PixelUnpack, YuvConvert

pytestmark = pytest.mark.gpu

C = native()
IMG = np.dtype([("off", "<i8"), ("slot", "<i4"), ("rec", "<i4")])
assert IMG.itemsize == C.B64_IMAGE_BYTES
OK, BAD_NUMBER = 0, 5
SENTINEL = -7.0

# name -> (HS, WS, C of a string's bytes, B, L, '=' characters)
CASES = {
    "rgb": (5, 4, 3, 60, 80, 0),
    "gray": (4, 4, 1, 16, 24, 2),
    "rgba": (5, 7, 4, 140, 188, 1),
    "bgr24": (5, 7, 3, 105, 140, 0),
    "i420": (6, 10, None, 90, 120, 0),
    "nv12": (6, 10, None, 90, 120, 0),
    "ingest-5x4x3": (5, 4, 3, 60, 80, 0),
    "ingest-4x4x1": (4, 4, 1, 16, 24, 2),
}


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


def mutants(clean: bytes):
    """The L + 1 strings of a case."""
    out = []
    for i in range(len(clean)):
        s = bytearray(clean)
        s[i] = ord("A") if clean[i:i + 1] == b"=" else ord("*")
        out.append(bytes(s))
    return out + [clean]


def host_parse(name, record, HS, WS, Cb):
    if name in ("i420", "nv12"):
        yc = YuvConvert(name)
        return C.parse_instances_yuv_host(record, HS, WS, name, [*yc.coeffs(), yc.yo])
    if name in ("gray", "rgba", "bgr24"):
        return C.parse_instances_packed_host(record, HS, WS, name)
    return C.parse_instances_b64_host(record, HS, WS, Cb)


def oracle(name, image, HS, WS, Cb):
    """float32 bits of the clean image: the numpy oracle of the format."""
    if name in ("i420", "nv12"):
        return YuvConvert(name).apply(image, HS, WS).astype(np.float32)
    if name in ("gray", "rgba", "bgr24"):
        return PixelUnpack(name).apply(image, HS, WS).astype(np.float32)
    return image.reshape(HS, WS, Cb).astype(np.float32)


@pytest.mark.parametrize("name", list(CASES))
def test_verdict_at_every_character_position(name):
    HS, WS, Cb, B, L, pad = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 20261021)
    image = rng.integers(0, 256, B, dtype=np.uint8)
    clean = base64.b64encode(image.tobytes())
    assert len(clean) == L and len(clean) - len(clean.rstrip(b"=")) == pad
    strings = mutants(clean)
    n = L + 1
    assert len(strings) == n and len(set(strings)) == n

    # the host parser's verdict on each one-image record, and its floats for the clean one
    host = [host_parse(name, b'{"instances":[{"b64":"' + s + b'"}]}', HS, WS, Cb)
            for s in strings]
    verdicts = np.array([st for st, _ in host])
    assert set(verdicts.tolist()) <= {OK, BAD_NUMBER} and verdicts[-1] == OK
    want_status = np.where(verdicts == BAD_NUMBER, 2, 0).astype(np.int32)
    # (every mutation is one the parsers refuse: nothing is left unjudged inside a string)
    assert (want_status[:L] == 2).all()

    raw, offs = stage(strings, [i % 16 for i in range(n)])
    assert [o % 16 for o in offs] == [i % 16 for i in range(n)]
    tab = np.zeros(n, dtype=IMG)
    tab["off"], tab["slot"], tab["rec"] = offs, range(n), range(n)
    d_raw = torch.from_numpy(raw.copy()).cuda()
    d_tab = torch.from_numpy(tab.view(np.int32).reshape(-1, 4).copy()).cuda()
    Co = 3 if Cb is None or name in ("gray", "rgba", "bgr24") else Cb   # floats per pixel
    per = HS * WS * Co
    flat = torch.full((n * per + 8,), SENTINEL, device="cuda")
    out = flat[4:4 + n * per]
    assert out.data_ptr() % 16 == 0
    status = torch.full((n,), 7 if name.startswith("ingest") else 0, dtype=torch.int32,
                        device="cuda")
    if name.startswith("ingest"):
        assert L <= C.B64_CHUNK_CHARS     # one decode workgroup, one verdict word, per image
        ops.ingest_crc_b64(d_raw, (HS, WS, Cb), arena=out.view(n, HS, WS, Cb), table=d_tab,
                           wg_bad=status)
    elif name == "rgb":
        ops.b64_decode_instances(d_raw, d_tab, (HS, WS, Cb), out, status)
    elif name in ("i420", "nv12"):
        ops.b64_yuv_instances(d_raw, d_tab, (HS, WS), out, status, YuvConvert(name))
    else:
        ops.b64_packed_instances(d_raw, d_tab, (HS, WS), out, status, PixelUnpack(name))
    torch.cuda.synchronize()

    got_status = status.cpu().numpy()
    wrong = np.flatnonzero(got_status != want_status)
    assert wrong.size == 0, (name, wrong.tolist(), got_status[wrong].tolist())
    f = flat.cpu().numpy()
    assert (f[:4] == SENTINEL).all() and (f[4 + n * per:] == SENTINEL).all()
    got_clean = f[4 + L * per:4 + n * per]
    want = oracle(name, image, HS, WS, Cb).reshape(-1)
    assert np.array_equal(got_clean.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(host[-1][1].reshape(-1).view(np.uint32), want.view(np.uint32))
