"""Device ingest of base64 image records (--b64-ingest) without a GPU: the option's sources and
validation, the host plan (CRC windows, dense arena slots, string offsets, the arena cut, section
alignment) against a Python re-derivation, and a stand-alone sanitizer run of the plan."""

import os
import shutil
import subprocess

import numpy as np
import pytest

from gale._native import native
from gale.cli import parse_topology_args
from gale.config import GaleConfig, from_sources
from gale.data import encode_records_b64, encode_records_text

C = native()
K = C.kafka
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 2, 1)
PER = 4
CHARS = 8                      # 4 * ceil(4 / 3)
ATTR = C.BATCH_ATTR_OFFSET


# ---- 1. configuration ---------------------------------------------------------------------------

def test_config_sources(tmp_path):
    cli = parse_topology_args(["t", "in", "out", "--input-format", "b64", "--b64-ingest"])
    env = from_sources(cli=dict(topology_name="t", input_format="b64"),
                       env={"GALE_B64_INGEST": "1"})
    toml = tmp_path / "g.toml"
    toml.write_text('[gale]\ninput-format = "b64"\nb64-ingest = true\n')
    tom = from_sources(cli=dict(topology_name="t"), env={}, toml_path=str(toml))
    for cfg in (cli, env, tom):
        assert cfg.b64_ingest is True
        d = cfg.engine_dict(32, 32, 3, 10)
        assert d["b64_ingest"] is True and d["input_format"] == "b64"
        assert d["text_pack"] is False          # text packing stays off in b64 mode
    # CLI > env > TOML
    assert from_sources(cli=dict(topology_name="t", b64_ingest=False),
                        env={"GALE_B64_INGEST": "1"}, toml_path=str(toml)).b64_ingest is False
    assert from_sources(cli=dict(topology_name="t"), env={"GALE_B64_INGEST": "0"},
                        toml_path=str(toml)).b64_ingest is False
    off = parse_topology_args(["t", "in", "out", "--input-format", "b64", "--no-b64-ingest"])
    assert off.b64_ingest is False


def test_default_is_off_and_json_refuses_it():
    base = GaleConfig(topology_name="t").validate()
    assert base.b64_ingest is False
    assert base.engine_dict(32, 32, 3, 10)["b64_ingest"] is False
    b64 = GaleConfig(topology_name="t", input_format="b64").validate()
    assert b64.engine_dict(32, 32, 3, 10)["b64_ingest"] is False
    with pytest.raises(ValueError):
        GaleConfig(topology_name="t", input_format="json", b64_ingest=True).validate()
    with pytest.raises(ValueError):
        parse_topology_args(["t", "in", "out", "--b64-ingest"])
    with pytest.raises(ValueError):    # the native engine refuses the pair too
        C.Engine(dict(base.engine_dict(4, 3, 3, 10), b64_ingest=True))


# ---- 2. the host plan ---------------------------------------------------------------------------

def fetch_of(counts, bad_at, seed=3):
    """A fetch-like buffer: per record a batch of its own - framing bytes, then the value. Record
    bad_at is a numeric record (non-OK scan). Returns (buffer, batches, plan records, flat
    offsets, per record offsets)."""
    rng = np.random.default_rng(seed)
    buf = bytearray()
    batches, recs, flat, per_rec = [], [], [], []
    for i, n in enumerate(counts):
        b0 = len(buf)
        buf += bytes(ATTR + 11 + i)
        x = rng.integers(0, 256, (n,) + SHAPE, dtype=np.uint8)
        v = encode_records_text(x, n)[0] if i == bad_at else encode_records_b64(x, n)[0]
        v_off = len(buf)
        buf += v
        batches.append((b0, len(buf) - b0))
        st, arr_off, arr_len, images = C.scan_instances_b64(bytes(v), *SHAPE)
        offs = []
        if st == 0:
            offs = C.b64_image_offsets(bytes(v[arr_off:arr_off + arr_len]), *SHAPE)
            assert len(offs) == images == n
        else:
            images = 0
        recs.append((st, images, v_off, len(v), arr_off))
        flat += offs
        per_rec.append(offs)
    return bytes(buf), batches, recs, flat, per_rec


def windows_of(batches):
    """GpuIngest's windows: aligned to each batch's end, the first one short."""
    wins, per_batch = [], []
    for off, ln in batches:
        rs, re = off + ATTR, off + ln
        n = -(-(re - rs) // 4096)
        per_batch.append((len(wins), n))
        for k in range(n):
            wins.append((re - 4096 * (n - 1 - k), (re - rs) - 4096 * (n - 1) if k == 0 else 4096))
    return wins, per_batch


COUNTS = [1, 3, 1, 2]          # records of 1, 3 and 2 images, a bad one (index 2) between them
BAD = 2


def test_plan_dense_slots_offsets_and_sections():
    buf, batches, recs, flat, per_rec = fetch_of(COUNTS, BAD)
    assert recs[BAD][0] != 0 and all(r[0] == 0 for i, r in enumerate(recs) if i != BAD)
    p = C.plan_b64_ingest(batches, recs, flat, *SHAPE, arena_bytes=64 * PER * 4,
                          fetch_size=len(buf))
    # dense slots 0..5 in record order, skipping the bad record
    assert p["slot0"] == [0, 1, -1, 4] and p["img0"] == [0, 1, -1, 4]
    assert [s for _, s, _ in p["images"]] == list(range(6))
    assert [r for _, _, r in p["images"]] == [0, 1, 1, 1, 3, 3]
    want_off = [recs[i][2] + recs[i][4] + o for i in (0, 1, 3) for o in per_rec[i]]
    assert [o for o, _, _ in p["images"]] == want_off
    for o, _, _ in p["images"]:        # each offset is a string's first character
        assert buf[o - 1:o] == b'"' and buf[o + CHARS:o + CHARS + 1] == b'"'
    assert p["chunks_per_image"] == 1
    wins, per_batch = windows_of(batches)
    assert p["windows"] == wins and [tuple(x) for x in p["batch_windows"]] == per_batch
    # the span holds every batch and every OK record
    assert p["lo"] == 0 and p["hi"] == len(buf)
    # plan [CrcChunk x nc][B64Image x ni], results [crc x nc][wg_bad x ni * chunks]: 16-aligned
    for k in ("o_chunks", "o_imgs", "plan_bytes", "o_crc", "o_bad", "result_bytes"):
        assert p[k] % 16 == 0, k
    nc, ni = len(wins), 6
    assert p["o_chunks"] == 0 and p["o_imgs"] >= 16 * nc
    assert p["plan_bytes"] >= p["o_imgs"] + 16 * ni
    assert p["o_crc"] == 0 and p["o_bad"] >= 4 * nc and p["result_bytes"] >= p["o_bad"] + 4 * ni
    # without CRC checks: no windows, the same descriptors
    q = C.plan_b64_ingest(batches, recs, flat, *SHAPE, arena_bytes=64 * PER * 4,
                          fetch_size=len(buf), check_crcs=False)
    assert q["windows"] == [] and q["images"] == p["images"] and q["o_imgs"] == 0


def test_plan_crc_windows_for_batch_lengths():
    """Batch lengths 1, 4096, 4097 and 9000 past the attributes offset."""
    lens = [1, 4096, 4097, 9000]
    batches = []
    pos = 7
    for ln in lens:
        batches.append((pos, ATTR + ln))
        pos += ATTR + ln + 5
    p = C.plan_b64_ingest(batches, [], [], *SHAPE, arena_bytes=0, fetch_size=pos)
    wins, per_batch = windows_of(batches)
    assert p["windows"] == wins
    assert [n for _, n in per_batch] == [1, 1, 2, 3]
    assert [tuple(x) for x in p["batch_windows"]] == per_batch
    assert [ln for _, ln in wins] == [1, 4096, 1, 4096, 808, 4096, 4096]
    for (off, ln), (first, n) in zip(batches, per_batch):
        assert wins[first + n - 1][0] == off + ln                 # aligned to the batch's end
        assert wins[first][0] - wins[first][1] == off + ATTR      # from the attributes on
    assert p["images"] == [] and p["o_bad"] % 16 == 0 and p["plan_bytes"] % 16 == 0


def test_plan_arena_cut():
    counts = [1, 3, 2, 1]
    buf, batches, recs, flat, _ = fetch_of(counts, bad_at=-1)
    # capacity for 4 images: the third record (2 images) does not fit, and a record that does
    # not fit ends the assignment - the 1-image record behind it stays without slots too
    p = C.plan_b64_ingest(batches, recs, flat, *SHAPE, arena_bytes=4 * PER * 4,
                          fetch_size=len(buf))
    assert p["slot0"] == [0, 1, -1, -1]
    assert [s for _, s, _ in p["images"]] == [0, 1, 2, 3]
    # the issue's case: records of 1, 3 and 2 images - the third, and only it, gets no slots
    buf3, b3, r3, f3, _ = fetch_of([1, 3, 2], bad_at=-1)
    p = C.plan_b64_ingest(b3, r3, f3, *SHAPE, arena_bytes=4 * PER * 4, fetch_size=len(buf3))
    assert p["slot0"] == [0, 1, -1] and len(p["images"]) == 4
    # one byte short of 4 images: the second record does not fit either
    p = C.plan_b64_ingest(b3, r3, f3, *SHAPE, arena_bytes=4 * PER * 4 - 1, fetch_size=len(buf3))
    assert p["slot0"] == [0, -1, -1]
    # capacity 0: no record gets slots and nothing throws; the windows are still planned
    p = C.plan_b64_ingest(b3, r3, f3, *SHAPE, arena_bytes=0, fetch_size=len(buf3))
    assert p["slot0"] == [-1, -1, -1] and p["images"] == [] and len(p["windows"]) == 3
    assert p["lo"] == 0 and p["hi"] == len(buf3)      # the records stay resident in the mirror


def test_plan_refuses_contradictory_scans():
    buf, batches, recs, flat, _ = fetch_of([2, 1], bad_at=-1)
    kw = dict(arena_bytes=1 << 20, fetch_size=len(buf))
    with pytest.raises(ValueError):                   # fewer offsets than images
        C.plan_b64_ingest(batches, recs, flat[:-1], *SHAPE, **kw)
    far = list(flat)
    far[1] = recs[0][3]                               # a string starting at the value's end
    with pytest.raises(ValueError):
        C.plan_b64_ingest(batches, recs, far, *SHAPE, **kw)
    with pytest.raises(ValueError):                   # a batch past the fetch
        C.plan_b64_ingest(batches + [(len(buf) - 4, 64)], recs, flat, *SHAPE, **kw)


def test_b64_engine_accepts_gpu_ingest_only_with_the_option():
    """enable_gpu_ingest keeps refusing b64 without b64_ingest (ValueError before any device is
    touched)."""
    cfg = GaleConfig(topology_name="t", input_topic="in", output_topic="out",
                     input_format="b64").validate()
    eng = C.Engine(cfg.engine_dict(32, 32, 3, 10))
    with pytest.raises(ValueError, match="b64_ingest"):
        eng.enable_gpu_ingest(0, 1, 20)


# ---- 3. stand-alone sanitizer run ---------------------------------------------------------------

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None,
                    reason="needs ROCm clang++ and make")
def test_plan_under_address_and_ub_sanitizers():
    target = "build/asan/b64_plan_check"
    b = subprocess.run(["make", "-C", ROOT, target], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, target), "3000"], capture_output=True, text=True,
                       timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "all checks passed" in out
    assert "AddressSanitizer" not in out and "runtime error" not in out
