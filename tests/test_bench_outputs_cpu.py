"""bench.py's plain / --full split and --dump-outputs, on CPU stub replicas: a plain run times
its steps and prints the result line, --full adds the offered-load latency phase, and
--dump-outputs writes the last timed step's predictions ordered by input image."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STUB = ["--stub", "--steps", "3", "--warmup", "1", "--batch", "32", "--distinct", "64",
        "--replicas-per-gpu", "2", "--step-images", "256", "--min-warmup-s", "0.2",
        "--timeout", "120"]


def _bench(*extra):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", *STUB, *extra], cwd=ROOT,
                         capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert out.returncode == 0, out.stderr[-3000:]
    (r,) = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    return r


def _stub_reference(x):
    """StubReplica's forward (csrc/runtime/replica.cpp): logit k = (k + 1) * mean of channel
    k % C, softmax in double."""
    n, classes = len(x), 10
    m = x.astype(np.float64).reshape(n, -1, x.shape[-1]).mean(axis=1)
    logits = np.stack([(k + 1) * m[:, k % x.shape[-1]] for k in range(classes)], axis=1)
    logits = logits.astype(np.float32).astype(np.float64)  # (stored as float before the exp)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def test_plain_run_times_its_steps_and_dumps_outputs(tmp_path):
    from gale.data import synthetic_images

    r = _bench("--dump-outputs", str(tmp_path / "out"))
    assert r["steps"] == 3 and r["full"] is False and r["value"] > 0
    assert r["unit"] == "images/s" and r["higher_is_better"] is True and r["dtype"] == "bf16"
    assert r["ms_per_step"] == pytest.approx(r["timed_s"] * 1e3 / 3, rel=2e-2, abs=1e-2)
    # no offered-load phase in a plain run: the latency is the backlog's fetch -> ack
    assert "latency_samples" not in r and "latency_stages_ms" not in r
    assert r["latency_definition"].startswith("fetch -> produce-ack under the backlog")
    d = r["dump_outputs"]
    assert d["file"] == "predictions.npy" and d["shape"] == [64, 10]
    assert d["images_unanswered"] == 0 and d["repeat_max_abs_diff"] == 0.0
    assert d["output_records"] == 256  # the last step's records, no more
    got = np.load(tmp_path / "out" / "predictions.npy")
    assert got.dtype == np.float32 and got.shape == (64, 10)
    ref = _stub_reference(synthetic_images(64, (32, 32, 3), seed=1234))
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-6)


def test_full_run_adds_the_latency_phase():
    r = _bench("--full", "--stub-null", "--latency-s", "0.5", "--latency-warmup-s", "0.2")
    assert r["full"] is True and r["steps"] == 3 and r["value"] > 0
    assert r["latency_samples"] > 0
    assert r["latency_definition"].startswith("Kafka record append -> prediction produce-ack")
    assert r["latency_offered_img_s"] == pytest.approx(0.8 * r["value"], rel=1e-3)


def test_latency_options_need_full():
    out = subprocess.run([sys.executable, "bench.py", "--stub", "--latency-sweep", "0.5"],
                         cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "need --full" in out.stderr
