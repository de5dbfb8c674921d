"""PixelSource (csrc/codec/pixel_source.h), the one holder of what a b64 string carries, without a
GPU: the stand-alone sanitizer driver (csrc/tests/pixel_source_check.cpp) - the seven names, the
bytes of a string, every refusal by its text, the ingest's dimensions and the host dispatch
against the three public decoders on mutated and truncated records."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None,
                    reason="needs ROCm clang++ and make")
def test_pixel_source_under_address_and_ub_sanitizers():
    target = "build/asan/pixel_source_check"
    b = subprocess.run(["make", "-C", ROOT, target], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, target)], capture_output=True, text=True, timeout=300,
                       env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "pixel_source_check OK" in out
