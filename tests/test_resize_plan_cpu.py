"""The input resize's host plan (csrc/runtime/resize_plan.h) without a GPU: the device image of
the tables that a replica uploads - one allocation, six sections, each on a 16-byte boundary,
zero padding - as seen from Python against the table builders, on the kernel tests' shapes in
both forms, and the stand-alone sanitizer driver (csrc/tests/resize_plan_check.cpp)."""

import os
import shutil
import subprocess

import numpy as np
import pytest

from gale._native import native
from test_input_antialias_cpu import KERNEL_SHAPES as AA_SHAPES
from test_input_resize_cpu import CROP, SHAPES

C = native()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the shapes of both kernel tests (tests/test_input_resize_gpu.py adds the last two to SHAPES)
KERNEL_SHAPES = list(dict.fromkeys(AA_SHAPES + SHAPES + [CROP, (9, 6, 9, 6, 8, 4, 1),
                                                         (7, 5, 9, 11, 6, 7, 3)]))
CASES = [(d, aa) for d in KERNEL_SHAPES for aa in (False, True)
         if not aa or (d[0] <= 8 * d[2] and d[1] <= 8 * d[3])]


def sections(dims, antialias):
    """resize_device_image's bytes sliced by its offsets into the six tables (the payload lengths
    are the tables': H or W entries, the antialiased weights H * ty and W * tx), the launch
    figures, and the mask of the bytes that belong to no payload."""
    HS, WS, HR, WR, H, W, _ = dims
    blob, offs, fig = C.resize_device_image(HS, WS, HR, WR, H, W, antialias)
    assert blob.dtype == np.uint8 and blob.ndim == 1 and len(offs) == 6 and len(fig) == 4
    ty, tx = fig[:2]
    words = [H, H, H * ty if antialias else H, W, W, W * tx if antialias else W]
    types = [np.int32, np.int32, np.float32] * 2
    padding = np.ones(blob.size, bool)
    out, end = [], 0
    for off, n, t in zip(offs, words, types):
        assert off % 16 == 0 and off >= end and off + 4 * n <= blob.size, (offs, words)
        end = off + 4 * n
        padding[off:end] = False
        out.append(blob[off:end].view(t))
    assert offs[0] == 0 and blob.size == (end + 15) // 16 * 16
    return out, tuple(fig), blob[padding]


@pytest.mark.parametrize("dims,antialias", CASES,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else
                         ("aa" if v else "plain"))
def test_device_image_sections_are_the_builders_tables(dims, antialias):
    got, fig, padding = sections(dims, antialias)
    if antialias:
        *want, ty, tx, band, rows = C.build_resize_aa_tables(*dims[:6], device=True)
        assert fig == (ty, tx, band, rows)
    else:
        want = C.build_resize_tables(*dims[:6])
        assert fig == (0, 0, 0, 0)
    assert len(want) == 6
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
    assert (padding == 0).all()


def test_every_section_of_the_small_shape_is_padded():
    """H = 5 and W = 7: tables of 20 and 28 bytes, so each section is followed by padding."""
    for antialias in (False, True):
        _, offs, _ = C.resize_device_image(21, 11, 7, 9, 5, 7, antialias)
        got, _, padding = sections((21, 11, 7, 9, 5, 7, 3), antialias)
        assert all((4 * g.size) % 16 for g in got) and padding.size >= 6 * 4
        assert list(offs) == sorted(offs) and len(set(offs)) == 6


def test_antialias_over_the_limit_is_refused_as_by_the_builder():
    for dims in [(33, 4, 4, 4, 4, 4), (4, 33, 4, 4, 4, 4), (4096, 4096, 511, 512, 2, 2)]:
        with pytest.raises(ValueError):
            C.resize_device_image(*dims, True)
        with pytest.raises(ValueError):
            C.build_resize_aa_tables(*dims, device=True)
        C.resize_device_image(*dims, False)  # the bilinear form has no such limit
    with pytest.raises(ValueError):
        C.resize_device_image(4, 4, 3, 4, 4, 4, False)  # no padding, either form
    C.resize_device_image(32, 32, 4, 4, 4, 4, True)  # exactly 8x


# ---- stand-alone sanitizer run ------------------------------------------------------------------

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None,
                    reason="needs ROCm clang++ and make")
def test_resize_plan_under_address_and_ub_sanitizers():
    target = "build/asan/resize_plan_check"
    b = subprocess.run(["make", "-C", ROOT, target], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, target)], capture_output=True, text=True, timeout=300,
                       env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "resize_plan_check OK" in out
