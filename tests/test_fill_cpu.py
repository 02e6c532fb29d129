"""gol_fill_random* without a GPU: the row routine of csrc/gol_fill.h proven by a
stand-alone host program (tests/fake_hip/fill_check.cpp, AddressSanitizer + UBSan),
the ABI's declarations, gol_fill_threshold and the null-context rule, the numpy
reference's own checks (tests/fill_ref.py), the runtime's side over the host-only
HIP stand-in (tests/fill_cpu_check.py) and the schedule with a fill between steps,
race-checked (tests/sched_fill_check.py)."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from fill_ref import FULL, fill_cells, fill_ref, threshold_of  # noqa: E402

FH = os.path.join(ROOT, "tests", "fake_hip")
LIB = os.path.join(FH, "libgolhip_fakehip.so")
SHIM = os.path.join(FH, "libfake_rccl_host.so")
EINVAL = -1


def run_script(name, **env):
    assert os.path.exists(LIB), "build the host-only runtime first (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", name)], env=dict(os.environ, GOL_LIB=LIB, **env),
                       capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_row_routine_host_check():
    exe = os.path.join(FH, "fill_check")
    assert os.path.exists(exe), "build the host check first (__graft_entry__.build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]


def test_header_declares_the_three_calls():
    h = open(os.path.join(ROOT, "include", "golhip.h")).read()
    assert re.search(r"int gol_fill_threshold\(double density, uint64_t \*threshold\);", h)
    assert re.search(r"int gol_fill_random\(gol_ctx \*ctx, uint64_t seed, uint64_t threshold\);", h)
    assert re.search(r"int gol_fill_random_window\(gol_ctx \*ctx, int64_t row0, int64_t col0, int64_t nrows, "
                     r"int64_t ncols,\s+uint64_t seed, uint64_t threshold\);", h)


def test_threshold_and_null_context():
    from mpi_amd import golhip
    L = golhip.load()
    assert golhip.fill_threshold(0) == 0 and golhip.fill_threshold(1) == FULL
    assert golhip.fill_threshold(0.5) == 1 << 31 and golhip.fill_threshold(0.375) == 3 << 29
    for p in (1 / 3, 0.03, 1e-10, 1 - 1e-12):
        assert golhip.fill_threshold(p) == threshold_of(p)
    t = ctypes.c_uint64(99)
    for p in (math.nan, -0.1, 1.1):
        assert L.gol_fill_threshold(p, ctypes.byref(t)) == EINVAL and t.value == 99
        with pytest.raises(golhip.GolError):
            golhip.fill_threshold(p)
    assert L.gol_fill_threshold(0.5, None) == EINVAL
    assert L.gol_fill_random(None, 0, 1 << 31) == EINVAL
    assert L.gol_fill_random_window(None, 0, 0, 1, 1, 0, 1 << 31) == EINVAL


def test_reference_word_level_equals_per_cell():
    for seed, t in ((0, 1 << 31), (12345, 0x55555555), (2**64 - 1, 3 << 29), (7, 1), (7, FULL - 1)):
        assert (fill_ref(seed, t, 40, 100, 3, 37) == fill_cells(seed, t, 40, 100, 3, 37)).all(), (seed, t)
    assert not fill_ref(1, 0, 40, 100, 0, 37).any() and fill_ref(1, FULL, 40, 100, 0, 37).all()


def test_reference_window_is_a_slice_of_the_whole():
    whole = fill_ref(12345, 3 << 29, 96, 300)
    for r0, c0, nr, nc in ((0, 0, 96, 300), (5, 37, 40, 100), (95, 299, 1, 1), (17, 64, 3, 33), (0, 31, 96, 2)):
        assert (fill_ref(12345, 3 << 29, nr, nc, r0, c0) == whole[r0:r0 + nr, c0:c0 + nc]).all()


@pytest.mark.parametrize("seed", (0, 1, 12345))
def test_reference_density(seed):
    """The live count of 512 x 1024 is binomial(n, p = T / 2^32): within 5 sigma + 1 of n p."""
    n = 512 * 1024
    for t in (1 << 31, 3 << 29, 0x55555555, 1 << 20, FULL - 1):
        p = t / FULL
        live = int(fill_ref(seed, t, 512, 1024).sum())
        print(seed, hex(t), live, n * p, (live - n * p) / max(1e-9, math.sqrt(n * p * (1 - p))))
        assert abs(live - n * p) <= 5 * math.sqrt(n * p * (1 - p)) + 1, (seed, t, live)
    assert int(fill_ref(seed, 0, 64, 128).sum()) == 0 and int(fill_ref(seed, FULL, 64, 128).sum()) == 64 * 128


def test_runtime_side_and_argument_rules_cpu():
    assert "fill cpu ok" in run_script("fill_cpu_check.py")


def test_rank_parts_tile_the_board_cpu():
    assert "fill cpu ranks ok" in run_script("fill_cpu_check.py", GOL_RCCL_SHIM=SHIM)


def test_fill_schedules_have_no_race_cpu():
    assert "sched fill ok" in run_script("sched_fill_check.py")
