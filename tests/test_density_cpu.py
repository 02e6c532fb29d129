"""gol_density* without a GPU: the row routine of csrc/gol_density.h proven by a
stand-alone host program (tests/fake_hip/density_check.cpp, AddressSanitizer +
UBSan), the numpy reference (tests/density_ref.py) against the per-cell
definition, the ABI's declarations and argument rules, the runtime's
bookkeeping over the host-only HIP stand-in (tests/density_cpu_check.py) and
the schedule with a map behind every step, race-checked
(tests/sched_density_check.py)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from density_ref import density_dims, density_ref, tile_cells  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    exe = os.path.join(FH, "density_check")
    assert os.path.exists(exe), "build the host check first (__graft_entry__.build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]


def test_reference_against_the_per_cell_definition():
    rng = np.random.default_rng(7)
    for (rows, cols), (th, tw) in (((37, 131), (4, 32)), ((64, 64), (64, 64)), ((9, 70), (1, 32)), ((5, 33), (7, 96))):
        b = (rng.random((rows, cols)) < 0.4).astype(np.uint8)
        want = np.zeros(density_dims(rows, cols, th, tw), np.uint32)
        for r, c in zip(*np.nonzero(b)):
            want[r // th, c // tw] += 1
        assert (density_ref(b, th, tw) == want).all()
    assert (tile_cells(100, 200, 16, 32) == np.outer([16] * 6 + [4], [32] * 6 + [8])).all()


def test_header_declares_the_four_calls():
    h = open(os.path.join(ROOT, "include", "golhip.h")).read()
    assert re.search(r"int gol_density_dims\(int64_t nrows, int64_t ncols, int64_t tile_rows, int64_t tile_cols,\s+"
                     r"int64_t \*trows, int64_t \*tcols\);", h)
    assert re.search(r"int gol_density\(gol_ctx \*ctx, int64_t tile_rows, int64_t tile_cols, uint32_t \*counts, "
                     r"int64_t ld\);", h)
    assert re.search(r"int gol_density_window\(gol_ctx \*ctx, int64_t row0, int64_t col0, int64_t nrows, "
                     r"int64_t ncols,\s+int64_t tile_rows, int64_t tile_cols, uint32_t \*counts, int64_t ld\);", h)
    assert re.search(r"int gol_density_async\(gol_ctx \*ctx, int64_t tile_rows, int64_t tile_cols, uint32_t \*counts, "
                     r"int64_t ld\);", h)


def test_null_context_is_einval():
    from mpi_amd import golhip
    L = golhip.load()
    d = (ctypes.c_uint32 * 4)()
    assert L.gol_density(None, 4, 32, d, 2) == EINVAL
    assert L.gol_density_window(None, 0, 0, 1, 1, 4, 32, d, 2) == EINVAL
    assert L.gol_density_async(None, 4, 32, d, 2) == EINVAL


def test_density_dims_arithmetic():
    from mpi_amd import golhip
    assert golhip.density_dims(100, 200, 16, 32) == (7, 7)
    assert golhip.density_dims(131072, 131072, 128, 128) == (1024, 1024)
    assert golhip.density_dims(37, 131, 1000, 4096) == (1, 1)
    assert golhip.density_dims(0, 0, 1, 32) == (0, 0)
    assert golhip.density_dims(33, 65, 32, 64) == (2, 2)


def test_runtime_bookkeeping_and_argument_rules_cpu():
    assert "density cpu ok" in run_script("density_cpu_check.py")


def test_rank_maps_add_cpu():
    assert "density cpu ranks ok" in run_script("density_cpu_check.py", GOL_RCCL_SHIM=SHIM)


def test_density_schedules_have_no_race_cpu():
    assert "sched density ok" in run_script("sched_density_check.py")


def test_density_rank_schedules_have_no_race_cpu():
    assert "sched density rccl ok" in run_script("sched_density_check.py", GOL_RCCL_SHIM=SHIM)
