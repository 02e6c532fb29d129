"""gol_download_bits* / gol_upload_bits* without a GPU: the row routines of
csrc/gol_bits.h proven by a stand-alone host program (tests/fake_hip/bits_check.cpp,
AddressSanitizer + UBSan), the ABI's declarations and null-context rule, the
runtime's side over the host-only HIP stand-in (tests/bits_cpu_check.py) and the
schedule with a packed download behind every step and a packed upload between
steps, race-checked (tests/sched_bits_check.py)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

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


def test_row_routines_host_check():
    exe = os.path.join(FH, "bits_check")
    assert os.path.exists(exe), "build the host check first (__graft_entry__.build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]


def test_header_declares_the_six_calls():
    h = open(os.path.join(ROOT, "include", "golhip.h")).read()
    win = r"gol_ctx \*ctx, int64_t row0, int64_t col0, int64_t nrows, int64_t ncols,\s+"
    assert re.search(r"int64_t gol_bits_row_bytes\(int64_t ncols\);", h)
    assert re.search(r"int gol_download_bits\(gol_ctx \*ctx, uint8_t \*host, int64_t ld\);", h)
    assert re.search(r"int gol_download_bits_window\(" + win + r"uint8_t \*host, int64_t ld\);", h)
    assert re.search(r"int gol_download_bits_window_async\(" + win + r"uint8_t \*host, int64_t ld\);", h)
    assert re.search(r"int gol_upload_bits\(gol_ctx \*ctx, const uint8_t \*host, int64_t ld\);", h)
    assert re.search(r"int gol_upload_bits_window\(" + win + r"const uint8_t \*host, int64_t ld\);", h)


def test_row_bytes_and_null_context():
    from mpi_amd import golhip
    L = golhip.load()
    assert [golhip.bits_row_bytes(n) for n in (0, 1, 8, 9, 131, 131072)] == [0, 1, 1, 2, 17, 16384]
    assert L.gol_bits_row_bytes(-1) == EINVAL
    buf = np.zeros(8, np.uint8)
    p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert L.gol_download_bits(None, p, 8) == EINVAL and L.gol_upload_bits(None, p, 8) == EINVAL
    assert L.gol_download_bits_window(None, 0, 0, 1, 1, p, 8) == EINVAL
    assert L.gol_download_bits_window_async(None, 0, 0, 1, 1, p, 8) == EINVAL
    assert L.gol_upload_bits_window(None, 0, 0, 1, 1, p, 8) == EINVAL


def test_runtime_side_and_argument_rules_cpu():
    assert "bits cpu ok" in run_script("bits_cpu_check.py")


def test_rank_parts_tile_the_board_cpu():
    assert "bits cpu ranks ok" in run_script("bits_cpu_check.py", GOL_RCCL_SHIM=SHIM)


def test_bits_schedules_have_no_race_cpu():
    assert "sched bits ok" in run_script("sched_bits_check.py")


def test_bits_rank_schedules_have_no_race_cpu():
    assert "sched bits rccl ok" in run_script("sched_bits_check.py", GOL_RCCL_SHIM=SHIM)
