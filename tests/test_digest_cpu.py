"""gol_digest* without a GPU: the row routine of csrc/gol_digest.h proven by a
stand-alone host program (tests/fake_hip/digest_check.cpp, AddressSanitizer +
UBSan), the ABI's declarations and argument checks, the runtime's bookkeeping
over the host-only HIP stand-in (tests/digest_cpu_check.py) and the schedule
with a digest behind every step, race-checked (tests/sched_digest_check.py)."""
import ctypes
import os
import re
import subprocess
import sys

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
    exe = os.path.join(FH, "digest_check")
    assert os.path.exists(exe), "build the host check first (__graft_entry__.build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]


def test_header_declares_the_three_calls():
    h = open(os.path.join(ROOT, "include", "golhip.h")).read()
    assert re.search(r"int gol_digest\(gol_ctx \*ctx, uint64_t digest\[2\]\);", h)
    assert re.search(r"int gol_digest_window\(gol_ctx \*ctx, int64_t row0, int64_t col0, int64_t nrows, "
                     r"int64_t ncols,\s+uint64_t digest\[2\]\);", h)
    assert re.search(r"int gol_digest_async\(gol_ctx \*ctx, uint64_t digest\[2\]\);", h)


def test_null_context_is_einval():
    from mpi_amd import golhip
    L = golhip.load()
    d = (ctypes.c_uint64 * 2)()
    assert L.gol_digest(None, d) == EINVAL
    assert L.gol_digest_window(None, 0, 0, 1, 1, d) == EINVAL
    assert L.gol_digest_async(None, d) == EINVAL


def test_runtime_bookkeeping_cpu():
    assert "digest cpu ok" in run_script("digest_cpu_check.py")


def test_digest_schedules_have_no_race_cpu():
    assert "sched digest ok" in run_script("sched_digest_check.py")


def test_digest_rank_schedules_have_no_race_cpu():
    assert "sched digest rccl ok" in run_script("sched_digest_check.py", GOL_RCCL_SHIM=SHIM)
