"""gol_copy_window / gol_copy without a GPU: the row routine of csrc/gol_copy.h proven
by a stand-alone host program (tests/fake_hip/copy_check.cpp, AddressSanitizer +
UBSan), the ABI's declarations and the null-context rule, the runtime's side over the
host-only HIP stand-in (tests/copy_cpu_check.py: the definition against numpy, slab
and column-run pairing, argument rules, the same context, pending async work, clones;
with the RCCL stand-in: rank contexts as source and destination) and the schedule
with copies between steps, race-checked in both contexts' traces
(tests/sched_copy_check.py).  The stand-in offers one device: the cross-device
refusal (GOL_EUNSUPPORTED) is not reached by any CPU test."""
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
    exe = os.path.join(FH, "copy_check")
    assert os.path.exists(exe), "build the host check first (__graft_entry__.build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]


def test_header_declares_the_calls():
    h = open(os.path.join(ROOT, "include", "golhip.h")).read()
    for name, value in (("REPLACE", 0), ("OR", 1), ("XOR", 2)):
        assert re.search(rf"#define GOL_COPY_{name}\s+{value}\b", h), name
    assert re.search(r"int gol_copy_window\(gol_ctx \*dst, int64_t drow0, int64_t dcol0,\s+"
                     r"gol_ctx \*src, int64_t srow0, int64_t scol0,\s+"
                     r"int64_t nrows, int64_t ncols, int op\);", h)
    assert re.search(r"int gol_copy\(gol_ctx \*dst, gol_ctx \*src\);", h)
    # the clock probe's paragraph names the calls among those that work beside it
    probe = h[h.index("Clock probe (measurement)"):h.index("int gol_clock_start")]
    assert "gol_copy[_window]" in probe


def test_null_context():
    from mpi_amd import golhip
    L = golhip.load()
    assert L.gol_copy_window(None, 0, 0, None, 0, 0, 1, 1, 0) == EINVAL
    assert L.gol_copy(None, None) == EINVAL
    assert golhip.COPY_OPS == {"replace": 0, "or": 1, "xor": 2}


def test_runtime_side_and_argument_rules_cpu():
    assert "copy cpu ok" in run_script("copy_cpu_check.py")


def test_rank_contexts_as_source_and_destination_cpu():
    assert "copy cpu ranks ok" in run_script("copy_cpu_check.py", GOL_RCCL_SHIM=SHIM)


def test_copy_schedules_have_no_race_cpu():
    assert "sched copy ok" in run_script("sched_copy_check.py")
