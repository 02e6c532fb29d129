"""RLE pattern text (gol_format_rle / gol_rle_bytes / gol_write_rle / gol_parse_rle /
gol_read_rle / gol_rle_header) without a GPU: the lane routines, the three passes and
the streaming parser of csrc/gol_rle.h proven by a stand-alone host program
(tests/fake_hip/rle_check.cpp, AddressSanitizer + UBSan), the reference encoder and
decoder (tests/rle_ref.py) on the Gosper gun, the ABI's declarations and null-context
rule, the runtime's side over the host-only HIP stand-in (tests/rle_cpu_check.py) and
the schedule with a format behind every step and a parse between steps, race-checked
(tests/sched_rle_check.py)."""
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
FH = os.path.join(ROOT, "tests", "fake_hip")
LIB = os.path.join(FH, "libgolhip_fakehip.so")
SHIM = os.path.join(FH, "libfake_rccl_host.so")
EINVAL = -1

GUN = (b"x = 36, y = 9, rule = B3/S23\n"
       b"24bo$22bobo$12b2o6b2o12b2o$11bo3bo4b2o12b2o$2o8bo5bo3b2o$2o8bo3bob2o4bobo$10bo5bo7bo$11bo3bo$12b2o!\n")


def run_script(name, **env):
    assert os.path.exists(LIB), "build the host-only runtime first (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", name)], env=dict(os.environ, GOL_LIB=LIB, **env),
                       capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_lane_routines_passes_and_parser_host_check():
    exe = os.path.join(FH, "rle_check")
    assert os.path.exists(exe), "build the host check first (__graft_entry__.build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]


def test_reference_on_the_gosper_gun():
    import rle_ref
    cells, (x, y, rule) = rle_ref.decode(GUN)
    assert (x, y, rule) == (36, 9, rle_ref.LIFE) and cells.shape == (9, 36) and int(cells.sum()) == 36
    # The file's tokens are the canonical tokens of its own cells.  Its body is one line of 98
    # characters; the format breaks lines after every 23rd token here (L = 70 / (1 + 2)), so the
    # canonical text is the file with two line breaks more, and nothing else differs.
    canon = rle_ref.encode(cells)
    head, body = canon.split(b"\n", 1)
    assert head + b"\n" + body.replace(b"\n", b"") + b"\n" == GUN
    assert body.count(b"\n") == 3 and max(len(line) for line in body.split(b"\n")) <= 70
    assert (rle_ref.decode(canon)[0] == cells).all()
    assert rle_ref.line_tokens(131072, 131072) == 10 and rle_ref.line_tokens(0, 0) == 35
    rng = np.random.default_rng(5)
    for _ in range(40):
        b = (rng.random((int(rng.integers(1, 30)), int(rng.integers(1, 300)))) < rng.random()).astype(np.uint8)
        text = rle_ref.encode(b, 0x48, 0xC)
        got, (x, y, rule) = rle_ref.decode(text)
        assert (got == b).all() and (x, y) == (b.shape[1], b.shape[0]) and rule == (0x48, 0xC)
        assert max(len(line) for line in text.split(b"\n")) <= 70


def test_header_declares_the_six_calls():
    h = open(os.path.join(ROOT, "include", "golhip.h")).read()
    win = r"gol_ctx \*ctx, int64_t row0, int64_t col0, int64_t nrows, int64_t ncols,\s*"
    assert re.search(r"int gol_rle_header\(const char \*text, int64_t len, int64_t \*x, int64_t \*y,\s+"
                     r"uint32_t \*birth, uint32_t \*survive, int \*has_rule, int64_t \*body\);", h)
    assert re.search(r"int gol_rle_bytes\(" + win + r"int64_t \*bytes\);", h)
    assert re.search(r"int gol_format_rle\(" + win + r"char \*out, int64_t cap, int64_t \*len\);", h)
    assert re.search(r"int gol_write_rle\(" + win + r"int fd\);", h)
    assert re.search(r"int gol_parse_rle\(gol_ctx \*ctx, int64_t row0, int64_t col0, const char \*text, int64_t len,\s+"
                     r"int64_t \*x, int64_t \*y\);", h)
    assert re.search(r"int gol_read_rle\(gol_ctx \*ctx, int64_t row0, int64_t col0, int fd, int64_t \*x, int64_t \*y\);", h)


def test_rle_header_and_null_contexts():
    import ctypes

    from mpi_amd import golhip
    L = golhip.load()
    assert golhip.rle_header(GUN) == (36, 9, (1 << 3, 0xC), 29)
    assert golhip.rle_header(b"#N Gosper glider gun\n#CXRLE Pos=5,7\nx=36,y=9\n24bo!") == (36, 9, None, 45)
    assert golhip.rle_header("x = 3, y = 3, rule = 23/3\nbo$2bo$3o!")[2] == (1 << 3, 0xC)
    for bad in (b"", b"#C only\n", b"y = 3, x = 3\n", b"x = 3\n", b"x = 3, y = 3, rule = B9/S\n", b"x = 3, y = 99999999999\n"):
        assert L.gol_rle_header(bad, len(bad), None, None, None, None, None, None) == EINVAL, bad
    n = ctypes.c_int64()
    buf = ctypes.create_string_buffer(64)
    assert L.gol_rle_bytes(None, 0, 0, 1, 1, ctypes.byref(n)) == EINVAL
    assert L.gol_format_rle(None, 0, 0, 1, 1, buf, 64, ctypes.byref(n)) == EINVAL
    assert L.gol_write_rle(None, 0, 0, 1, 1, 1) == EINVAL
    assert L.gol_parse_rle(None, 0, 0, GUN, len(GUN), None, None) == EINVAL
    assert L.gol_read_rle(None, 0, 0, 0, None, None) == EINVAL


def test_runtime_side_and_argument_rules_cpu():
    assert "rle cpu ok" in run_script("rle_cpu_check.py")


def test_rank_context_refuses_rows_it_does_not_hold_cpu():
    assert "rle cpu ranks ok" in run_script("rle_cpu_check.py", GOL_RCCL_SHIM=SHIM)


def test_rle_schedules_have_no_race_cpu():
    assert "sched rle ok" in run_script("sched_rle_check.py")
