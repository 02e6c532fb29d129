"""Life-like rules without a GPU: the rule stage of the rule-generic kernel,
proven exhaustively by a host program built with ASan + UBSan
(tests/fake_hip/rule_stage_check.cpp); gol_parse_rule (host-only, answered by
libgolhip.so on a machine with no GPU); gol_set_rule / gol_get_rule and the
step schedule of a context with a rule set, over the host-only HIP stand-in
(tests/rule_cpu_check.py)."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_hip")
LIB = os.path.join(FAKE, "libgolhip_fakehip.so")
EINVAL = -1


def test_rule_stage_exhaustive():
    """All 2^17 rules x all 2^7 stage inputs, mask all-ones and mask 0."""
    r = subprocess.run([os.path.join(FAKE, "rule_stage_check")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "12582912 cases checked, 0 bad" in r.stdout   # 2^17 rules x 96 reachable inputs


def bits(digits):
    return sum(1 << int(d) for d in digits)


ACCEPTED = [
    ("B3/S23", "3", "23"), ("b3/s23", "3", "23"), ("B36/S23", "36", "23"), ("b36/S23", "36", "23"),
    ("S23/B36", "36", "23"), ("s23/b3", "3", "23"), ("23/3", "3", "23"), ("23/36", "36", "23"),
    ("B2/S", "2", ""), ("S/B2", "2", ""), ("B/S", "", ""), ("B/S8", "", "8"), ("/2", "2", ""), ("1357/", "", "1357"),
    ("B1357/S1357", "1357", "1357"), ("B3678/S34678", "3678", "34678"), ("B012345678/S012345678", "012345678",
                                                                          "012345678"),
    ("B3/S012345678", "3", "012345678"), ("B0/S", "0", ""),   # the parser does not judge the rule
    ("B63/S32", "36", "23"),
]
REJECTED = ["", "/", "B3", "B3S23", "B3/S23/", "B3/S23 ", " B3/S23", "B3/B23", "S3/S23", "B9/S", "B3/S29", "23/9",
            "B33/S23", "B3/S223", "B3/23", "3/S23", "X3/S23", "B3\\S23", "B3/S2 3", "B-3/S23", "B3/S23x", "life",
            "B3/S23/B3", "23", "B3 /S23", "B3/ S23", "B/"]


@pytest.fixture(scope="module")
def lib():
    from mpi_amd import golhip
    return golhip.load()


@pytest.mark.parametrize("text,birth,survive", ACCEPTED)
def test_parse_rule_accepts(lib, text, birth, survive):
    from mpi_amd import golhip
    b, s = ctypes.c_uint32(0xdead), ctypes.c_uint32(0xbeef)
    assert lib.gol_parse_rule(text.encode(), ctypes.byref(b), ctypes.byref(s)) == 0
    assert (b.value, s.value) == (bits(birth), bits(survive))
    assert golhip.parse_rule(text) == (bits(birth), bits(survive))


@pytest.mark.parametrize("text", REJECTED)
def test_parse_rule_rejects(lib, text):
    from mpi_amd import golhip
    b, s = ctypes.c_uint32(0xdead), ctypes.c_uint32(0xbeef)
    assert lib.gol_parse_rule(text.encode(), ctypes.byref(b), ctypes.byref(s)) == EINVAL
    assert (b.value, s.value) == (0xdead, 0xbeef)   # outputs untouched
    with pytest.raises(golhip.GolError):
        golhip.parse_rule(text)


def test_parse_rule_null_arguments(lib):
    b = ctypes.c_uint32()
    assert lib.gol_parse_rule(None, ctypes.byref(b), ctypes.byref(b)) == EINVAL
    assert lib.gol_parse_rule(b"B3/S23", None, ctypes.byref(b)) == EINVAL
    assert lib.gol_parse_rule(b"B3/S23", ctypes.byref(b), None) == EINVAL


def test_header_and_binding_name_the_rule_calls():
    from mpi_amd import golhip
    h = open(os.path.join(ROOT, "include", "golhip.h")).read()
    assert "#define GOL_OPT_RULE_KERNEL 16" in h and golhip.OPT_RULE_KERNEL == 16
    for name in ("gol_parse_rule", "gol_set_rule", "gol_get_rule"):
        assert f"int {name}(" in h and name in golhip.EXPORTS
    assert "permanently dead" in h


def test_set_rule_limits_and_schedules_cpu():
    """Every GOL_EINVAL / GOL_EUNSUPPORTED case, B3/S23 accepted everywhere, and the race
    check of a 3-slab context with a rule set, dead and torus."""
    assert os.path.exists(LIB), "build the host-only runtime first (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rule_cpu_check.py")],
                       env=dict(os.environ, GOL_LIB=LIB), capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "rule abi ok" in r.stdout and "sched rule ok" in r.stdout
