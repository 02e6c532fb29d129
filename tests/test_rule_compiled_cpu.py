"""Compiled life-like rules without a GPU: the compiled-rule stage and its
synthesiser, proven exhaustively by a host program built with ASan + UBSan
(tests/fake_hip/rule_const_check.cpp); gol_compiled_rule (host-only, answered by
libgolhip.so on a machine with no GPU); gol_rule_path / GOL_OPT_RULE_COMPILED
and the step schedule of a context with a compiled rule set, over the host-only
HIP stand-in (tests/rule_compiled_cpu_check.py)."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_hip")
LIB = os.path.join(FAKE, "libgolhip_fakehip.so")
EINVAL = -1


def bits(digits):
    return sum(1 << int(d) for d in digits)


# the issue's list, in its order
LISTED = [("HighLife", "36", "23"), ("Day & Night", "3678", "34678"), ("Seeds", "2", ""),
          ("Life without Death", "3", "012345678"), ("Replicator", "1357", "1357"), ("2x2", "36", "125"),
          ("Maze", "3", "12345"), ("DryLife", "37", "23"), ("Pedestrian Life", "38", "23"),
          ("Diamoeba", "35678", "5678"), ("Morley", "368", "245"), ("Anneal", "4678", "35678")]


def test_rule_const_stage_exhaustive():
    """All 2^17 rules' synthesised immediates, and every listed rule's template instantiation,
    x all 2^7 stage inputs, mask all-ones and mask 0, against the definition and rule_bits."""
    r = subprocess.run([os.path.join(FAKE, "rule_const_check")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "12582912 synthesised cases checked" in r.stdout   # 2^17 rules x 96 reachable inputs
    assert "1152 template cases checked (12 rules), 0 bad" in r.stdout   # 12 rules x 96


@pytest.fixture(scope="module")
def lib():
    from mpi_amd import golhip
    return golhip.load()


def test_compiled_rule_enumerates_the_list(lib):
    from mpi_amd import golhip
    got = []
    for i in range(len(LISTED)):
        b, s, name = ctypes.c_uint32(0xdead), ctypes.c_uint32(0xbeef), ctypes.c_char_p()
        assert lib.gol_compiled_rule(i, ctypes.byref(b), ctypes.byref(s), ctypes.byref(name)) == 0
        got.append((name.value.decode(), b.value, s.value))
    assert got == [(n, bits(b), bits(s)) for n, b, s in LISTED]
    assert golhip.compiled_rules() == got
    for name, birth, survive in got:
        assert not ((birth | survive) & ~0x1ff) and not (birth & 1)        # rule_valid
        assert (birth, survive) != (1 << 3, (1 << 2) | (1 << 3)), name      # B3/S23 keeps its tuned kernels
        assert golhip.parse_rule("B%s/S%s" % LISTED[got.index((name, birth, survive))][1:]) == (birth, survive)
    assert len({(b, s) for _, b, s in got}) == len(got)


def test_compiled_rule_index_limits_and_null_outputs(lib):
    b, s, name = ctypes.c_uint32(0xdead), ctypes.c_uint32(0xbeef), ctypes.c_char_p(b"untouched")
    for index in (-1, len(LISTED), 1 << 20):
        assert lib.gol_compiled_rule(index, ctypes.byref(b), ctypes.byref(s), ctypes.byref(name)) == EINVAL
        assert (b.value, s.value, name.value) == (0xdead, 0xbeef, b"untouched")   # outputs untouched
    assert lib.gol_compiled_rule(0, None, None, None) == 0
    assert lib.gol_compiled_rule(1, ctypes.byref(b), None, None) == 0 and b.value == bits("3678")
    assert lib.gol_compiled_rule(2, None, ctypes.byref(s), None) == 0 and s.value == 0
    assert lib.gol_compiled_rule(4, None, None, ctypes.byref(name)) == 0 and name.value == b"Replicator"


def test_header_and_binding_name_the_compiled_rule_calls():
    from mpi_amd import golhip
    h = open(os.path.join(ROOT, "include", "golhip.h")).read()
    assert "#define GOL_OPT_RULE_COMPILED 17" in h and golhip.OPT_RULE_COMPILED == 17
    for name in ("gol_compiled_rule", "gol_rule_path"):
        assert f"int {name}(" in h and name in golhip.EXPORTS
    for i, name in enumerate(("TUNED", "GENERIC", "COMPILED")):
        assert f"#define GOL_RULE_PATH_{name} {i}" in h and golhip.RULE_PATHS[i] == name.lower()
    assert "any other rule runs the\n * rule-generic kernel.\n" not in h   # the corrected paragraph
    assert isinstance(golhip.Engine.rule_path, property)


def test_rule_path_dispatch_and_schedules_cpu():
    """gol_rule_path for B3/S23, listed and unlisted rules under both options and across rule
    changes; the option's errors; the race check of a 3-slab context on a compiled rule."""
    assert os.path.exists(LIB), "build the host-only runtime first (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rule_compiled_cpu_check.py")],
                       env=dict(os.environ, GOL_LIB=LIB), capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "rule path ok" in r.stdout and "sched compiled rule ok" in r.stdout
