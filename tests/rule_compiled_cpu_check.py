#!/usr/bin/env python3
"""gol_rule_path / GOL_OPT_RULE_COMPILED on the CPU: the runtime's host code over
tests/fake_hip (as tests/rule_cpu_check.py runs it).  Which path a context picks
for B3/S23, a listed rule and an unlisted one under every combination of the two
options and after the rule changes between steps; the option's errors; and that
the step schedule of a context with a compiled rule set has no race
(sched_race.py) at 3 slabs, dead and torus.  Run by
tests/test_rule_compiled_cpu.py in a subprocess.

    GOL_LIB=tests/fake_hip/libgolhip_fakehip.so python tests/rule_compiled_cpu_check.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from mpi_amd import golhip as gh  # noqa: E402
from sched_race import WAIT, find_races  # noqa: E402

EINVAL, EUNSUPPORTED = -1, -5
LIFE = (1 << 3, (1 << 2) | (1 << 3))
UNLISTED = (1 << 1, 1 << 8)   # B1/S8


def refused(fn, code, names):
    try:
        fn()
    except gh.GolError as ex:
        assert ex.code == code, (ex, code)
        assert names in str(ex), (str(ex), names)
        return
    raise SystemExit(f"accepted, expected {code} naming {names!r}")


def want_path(rule, rule_kernel, rule_compiled, listed):
    if rule == LIFE and not rule_kernel:
        return "tuned"
    if rule in listed and rule_compiled and not rule_kernel:
        return "compiled"
    return "generic"


def paths():
    listed = [(b, s) for _, b, s in gh.compiled_rules()]
    assert len(listed) == 12 and LIFE not in listed and UNLISTED not in listed
    n = 0
    for k in range(1, 8):
        for boundary, slabs in (("dead", 1), ("torus", 3)):
            with gh.Engine(90, 70, layout="bit", boundary=boundary, n_gpus=slabs, tblock_k=k) as e:
                assert e.rule_path == "tuned" and e.get_option(gh.OPT_RULE_COMPILED) == 1
                # every rule of the list (k = 1 and 7) or two of them, under the four option pairs
                for rule in [LIFE, UNLISTED] + (listed if k in (1, 7) else [listed[0], listed[4]]):
                    e.set_rule(rule)
                    for rule_kernel in (0, 1):
                        for rule_compiled in (1, 0):
                            e.set_option(gh.OPT_RULE_KERNEL, rule_kernel)
                            e.set_option(gh.OPT_RULE_COMPILED, rule_compiled)
                            assert (e.get_option(gh.OPT_RULE_KERNEL), e.get_option(gh.OPT_RULE_COMPILED)) == \
                                (rule_kernel, rule_compiled)
                            assert e.rule_path == want_path(rule, rule_kernel, rule_compiled, listed), \
                                (k, rule, rule_kernel, rule_compiled, e.rule_path)
                            n += 1
                # the rule changed between steps, each option pair held across the changes
                for rule_kernel, rule_compiled in ((0, 1), (0, 0), (1, 1)):
                    e.set_option(gh.OPT_RULE_KERNEL, rule_kernel)
                    e.set_option(gh.OPT_RULE_COMPILED, rule_compiled)
                    for rule in (LIFE, listed[0], UNLISTED, listed[2], LIFE, listed[4]):
                        e.set_rule(rule)
                        assert e.rule_path == want_path(rule, rule_kernel, rule_compiled, listed)
                        e.step(k + 1)   # a full block and a short one; no sync
                        assert e.rule_path == want_path(rule, rule_kernel, rule_compiled, listed)
                        n += 1
                e.sync()
    print(f"rule path: {n} cases")
    # the option's errors; it is local state, accepted by contexts that take no rules
    with gh.Engine(64, 64, layout="bit", tblock_k=4, rule="B36/S23") as e:
        for v in (2, -1, 17):
            refused(lambda: e.set_option(gh.OPT_RULE_COMPILED, v), EINVAL, "0 or 1")
            assert e.get_option(gh.OPT_RULE_COMPILED) == 1 and e.rule_path == "compiled"
        refused(lambda: e.set_option(gh.OPT_RULE_KERNEL, 2), EINVAL, "0 or 1")
        p = ctypes.c_int(7)
        assert e.lib.gol_rule_path(None, ctypes.byref(p)) == EINVAL and p.value == 7
        assert e.lib.gol_rule_path(e._c, None) == EINVAL
    for kw, names in ((dict(layout="bit", tblock_k=8), "tblock_k = 1 .. 7"),
                      (dict(layout="bit", tblock_k=16), "tblock_k = 1 .. 7"),
                      (dict(layout="byte", tblock_k=4), "byte layout"),
                      (dict(layout="bit", boundary="serial_compat", tblock_k=4), "GOL_SERIAL_COMPAT")):
        with gh.Engine(128, 128, **kw) as e:
            refused(lambda: e.set_rule("B36/S23"), EUNSUPPORTED, "gol_set_rule: ")
            refused(lambda: e.set_rule("B36/S23"), EUNSUPPORTED, names)
            refused(lambda: e.set_rule("B1357/S1357"), EUNSUPPORTED, names)
            e.set_option(gh.OPT_RULE_COMPILED, 0)
            assert e.rule_path == "tuned" and e.rule == LIFE
            e.set_option(gh.OPT_RULE_COMPILED, 1)
            refused(lambda: e.set_option(gh.OPT_RULE_COMPILED, 2), EINVAL, "0 or 1")
            e.step(2 * kw["tblock_k"] + 1)
            e.sync()
            assert e.rule_path == "tuned"
    with gh.Engine(128, 128, layout="bit", tblock_k=8) as e:   # the unchanged message, in full
        refused(lambda: e.set_rule("B36/S23"), EUNSUPPORTED,
                "gol_set_rule: the rule-generic kernel fuses tblock_k = 1 .. 7 generations (2-word groups)")
    print("rule path ok")


def schedules():
    bad = n = 0
    for boundary in ("dead", "torus"):
        for k in (1, 4, 7):
            for split in (1, 2):
                for overlap in (1, 0):
                    slabs = 3
                    rows = slabs * (2 * 32 * k + 2 * k + 5) + 1 if split == 2 else slabs * (2 * k + 3) + 1
                    for steps in ([k, max(1, k - 3), k, k, 1, k], [1, k, k]):
                        with gh.Engine(rows, 200, n_gpus=slabs, layout="bit", boundary=boundary, tblock_k=k,
                                       rule="B1357/S1357") as e:
                            assert e.rule_path == "compiled"
                            e.upload(np.zeros((rows, 200), np.uint8))
                            e.set_option(gh.OPT_OVERLAP, overlap)
                            e.set_option(gh.OPT_INTERIOR_SPLIT, split)
                            e.set_option(gh.OPT_SCHED_TRACE, 1)
                            for i, st in enumerate(steps):
                                e.step(st)
                                if i == 1:   # the path changed in flight (synchronises), then back
                                    e.set_option(gh.OPT_RULE_COMPILED, 0)
                                if i == 2:
                                    e.set_option(gh.OPT_RULE_COMPILED, 1)
                                    e.set_rule("B3678/S34678")
                            assert e.rule_path == "compiled"
                            e.sync()
                            ops = e.sched_trace()
                        n += 1
                        races = find_races(ops)
                        if races or len(ops) == 0:
                            bad += 1
                            print("RACE", boundary, k, split, overlap, steps, races[:1], flush=True)
    # control: the same kind of schedule without its event waits must race
    with gh.Engine(3 * 40, 200, n_gpus=3, layout="bit", tblock_k=4, rule="B36/S23") as e:
        assert e.rule_path == "compiled"
        e.set_option(gh.OPT_SCHED_TRACE, 1)
        for st in (4, 3, 4, 4):
            e.step(st)
        e.sync()
        ops = e.sched_trace()
    control = len(find_races(ops[ops[:, 0] != WAIT]))
    print(f"sched compiled rule: {n} contexts, {bad} bad; control (waits stripped) {control} races", flush=True)
    if bad or control == 0:
        raise SystemExit(1)
    print("sched compiled rule ok")


if __name__ == "__main__":
    paths()
    schedules()
