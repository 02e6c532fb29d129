#!/usr/bin/env python3
"""gol_set_rule / gol_get_rule / GOL_OPT_RULE_KERNEL on the CPU: the runtime's
host code over tests/fake_hip (as tests/sched_cpu_check.py runs it).  Which
contexts take which rules, that a refused call leaves the context usable, and
that the step schedule of a context with a rule set has no race (sched_race.py)
at 3 slabs, dead and torus.  Run by tests/test_rule_cpu.py in a subprocess.

    GOL_LIB=tests/fake_hip/libgolhip_fakehip.so python tests/rule_cpu_check.py
"""
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
HIGHLIFE = ((1 << 3) | (1 << 6), (1 << 2) | (1 << 3))


def refused(fn, code, names):
    try:
        fn()
    except gh.GolError as ex:
        assert ex.code == code, (ex, code)
        assert names in str(ex), (str(ex), names)
        return
    raise SystemExit(f"accepted, expected {code} naming {names!r}")


def abi():
    # a fresh context runs B3/S23 on the tuned kernels
    with gh.Engine(64, 64, layout="bit", tblock_k=4) as e:
        assert e.rule == LIFE and e.get_option(gh.OPT_RULE_KERNEL) == 0
        e.set_rule("B36/S23")
        assert e.rule == HIGHLIFE
        e.set_rule((0b111111110, 0b111111111))   # every bit a rule may set
        assert e.rule == (0b111111110, 0b111111111)
        e.set_rule((0, 0))                       # nothing is born, nothing survives: a rule
        # GOL_EINVAL: bits above 8, B0; the rule in force is kept
        for birth, survive, names in ((1 << 9, 0, "above 8"), (0, 1 << 9, "above 8"), (1 << 31, 0, "above 8"),
                                      (1, 0, "B0"), (0b1001, 0b1100, "B0")):
            refused(lambda: e.set_rule((birth, survive)), EINVAL, names)
            assert e.rule == (0, 0)
        refused(lambda: e.set_option(gh.OPT_RULE_KERNEL, 2), EINVAL, "0 or 1")
        e.set_option(gh.OPT_RULE_KERNEL, 1)
        assert e.get_option(gh.OPT_RULE_KERNEL) == 1
        e.set_rule(LIFE)
        e.step(9)
        e.sync()
    with gh.Engine(64, 64, layout="bit", tblock_k=2, rule="s23/b36") as e:
        assert e.rule == HIGHLIFE
    # supported: bit layout, k = 1..7, dead and torus, any slab count
    for k in range(1, 8):
        for boundary in ("dead", "torus"):
            for slabs in (1, 3):
                with gh.Engine(90, 70, layout="bit", boundary=boundary, n_gpus=slabs, tblock_k=k) as e:
                    e.set_rule(HIGHLIFE)
                    e.set_option(gh.OPT_RULE_KERNEL, 1)
                    e.step(2 * k + 1)
                    e.sync()
    # GOL_EUNSUPPORTED, naming the limit; B3/S23 itself is accepted; the context stays usable
    limits = [
        (dict(layout="byte", tblock_k=4), "byte layout"),
        (dict(layout="byte", boundary="torus", tblock_k=8), "byte layout"),
        (dict(layout="bit", tblock_k=8), "tblock_k = 1 .. 7"),
        (dict(layout="bit", tblock_k=16), "tblock_k = 1 .. 7"),
        (dict(layout="bit", tblock_k=32, boundary="torus"), "tblock_k = 1 .. 7"),
        (dict(layout="bit", boundary="serial_compat", tblock_k=4), "GOL_SERIAL_COMPAT"),
        (dict(layout="bit", boundary="mesh_compat", mesh_m=2, tblock_k=4), "GOL_MESH_COMPAT"),
    ]
    for kw, names in limits:
        with gh.Engine(128, 128, **kw) as e:
            refused(lambda: e.set_rule(HIGHLIFE), EUNSUPPORTED, names)
            refused(lambda: e.set_rule("B2/S"), EUNSUPPORTED, names)
            refused(lambda: e.set_option(gh.OPT_RULE_KERNEL, 1), EUNSUPPORTED, names)
            assert e.rule == LIFE and e.get_option(gh.OPT_RULE_KERNEL) == 0
            e.set_rule(LIFE)
            e.set_rule("B3/S23")
            e.set_option(gh.OPT_RULE_KERNEL, 0)
            refused(lambda: e.set_rule((1, 0)), EINVAL, "B0")   # EINVAL comes before the context's limits
            e.step(2 * kw["tblock_k"] + 1)
            e.sync()
        try:
            gh.Engine(128, 128, rule="B36/S23", **kw)
        except gh.GolError as ex:
            assert ex.code == EUNSUPPORTED
        else:
            raise SystemExit(f"Engine(rule=...) accepted on {kw}")
    print("rule abi ok")


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
                            e.upload(np.zeros((rows, 200), np.uint8))
                            e.set_option(gh.OPT_OVERLAP, overlap)
                            e.set_option(gh.OPT_INTERIOR_SPLIT, split)
                            e.set_option(gh.OPT_SCHED_TRACE, 1)
                            for i, st in enumerate(steps):
                                e.step(st)
                                if i == 1:   # the rule changed in flight (synchronises), then back
                                    e.set_rule("B3/S23")
                                if i == 2:
                                    e.set_rule("B2/S")
                            e.sync()
                            ops = e.sched_trace()
                        n += 1
                        races = find_races(ops)
                        if races or len(ops) == 0:
                            bad += 1
                            print("RACE", boundary, k, split, overlap, steps, races[:1], flush=True)
    # control: the same kind of schedule without its event waits must race
    with gh.Engine(3 * 40, 200, n_gpus=3, layout="bit", tblock_k=4, rule="B36/S23") as e:
        e.set_option(gh.OPT_SCHED_TRACE, 1)
        for st in (4, 3, 4, 4):
            e.step(st)
        e.sync()
        ops = e.sched_trace()
    control = len(find_races(ops[ops[:, 0] != WAIT]))
    print(f"sched rule: {n} contexts, {bad} bad; control (waits stripped) {control} races", flush=True)
    if bad or control == 0:
        raise SystemExit(1)
    print("sched rule ok")


if __name__ == "__main__":
    abi()
    schedules()
