#!/usr/bin/env python3
"""Step schedules with a gol_fill_random between steps, recorded with
GOL_OPT_SCHED_TRACE and race-checked by happens-before (sched_race.py): the fill
writes the current buffer on every slab's compute stream (and, on a torus,
refreshes its ghost columns there) after the steps before it and before the steps
that follow.  1 and 3 slabs, dead and torus boundaries, interior split 1 and 2,
k = 1, 8, 16, uneven step lists, whole-board and window fills; the fill must appear
as a WRITE of exactly the rows it covers in each slab.

Over the host-only HIP stand-in (tests/test_fill_cpu.py):
    GOL_LIB=tests/fake_hip/libgolhip_fakehip.so python tests/sched_fill_check.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from mpi_amd import golhip as gh  # noqa: E402
from sched_race import WAIT, WRITE, find_races  # noqa: E402
from sched_torus_check import step_lists  # noqa: E402


def trace_len(e):
    n = ctypes.c_int64()
    e._chk(e.lib.gol_sched_trace(e._c, None, 0, ctypes.byref(n)), "gol_sched_trace")
    return n.value


def run_steps(e, steps, window):
    """Steps with a fill after the second and the fourth; returns (ops, [(first op, end op)] per fill)."""
    e.set_option(gh.OPT_SCHED_TRACE, 1)
    spans = []
    for i, st in enumerate(steps):
        e.step(st)
        if i in (1, 3):
            a = trace_len(e)
            e.fill_random(0.5, seed=i, window=window if i == 3 else None)
            spans.append((a, trace_len(e)))
    e.sync()
    return e.sched_trace(), spans


def shape(slabs, split, k):
    rows = slabs * (2 * 32 * k + 2 * k + 5) + 1 if split == 2 else slabs * (2 * k + 3) + 1
    return rows, 200


def one_context(layout, boundary, k, slabs, split, steps):
    rows, cols = shape(slabs, split, k)
    window = (rows // 3, 37, rows // 2, 101)   # rows [rows/3, rows/3 + rows/2): across a seam when there is one
    with gh.Engine(rows, cols, n_gpus=slabs, layout=layout, boundary=boundary, tblock_k=k) as e:
        e.upload(np.zeros((rows, cols), np.uint8))
        e.set_option(gh.OPT_INTERIOR_SPLIT, split)
        ops, spans = run_steps(e, steps, window)
    what = dict(layout=layout, boundary=boundary, k=k, slabs=slabs, split=split, rows=rows, steps=steps)
    races = find_races(ops)
    if races:
        print("RACE", what, races[0][2], flush=True)
        return 1
    for (a, b), (w0, wn) in zip(spans, ((0, rows), (window[0], window[2]))):
        want = []
        for s in range(slabs):
            row0, h = gh.slab_plan(rows, slabs, s)
            lo, hi = max(w0, row0), min(w0 + wn, row0 + h)
            if hi > lo:
                want.append((s, k + lo - row0, k + hi - row0))
        writes = sorted(set((int(o[3]), int(o[5]), int(o[6])) for o in ops[a:b] if o[0] == WRITE))
        if writes != sorted(want):
            print("WRITES", what, f"fill ops [{a}, {b}) wrote {writes}, want {want}", flush=True)
            return 1
    return 0


def contexts():
    bad = n = 0
    for boundary in ("dead", "torus"):
        for k in (1, 8, 16):
            for slabs in (1, 3):
                for split in (1, 2):
                    for steps in step_lists(k):
                        layout = ("bit", "byte")[n % 2]
                        n += 1
                        bad += one_context(layout, boundary, k, slabs, split, steps)
    # control: without its event waits the split schedule with fills must race
    rows, cols = shape(1, 2, 8)
    with gh.Engine(rows, cols, layout="bit", tblock_k=8) as e:
        e.set_option(gh.OPT_INTERIOR_SPLIT, 2)
        ops, _ = run_steps(e, (8, 3, 8, 8), None)
    control = len(find_races(ops[ops[:, 0] != WAIT]))
    print(f"sched fill: {n} contexts, {bad} bad; control (waits stripped) {control} races", flush=True)
    if bad or control == 0:
        raise SystemExit(1)
    print("sched fill ok")


if __name__ == "__main__":
    contexts()
