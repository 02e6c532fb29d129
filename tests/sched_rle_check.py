#!/usr/bin/env python3
"""Step schedules with a gol_format_rle behind every step and a gol_parse_rle between
steps, recorded with GOL_OPT_SCHED_TRACE and race-checked by happens-before
(sched_race.py): the RLE calls work on the slab's comm stream (staging cleared, packed
rows, the three passes, the copies; on reading the merge, the ghost refresh) while the
step path owns the compute stream, so every block must be ordered behind the steps
before it and ahead of the steps after it.  1 and 3 slabs, dead and torus boundaries,
k = 1, 8, 16, both layouts, uneven step lists; every format must appear as a READ and
the parse as a WRITE of each slab's rows.

Over the host-only HIP stand-in (tests/test_rle_cpu.py):
    GOL_LIB=tests/fake_hip/libgolhip_fakehip.so python tests/sched_rle_check.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import rle_ref  # noqa: E402
from mpi_amd import golhip as gh  # noqa: E402
from sched_race import READ, WRITE, find_races  # noqa: E402
from sched_torus_check import step_lists  # noqa: E402


def trace_len(e):
    n = ctypes.c_int64()
    e._chk(e.lib.gol_sched_trace(e._c, None, 0, ctypes.byref(n)), "gol_sched_trace")
    return n.value


def run_steps(e, steps, rows, cols, text):
    e.set_option(gh.OPT_SCHED_TRACE, 1)
    spans, up = [], None
    for i, st in enumerate(steps):
        e.step(st)
        a = trace_len(e)
        e.format_rle()
        spans.append((a, trace_len(e)))
        if i == 1:
            a = trace_len(e)
            assert e.parse_rle(text) == (cols, rows)
            up = (a, trace_len(e))
    e.sync()
    return e.sched_trace(), spans, up


def check(ops, spans, up, slab_rows, k, what):
    races = find_races(ops)
    if races:
        print("RACE", what, races[0][2], flush=True)
        return 1
    want = sorted((s, k, k + h) for s, h in slab_rows)
    for a, b in spans:
        # (Engine.format_rle counts first: gol_rle_bytes, then gol_format_rle, read the same rows)
        reads = sorted(set((int(o[3]), int(o[5]), int(o[6])) for o in ops[a:b] if o[0] == READ))
        if reads != want:
            print("READS", what, f"format ops [{a}, {b}) read {reads}, want {want}", flush=True)
            return 1
    if up is not None:
        writes = sorted(set((int(o[3]), int(o[5]), int(o[6])) for o in ops[up[0]:up[1]] if o[0] == WRITE))
        if writes != want:
            print("WRITES", what, f"parse ops [{up[0]}, {up[1]}) wrote {writes}, want {want}", flush=True)
            return 1
    return 0


def contexts():
    bad = n = 0
    for boundary in ("dead", "torus"):
        for k in (1, 8, 16):
            for slabs in (1, 3):
                rows, cols = slabs * (2 * k + 3) + 1, 200
                soup = (np.random.default_rng(k).random((rows, cols)) < 0.3).astype(np.uint8)
                soup[:, -1] = 1   # every row carries its x columns
                text = rle_ref.encode(soup)
                for steps in step_lists(k):
                    layout = ("bit", "byte")[n % 2]
                    n += 1
                    with gh.Engine(rows, cols, n_gpus=slabs, layout=layout, boundary=boundary, tblock_k=k) as e:
                        e.upload(np.zeros((rows, cols), np.uint8))
                        ops, spans, up = run_steps(e, steps, rows, cols, text)
                    slab_rows = [(s, gh.slab_plan(rows, slabs, s)[1]) for s in range(slabs)]
                    bad += check(ops, spans, up, slab_rows, k, dict(layout=layout, boundary=boundary, k=k, slabs=slabs,
                                                                    rows=rows, steps=steps))
    print(f"sched rle: {n} contexts, {bad} bad", flush=True)
    if bad:
        raise SystemExit(1)
    print("sched rle ok")


if __name__ == "__main__":
    contexts()
