#!/usr/bin/env python3
"""Step schedules with gol_copy_window between steps, recorded with
GOL_OPT_SCHED_TRACE and race-checked by happens-before (sched_race.py).  The copy
reads the source's current buffer and writes the destination's on the DESTINATION
slab's compute stream; the read is recorded in the source's trace and the write in
the destination's (one trace when they are one context), each followed by the host's
stream sync.  Two contexts with different slab counts, boundaries and depths (copies
either way between steps of both), and one context onto itself, with the overlapped
halo exchange and the split interior on; every trace must be race-free, and the copy
must appear as a READ of exactly the source rows and a WRITE of exactly the
destination rows of every slab pair.

Over the host-only HIP stand-in (tests/test_copy_cpu.py):
    GOL_LIB=tests/fake_hip/libgolhip_fakehip.so python tests/sched_copy_check.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from mpi_amd import golhip as gh  # noqa: E402
from sched_race import EVENT_SYNC, READ, STREAM_SYNC, WRITE, find_races  # noqa: E402
from sched_torus_check import step_lists  # noqa: E402


def trace_len(e):
    n = ctypes.c_int64()
    e._chk(e.lib.gol_sched_trace(e._c, None, 0, ctypes.byref(n)), "gol_sched_trace")
    return n.value


def shape(slabs, split, k):
    rows = slabs * (2 * 32 * k + 2 * k + 5) + 1 if split == 2 else slabs * (2 * k + 9) + 1
    return rows, 200


def rows_of(e_rows, slabs, k, r0, nr):
    """(slab, storage row0, storage row1) of global rows [r0, r0 + nr) per slab that holds some."""
    out = []
    for s in range(slabs):
        row0, h = gh.slab_plan(e_rows, slabs, s)
        lo, hi = max(r0, row0), min(r0 + nr, row0 + h)
        if hi > lo:
            out.append((s, k + lo - row0, k + hi - row0))
    return out


def merge(spans):
    """Union of (slab, r0, r1) spans per slab (pieces of one slab are adjacent)."""
    out = {}
    for s, a, b in spans:
        lo, hi = out.get(s, (a, b))
        out[s] = (min(lo, a), max(hi, b))
    return sorted((s, a, b) for s, (a, b) in out.items())


def accesses(ops, a, b, kind, wraps=False):
    """Spans of `kind` among ops [a, b); a torus wrap (READ then WRITE of the same rows of one
    buffer) is the destination's own refresh and is left out of the reads."""
    got = []
    seg = ops[a:b]
    for i, o in enumerate(seg):
        if o[0] != kind:
            continue
        if kind == READ and not wraps and i + 1 < len(seg) and seg[i + 1][0] == WRITE and \
                (seg[i + 1][3:] == o[3:]).all():
            continue
        got.append((int(o[3]), int(o[5]), int(o[6])))
    return merge(got)


def two_contexts(a_kw, a_slabs, a_split, b_kw, b_slabs, b_split, steps_a, steps_b):
    ka, kb = a_kw["tblock_k"], b_kw["tblock_k"]
    ra, ca = shape(a_slabs, a_split, ka)
    rb, cb = shape(b_slabs, b_split, kb)
    nr = min(ra, rb) - 7
    win_a, at_b = (3, 37, nr, 101), (5, 12)      # a -> b, across the seams of both where there are any
    win_b, at_a = (1, 0, nr + 2, 150), (2, 49)   # b -> a
    what = dict(a=a_kw, a_slabs=a_slabs, a_split=a_split, b=b_kw, b_slabs=b_slabs, b_split=b_split)
    with gh.Engine(ra, ca, n_gpus=a_slabs, **a_kw) as A, gh.Engine(rb, cb, n_gpus=b_slabs, **b_kw) as B:
        for e, split in ((A, a_split), (B, b_split)):
            e.upload(np.zeros((e.rows, e.cols), np.uint8))
            e.set_option(gh.OPT_INTERIOR_SPLIT, split)
            e.set_option(gh.OPT_OVERLAP, 1)
            e.set_option(gh.OPT_SCHED_TRACE, 1)
        spans = []
        for i in range(max(len(steps_a), len(steps_b))):
            if i < len(steps_a):
                A.step(steps_a[i])
            if i < len(steps_b):
                B.step(steps_b[i])
            if i % 2 == 0:   # no sync of our own: the steps are in flight when the copy is called
                la, lb = trace_len(A), trace_len(B)
                if i % 4 == 0:
                    B.copy_from(A, win_a, at_b, ("replace", "or", "xor")[i % 3])
                    spans.append((A, ka, a_slabs, win_a[0], B, kb, b_slabs, at_b[0], nr, la, lb))
                else:
                    A.copy_from(B, win_b, at_a, "xor")
                    spans.append((B, kb, b_slabs, win_b[0], A, ka, a_slabs, at_a[0], nr + 2, lb, la))
                spans[-1] += (trace_len(spans[-1][0]), trace_len(spans[-1][4]))
        A.sync()
        B.sync()
        traces = {id(A): A.sched_trace(), id(B): B.sched_trace()}
    for name, e in (("a", A), ("b", B)):
        races = find_races(traces[id(e)])
        if races:
            print("RACE", name, what, races[0][2], flush=True)
            return 1, 0
    for src, sk, ss, sr0, dst, dk, dsl, dr0, n, s0, d0, s1, d1 in spans:
        reads = accesses(traces[id(src)], s0, s1, READ)
        writes = accesses(traces[id(dst)], d0, d1, WRITE)
        if reads != rows_of(src.rows, ss, sk, sr0, n) or writes != rows_of(dst.rows, dsl, dk, dr0, n):
            print("ACCESSES", what, f"read {reads} want {rows_of(src.rows, ss, sk, sr0, n)}; wrote {writes} "
                                    f"want {rows_of(dst.rows, dsl, dk, dr0, n)}", flush=True)
            return 1, 0
    # control: without the host syncs the copies' reads on the other context's streams must race
    # with the source's own later steps
    ops = traces[id(A)]
    control = len(find_races(ops[(ops[:, 0] != STREAM_SYNC) & (ops[:, 0] != EVENT_SYNC)]))
    return 0, control


def one_context(kw, slabs, split, steps):
    k = kw["tblock_k"]
    rows, cols = shape(slabs, split, k)
    nr = rows // 2 - 2
    win, at = (1, 5, nr, 45), (rows - nr - 1, 50)   # rows across the seams; columns that share storage words
    with gh.Engine(rows, cols, n_gpus=slabs, **kw) as e:
        e.upload(np.zeros((rows, cols), np.uint8))
        e.set_option(gh.OPT_INTERIOR_SPLIT, split)
        e.set_option(gh.OPT_OVERLAP, 1)
        e.set_option(gh.OPT_SCHED_TRACE, 1)
        spans = []
        for i, st in enumerate(steps):
            e.step(st)
            if i % 2 == 0:
                a = trace_len(e)
                e.copy_from(e, win, at, ("replace", "or", "xor")[i % 3])
                spans.append((a, trace_len(e)))
        e.sync()
        ops = e.sched_trace()
    what = dict(kw=kw, slabs=slabs, split=split, rows=rows, steps=steps)
    races = find_races(ops)
    if races:
        print("RACE", what, races[0][2], flush=True)
        return 1
    for a, b in spans:
        reads, writes = accesses(ops, a, b, READ), accesses(ops, a, b, WRITE)
        if reads != rows_of(rows, slabs, k, win[0], nr) or writes != rows_of(rows, slabs, k, at[0], nr):
            print("ACCESSES", what, f"read {reads}, wrote {writes}", flush=True)
            return 1
    return 0


def contexts():
    bad = n = control = 0
    pairs = ((dict(layout="bit", boundary="dead", tblock_k=8), 3, 2, dict(layout="byte", boundary="torus", tblock_k=1), 2, 1),
             (dict(layout="bit", boundary="torus", tblock_k=1), 1, 1, dict(layout="bit", boundary="dead", tblock_k=8), 1, 2),
             (dict(layout="byte", boundary="dead", tblock_k=16), 2, 1, dict(layout="bit", boundary="torus", tblock_k=8), 3, 2),
             (dict(layout="bit", boundary="dead", tblock_k=16), 1, 2, dict(layout="bit", boundary="dead", tblock_k=16), 3, 2))
    for a_kw, a_slabs, a_split, b_kw, b_slabs, b_split in pairs:
        for sa, sb in zip(step_lists(a_kw["tblock_k"]), step_lists(b_kw["tblock_k"])):
            b, c = two_contexts(a_kw, a_slabs, a_split, b_kw, b_slabs, b_split, sa, sb)
            bad += b
            control += c
            n += 1
    for boundary in ("dead", "torus"):
        for k in (1, 8, 16):
            for slabs in (1, 3):
                for split in (1, 2):
                    for steps in step_lists(k):
                        kw = dict(layout=("bit", "byte")[n % 2], boundary=boundary, tblock_k=k)
                        n += 1
                        bad += one_context(kw, slabs, split, steps)
    print(f"sched copy: {n} schedules, {bad} bad; control (host syncs stripped) {control} races", flush=True)
    if bad or control == 0:
        raise SystemExit(1)
    print("sched copy ok")


if __name__ == "__main__":
    contexts()
