#!/usr/bin/env python3
"""Step schedules with a gol_download_bits_window_async behind every step and a
gol_upload_bits in the middle, recorded with GOL_OPT_SCHED_TRACE and
race-checked by happens-before (sched_race.py): the packed download reads the
current buffer on the compute stream while later steps' other streams (comm,
interior parts) go on; the step after next overwrites that buffer, so the read
must be ordered before it; the upload writes the current buffer (and, on a
torus, refreshes its ghost columns) before the steps that follow.  1 and 3
slabs, interior split 1 and 2, overlap on and off, k = 1, 8, 16, dead and torus
boundaries, uneven step lists; every download must appear as a READ and the
upload as a WRITE of each slab's rows.

Over the host-only HIP stand-in (tests/test_bits_cpu.py):
    GOL_LIB=tests/fake_hip/libgolhip_fakehip.so python tests/sched_bits_check.py
    GOL_LIB=... GOL_RCCL_SHIM=tests/fake_hip/libfake_rccl_host.so python tests/sched_bits_check.py
"""
import ctypes
import os
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
if os.environ.get("GOL_RCCL_SHIM"):
    ctypes.CDLL(os.environ["GOL_LIB"], mode=ctypes.RTLD_GLOBAL)
    ctypes.CDLL(os.environ["GOL_RCCL_SHIM"], mode=ctypes.RTLD_GLOBAL)
from mpi_amd import golhip as gh  # noqa: E402
from sched_race import READ, WAIT, WRITE, find_races  # noqa: E402
from sched_torus_check import step_lists  # noqa: E402


def trace_len(e):
    n = ctypes.c_int64()
    e._chk(e.lib.gol_sched_trace(e._c, None, 0, ctypes.byref(n)), "gol_sched_trace")
    return n.value


def run_steps(e, steps, rows, cols):
    """Steps with a packed async download behind each, a packed upload after the second step;
    returns (ops, [(first op, end op)] per download, (first op, end op) of the upload)."""
    e.set_option(gh.OPT_SCHED_TRACE, 1)
    spans, outs, up = [], [], None
    for i, st in enumerate(steps):
        e.step(st)
        a = trace_len(e)
        outs.append(e.download_bits_window_async(0, 0, rows, cols))
        spans.append((a, trace_len(e)))
        if i == 1:
            a = trace_len(e)
            e.upload_bits(np.zeros((rows, gh.bits_row_bytes(cols)), np.uint8))
            up = (a, trace_len(e))
    e.sync()
    return e.sched_trace(), spans, up


def check(ops, spans, up, slab_rows, k, what):
    """No race; every download is a READ of rows [k, k + H) of every local slab; the upload WRITEs them."""
    races = find_races(ops)
    if races:
        print("RACE", what, races[0][2], flush=True)
        return 1
    want = sorted((s, k, k + h) for s, h in slab_rows)
    for a, b in spans:
        reads = sorted((int(o[3]), int(o[5]), int(o[6])) for o in ops[a:b] if o[0] == READ)
        if reads != want:
            print("READS", what, f"download ops [{a}, {b}) read {reads}, want {want}", flush=True)
            return 1
    if up is not None:
        writes = sorted(set((int(o[3]), int(o[5]), int(o[6])) for o in ops[up[0]:up[1]] if o[0] == WRITE))
        if writes != want:
            print("WRITES", what, f"upload ops [{up[0]}, {up[1]}) wrote {writes}, want {want}", flush=True)
            return 1
    return 0


def shape(slabs, split, k):
    # with the split, room for two parts per slab (32·K rows each); else thin and uneven slabs
    rows = slabs * (2 * 32 * k + 2 * k + 5) + 1 if split == 2 else slabs * (2 * k + 3) + 1
    return rows, 200


def one_context(layout, boundary, k, slabs, split, overlap, steps):
    rows, cols = shape(slabs, split, k)
    with gh.Engine(rows, cols, n_gpus=slabs, layout=layout, boundary=boundary, tblock_k=k) as e:
        e.upload(np.zeros((rows, cols), np.uint8))
        e.set_option(gh.OPT_OVERLAP, overlap)
        e.set_option(gh.OPT_INTERIOR_SPLIT, split)
        ops, spans, up = run_steps(e, steps, rows, cols)
    slab_rows = [(s, gh.slab_plan(rows, slabs, s)[1]) for s in range(slabs)]
    return check(ops, spans, up, slab_rows, k, dict(layout=layout, boundary=boundary, k=k, slabs=slabs, split=split,
                                                    overlap=overlap, rows=rows, steps=steps))


def contexts():
    bad = n = 0
    for boundary in ("dead", "torus"):
        for k in (1, 8, 16):
            for slabs in (1, 3):
                for split in (1, 2):
                    for overlap in (1, 0):
                        for steps in step_lists(k):
                            layout = ("bit", "byte")[n % 2]
                            n += 1
                            bad += one_context(layout, boundary, k, slabs, split, overlap, steps)
    # control: without its event waits the split schedule with downloads must race
    rows, cols = shape(1, 2, 8)
    with gh.Engine(rows, cols, layout="bit", tblock_k=8) as e:
        e.set_option(gh.OPT_INTERIOR_SPLIT, 2)
        ops, _, _ = run_steps(e, (8, 3, 8, 8), rows, cols)
    control = len(find_races(ops[ops[:, 0] != WAIT]))
    print(f"sched bits: {n} contexts, {bad} bad; control (waits stripped) {control} races", flush=True)
    if bad or control == 0:
        raise SystemExit(1)
    print("sched bits ok")


def ranks():
    bad = n = 0
    for world in (2, 3):
        for boundary in ("dead", "torus"):
            for layout, k, split in (("bit", 1, 1), ("bit", 8, 2), ("byte", 16, 1)):
                rows, cols = shape(world, split, k)
                for steps in step_lists(k)[:2]:
                    uid = gh.unique_id()
                    out, errs = [None] * world, []

                    def worker(r):
                        try:
                            with gh.Engine(rows, cols, rank=r, world=world, device=0, uid=uid, layout=layout,
                                           boundary=boundary, tblock_k=k) as e:
                                e.upload(np.zeros((rows, cols), np.uint8))
                                e.set_option(gh.OPT_INTERIOR_SPLIT, split)
                                row0, h = gh.slab_plan(rows, world, r)
                                e.set_option(gh.OPT_SCHED_TRACE, 1)
                                spans, keep = [], []
                                for st in steps:   # (no upload here: it synchronises one rank only)
                                    e.step(st)
                                    a = trace_len(e)
                                    keep.append(e.download_bits_window_async(row0, 0, h, cols))
                                    spans.append((a, trace_len(e)))
                                e.sync()
                                out[r] = (e.sched_trace(), spans)
                        except Exception as ex:   # noqa: BLE001
                            errs.append((r, repr(ex)))

                    ts = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(world)]
                    for t in ts:
                        t.start()
                    for t in ts:
                        t.join(timeout=60)
                    if errs or any(t.is_alive() for t in ts):
                        raise SystemExit(f"rank threads failed or hung: {errs}")
                    for r, (ops, spans) in enumerate(out):
                        n += 1
                        bad += check(ops, spans, None, [(r, gh.slab_plan(rows, world, r)[1])], k,
                                     dict(world=world, rank=r, layout=layout, boundary=boundary, k=k, split=split,
                                          steps=steps))
    print(f"sched bits rccl: {n} rank schedules, {bad} bad", flush=True)
    if bad:
        raise SystemExit(1)
    print("sched bits rccl ok")


if __name__ == "__main__":
    if os.environ.get("GOL_RCCL_SHIM"):
        ranks()
    else:
        contexts()
