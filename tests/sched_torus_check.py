#!/usr/bin/env python3
"""Step schedules of GOL_TORUS contexts, recorded on the CPU (the runtime's host
code over tests/fake_hip, as tests/sched_cpu_check.py does) and race-checked by
happens-before (sched_race.py): the halo ring of 1, 2 and 3 slabs (a single
slab exchanges with itself; with two, both neighbours are the same slab), the
wrap launch behind every stencil launch, interior split 1 and 2, k = 1, 8, 16,
both layouts, overlap on and off, uneven steps with a short block followed by
a full one (the exchange's "grow" dependency), an async window copy mid-run.
Run by tests/test_torus_cpu.py in a subprocess.

    GOL_LIB=tests/fake_hip/libgolhip_fakehip.so python tests/sched_torus_check.py
    GOL_LIB=... GOL_RCCL_SHIM=tests/fake_hip/libfake_rccl_host.so python tests/sched_torus_check.py
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


def step_lists(k):
    # a short block followed by a full one, twice; a run of full ones; single generations
    return [[k, max(1, k - 3), k, k, 1, k, max(1, k // 2), k, k], [1, k, k], [k] * 5]


def wraps_and_launches(ops):
    """(wrap launches, stencil launches) of a trace.  A wrap is a READ directly followed
    by a WRITE of the same rows of the SAME buffer on one stream; a stencil launch reads
    one buffer and writes the other; the exchange copies between different rows."""
    ops = np.asarray(ops)
    wraps = stencils = 0
    for a, b in zip(ops[:-1], ops[1:]):
        if a[0] == READ and b[0] == WRITE and a[1] == b[1] and a[3] == b[3]:
            if a[4] == b[4] and a[5] == b[5] and a[6] == b[6]:
                wraps += 1
            elif a[4] != b[4]:
                stencils += 1
    return wraps, stencils


def check(ops, what):
    races = find_races(ops)
    wraps, stencils = wraps_and_launches(ops)
    if races:
        print("RACE", what, races[0][2], flush=True)
        return 1
    if stencils == 0 or wraps != stencils:
        print("WRAPS", what, f"{wraps} wrap launches for {stencils} stencil launches", flush=True)
        return 1
    return 0


def contexts():
    bad = n = 0
    for layout in ("bit", "byte"):
        for k in (1, 8, 16):
            for slabs in (1, 2, 3):
                for split in (1, 2):
                    for overlap in (1, 0):
                        # rows: with the split, room for two parts per slab (32·K rows each); else thin and uneven slabs
                        rows = slabs * (2 * 32 * k + 2 * k + 5) + 1 if split == 2 else slabs * (2 * k + 3) + 1
                        cols = 200
                        for steps in step_lists(k):
                            with gh.Engine(rows, cols, n_gpus=slabs, layout=layout, boundary="torus", tblock_k=k) as e:
                                e.upload(np.zeros((rows, cols), np.uint8))
                                e.set_option(gh.OPT_OVERLAP, overlap)
                                e.set_option(gh.OPT_INTERIOR_SPLIT, split)
                                e.set_option(gh.OPT_SCHED_TRACE, 1)
                                for i, st in enumerate(steps):
                                    e.step(st)
                                    if i == 1:
                                        e.download_window_async(rows // 2, 0, 2, 40)
                                e.sync()
                                ops = e.sched_trace()
                            n += 1
                            bad += check(ops, dict(layout=layout, k=k, slabs=slabs, split=split, overlap=overlap,
                                                   rows=rows, steps=steps))
    # control: the two-slab ring's schedule without its event waits must race
    with gh.Engine(2 * 600, 200, n_gpus=2, layout="bit", boundary="torus", tblock_k=8) as e:
        e.set_option(gh.OPT_INTERIOR_SPLIT, 2)
        e.set_option(gh.OPT_SCHED_TRACE, 1)
        for st in (8, 3, 8, 8):
            e.step(st)
        e.sync()
        ops = e.sched_trace()
    control = len(find_races(ops[ops[:, 0] != WAIT]))
    print(f"sched torus: {n} contexts, {bad} bad; control (waits stripped) {control} races", flush=True)
    if bad or control == 0:
        raise SystemExit(1)
    print("sched torus ok")


def ranks():
    bad = n = 0
    for world in (1, 2, 3):
        for layout, k, split in (("bit", 1, 1), ("bit", 8, 2), ("bit", 16, 1), ("byte", 8, 1), ("byte", 16, 2)):
            rows = world * (2 * 32 * k + 2 * k + 5) + 1 if split == 2 else world * (2 * k + 3) + 1
            cols = 200
            for steps in step_lists(k)[:2]:
                uid = gh.unique_id()
                out, errs = [None] * world, []

                def worker(r):
                    try:
                        with gh.Engine(rows, cols, rank=r, world=world, device=0, uid=uid, layout=layout,
                                       boundary="torus", tblock_k=k) as e:
                            e.upload(np.zeros((rows, cols), np.uint8))
                            e.set_option(gh.OPT_INTERIOR_SPLIT, split)
                            e.set_option(gh.OPT_SCHED_TRACE, 1)
                            for i, st in enumerate(steps):
                                e.step(st)
                                if i == 1:
                                    r0, nr = gh.slab_plan(rows, world, r)
                                    e.download_window_async(r0 + nr // 2, 0, 2, 40)
                            e.sync()
                            out[r] = e.sched_trace()
                    except Exception as ex:   # noqa: BLE001
                        errs.append((r, repr(ex)))

                ts = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(world)]
                for t in ts:
                    t.start()
                for t in ts:
                    t.join(timeout=60)
                if errs or any(t.is_alive() for t in ts):
                    raise SystemExit(f"rank threads failed or hung: {errs}")
                for r, ops in enumerate(out):
                    n += 1
                    bad += check(ops, dict(world=world, rank=r, layout=layout, k=k, split=split, steps=steps))
    print(f"sched torus rccl: {n} rank schedules, {bad} bad", flush=True)
    if bad:
        raise SystemExit(1)
    print("sched torus rccl ok")


if __name__ == "__main__":
    ranks() if os.environ.get("GOL_RCCL_SHIM") else contexts()
