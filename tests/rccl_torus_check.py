"""GOL_TORUS through the library's RCCL transport on ONE GPU: every rank a host
thread with its own gol_ctx over tests/shim/libfake_rccl.so (see
tests/rccl_shim_check.py), the halo exchange closed into a ring — peers
(rank ± 1) mod world; with two ranks both peers are the same rank and the
order of the sends and receives pairs the halos; one rank copies to itself —
checked bit-exactly against tests/torus_ref.py, and one world's recorded
schedules race-checked (tests/sched_race.py).  Started in a fresh process by
tests/test_gpu_torus.py.

    python tests/rccl_torus_check.py <libfake_rccl.so>
"""
import ctypes
import os
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
ctypes.CDLL(sys.argv[1], mode=ctypes.RTLD_GLOBAL)

import numpy as np  # noqa: E402

import torus_ref  # noqa: E402
from mpi_amd import golhip as gh  # noqa: E402
from sched_race import find_races  # noqa: E402


def run_ranks(world, b0, layout, k, steps, split=None, trace=False):
    rows, cols = b0.shape
    uid = gh.unique_id()
    out, errs = [None] * world, []

    def worker(r):
        try:
            with gh.Engine(rows, cols, rank=r, world=world, device=0, uid=uid, layout=layout, tblock_k=k,
                           boundary="torus") as e:
                if split is not None:
                    e.set_option(gh.OPT_INTERIOR_SPLIT, split)
                e.upload(b0)
                if trace:
                    e.set_option(gh.OPT_SCHED_TRACE, 1)
                for st in steps:
                    e.step(st)
                e.sync()
                ops = e.sched_trace() if trace else None
                row0, n = gh.slab_plan(rows, world, r)
                out[r] = (row0, e.download_window(row0, 0, n, cols), e.popcount(), ops)
        except Exception as ex:   # noqa: BLE001
            errs.append((r, repr(ex)))

    ts = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    if any(t.is_alive() for t in ts):
        raise SystemExit(f"rank threads hung (world={world})")
    if errs:
        raise SystemExit(f"rank errors: {errs}")
    got = np.zeros((rows, cols), np.uint8)
    for row0, w, _, _ in out:
        got[row0:row0 + w.shape[0]] = w
    return got, sum(o[2] for o in out), [o[3] for o in out]


def main():
    rng = np.random.default_rng(31)
    for world in (1, 2, 3):
        for layout in ("bit", "byte"):
            for k in (1, 8, 16):
                # thin slabs of uneven height; a short block followed by full ones
                rows, cols = world * (2 * k + 1) + (world > 1), 200 + 3 * k
                steps = [k, max(1, k - 3), k, 2 * k]
                b0 = (rng.random((rows, cols)) < 0.4).astype(np.uint8)
                want = torus_ref.run(b0, sum(steps))
                got, live, _ = run_ranks(world, b0, layout, k, steps)
                bad = int((got != want).sum())
                print(f"world={world} {rows}x{cols} {layout} k={k} steps={steps}: "
                      f"{'ok' if bad == 0 and live == int(want.sum()) else f'{bad} cells differ, live {live}'}",
                      flush=True)
                if bad or live != int(want.sum()):
                    raise SystemExit(1)
    print("rccl torus ok")
    # slabs with an overlapped, split interior, the schedule recorded and race-checked
    for world in (2, 3):
        k = 8
        rows, cols = world * (2 * 32 * k + 2 * k + 5), 300
        steps = [8, 3, 8, 8, 1, 8]
        b0 = (rng.random((rows, cols)) < 0.4).astype(np.uint8)
        want = torus_ref.run(b0, sum(steps))
        got, live, traces = run_ranks(world, b0, "bit", k, steps, split=2, trace=True)
        races = [(r, find_races(ops)) for r, ops in enumerate(traces)]
        bad = int((got != want).sum())
        print(f"sched world={world} {rows}x{cols} bit k={k} split=2: ops {[len(o) for o in traces]}, "
              f"{bad} cells differ, races {[r for r in races if r[1]]}", flush=True)
        if bad or live != int(want.sum()) or any(r[1] for r in races):
            raise SystemExit(1)
    print("rccl torus sched ok")


if __name__ == "__main__":
    main()
