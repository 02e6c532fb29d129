"""gol_fill_random on rank contexts, on ONE GPU: every rank a host thread with its own
gol_ctx over tests/shim/libfake_rccl.so (see tests/rccl_shim_check.py).  A rank fills
its own rows with no word from the others; the ranks' parts tile the board's fill
(tests/fill_ref.py), their digests add up to the board's, and after the same steps
the parts equal a single context's board.  Started in a fresh process by
tests/test_gpu_fill.py.

    python tests/fill_rank_check.py <libfake_rccl.so>
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

from mpi_amd import golhip as gh  # noqa: E402
from digest_ref import add, digest_ref  # noqa: E402
from fill_ref import fill_ref  # noqa: E402


def run_ranks(world, rows, cols, seed, threshold, steps, **kw):
    uid = gh.unique_id()
    out, errs = [None] * world, []

    def worker(r):
        try:
            with gh.Engine(rows, cols, rank=r, world=world, device=0, uid=uid, **kw) as e:
                e.fill_random(seed=seed, threshold=threshold)
                row0, n = gh.slab_plan(rows, world, r)
                filled, d = e.download_window(row0, 0, n, cols), e.digest()
                # a window with no local rows: GOL_OK, nothing written
                other = gh.slab_plan(rows, world, (r + 1) % world)[0]
                e.fill_random(1.0, seed=1, window=(other, 0, 1, cols))
                assert (e.download_window(row0, 0, n, cols) == filled).all(), (r, "foreign window")
                for st in steps:
                    e.step(st)
                out[r] = (row0, n, filled, d, e.download_window(row0, 0, n, cols))
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
    return out


def main():
    for world in (2, 3):
        for boundary in ("dead", "torus"):
            for layout, k in (("bit", 8), ("byte", 2)):
                rows, cols = world * (2 * k + 1) + 1, 200 + 3 * k
                steps = [k, max(1, k - 3), k]
                seed, t = 1000 + world, 3 << 29
                b0 = fill_ref(seed, t, rows, cols)
                out = run_ranks(world, rows, cols, seed, t, steps, layout=layout, boundary=boundary, tblock_k=k)
                with gh.Engine(rows, cols, layout=layout, boundary=boundary, tblock_k=k) as one:
                    one.upload(b0)
                    for st in steps:
                        one.step(st)
                    want = one.download()
                ok = want.any() and add(*(o[3] for o in out)) == digest_ref(b0)
                for row0, n, filled, _, cells in out:
                    ok = ok and (filled == b0[row0:row0 + n]).all() and (cells == want[row0:row0 + n]).all()
                print(f"world={world} {boundary} {rows}x{cols} {layout} k={k}: {'ok' if ok else 'MISMATCH'}", flush=True)
                if not ok:
                    raise SystemExit(1)
    print("fill ranks ok")


if __name__ == "__main__":
    main()
