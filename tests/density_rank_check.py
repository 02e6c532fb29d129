"""gol_density on rank contexts, on ONE GPU: every rank a host thread with its own
gol_ctx over tests/shim/libfake_rccl.so (see tests/rccl_shim_check.py).  A rank
returns the counts of its own slab's rows and 0 in every tile it holds nothing
of; the maps, added by the caller (no collective), must equal the reference
map of the ranks' assembled downloads.  Two ranks, tile rows of 7 so that a
tile straddles the seam.  Started in a fresh process by tests/test_gpu_density.py.

    python tests/density_rank_check.py <libfake_rccl.so>
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

from density_ref import density_ref  # noqa: E402
from mpi_amd import golhip as gh  # noqa: E402

TH, TW = 7, 32


def run_ranks(world, b0, steps, **kw):
    rows, cols = b0.shape
    uid = gh.unique_id()
    out, errs = [None] * world, []

    def worker(r):
        try:
            with gh.Engine(rows, cols, rank=r, world=world, device=0, uid=uid, **kw) as e:
                e.upload(b0)
                for st in steps:
                    e.step(st)
                pending = e.density_async(TH, TW)
                part = e.density(TH, TW)   # synchronises: fills the pending one too
                assert (pending == part).all(), (r, "async part")
                row0, n = gh.slab_plan(rows, world, r)
                out[r] = (row0, e.download_window(row0, 0, n, cols), part)
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
    rng = np.random.default_rng(43)
    world = 2
    for boundary in ("dead", "torus"):
        for layout, k in (("bit", 8), ("byte", 2)):
            rows, cols = world * (2 * k + 1) + 1, 200 + 3 * k
            steps = [k, max(1, k - 3), k]
            b0 = (rng.random((rows, cols)) < 0.4).astype(np.uint8)
            out = run_ranks(world, b0, steps, layout=layout, boundary=boundary, tblock_k=k)
            got = np.zeros((rows, cols), np.uint8)
            for row0, w, _ in out:
                got[row0:row0 + w.shape[0]] = w
            ok = got.any() and (sum(o[2] for o in out) == density_ref(got, TH, TW)).all()
            for row0, w, part in out:   # each rank's map: its own rows at their global place, 0 elsewhere
                mine = np.zeros_like(got)
                mine[row0:row0 + w.shape[0]] = w
                ok = ok and (part == density_ref(mine, TH, TW)).all()
            print(f"world={world} {boundary} {rows}x{cols} {layout} k={k}: {'ok' if ok else 'MISMATCH'}", flush=True)
            if not ok:
                raise SystemExit(1)
    print("density ranks ok")


if __name__ == "__main__":
    main()
