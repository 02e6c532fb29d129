"""gol_digest on rank contexts, on ONE GPU: every rank a host thread with its own
gol_ctx over tests/shim/libfake_rccl.so (see tests/rccl_shim_check.py).  A rank
returns the digest of its own slab's rows; the parts, added mod 2^64 by the
caller (no collective), must equal the digest of a single context that ran the
same board, and the reference digest of the ranks' assembled downloads.  2 and
3 ranks, dead and torus boundaries.  Started in a fresh process by
tests/test_gpu_digest.py.

    python tests/digest_rank_check.py <libfake_rccl.so>
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

from digest_ref import add, digest_ref  # noqa: E402
from mpi_amd import golhip as gh  # noqa: E402


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
                pending = e.digest_async()
                part = e.digest()   # synchronises: fills the pending one too
                row0, n = gh.slab_plan(rows, world, r)
                # a window reaching into the neighbours' rows: only the rows held here count
                lo, hi = max(0, row0 - 2), min(rows, row0 + n + 2)
                assert e.digest_window(lo, 0, hi - lo, cols) == part, (r, "window past the slab")
                assert (int(pending[0]), int(pending[1])) == part, (r, "async part")
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
    got = np.zeros((rows, cols), np.uint8)
    for row0, w, _ in out:
        got[row0:row0 + w.shape[0]] = w
    return got, [o[2] for o in out], [(o[0], o[1]) for o in out]


def main():
    rng = np.random.default_rng(41)
    for world in (2, 3):
        for boundary in ("dead", "torus"):
            for layout, k in (("bit", 8), ("bit", 3), ("byte", 2)):
                rows, cols = world * (2 * k + 1) + 1, 200 + 3 * k
                steps = [k, max(1, k - 3), k]
                b0 = (rng.random((rows, cols)) < 0.4).astype(np.uint8)
                kw = dict(layout=layout, boundary=boundary, tblock_k=k)
                got, parts, slabs = run_ranks(world, b0, steps, **kw)
                with gh.Engine(rows, cols, **kw) as e:
                    e.upload(b0)
                    for st in steps:
                        e.step(st)
                    single, board = e.digest(), e.download()
                ok = (got == board).all() and add(*parts) == single == digest_ref(got)
                # each part is the reference digest of that rank's rows at their global place
                ok = ok and all(p == digest_ref(w, row0, 0) for p, (row0, w) in zip(parts, slabs))
                print(f"world={world} {boundary} {rows}x{cols} {layout} k={k}: {'ok' if ok else 'MISMATCH'}", flush=True)
                if not ok:
                    raise SystemExit(1)
    print("digest ranks ok")


if __name__ == "__main__":
    main()
