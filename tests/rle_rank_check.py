"""RLE pattern text on rank contexts, on ONE GPU: every rank a host thread with its
own gol_ctx over tests/shim/libfake_rccl.so (see tests/rccl_shim_check.py).  A rank
formats the rows it holds (its part, as the driver's --format rle writes it), refuses
a window with a row of its neighbour's, and reads a pattern into its own rows; the
parts, placed at their origins, must tile a single context's board after the same
steps.  Started in a fresh process by tests/test_gpu_rle.py.

    python tests/rle_rank_check.py <libfake_rccl.so>
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

import rle_ref  # noqa: E402
from mpi_amd import golhip as gh  # noqa: E402


def run_ranks(world, b0, steps, **kw):
    rows, cols = b0.shape
    uid = gh.unique_id()
    out, errs = [None] * world, []

    def worker(r):
        try:
            with gh.Engine(rows, cols, rank=r, world=world, device=0, uid=uid, **kw) as e:
                row0, n = gh.slab_plan(rows, world, r)
                # the rank's rows come in as a pattern
                assert e.parse_rle(rle_ref.encode(b0[row0:row0 + n]), at=(row0, 0)) == (cols, n)
                for st in steps:
                    e.step(st)
                part = e.format_rle((row0, 0, n, cols))
                assert e.rle_bytes((row0, 0, n, cols)) == len(part)
                cnt = ctypes.c_int64()
                other = (row0 - 1, 0, 2, cols) if r else (row0 + n - 1, 0, 2, cols)
                assert e.lib.gol_rle_bytes(e._c, *other, ctypes.byref(cnt)) == -1
                assert b"not all held" in e.lib.gol_last_error(e._c)
                out[r] = (row0, n, part, e.download_window(row0, 0, n, cols))
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
    rng = np.random.default_rng(53)
    world = 2
    for boundary in ("dead", "torus"):
        for layout, k in (("bit", 8), ("byte", 2)):
            rows, cols = world * (2 * k + 1) + 1, 200 + 3 * k
            steps = [k, max(1, k - 3), k]
            b0 = (rng.random((rows, cols)) < 0.4).astype(np.uint8)
            out = run_ranks(world, b0, steps, layout=layout, boundary=boundary, tblock_k=k)
            with gh.Engine(rows, cols, layout=layout, boundary=boundary, tblock_k=k) as one:
                one.upload(b0)
                for st in steps:
                    one.step(st)
                want = one.download()
            ok = bool(want.any())
            for row0, n, part, cells in out:
                ok = ok and part == rle_ref.encode(want[row0:row0 + n]) and (cells == want[row0:row0 + n]).all()
            print(f"world={world} {boundary} {rows}x{cols} {layout} k={k}: {'ok' if ok else 'MISMATCH'}", flush=True)
            if not ok:
                raise SystemExit(1)
    print("rle ranks ok")


if __name__ == "__main__":
    main()
