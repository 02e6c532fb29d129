"""gol_download_bits / gol_upload_bits on rank contexts, on ONE GPU: every rank a host
thread with its own gol_ctx over tests/shim/libfake_rccl.so (see
tests/rccl_shim_check.py).  A rank takes its own rows of a whole-board packed
buffer and fills its own rows only; the ranks' parts tile the board, which must
equal a single context's after the same steps.  Started in a fresh process by
tests/test_gpu_bits.py.

    python tests/bits_rank_check.py <libfake_rccl.so>
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


def run_ranks(world, b0, steps, **kw):
    rows, cols = b0.shape
    uid = gh.unique_id()
    out, errs = [None] * world, []
    packed = np.packbits(b0, axis=1)

    def worker(r):
        try:
            with gh.Engine(rows, cols, rank=r, world=world, device=0, uid=uid, **kw) as e:
                e.upload_bits(packed)   # the whole board's rows: the rank takes its own
                for st in steps:
                    e.step(st)
                row0, n = gh.slab_plan(rows, world, r)
                pending = e.download_bits_window_async(row0, 0, n, cols)
                part = e.download_bits()   # synchronises: fills the pending one too
                assert (pending == part[row0:row0 + n]).all(), (r, "async part")
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
    rng = np.random.default_rng(47)
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
            ok = want.any()
            for row0, n, part, cells in out:   # its own rows at their global place, 0 (untouched) elsewhere
                mine = np.zeros_like(want)
                mine[row0:row0 + n] = want[row0:row0 + n]
                ok = ok and (part == np.packbits(mine, axis=1)).all() and (cells == want[row0:row0 + n]).all()
            print(f"world={world} {boundary} {rows}x{cols} {layout} k={k}: {'ok' if ok else 'MISMATCH'}", flush=True)
            if not ok:
                raise SystemExit(1)
    print("bits ranks ok")


if __name__ == "__main__":
    main()
