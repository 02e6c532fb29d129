"""gol_copy_window on rank contexts, on ONE GPU: every rank a host thread with its own
gol_ctx over tests/shim/libfake_rccl.so (see tests/rccl_shim_check.py).  A rank context
as destination takes the rows it holds from a single-process board and skips the
others; as source it hands its rows to a single-slab context of another layout: the
ranks' copies tile the source board; a source row the rank does not hold is refused.
Started in a fresh process by tests/test_gpu_copy.py.

    python tests/copy_rank_check.py <libfake_rccl.so>
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


def run_ranks(world, rows, cols, board, layout, k, other):
    uid = gh.unique_id()
    out, errs = [None] * world, []

    def worker(r):
        try:
            row0, n = gh.slab_plan(rows, world, r)
            mine = np.zeros_like(board)
            mine[row0:row0 + n] = board[row0:row0 + n]
            with gh.Engine(rows, cols, rank=r, world=world, device=0, uid=uid, layout=layout, tblock_k=k) as e, \
                    gh.Engine(rows, cols, layout=other[0], tblock_k=other[1]) as full, \
                    gh.Engine(rows + 3, cols + 40, layout=other[0], tblock_k=other[1]) as got:
                full.upload(board)
                e.copy_from(full)   # destination: the rows it holds, the others are skipped
                assert (e.download() == mine).all(), (r, "as destination")
                nxt = gh.slab_plan(rows, world, (r + 1) % world)[0]
                e.copy_from(full, (0, 0, 1, cols), (nxt, 0), "xor")   # none of its rows: GOL_OK, nothing written
                assert (e.download() == mine).all(), (r, "foreign rows")
                got.copy_from(e, (row0, 5, n, cols - 5), (row0 + 3, 38))   # source: its rows, shifted by 33 columns
                part = got.download()
                for win in ((0, 0, rows, cols), (nxt, 0, 1, cols)):   # rows it does not hold: refused
                    rc = e.lib.gol_copy_window(got._c, 0, 0, e._c, *win, 0)
                    assert rc == -1 and b"does not hold" in e.lib.gol_last_error(got._c), (r, win, rc)
                assert (got.download() == part).all(), (r, "refused copies wrote")
                out[r] = part
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
    rng = np.random.default_rng(17)
    for world in (2, 3):
        for layout, k, other in (("bit", 8, ("byte", 1)), ("byte", 2, ("bit", 8)), ("bit", 1, ("bit", 8))):
            rows, cols = world * (2 * k + 1) + 1, 200 + 3 * k
            board = (rng.random((rows, cols)) < 0.5).astype(np.uint8)
            out = run_ranks(world, rows, cols, board, layout, k, other)
            want = np.zeros((rows + 3, cols + 40), np.uint8)
            want[3:rows + 3, 38:cols + 33] = board[:, 5:]
            ok = board.any() and (sum(out) == want).all()   # the ranks' copies tile the source board
            print(f"world={world} {rows}x{cols} {layout} k={k} -> {other}: {'ok' if ok else 'MISMATCH'}", flush=True)
            if not ok:
                raise SystemExit(1)
    print("copy ranks ok")


if __name__ == "__main__":
    main()
