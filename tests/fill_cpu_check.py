#!/usr/bin/env python3
"""The runtime's side of gol_fill_random* over the host-only HIP stand-in (no GPU):
tests/fake_hip/fake_hip_fill.cpp runs the row routine of gol_fill.h on the
stand-in's host "device" memory, and a byte-layout board's byte downloads are plain
copies there, so a filled byte board must download as tests/fill_ref.py's board:
the whole board, windows at any column, slabs with seams, the torus ghost margin,
MESH_COMPAT column runs, SERIAL_COMPAT's dead last row and column and the argument
rules.  Run by tests/test_fill_cpu.py in a subprocess:

    GOL_LIB=tests/fake_hip/libgolhip_fakehip.so python tests/fill_cpu_check.py
    GOL_LIB=... GOL_RCCL_SHIM=tests/fake_hip/libfake_rccl_host.so python tests/fill_cpu_check.py
(the second form: three rank contexts over the RCCL host stand-in, whose parts tile the board's fill)
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
from fill_ref import FULL, fill_ref  # noqa: E402

EINVAL = -1
rng = np.random.default_rng(29)
THRESHOLDS = (1 << 31, 3 << 29, 0x55555555, 1 << 20, FULL - 1, 0, FULL)


def expect(kw, board):
    if kw.get("boundary") == "serial_compat":
        board = board.copy()
        board[-1] = 0
        board[:, -1] = 0
    return board


def boards():
    n = 0
    for rows, cols, kw in ((64, 200, dict()),                                  # 1 slab
                           (64, 200, dict(n_gpus=3, tblock_k=2)),              # seams at rows 22 and 43
                           (37, 131, dict(n_gpus=2)),
                           (64, 64, dict(boundary="torus", tblock_k=3)),       # ghost margin of 3 columns
                           (40, 131, dict(boundary="torus", tblock_k=16, n_gpus=2)),
                           (48, 48, dict(boundary="mesh_compat", mesh_m=2)),   # two reversed 24-column blocks
                           (48, 48, dict(boundary="mesh_compat", mesh_m=4)),
                           (37, 37, dict(boundary="serial_compat"))):
        with gh.Engine(rows, cols, layout="byte", **kw) as e:
            for i, t in enumerate(THRESHOLDS):
                seed = (0, 1, 12345, 2**64 - 1)[i % 4]
                e.fill_random(seed=seed, threshold=t)
                assert e.generation == 0
                want = expect(kw, fill_ref(seed, t, rows, cols))
                assert (e.download() == want).all(), (rows, cols, kw, seed, t)
            # windows at any column: exactly the window changes, to the same cells of a whole-board fill
            cur = e.download()
            for i in range(24):
                r0, c0 = int(rng.integers(0, rows)), int(rng.integers(0, cols))
                nr, nc = int(rng.integers(1, rows - r0 + 1)), int(rng.integers(1, cols - c0 + 1))
                seed, t = int(rng.integers(0, 2**63)), THRESHOLDS[i % 5]
                e.fill_random(seed=seed, threshold=t, window=(r0, c0, nr, nc))
                cur[r0:r0 + nr, c0:c0 + nc] = fill_ref(seed, t, rows, cols)[r0:r0 + nr, c0:c0 + nc]
                cur = expect(kw, cur)
                assert (e.download() == cur).all(), (rows, cols, kw, r0, c0, nr, nc)
            n += 1
    return n


def seams_window():
    """3 slabs (seams at rows 22 and 43): one window across both seams, on a board of ones."""
    with gh.Engine(64, 200, layout="byte", n_gpus=3, tblock_k=2) as e:
        e.step(2)   # (one k-step: the current buffer is the second one)
        e.upload(np.ones((64, 200), np.uint8))
        before = e.download()
        assert before.all()
        e.fill_random(0.375, seed=5, window=(10, 37, 45, 101))
        assert e.generation == 2   # the generation stays
        want = before.copy()
        want[10:55, 37:138] = fill_ref(5, 3 << 29, 45, 101, 10, 37)
        assert (e.download() == want).all()
        e.step(2)   # and the context steps on
        assert e.generation == 4


def arguments():
    L = gh.load()
    t = ctypes.c_uint64()
    assert L.gol_fill_threshold(0.5, None) == EINVAL
    assert L.gol_fill_random(None, 0, 0) == EINVAL and L.gol_fill_random_window(None, 0, 0, 1, 1, 0, 0) == EINVAL
    assert L.gol_fill_threshold(0.25, ctypes.byref(t)) == 0 and t.value == 1 << 30
    with gh.Engine(20, 100, layout="byte") as e:
        e.fill_random(0.5, seed=9)
        want = fill_ref(9, 1 << 31, 20, 100)
        e.step(3)
        e.upload(want)
        for win in ((0, 0, 21, 100), (0, 0, 20, 101), (-1, 0, 1, 1), (0, -1, 1, 1), (5, 32, -1, 1), (19, 96, 2, 1),
                    (0, 99, 1, 2)):
            assert L.gol_fill_random_window(e._c, *win, 1, 1 << 31) == EINVAL, win
            assert b"outside the grid" in L.gol_last_error(e._c)
            assert (e.download() == want).all()   # usable, unchanged
        for call in (lambda: L.gol_fill_random(e._c, 1, FULL + 1),
                     lambda: L.gol_fill_random_window(e._c, 0, 0, 5, 5, 1, FULL + 1),
                     lambda: L.gol_fill_random(e._c, 1, 2**64 - 1)):
            assert call() == EINVAL and b"threshold" in L.gol_last_error(e._c)
            assert (e.download() == want).all()
        # an empty window: GOL_OK, nothing written
        for win in ((20, 100, 0, 0), (3, 32, 0, 5), (3, 32, 5, 0)):
            assert L.gol_fill_random_window(e._c, *win, 1, FULL) == 0
        assert (e.download() == want).all() and e.generation == 3
        # (a fill beside the clock probe: tests/test_gpu_fill.py — the stand-in has no probe kernel)
    for p in (-0.1, 1.1, float("nan"), float("inf")):
        try:
            gh.fill_threshold(p)
        except gh.GolError as ex:
            assert ex.code == EINVAL
        else:
            raise AssertionError(p)


def ranks():
    rows, cols, world = 64, 200, 3
    want = fill_ref(77, 3 << 29, rows, cols)
    uid = gh.unique_id()
    out, errs = [None] * world, []

    def worker(r):
        try:
            with gh.Engine(rows, cols, rank=r, world=world, device=0, uid=uid, layout="byte") as e:
                e.fill_random(0.375, seed=77)   # a rank fills its own rows
                part = e.download()
                # a window with no local rows is GOL_OK for a rank context, and writes nothing
                other = gh.slab_plan(rows, world, (r + 1) % world)[0]
                e.fill_random(1.0, seed=1, window=(other, 0, 1, cols))
                assert (e.download() == part).all()
                out[r] = part
        except Exception as ex:   # noqa: BLE001
            errs.append((r, repr(ex)))

    ts = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=60)
    if errs or any(t.is_alive() for t in ts):
        raise SystemExit(f"rank threads failed or hung: {errs}")
    for r in range(world):
        row0, n = gh.slab_plan(rows, world, r)
        mine = np.zeros_like(want)
        mine[row0:row0 + n] = want[row0:row0 + n]
        assert (out[r] == mine).all(), r   # untouched (0) outside its slab
    assert (sum(out) == want).all()
    print("fill cpu ranks ok")


if __name__ == "__main__":
    if os.environ.get("GOL_RCCL_SHIM"):
        ranks()
    else:
        n = boards()
        seams_window()
        arguments()
        print(f"fill cpu ok: {n} boards")
