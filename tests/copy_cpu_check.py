#!/usr/bin/env python3
"""The runtime's side of gol_copy_window / gol_copy over the host-only HIP stand-in
(no GPU): tests/fake_hip/fake_hip_copy.cpp runs the row routine of gol_copy.h on the
stand-in's host "device" memory, and boards go in and out as packed bits
(fake_hip_bits.cpp runs gol_bits.h's row routines for every layout), so after a copy
`dst` must download as the numpy statement of the definition applied to the two
downloads: mixed layouts, group widths, depths and boundaries (torus ghost margin,
MESH_COMPAT's reversed blocks, SERIAL_COMPAT's dead last row and column), different
slab counts with windows across the seams of both sides, either buffer current, the
same context with disjoint rectangles, every argument rule with `dst` verified
unchanged, pending async windows of both contexts delivered by the call.  The
stand-in offers one device, so the cross-device refusal is not reached here.
Run by tests/test_copy_cpu.py in a subprocess:

    GOL_LIB=tests/fake_hip/libgolhip_fakehip.so python tests/copy_cpu_check.py
    GOL_LIB=... GOL_RCCL_SHIM=tests/fake_hip/libfake_rccl_host.so python tests/copy_cpu_check.py
(the second form: rank contexts over the RCCL host stand-in as source and as destination)
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

EINVAL = -1
rng = np.random.default_rng(31)
OPS = ("replace", "or", "xor")


def put(e, board):
    e.upload_bits(np.packbits(board, axis=1))


def get(e):
    return np.unpackbits(e.download_bits(), axis=1)[:, :e.cols]


def soup(rows, cols, kw):
    b = (rng.random((rows, cols)) < 0.5).astype(np.uint8)
    if kw.get("boundary") == "serial_compat":
        b[-1] = 0
        b[:, -1] = 0
    return b


def merged(dst, src, win, at, op, kw):
    """The definition: numpy on the two downloads."""
    r0, c0, nr, nc = win
    out = dst.copy()
    s, o = src[r0:r0 + nr, c0:c0 + nc], out[at[0]:at[0] + nr, at[1]:at[1] + nc]
    out[at[0]:at[0] + nr, at[1]:at[1] + nc] = s if op == "replace" else (o | s) if op == "or" else (o ^ s)
    if kw.get("boundary") == "serial_compat":
        out[-1] = 0
        out[:, -1] = 0
    return out


CONFIGS = (
    (40, 300, dict(layout="bit", tblock_k=1)),                                     # 2-word groups
    (40, 300, dict(layout="bit", tblock_k=8)),                                     # 4-word groups
    (40, 300, dict(layout="byte", tblock_k=1)),
    (64, 200, dict(layout="bit", tblock_k=2, n_gpus=3)),                           # seams at rows 22 and 43
    (64, 200, dict(layout="byte", tblock_k=2, n_gpus=2)),                          # a seam at row 32
    (50, 131, dict(layout="bit", boundary="torus", tblock_k=8)),                   # ghost margin of 8 columns
    (50, 131, dict(layout="byte", boundary="torus", tblock_k=3, n_gpus=2)),
    (48, 48, dict(layout="bit", boundary="mesh_compat", mesh_m=4, tblock_k=2)),    # four reversed 12-column blocks
    (48, 48, dict(layout="byte", boundary="mesh_compat", mesh_m=2)),
    (30, 1024, dict(layout="bit", boundary="mesh_compat", mesh_m=2, tblock_k=2)),
    (37, 37, dict(layout="bit", boundary="serial_compat", tblock_k=16)),
    (37, 37, dict(layout="byte", boundary="serial_compat")),
)


def definition():
    n = 0
    for si, (srows, scols, skw) in enumerate(CONFIGS):
        for di, (drows, dcols, dkw) in enumerate(CONFIGS):
            with gh.Engine(srows, scols, **skw) as src, gh.Engine(drows, dcols, **dkw) as dst:
                # either buffer current: one k-step flips it (the stand-in's kernels compute nothing)
                if (si + di) % 2:
                    src.step(src.tblock_k)
                if di % 2:
                    dst.step(2 * dst.tblock_k)
                    dst.step(dst.tblock_k)
                sb, db = soup(srows, scols, skw), soup(drows, dcols, dkw)
                put(src, sb)
                put(dst, db)
                gens = src.generation, dst.generation
                for i in range(6):
                    nr, nc = int(rng.integers(1, min(srows, drows) + 1)), int(rng.integers(1, min(scols, dcols) + 1))
                    if i == 0:   # as large as fits: the last row and column of the smaller board
                        nr, nc = min(srows, drows), min(scols, dcols)
                    win = (int(rng.integers(0, srows - nr + 1)), int(rng.integers(0, scols - nc + 1)), nr, nc)
                    at = (int(rng.integers(0, drows - nr + 1)), int(rng.integers(0, dcols - nc + 1)))
                    op = OPS[(i + si + di) % 3]
                    dst.copy_from(src, win, at, op)
                    db = merged(db, sb, win, at, op, dkw)
                    assert (get(dst) == db).all(), (skw, dkw, win, at, op)
                    assert (get(src) == sb).all(), (skw, dkw, win, at, op)
                    n += 1
                assert (src.generation, dst.generation) == gens
                if (srows, scols) == (drows, dcols):   # gol_copy: the whole board, REPLACE
                    dst._chk(dst.lib.gol_copy(dst._c, src._c), "gol_copy")
                    assert (get(dst) == merged(db, sb, (0, 0, srows, scols), (0, 0), "replace", dkw)).all()
    return n


def seams():
    """3 slabs -> 2 slabs and 1 slab, row offsets that put seams of both sides inside the window."""
    sb = soup(64, 200, {})
    with gh.Engine(64, 200, layout="bit", tblock_k=2, n_gpus=3) as src:   # seams at 22, 43
        put(src, sb)
        for kw in (dict(layout="byte", tblock_k=2, n_gpus=2), dict(layout="bit", tblock_k=8, n_gpus=1),
                   dict(layout="bit", tblock_k=1, n_gpus=2)):
            with gh.Engine(70, 260, **kw) as dst:   # 2 slabs: a seam at 35
                db = soup(70, 260, kw)
                put(dst, db)
                for win, at in (((5, 3, 55, 190), (9, 33)),     # source seams at dst rows 26, 47; dst seam at src row 31
                                ((0, 0, 64, 200), (6, 60)), ((21, 0, 3, 200), (34, 1)), ((10, 7, 40, 1), (30, 259))):
                    for op in OPS:
                        dst.copy_from(src, win, at, op)
                        db = merged(db, sb, win, at, op, kw)
                        assert (get(dst) == db).all(), (kw, win, at, op)


def same_context():
    for kw in (dict(layout="bit", tblock_k=1), dict(layout="bit", tblock_k=8, n_gpus=2), dict(layout="byte"),
               dict(layout="bit", boundary="torus", tblock_k=8)):
        with gh.Engine(60, 300, **kw) as e:
            b = soup(60, 300, kw)
            put(e, b)
            L = e.lib
            # a 20 x 45 window tiled across the board: same rows (shared storage words), other rows, both
            for at, op in (((3, 50), "replace"), ((3, 96), "or"), ((3, 141), "xor"), ((30, 5), "replace"),
                           ((23, 49), "xor"), ((40, 255), "or")):
                e.copy_from(e, (3, 5, 20, 45), at, op)
                b = merged(b, b, (3, 5, 20, 45), at, op, kw)
                assert (get(e) == b).all(), (kw, at, op)
            for at in ((3, 5), (3, 49), (22, 49), (0, 0), (22, 5)):   # overlap: refused, unchanged
                assert L.gol_copy_window(e._c, at[0], at[1], e._c, 3, 5, 20, 45, 0) == EINVAL, at
                assert b"overlap" in L.gol_last_error(e._c)
                assert (get(e) == b).all()
            assert L.gol_copy(e._c, e._c) == EINVAL and b"overlap" in L.gol_last_error(e._c)
            assert L.gol_copy_window(e._c, 3, 5, e._c, 3, 5, 0, 45, 0) == 0   # empty: nothing overlaps


def arguments():
    L = gh.load()
    with gh.Engine(20, 100, layout="bit", tblock_k=8) as src, gh.Engine(30, 90, layout="byte") as dst:
        sb, db = soup(20, 100, {}), soup(30, 90, {})
        put(src, sb)
        dst.step(3)
        put(dst, db)
        assert L.gol_copy_window(None, 0, 0, src._c, 0, 0, 1, 1, 0) == EINVAL
        assert L.gol_copy_window(dst._c, 0, 0, None, 0, 0, 1, 1, 0) == EINVAL
        assert L.gol_copy(None, src._c) == EINVAL and L.gol_copy(dst._c, None) == EINVAL

        def refused(args, text):
            assert L.gol_copy_window(dst._c, args[0], args[1], src._c, *args[2:]) == EINVAL, args
            assert text in L.gol_last_error(dst._c), (args, L.gol_last_error(dst._c))
            assert (get(dst) == db).all() and (get(src) == sb).all() and dst.generation == 3

        # (drow0, dcol0, srow0, scol0, nrows, ncols, op)
        for a in ((0, 0, 0, 0, 21, 1, 0), (0, 0, 0, 11, 1, 90, 0), (0, 0, -1, 0, 1, 1, 0), (0, 0, 0, -1, 1, 1, 0),
                  (0, 0, 19, 0, 2, 1, 0), (0, 0, 0, 99, 1, 2, 0), (0, 0, 20, 100, 1, 1, 0)):
            refused(a, b"source window outside")
        for a in ((11, 0, 0, 0, 20, 1, 0), (0, 0, 0, 0, 1, 91, 0), (-1, 0, 0, 0, 1, 1, 0), (0, -1, 0, 0, 1, 1, 0),
                  (29, 0, 0, 0, 2, 1, 0), (0, 89, 0, 0, 1, 2, 0), (30, 90, 0, 0, 1, 1, 0)):
            refused(a, b"destination window outside")
        for a in ((0, 0, 0, 0, -1, 1, 0), (0, 0, 0, 0, 1, -1, 0), (5, 5, 5, 5, -3, -3, 1)):
            refused(a, b"negative")
        for op in (-1, 3, 7):
            refused((0, 0, 0, 0, 5, 5, op), b"unknown copy op")
        assert L.gol_copy(dst._c, src._c) == EINVAL and b"one size" in L.gol_last_error(dst._c)
        assert (get(dst) == db).all()
        # an empty window: GOL_OK, nothing written (at the far corner of both grids too)
        for a in ((0, 0, 0, 0, 0, 5, 0), (0, 0, 0, 0, 5, 0, 2), (30, 90, 20, 100, 0, 0, 0)):
            assert L.gol_copy_window(dst._c, a[0], a[1], src._c, *a[2:]) == 0
        assert (get(dst) == db).all() and dst.generation == 3
        # op names of the Python layer
        try:
            dst.copy_from(src, op="and")
        except ValueError:
            pass
        else:
            raise AssertionError("op")


def pending_delivered():
    """Async windows of both contexts pending at the call are delivered by it."""
    with gh.Engine(40, 200, layout="byte", n_gpus=2) as src, gh.Engine(40, 200, layout="bit", tblock_k=8) as dst:
        sb, db = soup(40, 200, {}), soup(40, 200, {})
        put(src, sb)
        put(dst, db)
        dg = src.digest()
        ws = src.download_window_async(3, 7, 30, 100)
        wd = dst.download_bits_window_async(2, 9, 20, 64)
        pend = src.digest_async()
        assert not ws.any() and not wd.any() and not pend.any()   # (not delivered yet)
        dst.copy_from(src, (0, 0, 10, 50), (25, 120))
        assert (ws == sb[3:33, 7:107]).all()
        assert (wd == np.packbits(db[2:22, 9:73], axis=1)).all()   # the board as it stood before the copy
        assert (int(pend[0]), int(pend[1])) == dg
        assert (get(dst) == merged(db, sb, (0, 0, 10, 50), (25, 120), "replace", {})).all()


def clones():
    with gh.Engine(40, 300, layout="bit", tblock_k=4, n_gpus=2, rule="B36/S23") as e:
        b = soup(40, 300, {})
        put(e, b)
        with e.clone() as c:
            assert (c.rows, c.cols, c.layout, c.tblock_k, c.n_gpus, c.rule) == (40, 300, "bit", 4, 2, e.rule)
            assert c.generation == 0 and (get(c) == b).all() and c.digest() == e.digest()
        with e.clone(tblock_k=1, n_gpus=1, boundary="torus") as c:
            assert c.rule == e.rule and (get(c) == b).all() and c.digest() == e.digest()
        with e.clone(rows=50, cols=310) as c:   # a larger board: the old one in its top left corner
            want = np.zeros((50, 310), np.uint8)
            want[:40, :300] = b
            assert (get(c) == want).all()
        for kw in (dict(tblock_k=8), dict(layout="byte")):   # targets that cannot run HighLife
            try:
                e.clone(**kw)
            except gh.GolError as ex:
                assert ex.code == -5, ex
            else:
                raise AssertionError(kw)
        with e.clone(layout="byte", rule="B3/S23") as c:
            assert (get(c) == b).all()


def ranks():
    rows, cols, world = 64, 200, 3
    board = (np.random.default_rng(5).random((rows, cols)) < 0.5).astype(np.uint8)
    uid = gh.unique_id()
    out, errs = [None] * world, []

    def worker(r):
        try:
            row0, n = gh.slab_plan(rows, world, r)
            mine = np.zeros_like(board)
            mine[row0:row0 + n] = board[row0:row0 + n]
            with gh.Engine(rows, cols, rank=r, world=world, device=0, uid=uid, layout="bit", tblock_k=2) as e, \
                    gh.Engine(rows, cols, layout="byte") as full, gh.Engine(rows, cols, layout="bit", tblock_k=8) as got:
                L = e.lib
                put(full, board)
                # a rank context as destination: the rows it holds are written, the others skipped
                e.copy_from(full)
                assert (get(e) == mine).all(), r
                e._chk(L.gol_copy(e._c, full._c), "gol_copy")
                assert (get(e) == mine).all(), r
                # ... and a window with none of its rows is GOL_OK and writes nothing
                other = gh.slab_plan(rows, world, (r + 1) % world)[0]
                e.copy_from(full, (0, 0, 1, cols), (other, 0), "xor")
                assert (get(e) == mine).all(), r
                # a rank context as source: its rows into a single-slab context
                got.copy_from(e, (row0, 0, n, cols), (row0, 0))
                out[r] = get(got)
                assert (out[r] == mine).all(), r
                # a source row the rank does not hold: refused, nothing written
                for win in ((0, 0, rows, cols), (other, 0, 1, cols)):
                    assert L.gol_copy_window(got._c, win[0], 0, e._c, *win, 0) == EINVAL, (r, win)
                    assert b"does not hold" in L.gol_last_error(got._c)
                    assert (get(got) == mine).all(), r
                try:
                    e.clone()
                except ValueError:
                    pass
                else:
                    raise AssertionError("clone of a rank context")
        except Exception as ex:   # noqa: BLE001
            errs.append((r, repr(ex)))

    ts = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=60)
    if errs or any(t.is_alive() for t in ts):
        raise SystemExit(f"rank threads failed or hung: {errs}")
    assert (sum(out) == board).all()   # the ranks' copies tile the board
    print("copy cpu ranks ok")


if __name__ == "__main__":
    if os.environ.get("GOL_RCCL_SHIM"):
        ranks()
    else:
        n = definition()
        seams()
        same_context()
        arguments()
        pending_delivered()
        clones()
        print(f"copy cpu ok: {n} copies")
