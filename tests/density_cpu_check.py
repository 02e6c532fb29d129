#!/usr/bin/env python3
"""The runtime's side of gol_density* over the host-only HIP stand-in (no GPU):
tests/fake_hip/fake_hip_density.cpp runs the row routine of gol_density.h on the
stand-in's host "device" memory, and a byte-layout board's uploads and
downloads are plain copies there, so for byte boards (no stepping: the stencil
stand-ins do nothing) density() must equal the reference map of download():
per-slab parts and their sum (tiles that straddle slab seams), MESH_COMPAT
column runs, the torus ghost margin, SERIAL_COMPAT's dead last row and column,
offset windows, several pending async maps, the argument rules and a failed
call that must leave no pending write.  Run by tests/test_density_cpu.py in a
subprocess:

    GOL_LIB=tests/fake_hip/libgolhip_fakehip.so python tests/density_cpu_check.py
    GOL_LIB=... GOL_RCCL_SHIM=tests/fake_hip/libfake_rccl_host.so python tests/density_cpu_check.py
(the second form: two rank contexts over the RCCL host stand-in, whose maps add)
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
from density_ref import density_dims, density_ref  # noqa: E402

EINVAL, ESTATE = -1, -6
rng = np.random.default_rng(13)
U32P = ctypes.POINTER(ctypes.c_uint32)


def soup(rows, cols):
    return (rng.random((rows, cols)) < 0.4).astype(np.uint8)


def same(e, got, th, tw, what):
    d = e.density(th, tw)
    want = density_ref(got, th, tw)
    assert d.dtype == np.uint32 and d.shape == want.shape and (d == want).all(), (what, th, tw, d, want)
    assert int(d.sum()) == int(got.sum())


def boards():
    n = 0
    for rows, cols, kw in ((64, 200, dict()),                                  # 1 slab
                           (64, 200, dict(n_gpus=3, tblock_k=2)),              # seams at rows 22 and 43
                           (64, 64, dict(boundary="torus", tblock_k=3)),       # ghost margin of 3 columns
                           (40, 131, dict(boundary="torus", tblock_k=16, n_gpus=2)),
                           (48, 48, dict(boundary="mesh_compat", mesh_m=4)),   # 12-column blocks: a tile spans 3 runs
                           (37, 37, dict(boundary="serial_compat"))):
        b = soup(rows, cols)
        if kw.get("boundary") == "torus":
            b[:, :2] = 1
            b[:, -2:] = 1
        with gh.Engine(rows, cols, layout="byte", **kw) as e:
            assert not e.density(7, 32).any()   # the empty board
            e.upload(b)
            got = e.download()
            if kw.get("boundary") == "serial_compat":
                assert not got[-1].any() and not got[:, -1].any()
            else:
                assert (got == b).all()
            for th, tw in ((7, 32), (1, 32), (3, 64), (64, 96), (1000, 4096), (5, 160)):
                same(e, got, th, tw, (rows, cols, kw))
            # offset windows: row0 anything, col0 a multiple of 32, ending mid-tile
            for _ in range(12):
                r0 = int(rng.integers(0, rows))
                c0 = 32 * int(rng.integers(0, (cols - 1) // 32 + 1))
                nr, nc = int(rng.integers(1, rows - r0 + 1)), int(rng.integers(1, cols - c0 + 1))
                th, tw = int(rng.integers(1, 12)), 32 * int(rng.integers(1, 4))
                d = e.density_window(r0, c0, nr, nc, th, tw)
                assert (d == density_ref(got[r0:r0 + nr, c0:c0 + nc], th, tw)).all(), (rows, cols, kw, r0, c0, nr, nc)
            n += 1
    return n


def leading_dimension():
    b = soup(30, 100)
    with gh.Engine(30, 100, layout="byte", n_gpus=2) as e:
        e.upload(b)
        out = np.full((5, 9), 77, np.uint32)   # 5 x 4 tiles in rows of 9
        e._chk(e.lib.gol_density(e._c, 7, 32, out.ctypes.data_as(U32P), 9), "gol_density")
        assert (out[:, :4] == density_ref(b, 7, 32)).all() and (out[:, 4:] == 77).all()


def arguments():
    L = gh.load()
    assert gh.density_dims(100, 200, 16, 32) == (7, 7) == density_dims(100, 200, 16, 32)
    assert gh.density_dims(0, 5, 3, 32) == (0, 1) and gh.density_dims(64, 64, 64, 64) == (1, 1)
    assert gh.density_dims(65, 65, 64, 64) == (2, 2)
    tr, tc = ctypes.c_int64(), ctypes.c_int64()
    assert L.gol_density_dims(1, 1, 1, 32, None, ctypes.byref(tc)) == EINVAL
    assert L.gol_density_dims(1, 1, 1, 32, ctypes.byref(tr), None) == EINVAL
    assert L.gol_density_dims(1, 1, 0, 32, ctypes.byref(tr), ctypes.byref(tc)) == EINVAL
    assert L.gol_density_dims(-1, 1, 1, 32, ctypes.byref(tr), ctypes.byref(tc)) == EINVAL
    d = (ctypes.c_uint32 * 64)()
    assert L.gol_density(None, 4, 32, d, 8) == EINVAL and L.gol_density_async(None, 4, 32, d, 8) == EINVAL
    assert L.gol_density_window(None, 0, 0, 1, 1, 4, 32, d, 8) == EINVAL
    b = soup(20, 100)
    with gh.Engine(20, 100, layout="byte") as e:
        e.upload(b)
        assert L.gol_density(e._c, 4, 32, None, 8) == EINVAL and L.gol_density_async(e._c, 4, 32, None, 8) == EINVAL
        assert L.gol_density_window(e._c, 0, 0, 1, 1, 4, 32, None, 8) == EINVAL
        for win in ((0, 0, 21, 100), (0, 0, 20, 101), (-1, 0, 1, 1), (0, -32, 1, 1), (5, 32, -1, 1), (19, 96, 2, 1)):
            assert L.gol_density_window(e._c, *win, 4, 32, d, 8) == EINVAL, win
            assert b"outside the grid" in L.gol_last_error(e._c)
        for tiles, msg in (((0, 32), b"tile_rows"), ((-3, 32), b"tile_rows"), ((4, 0), b"multiple of 32"),
                           ((4, 31), b"multiple of 32"), ((4, 48), b"multiple of 32"), ((4, -32), b"multiple of 32"),
                           ((1 << 27, 32), b"2^32"), ((1 << 31, 1 << 31), b"2^32")):
            assert L.gol_density_window(e._c, 0, 0, 20, 100, *tiles, d, 8) == EINVAL, tiles
            assert msg in L.gol_last_error(e._c), (tiles, L.gol_last_error(e._c))
            assert L.gol_density(e._c, *tiles, d, 8) == EINVAL and L.gol_density_async(e._c, *tiles, d, 8) == EINVAL
        for c0 in (1, 31, 33, 48):
            assert L.gol_density_window(e._c, 0, c0, 1, 1, 4, 32, d, 8) == EINVAL
            assert b"col0" in L.gol_last_error(e._c)
        # 5 x 4 tiles: ld = 3 is too small
        assert L.gol_density(e._c, 4, 32, d, 3) == EINVAL and b"ld" in L.gol_last_error(e._c)
        assert L.gol_density_async(e._c, 4, 32, d, 3) == EINVAL
        assert L.gol_density_window(e._c, 0, 32, 20, 68, 4, 32, d, 2) == EINVAL
        # the largest legal tile, and an empty window: GOL_OK, nothing written
        assert (e.density((1 << 27) - 1, 32) == density_ref(b, 20, 32)).all()   # (one tile row either way)
        for i in range(64):
            d[i] = 99
        assert L.gol_density_window(e._c, 20, 96, 0, 0, 4, 32, d, 0) == 0
        assert L.gol_density_window(e._c, 3, 32, 0, 5, 4, 32, d, 1) == 0
        assert L.gol_density_window(e._c, 3, 32, 5, 0, 4, 32, d, 0) == 0
        assert all(v == 99 for v in d)
        # the context stays usable
        same(e, e.download(), 4, 32, "after the refused calls")


def pending():
    b = soup(64, 200)
    with gh.Engine(64, 200, layout="byte", n_gpus=3) as e:
        e.upload(b)
        outs = [(th, tw, e.density_async(th, tw)) for th, tw in ((7, 32), (7, 32), (1, 64), (64, 224), (3, 96))]
        assert not any(o.any() for _, _, o in outs)   # nothing is delivered before a synchronising call
        e.sync()
        for th, tw, o in outs:
            assert (o == density_ref(b, th, tw)).all(), (th, tw)
        o = e.density_async(7, 32)
        assert (e.download() == b).all()   # any synchronising call delivers
        assert (o == density_ref(b, 7, 32)).all()


def failed_call_leaves_nothing():
    """Two slabs; the stand-in fails the second launch, i.e. slab 1's, after slab 0's part is
    enqueued: the call fails (GOL_EHIP), the next sync writes nothing into the caller's block,
    and the parts' staging is free again afterwards."""
    EHIP = -2
    b = soup(64, 200)
    with gh.Engine(64, 200, layout="byte", n_gpus=2) as e:
        e.upload(b)
        before = e.density_async(7, 32)   # a pending map ahead of the failing call is still delivered
        e.lib.fake_hip_density_fail_at(2)
        out = np.full((10, 7), 0xABABABAB, np.uint32)
        rc = e.lib.gol_density_async(e._c, 7, 32, out.ctypes.data_as(U32P), 7)
        assert rc == EHIP, rc
        e.sync()
        assert (out == 0xABABABAB).all()
        assert (before == density_ref(b, 7, 32)).all()
        # the synchronising form fails alike and leaves nothing either
        e.lib.fake_hip_density_fail_at(2)
        rc = e.lib.gol_density(e._c, 7, 32, out.ctypes.data_as(U32P), 7)
        assert rc == EHIP, rc
        e.sync()
        assert (out == 0xABABABAB).all()
        same(e, b, 7, 32, "after the failed calls")


def ranks():
    rows, cols, world = 64, 200, 2
    b = soup(rows, cols)
    uid = gh.unique_id()
    out, errs = [None] * world, []

    def worker(r):
        try:
            with gh.Engine(rows, cols, rank=r, world=world, device=0, uid=uid, layout="byte") as e:
                e.upload(b)
                pend = e.density_async(7, 32)
                part = e.density(7, 32)
                assert (pend == part).all()
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
    assert (out[0] + out[1] == density_ref(b, 7, 32)).all()
    for r in range(world):
        row0, n = gh.slab_plan(rows, world, r)
        mine = np.zeros_like(b)
        mine[row0:row0 + n] = b[row0:row0 + n]
        assert (out[r] == density_ref(mine, 7, 32)).all(), r   # 0 in the tiles it holds nothing of
    print("density cpu ranks ok")


if __name__ == "__main__":
    if os.environ.get("GOL_RCCL_SHIM"):
        ranks()
    else:
        n = boards()
        leading_dimension()
        arguments()
        pending()
        failed_call_leaves_nothing()
        print(f"density cpu ok: {n} boards")
