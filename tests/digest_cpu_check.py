#!/usr/bin/env python3
"""The runtime's side of gol_digest* over the host-only HIP stand-in (no GPU):
tests/fake_hip/fake_hip_digest.cpp runs the row routine of gol_digest.h on the
stand-in's host "device" memory, and a byte-layout board's uploads and
downloads are plain copies there, so for byte boards (no stepping: the stencil
stand-ins do nothing) digest() must equal the reference digest of download():
slabs, MESH_COMPAT column runs, the torus ghost margin, SERIAL_COMPAT's dead
last row and column, windows, the pending ring and the argument checks.
Run by tests/test_digest_cpu.py in a subprocess:

    GOL_LIB=tests/fake_hip/libgolhip_fakehip.so python tests/digest_cpu_check.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from mpi_amd import golhip as gh  # noqa: E402
from digest_ref import add, digest_ref  # noqa: E402

EINVAL, ESTATE = -1, -6
rng = np.random.default_rng(11)


def soup(rows, cols):
    return (rng.random((rows, cols)) < 0.4).astype(np.uint8)


def boards():
    n = 0
    for rows, cols, kw in ((37, 131, dict()), (100, 300, dict(n_gpus=3, tblock_k=2)),
                           (64, 64, dict(boundary="torus", tblock_k=3)),
                           (40, 131, dict(boundary="torus", tblock_k=16, n_gpus=2)),
                           (48, 48, dict(boundary="mesh_compat", mesh_m=4)),
                           (37, 37, dict(boundary="serial_compat"))):
        b = soup(rows, cols)
        with gh.Engine(rows, cols, layout="byte", **kw) as e:
            e.upload(b)
            got = e.download()
            if kw.get("boundary") == "serial_compat":
                assert not got[-1].any() and not got[:, -1].any()
            else:
                assert (got == b).all()
            assert e.digest() == digest_ref(got), (rows, cols, kw)
            # windows: each equals the reference with its origin, and a tiling adds up
            for _ in range(10):
                r0, c0 = int(rng.integers(0, rows)), int(rng.integers(0, cols))
                nr, nc = int(rng.integers(0, rows - r0 + 1)), int(rng.integers(0, cols - c0 + 1))
                assert e.digest_window(r0, c0, nr, nc) == digest_ref(got[r0:r0 + nr, c0:c0 + nc], r0, c0)
            rc, cc = rows // 3, cols // 2 + 1
            tiles = [e.digest_window(0, 0, rc, cc), e.digest_window(0, cc, rc, cols - cc),
                     e.digest_window(rc, 0, rows - rc, cols)]
            assert add(*tiles) == e.digest()
            n += 1
    return n


def arguments():
    L = gh.load()
    d = (ctypes.c_uint64 * 2)()
    assert L.gol_digest(None, d) == EINVAL and L.gol_digest_async(None, d) == EINVAL
    assert L.gol_digest_window(None, 0, 0, 1, 1, d) == EINVAL
    with gh.Engine(20, 50, layout="byte") as e:
        assert L.gol_digest(e._c, None) == EINVAL and L.gol_digest_async(e._c, None) == EINVAL
        assert L.gol_digest_window(e._c, 0, 0, 1, 1, None) == EINVAL
        for win in ((0, 0, 21, 50), (0, 0, 20, 51), (-1, 0, 1, 1), (0, -1, 1, 1), (5, 5, -1, 1), (19, 49, 2, 1)):
            assert L.gol_digest_window(e._c, *win, d) == EINVAL, win
            assert b"outside the grid" in L.gol_last_error(e._c)
        assert e.digest_window(20, 50, 0, 0) == (0, 0)   # empty windows are (0, 0)
        assert e.digest() == (0, 0)


def pending_ring():
    b = soup(30, 70)
    with gh.Engine(30, 70, layout="byte", n_gpus=2) as e:
        e.upload(b)
        outs = [e.digest_async() for _ in range(1024)]
        try:
            e.digest_async()
        except gh.GolError as ex:
            assert ex.code == ESTATE and "sync first" in str(ex), ex
        else:
            raise SystemExit("pending digest 1025 was accepted")
        e.sync()   # the context stays usable: all 1024 delivered, and the ring is free again
        want = digest_ref(b)
        assert all((int(o[0]), int(o[1])) == want for o in outs)
        o = e.digest_async()
        assert e.digest() == want and (int(o[0]), int(o[1])) == want


if __name__ == "__main__":
    n = boards()
    arguments()
    pending_ring()
    print(f"digest cpu ok: {n} boards")
