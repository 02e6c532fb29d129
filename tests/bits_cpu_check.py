#!/usr/bin/env python3
"""The runtime's side of gol_download_bits* / gol_upload_bits* over the host-only
HIP stand-in (no GPU): tests/fake_hip/fake_hip_bits.cpp runs the row routines of
gol_bits.h on the stand-in's host "device" memory, and a byte-layout board's byte
uploads and downloads are plain copies there, so for byte boards the packed calls
must agree with np.packbits of the byte calls: slabs with seams, windows at any
column, the torus ghost margin, MESH_COMPAT column runs that share packed bytes,
SERIAL_COMPAT's dead last row and column, a leading dimension above the row's
bytes, pad bits, pending async windows across later steps, the argument rules and
a failed call that must leave no pending write.  Run by tests/test_bits_cpu.py in
a subprocess:

    GOL_LIB=tests/fake_hip/libgolhip_fakehip.so python tests/bits_cpu_check.py
    GOL_LIB=... GOL_RCCL_SHIM=tests/fake_hip/libfake_rccl_host.so python tests/bits_cpu_check.py
(the second form: two rank contexts over the RCCL host stand-in, whose parts tile the board)
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

EINVAL, EHIP = -1, -2
rng = np.random.default_rng(17)
U8P = ctypes.POINTER(ctypes.c_uint8)


def soup(rows, cols):
    return (rng.random((rows, cols)) < 0.4).astype(np.uint8)


def p8(a):
    return a.ctypes.data_as(U8P)


def pack(b):
    return np.packbits(b, axis=1)


def boards():
    n = 0
    for rows, cols, kw in ((64, 200, dict()),                                  # 1 slab
                           (64, 200, dict(n_gpus=3, tblock_k=2)),              # seams at rows 22 and 43
                           (37, 131, dict(n_gpus=2)),                          # 5 pad bits
                           (64, 64, dict(boundary="torus", tblock_k=3)),       # ghost margin of 3 columns
                           (40, 131, dict(boundary="torus", tblock_k=16, n_gpus=2)),
                           (48, 48, dict(boundary="mesh_compat", mesh_m=4)),   # 12-column runs share packed bytes
                           (37, 37, dict(boundary="serial_compat"))):
        b = soup(rows, cols)
        if kw.get("boundary") == "torus":
            b[:, :2] = 1
            b[:, -2:] = 1
        serial = kw.get("boundary") == "serial_compat"
        with gh.Engine(rows, cols, layout="byte", **kw) as e, gh.Engine(rows, cols, layout="byte", **kw) as e2:
            assert not e.download_bits().any()   # the empty board
            e.upload(b)
            got = e.download()
            if serial:
                assert not got[-1].any() and not got[:, -1].any()
            else:
                assert (got == b).all()
            bits = e.download_bits()
            assert bits.dtype == np.uint8 and bits.shape == (rows, gh.bits_row_bytes(cols))
            assert (bits == pack(got)).all(), (rows, cols, kw)
            # the round trip, with every pad bit set: ignored on upload, 0 on download
            dirty = pack(b)
            if cols % 8:
                dirty[:, -1] |= (1 << (8 - cols % 8)) - 1
            e2.upload_bits(dirty)
            assert (e2.download() == got).all(), (rows, cols, kw)
            assert (e2.download_bits() == bits).all()
            # windows at any column; a window upload changes exactly the window's cells
            cur2 = got.copy()   # e2's board
            for _ in range(24):
                r0, c0 = int(rng.integers(0, rows)), int(rng.integers(0, cols))
                nr, nc = int(rng.integers(1, rows - r0 + 1)), int(rng.integers(1, cols - c0 + 1))
                w = e.download_bits_window(r0, c0, nr, nc)
                assert (w == pack(got[r0:r0 + nr, c0:c0 + nc])).all(), (rows, cols, kw, r0, c0, nr, nc)
                fresh = soup(nr, nc)
                pw = pack(fresh)
                if nc % 8:
                    pw[:, -1] |= (1 << (8 - nc % 8)) - 1   # pad bits: ignored
                e2.upload_bits_window(r0, c0, nc, pw)
                cur2[r0:r0 + nr, c0:c0 + nc] = fresh
                if serial:
                    cur2[-1] = 0
                    cur2[:, -1] = 0
                assert (e2.download() == cur2).all(), (rows, cols, kw, r0, c0, nr, nc)
            assert (e2.download_bits() == pack(cur2)).all()
            n += 1
    return n


def serial_all_ones():
    with gh.Engine(37, 37, layout="byte", boundary="serial_compat") as e:
        e.upload_bits(np.full((37, 5), 0xFF, np.uint8))
        got = e.download()
        assert got[:-1, :-1].all() and not got[-1].any() and not got[:, -1].any()
        assert (e.download_bits() == pack(got)).all()


def leading_dimension():
    b = soup(30, 100)   # 13 bytes per row, 4 pad bits
    with gh.Engine(30, 100, layout="byte", n_gpus=2) as e:
        e.upload(b)
        out = np.full((30, 20), 0xA5, np.uint8)
        e._chk(e.lib.gol_download_bits(e._c, p8(out), 20), "gol_download_bits")
        assert (out[:, :13] == pack(b)).all() and (out[:, 13:] == 0xA5).all()
        assert not (out[:, 12] & 0x0F).any()   # pad bits are written as 0
        out = np.full((7, 20), 0xA5, np.uint8)
        e._chk(e.lib.gol_download_bits_window(e._c, 11, 3, 7, 70, p8(out), 20), "gol_download_bits_window")
        assert (out[:, :9] == pack(b[11:18, 3:73])).all() and (out[:, 9:] == 0xA5).all()
        # upload from rows of 20 bytes whose tails are junk
        src = np.full((30, 20), 0xFF, np.uint8)
        b2 = soup(30, 100)
        src[:, :13] = pack(b2) | np.array([0] * 12 + [0x0F], np.uint8)
        e._chk(e.lib.gol_upload_bits(e._c, p8(src), 20), "gol_upload_bits")
        assert (e.download() == b2).all()


def arguments():
    L = gh.load()
    assert [gh.bits_row_bytes(n) for n in (0, 1, 7, 8, 9, 131072)] == [0, 1, 1, 1, 2, 16384]
    assert L.gol_bits_row_bytes(-1) == EINVAL
    buf = np.full((64, 32), 0x5A, np.uint8)
    for call in (L.gol_download_bits, L.gol_upload_bits):
        assert call(None, p8(buf), 32) == EINVAL
    for call in (L.gol_download_bits_window, L.gol_download_bits_window_async, L.gol_upload_bits_window):
        assert call(None, 0, 0, 1, 1, p8(buf), 32) == EINVAL
    b = soup(20, 100)
    with gh.Engine(20, 100, layout="byte") as e:
        e.upload(b)
        wins = (L.gol_download_bits_window, L.gol_download_bits_window_async, L.gol_upload_bits_window)
        for call in wins:
            for win in ((0, 0, 21, 100), (0, 0, 20, 101), (-1, 0, 1, 1), (0, -1, 1, 1), (5, 32, -1, 1), (19, 96, 2, 1),
                        (0, 99, 1, 2)):
                assert call(e._c, *win, p8(buf), 32) == EINVAL, win
                assert b"outside the grid" in L.gol_last_error(e._c)
            assert call(e._c, 0, 0, 20, 100, p8(buf), 12) == EINVAL and b"ld" in L.gol_last_error(e._c)
            assert call(e._c, 0, 3, 20, 9, p8(buf), 1) == EINVAL and b"ld" in L.gol_last_error(e._c)
            assert call(e._c, 0, 0, 20, 100, None, 32) == EINVAL and b"null" in L.gol_last_error(e._c)
            # an empty window: GOL_OK, nothing written (or read)
            assert call(e._c, 20, 100, 0, 0, p8(buf), 0) == 0
            assert call(e._c, 3, 32, 0, 5, p8(buf), 1) == 0
            assert call(e._c, 3, 32, 5, 0, None, 0) == 0
        for call in (L.gol_download_bits, L.gol_upload_bits):
            assert call(e._c, p8(buf), 12) == EINVAL and b"ld" in L.gol_last_error(e._c)
            assert call(e._c, None, 32) == EINVAL and b"null" in L.gol_last_error(e._c)
        e.sync()
        assert (buf == 0x5A).all()
        # the context stays usable, and the refused uploads changed nothing
        assert (e.download_bits() == pack(b)).all()


def pending():
    b = soup(64, 200)
    with gh.Engine(64, 200, layout="byte", n_gpus=3, tblock_k=2) as e:
        e.upload(b)
        outs = [(w, e.download_bits_window_async(*w)) for w in ((0, 0, 64, 200), (0, 0, 64, 200), (5, 33, 40, 131),
                                                                 (63, 199, 1, 1), (20, 7, 30, 9))]
        assert not any(o.any() for _, o in outs)   # nothing is delivered before a synchronising call
        e.step(4)                                  # later steps do not disturb what is pending
        late = e.download_bits_window_async(0, 0, 64, 200)
        e.step(2)
        assert not any(o.any() for _, o in outs)
        e.sync()
        for (r0, c0, nr, nc), o in outs:
            assert (o == pack(b[r0:r0 + nr, c0:c0 + nc])).all(), (r0, c0, nr, nc)
        assert late.shape == (64, 25)
        o = e.download_bits_window_async(1, 1, 3, 3)
        cur = e.download()   # any synchronising call delivers
        assert (o == pack(cur[1:4, 1:4])).all()


def failed_call_leaves_nothing():
    """Two slabs; the stand-in fails the second launch, i.e. slab 1's, after slab 0's part is
    enqueued: the call fails (GOL_EHIP), the next sync writes nothing into the caller's rows,
    and the staging is free again afterwards."""
    b = soup(64, 200)
    with gh.Engine(64, 200, layout="byte", n_gpus=2) as e:
        e.upload(b)
        before = e.download_bits_window_async(0, 0, 64, 200)   # pending ahead of the failing call: delivered
        e.lib.fake_hip_bits_fail_at(2)
        out = np.full((64, 25), 0xAB, np.uint8)
        rc = e.lib.gol_download_bits_window_async(e._c, 0, 0, 64, 200, p8(out), 25)
        assert rc == EHIP, rc
        e.sync()
        assert (out == 0xAB).all()
        assert (before == pack(b)).all()
        # the synchronising form: slab 0's rows are delivered, the failing slab's are not
        e.lib.fake_hip_bits_fail_at(2)
        rc = e.lib.gol_download_bits(e._c, p8(out), 25)
        assert rc == EHIP, rc
        e.sync()
        assert (out[32:] == 0xAB).all()
        # a failing upload reports the error; the context stays usable
        e.lib.fake_hip_bits_fail_at(1)
        assert e.lib.gol_upload_bits(e._c, p8(pack(b)), 25) == EHIP
        e.upload_bits(pack(b))
        assert (e.download_bits() == pack(b)).all() and (e.download() == b).all()


def ranks():
    rows, cols, world = 64, 200, 2
    b = soup(rows, cols)
    uid = gh.unique_id()
    out, errs = [None] * world, []

    def worker(r):
        try:
            with gh.Engine(rows, cols, rank=r, world=world, device=0, uid=uid, layout="byte") as e:
                row0, n = gh.slab_plan(rows, world, r)
                e.upload_bits(pack(b))           # a rank takes its own rows of the whole board's buffer
                assert (e.download()[row0:row0 + n] == b[row0:row0 + n]).all()
                out[r] = e.download_bits()       # ... and fills its own rows only
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
        mine = np.zeros_like(b)
        mine[row0:row0 + n] = b[row0:row0 + n]
        assert (out[r] == pack(mine)).all(), r   # untouched (0) outside its slab
    assert ((out[0] | out[1]) == pack(b)).all()
    print("bits cpu ranks ok")


if __name__ == "__main__":
    if os.environ.get("GOL_RCCL_SHIM"):
        ranks()
    else:
        n = boards()
        serial_all_ones()
        leading_dimension()
        arguments()
        pending()
        failed_call_leaves_nothing()
        print(f"bits cpu ok: {n} boards")
