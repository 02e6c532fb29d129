#!/usr/bin/env python3
"""The runtime's side of gol_format_rle / gol_rle_bytes / gol_write_rle / gol_parse_rle /
gol_read_rle over the host-only HIP stand-in (no GPU): tests/fake_hip/fake_hip_rle.cpp runs
the three passes of gol_rle.h on the stand-in's host "device" memory and
fake_hip_bits.cpp / fake_hip_fill.cpp the packed-row and fill launchers, so the blocks, the
slab pieces, the carries between them, the exact-size copies and the parser's row blocks
run on the CPU, against tests/rle_ref.py.  Boards are written with upload_bits and read
with download_bits_window (the stand-in computes those for every storage form).  Run by
tests/test_rle_cpu.py in a subprocess:

    GOL_LIB=tests/fake_hip/libgolhip_fakehip.so python tests/rle_cpu_check.py
    GOL_LIB=... GOL_RCCL_SHIM=tests/fake_hip/libfake_rccl_host.so python tests/rle_cpu_check.py
(the second form: two rank contexts over the RCCL host stand-in; a window with rows the
rank does not hold is refused)
"""
import ctypes
import os
import sys
import tempfile
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
if os.environ.get("GOL_RCCL_SHIM"):
    ctypes.CDLL(os.environ["GOL_LIB"], mode=ctypes.RTLD_GLOBAL)
    ctypes.CDLL(os.environ["GOL_RCCL_SHIM"], mode=ctypes.RTLD_GLOBAL)
import rle_ref  # noqa: E402
from mpi_amd import golhip as gh  # noqa: E402

EINVAL = -1
rng = np.random.default_rng(23)

KINDS = (dict(layout="bit", tblock_k=1), dict(layout="bit", tblock_k=8), dict(layout="byte", tblock_k=1),
         dict(layout="bit", tblock_k=8, boundary="torus"), dict(layout="bit", boundary="mesh_compat", mesh_m=2),
         dict(layout="byte", tblock_k=2, n_gpus=3))


def shape(kw):
    return (64, 64) if kw.get("boundary") == "mesh_compat" else (64, 200)


def put(e, b):
    e.upload_bits(np.packbits(b, axis=1))


def cells(e, win=None):
    r0, c0, nr, nc = win or (0, 0, e.rows, e.cols)
    return np.unpackbits(e.download_bits_window(r0, c0, nr, nc), axis=1)[:, :nc]


def gappy(rows, cols):
    """Empty-row gaps of 1, 2, 10 and 11 rows, which straddle one-row blocks and the seams of 3 slabs."""
    b = np.zeros((rows, cols), np.uint8)
    r = 0
    for gap in (1, 2, 10, 11, 1, 2, 10, 11):
        r += gap
        if r >= rows:
            break
        b[r] = rng.random(cols) < 0.3
        b[r, int(rng.integers(0, cols))] = 1
        r += 1
    return b


def check_format(e, b, windows):
    n = 0
    for win in windows:
        r0, c0, nr, nc = win
        want = rle_ref.encode(cells(e, win), *e.rule)
        assert (cells(e, win) == b[r0:r0 + nr, c0:c0 + nc]).all()
        got = e.format_rle(win)
        assert got == want, (win, got[:200], want[:200])
        assert e.rle_bytes(win) == len(want)
        # a buffer one byte short: GOL_EINVAL and the bytes needed
        buf, need = ctypes.create_string_buffer(len(want)), ctypes.c_int64()
        rc = e.lib.gol_format_rle(e._c, *win, buf, len(want) - 1, ctypes.byref(need))
        assert rc == EINVAL and need.value == len(want), (rc, need.value, len(want))
        rc = e.lib.gol_format_rle(e._c, *win, buf, len(want), ctypes.byref(need))
        assert rc == 0 and need.value == len(want) and buf.raw == want
        n += 1
    return n


def formats():
    n = 0
    for block in (None, 1):
        for kw in KINDS:
            rows, cols = shape(kw)
            for b in ((rng.random((rows, cols)) < 0.4).astype(np.uint8), gappy(rows, cols)):
                with gh.Engine(rows, cols, **kw) as e:
                    if block:
                        e.set_option(gh.OPT_TEXT_BLOCK_BYTES, block)
                    put(e, b)
                    wins = [(0, 0, rows, cols), (3, 1, 60, cols - 3), (0, 0, 1, 1), (5, 37 % cols, 9, min(96, cols - 37 % cols)),
                            (20, 0, 44, cols), (7, 5, 0, 9), (7, 5, 9, 0)]
                    n += check_format(e, b, wins)
                    with tempfile.TemporaryDirectory() as d:
                        path = os.path.join(d, "w.rle")
                        e.save_rle(path, wins[1])
                        assert open(path, "rb").read() == e.format_rle(wins[1])
    # an empty board and an empty window
    with gh.Engine(40, 70, layout="bit") as e:
        assert e.format_rle() == b"x = 70, y = 40, rule = B3/S23\n!\n" == rle_ref.encode(np.zeros((40, 70), np.uint8))
        assert e.format_rle((3, 3, 0, 5)) == b"x = 5, y = 0, rule = B3/S23\n!\n"
        assert e.generation == 0
    return n


def round_trips():
    """Text formatted by one kind, parsed into a context of the next kind that was filled with ones:
    the box is replaced, nothing else changes; from memory and from a file read in chunks."""
    for i, kw in enumerate(KINDS):
        kw2 = KINDS[(i + 1) % len(KINDS)]
        rows, cols = shape(kw)
        rows2, cols2 = shape(kw2)
        for block in (None, 1):
            b = gappy(rows, cols) if block else (rng.random((rows, cols)) < 0.4).astype(np.uint8)
            win = (3, 1, 50, min(cols, cols2) - 9)
            with gh.Engine(rows, cols, **kw) as e, gh.Engine(rows2, cols2, **kw2) as e2:
                if block:
                    e2.set_option(gh.OPT_TEXT_BLOCK_BYTES, block)
                put(e, b)
                text = e.format_rle(win)
                ones = np.ones((rows2, cols2), np.uint8)
                put(e2, ones)
                assert e2.parse_rle(text, at=(7, 5)) == (win[3], win[2])
                want = ones.copy()
                want[7:7 + win[2], 5:5 + win[3]] = b[3:53, 1:1 + win[3]]
                assert (cells(e2) == want).all(), (kw, kw2, block)
                put(e2, ones)
                with tempfile.TemporaryDirectory() as d:
                    path = os.path.join(d, "p.rle")
                    with open(path, "wb") as f:
                        f.write(b"#C a comment\n#CXRLE Pos=1,3\n" + text + b"anything behind the pattern")
                    assert e2.load_rle(path, at=(7, 5)) == (win[3], win[2])
                assert (cells(e2) == want).all(), (kw, kw2, block)
                assert e2.rule == rle_ref.LIFE and e2.generation == 0


def reading_accepts():
    with gh.Engine(20, 40, layout="byte") as e:
        put(e, np.ones((20, 40), np.uint8))
        assert e.parse_rle(b"x=3,y=3\n b o $ \r\n 2b o $ \t 3o ! junk 0x", at=(2, 4)) == (3, 3)
        want = np.ones((20, 40), np.uint8)
        want[2:5, 4:7] = [[0, 1, 0], [0, 0, 1], [1, 1, 1]]
        assert (cells(e) == want).all()
        for rule in (b"b3/s23", b"23/3", b"B36/S23"):
            assert e.parse_rle(b"x = 1, y = 1, rule = " + rule + b"\no!") == (1, 1)
        assert e.rule == rle_ref.LIFE   # the header's rule is not set
        # x = 0 or y = 0: GOL_OK, nothing written, no body needed
        before = cells(e)
        assert e.parse_rle(b"x = 0, y = 5\n") == (0, 5) and e.parse_rle(b"x = 5, y = 0\n3o!") == (5, 0)
        assert (cells(e) == before).all()
        assert gh.rle_header(b"#C x\nx = 36, y = 9, rule = B36/S23\n24bo!") == (36, 9, (0x48, 0xC), 35)
        assert gh.rle_header("x=3,y=2") == (3, 2, None, 7)


def errors():
    """Every refusal with its byte offset, against the reference decoder's."""
    L = gh.load()
    head = b"x = 5, y = 3\n"
    bad = [b"3o$.o!", b"3o$Ao!", b"3o$2Xo!", b"3o$0o!", b"3o$00b!", b"3o$2147483649b!", b"3o$99999999999b!", b"6o!",
           b"3o$3b3o!", b"3o$$$o!", b"3o4$!", b"3o$2o", b"3o$2", b"", b"3o$2 o!", b"3o$2\no!", b"3o$3!", b"3o\x00!", b"3o$\xffo!"]
    with gh.Engine(20, 40, layout="byte") as e:
        put(e, np.ones((20, 40), np.uint8))
        for body in bad:
            text = head + body
            try:
                rle_ref.decode(text)
                raise AssertionError(f"the reference accepts {text!r}")
            except rle_ref.RleError as ex:
                off = ex.offset
            x, y = ctypes.c_int64(), ctypes.c_int64()
            rc = L.gol_parse_rle(e._c, 1, 1, text, len(text), ctypes.byref(x), ctypes.byref(y))
            msg = L.gol_last_error(e._c).decode()
            assert rc == EINVAL and f"at byte {off}:" in msg, (text, off, rc, msg)
        for text, off in ((b"x = 5, z = 3\no!", 7), (b"y = 5\no!", 0), (b"#C only a comment", 17), (b"x = 5, y = 3, rule = B9/S2\no!", 21),
                          (b"x = 5, y = 3, rule = \no!", 21), (b"x = 5, y = 3, bogus\no!", 14)):
            rc = L.gol_parse_rle(e._c, 1, 1, text, len(text), None, None)
            msg = L.gol_last_error(e._c).decode()
            assert rc == EINVAL and f"at byte {off}" in msg, (text, off, rc, msg)
            assert L.gol_rle_header(text, len(text), None, None, None, None, None, None) == EINVAL
        # a box that leaves the grid: refused before anything is written
        put(e, np.ones((20, 40), np.uint8))
        for at in ((18, 0), (0, 36), (-1, 0), (0, -1)):
            rc = L.gol_parse_rle(e._c, at[0], at[1], head + b"5o$5o$5o!", 22, None, None)
            assert rc == EINVAL and b"leaves the grid" in L.gol_last_error(e._c), at
        assert cells(e).all()
        assert e.parse_rle(head + b"5o$5o$5o!", at=(17, 35)) == (5, 3)
        # windows outside the grid
        n = ctypes.c_int64()
        for win in ((0, 0, 21, 40), (0, 0, 20, 41), (-1, 0, 1, 1), (5, 39, 1, 2), (0, 0, -1, 1)):
            assert L.gol_rle_bytes(e._c, *win, ctypes.byref(n)) == EINVAL and b"outside the grid" in L.gol_last_error(e._c)
            assert L.gol_format_rle(e._c, *win, None, 0, ctypes.byref(n)) == EINVAL
            assert L.gol_write_rle(e._c, *win, 1) == EINVAL
        # null contexts and pointers
        buf = ctypes.create_string_buffer(64)
        assert L.gol_rle_bytes(None, 0, 0, 1, 1, ctypes.byref(n)) == EINVAL and L.gol_rle_bytes(e._c, 0, 0, 1, 1, None) == EINVAL
        assert L.gol_format_rle(None, 0, 0, 1, 1, buf, 64, ctypes.byref(n)) == EINVAL
        assert L.gol_format_rle(e._c, 0, 0, 1, 1, buf, 64, None) == EINVAL
        assert L.gol_write_rle(None, 0, 0, 1, 1, 1) == EINVAL and L.gol_write_rle(e._c, 0, 0, 1, 1, -1) == EINVAL
        assert L.gol_parse_rle(None, 0, 0, b"x", 1, None, None) == EINVAL and L.gol_parse_rle(e._c, 0, 0, None, 0, None, None) == EINVAL
        assert L.gol_read_rle(None, 0, 0, 0, None, None) == EINVAL and L.gol_read_rle(e._c, 0, 0, -1, None, None) == EINVAL
        assert L.gol_rle_header(None, 0, None, None, None, None, None, None) == EINVAL
        # a malformed body may leave the box partly written; the context stays usable
        assert e.format_rle((0, 0, 1, 1)) == b"x = 1, y = 1, rule = B3/S23\no!\n"


def ranks():
    rows, cols, world = 64, 200, 2
    b = (rng.random((rows, cols)) < 0.4).astype(np.uint8)
    uid = gh.unique_id()
    errs = []

    def worker(r):
        try:
            with gh.Engine(rows, cols, rank=r, world=world, device=0, uid=uid, layout="byte") as e:
                row0, n = gh.slab_plan(rows, world, r)
                e.upload_bits(np.packbits(b, axis=1))
                mine = (row0, 3, n, 150)
                assert e.format_rle(mine) == rle_ref.encode(b[row0:row0 + n, 3:153])
                cnt = ctypes.c_int64()
                for win in ((0, 0, rows, cols), (row0 - 1 if r else row0 + n - 3, 0, 4, cols)):
                    assert e.lib.gol_rle_bytes(e._c, *win, ctypes.byref(cnt)) == EINVAL
                    assert b"not all held" in e.lib.gol_last_error(e._c)
                text = rle_ref.encode(b[:4])
                at = row0 - 1 if r else row0 + n - 3
                rc = e.lib.gol_parse_rle(e._c, at, 0, text, len(text), None, None)
                assert rc == EINVAL and b"not all held" in e.lib.gol_last_error(e._c)
                assert e.parse_rle(text, at=(row0 + 2, 0)) == (cols, 4)
                assert (cells(e, (row0 + 2, 0, 4, cols)) == b[:4]).all()
        except Exception as ex:   # noqa: BLE001
            errs.append((r, repr(ex)))

    ts = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=60)
    if errs or any(t.is_alive() for t in ts):
        raise SystemExit(f"rank threads failed or hung: {errs}")
    print("rle cpu ranks ok")


if __name__ == "__main__":
    if os.environ.get("GOL_RCCL_SHIM"):
        ranks()
    else:
        n = formats()
        round_trips()
        reading_accepts()
        errors()
        print(f"rle cpu ok: {n} windows")
