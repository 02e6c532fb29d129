"""gol_download_bits* / gol_upload_bits* on the GPU.  The master property: in every
state of every context download_bits() equals np.packbits(download(), axis=1), and
upload_bits of those rows into a second context of the same kind gives a board
whose download() is the same — every layout and group width, partial words and
units, the seam between two wave items at a column shift, windows at any column,
the torus ghost margin, MESH_COMPAT's reversed column blocks (runs that share
packed bytes), SERIAL_COMPAT's dead last row and column, pad bits, slabs, rank
contexts, pending async windows, and bin/gol --format pbm."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mpi_amd", "bin", "gol")
SHIM = os.path.join(ROOT, "tests", "shim", "libfake_rccl.so")

BIT_BYTE_K = [("bit", 1), ("bit", 3), ("bit", 7), ("bit", 8), ("bit", 16), ("byte", 1), ("byte", 16)]


@pytest.fixture(scope="module")
def gh():
    from mpi_amd import golhip
    golhip.load()
    return golhip


def soup(seed, rows, cols, p=0.4):
    return (np.random.default_rng(seed).random((rows, cols)) < p).astype(np.uint8)


def pack(b):
    return np.packbits(b, axis=1)


def dirty(bits, ncols):
    """The packed rows with every pad bit set."""
    out = bits.copy()
    if ncols % 8:
        out[:, -1] |= (1 << (8 - ncols % 8)) - 1
    return out


def first_diff(a, b):
    bad = np.argwhere(a != b)
    return f"{len(bad)} differ, first at {bad[0]}: {a[tuple(bad[0])]} want {b[tuple(bad[0])]}"


def master(e, e2, what):
    """download_bits == packbits(download); upload_bits of it into e2 (whatever e2 held) gives the board."""
    got, bits = e.download(), e.download_bits()
    assert bits.dtype == np.uint8 and bits.shape == (e.rows, (e.cols + 7) // 8), (what, bits.shape)
    assert (bits == pack(got)).all(), f"{what} download_bits: {first_diff(bits, pack(got))}"
    e2.upload_bits(dirty(bits, e.cols))
    back = e2.download()
    assert (back == got).all(), f"{what} upload_bits: {first_diff(back, got)}"
    return got


def block_steps(k):
    return [k, max(1, k - 3), 1, k]   # both ping-pong buffers and a short block are read


# ------------------------------------------------------------------ layouts and shapes
@pytest.mark.parametrize("layout,k", BIT_BYTE_K)
def test_layouts_shapes_and_depths(gh, layout, k):
    for rows, cols in ((37, 131), (8, 8), (64, 257), (100, 4096)):
        kw = dict(layout=layout, tblock_k=k)
        with gh.Engine(rows, cols, **kw) as e, gh.Engine(rows, cols, **kw) as e2:
            e2.upload(soup(1, rows, cols))
            assert not master(e, e2, (layout, k, rows, cols, "empty")).any()   # the empty board, over a soup
            e.upload(soup(rows + cols, rows, cols))
            assert master(e, e2, (layout, k, rows, cols, 0)).any()
            for s in block_steps(k):
                e.step(s)
                master(e, e2, (layout, k, rows, cols, e.generation))


def test_known_bytes(gh):
    b = np.zeros((3, 19), np.uint8)
    b[0, 0] = b[0, 7] = b[1, 8] = b[2, 18] = 1
    want = np.array([[0x81, 0, 0], [0, 0x80, 0], [0, 0, 0x20]], np.uint8)
    for layout, k in (("bit", 1), ("bit", 8), ("byte", 1)):
        with gh.Engine(3, 19, layout=layout, tblock_k=k) as e:
            e.upload(b)
            assert (e.download_bits() == want).all(), (layout, k)
            e.upload_bits(want[::-1].copy())
            assert (e.download() == b[::-1]).all(), (layout, k)


# ------------------------------------------------------------------ the seam between two wave items
@pytest.mark.parametrize("layout,k,cols", [("bit", 1, 8300), ("bit", 8, 8300), ("byte", 1, 2100)])
def test_wave_item_seam(gh, layout, k, cols):
    """More than 64 units in a row: the carry of lane 63 belongs to the next item's lane 0
    (storage columns 8192 resp. 2048), at shifts 0, 1 and 33 - 32."""
    kw = dict(layout=layout, tblock_k=k)
    b = soup(cols, 3, cols, 0.5)
    with gh.Engine(3, cols, **kw) as e, gh.Engine(3, cols, **kw) as e2:
        e.upload(b)
        master(e, e2, (layout, k, cols))
        for col0 in (1, 33):
            n = cols - col0
            w = e.download_bits_window(0, col0, 3, n)
            assert (w == pack(b[:, col0:])).all(), (layout, col0, first_diff(w, pack(b[:, col0:])))
            fresh = soup(col0, 3, n, 0.5)
            e2.upload_bits_window(0, col0, n, dirty(pack(fresh), n))
            want = b.copy()
            want[:, col0:] = fresh
            got = e2.download()
            assert (got == want).all(), (layout, col0, first_diff(got, want))
            e2.upload(b)


# ------------------------------------------------------------------ windows
@pytest.mark.parametrize("layout,k", [("bit", 1), ("bit", 8), ("byte", 1)])
def test_windows(gh, layout, k):
    rows, cols = 40, 260
    b = soup(5, rows, cols)
    with gh.Engine(rows, cols, layout=layout, tblock_k=k) as e:
        e.upload(b)
        e.step(k)
        got = e.download()
        for col0 in (0, 1, 7, 31, 32, 33, 95):
            for ncols in (1, 7, 8, 9, 31, 32, 33, 64, 65, 100):
                for row0, nrows in ((0, rows), (13, 5)):
                    w = e.download_bits_window(row0, col0, nrows, ncols)
                    want = pack(got[row0:row0 + nrows, col0:col0 + ncols])
                    assert w.shape == want.shape and (w == want).all(), (layout, row0, col0, nrows, ncols)


@pytest.mark.parametrize("layout,k,boundary", [("bit", 1, "dead"), ("bit", 8, "dead"), ("byte", 1, "dead"),
                                               ("bit", 8, "torus"), ("byte", 3, "torus")])
def test_window_upload_changes_exactly_the_window(gh, layout, k, boundary):
    rows, cols = 40, 260
    cur = soup(6, rows, cols)
    with gh.Engine(rows, cols, layout=layout, boundary=boundary, tblock_k=k) as e:
        e.upload(cur)
        n = 0
        for col0 in (0, 1, 7, 31, 32, 33, 95):
            for ncols in (1, 7, 8, 9, 31, 32, 33, 64, 65, 100):
                row0, nrows = ((0, rows), (13, 5), (39, 1))[n % 3]
                n += 1
                fresh = soup(n, nrows, ncols, 0.5)
                e.upload_bits_window(row0, col0, ncols, dirty(pack(fresh), ncols))
                cur[row0:row0 + nrows, col0:col0 + ncols] = fresh
                got = e.download()
                assert (got == cur).all(), (layout, row0, col0, nrows, ncols, first_diff(got, cur))
        assert (e.download_bits() == pack(cur)).all()


# ------------------------------------------------------------------ boundaries
@pytest.mark.parametrize("layout,k", [("bit", 3), ("bit", 8), ("bit", 16), ("bit", 32), ("byte", 16)])
def test_torus_ghosts_are_not_exported_and_are_refreshed(gh, layout, k):
    for rows, cols in ((64, 64), (40, 131)):
        kw = dict(layout=layout, boundary="torus", tblock_k=k)
        # live cells in the first and last two columns: their copies sit in the ghost margins
        b = soup(k, rows, cols)
        b[:, :2] = 1
        b[:, -2:] = 1
        with gh.Engine(rows, cols, **kw) as e, gh.Engine(rows, cols, **kw) as twin:
            e.upload(b)
            assert (e.download_bits() == pack(b)).all(), (layout, k, rows, cols)
            # the packed upload over a full board: stale ghosts would feed the next step
            twin.upload(np.ones((rows, cols), np.uint8))
            twin.upload_bits(dirty(pack(b), cols))
            for s in (k, 1):
                e.step(s)
                twin.step(s)
                got, want = twin.download(), e.download()
                assert (got == want).all(), (layout, k, rows, cols, first_diff(got, want))
                assert (twin.download_bits() == pack(want)).all()


@pytest.mark.parametrize("layout", ["bit", "byte"])
@pytest.mark.parametrize("m,n", [(4, 48), (2, 1024)])
def test_mesh_compat_rows_are_in_logical_columns(gh, layout, m, n):
    kw = dict(layout=layout, boundary="mesh_compat", mesh_m=m, tblock_k=2)
    with gh.Engine(n, n, **kw) as e, gh.Engine(n, n, **kw) as e2:
        e.upload(soup(m, n, n))
        master(e, e2, (layout, m, n, 0))
        e.step(3)
        got = master(e, e2, (layout, m, n, 3))
        # windows across block seams (n / m columns per block), at odd columns
        cur2 = got.copy()   # e2's board
        for col0, nc in ((5, n // m + 9), (n // m - 3, 7), (1, n - 2)):
            w = e.download_bits_window(5, col0, 20, nc)
            assert (w == pack(got[5:25, col0:col0 + nc])).all(), (layout, m, n, col0, nc)
            fresh = soup(col0, 20, nc)
            e2.upload_bits_window(5, col0, nc, dirty(pack(fresh), nc))
            cur2[5:25, col0:col0 + nc] = fresh
            back = e2.download()
            assert (back == cur2).all(), (layout, m, n, col0, nc, first_diff(back, cur2))


@pytest.mark.parametrize("layout", ["bit", "byte"])
def test_serial_compat_stores_a_dead_last_row_and_column(gh, layout):
    with gh.Engine(37, 37, layout=layout, boundary="serial_compat", tblock_k=2) as e:
        e.upload_bits(np.full((37, 5), 0xFF, np.uint8))
        got = e.download()
        assert got[:-1, :-1].all() and not got[-1].any() and not got[:, -1].any()
        assert (e.download_bits() == pack(got)).all() and e.popcount() == 36 * 36
        e.step(5)
        assert (e.download_bits() == pack(e.download())).all()


@pytest.mark.parametrize("layout,k", [("bit", 1), ("bit", 8), ("byte", 1), ("byte", 8)])
def test_pad_bits_do_not_leak_past_the_right_edge(gh, layout, k):
    from oracle import golcpu as g
    b = soup(k, 37, 131)
    b[:, -3:] = 1   # a busy right edge: a live pad column would change it
    with gh.Engine(37, 131, layout=layout, tblock_k=k) as e:
        e.upload_bits(dirty(pack(b), 131))
        e.step(2 * k)
        got, want = e.download(), g.run(b, 2 * k, g.DEAD)
        assert (got == want).all(), (layout, k, first_diff(got, want))
        bits = e.download_bits()
        assert (bits == pack(want)).all() and not (bits[:, -1] & 0x1F).any()


# ------------------------------------------------------------------ slabs and ranks
@pytest.mark.parametrize("layout,k", [("bit", 8), ("byte", 4)])
def test_three_slabs(gh, layout, k):
    b = soup(9, 64, 200)
    kw = dict(n_gpus=3, layout=layout, tblock_k=k)
    with gh.Engine(64, 200, **kw) as e, gh.Engine(64, 200, **kw) as e2, \
            gh.Engine(64, 200, layout=layout, tblock_k=k) as one:
        e.upload(b)
        one.upload(b)
        for s in block_steps(k):
            e.step(s)
            one.step(s)
            master(e, e2, (layout, k, e.generation))
        assert (e.download_bits() == one.download_bits()).all()
        w = e.download_bits_window(20, 3, 30, 150)   # across both seams
        assert (w == pack(one.download()[20:50, 3:153])).all()


def test_rank_parts_tile_the_board(gh):
    assert os.path.exists(SHIM), "build the shim first (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bits_rank_check.py"), SHIM],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "bits ranks ok" in r.stdout


# ------------------------------------------------------------------ async
@pytest.mark.parametrize("layout,k,slabs,boundary,rows", [("bit", 8, 1, "dead", 700), ("bit", 4, 3, "dead", 100),
                                                          ("byte", 16, 2, "torus", 90)])
def test_async_windows_between_steps(gh, layout, k, slabs, boundary, rows):
    cols = 300
    b = soup(21, rows, cols)
    kw = dict(n_gpus=slabs, layout=layout, boundary=boundary, tblock_k=k)
    with gh.Engine(rows, cols, **kw) as e, gh.Engine(rows, cols, **kw) as ref:
        e.upload(b)
        ref.upload(b)
        for _ in range(2):
            outs, wants = [], []
            for win in ((0, 0, rows, cols), (7, 33, rows - 9, 131)):   # two pending at once, 2k steps after each
                outs.append(e.download_bits_window_async(*win))
                cur = ref.download()
                wants.append(pack(cur[win[0]:win[0] + win[2], win[1]:win[1] + win[3]]))
                e.step(2 * k)
                ref.step(2 * k)
            assert not any(o.any() for o in outs)
            e.sync()      # one synchronising call delivers both: the boards of the enqueue generations
            for o, w in zip(outs, wants):
                assert o.shape == w.shape and (o == w).all() and w.any(), (layout, k, slabs)


# ------------------------------------------------------------------ errors
def test_errors_leave_the_context_usable(gh):
    b = soup(2, 20, 100)
    with gh.Engine(20, 100, layout="bit") as e:
        e.upload(b)
        for bad in ((0, 0, 21, 100), (0, 0, 20, 101), (-1, 0, 1, 1), (0, -1, 1, 1), (19, 96, 2, 1), (0, 99, 1, 2)):
            for call in (e.download_bits_window, e.download_bits_window_async):
                with pytest.raises(gh.GolError) as ex:
                    call(*bad)
                assert ex.value.code == -1 and "outside the grid" in str(ex.value)
            with pytest.raises(gh.GolError) as ex:
                e.upload_bits_window(bad[0], bad[1], max(bad[3], 0), np.zeros((max(bad[2], 0), (max(bad[3], 0) + 7) // 8),
                                                                              np.uint8))
            assert ex.value.code == -1
        buf = np.full((20, 16), 0x5A, np.uint8)
        p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        for call in (e.lib.gol_download_bits_window, e.lib.gol_download_bits_window_async, e.lib.gol_upload_bits_window):
            assert call(e._c, 0, 0, 20, 100, p, 12) == -1 and b"ld" in e.lib.gol_last_error(e._c)
            assert call(e._c, 0, 0, 20, 100, None, 16) == -1 and b"null" in e.lib.gol_last_error(e._c)
            assert call(e._c, 5, 5, 0, 3, p, 1) == 0 and call(e._c, 5, 5, 3, 0, None, 0) == 0   # empty: nothing moves
        assert e.lib.gol_download_bits(e._c, p, 12) == -1 and e.lib.gol_upload_bits(e._c, None, 16) == -1
        e.sync()
        assert (buf == 0x5A).all()
        assert (e.download_bits() == pack(b)).all() and (e.download() == b).all()


# ------------------------------------------------------------------ bin/gol --format pbm
def _run(args, cwd, check=True):
    return subprocess.run([EXE] + args, cwd=cwd, check=check, capture_output=True, text=True, timeout=120)


def _main_name(d):
    return [f for f in os.listdir(d) if f.endswith(".gol") and "_" not in f][0][:-4]


def read_pbm(path):
    raw = open(path, "rb").read()
    m = re.match(rb"P4\n# gol (\d+) (\d+) (\d+) (\d+)\n(\d+) (\d+)\n", raw)
    assert m, raw[:60]
    hdr = tuple(int(x) for x in m.groups()[:4])
    ncols, nrows = int(m.group(5)), int(m.group(6))
    body = raw[m.end():]
    assert len(body) == nrows * ((ncols + 7) // 8)
    return hdr, np.frombuffer(body, np.uint8).reshape(nrows, (ncols + 7) // 8)


def read_gol(path):
    lines = open(path).read().splitlines()
    hdr = tuple(int(x) for x in (lines[0] + " " + lines[1]).split())
    return hdr, np.array([[int(t) for t in ln.split()] for ln in lines[2:]], np.uint8)


def test_driver_pbm_snapshots_and_resume(gh, tmp_path):
    args = ["--mode", "dead", "--save", "--gpus", "2", "-k", "3", "--seed", "11"]
    a, t = tmp_path / "a", tmp_path / "t"
    a.mkdir()
    t.mkdir()
    _run(args + ["--format", "pbm", "96", "200", "5", "20"], a)
    _run(args + ["96", "200", "5", "20"], t)   # the twin: the same run in text
    name, tname = _main_name(a), _main_name(t)
    assert not [f for f in os.listdir(a) if f.endswith(".gol") and "_" in f]   # pbm parts only
    for it in (0, 5, 10, 15, 20):
        for p in range(2):
            hdr, bits = read_pbm(a / f"{name}_{it}_{p}.pbm")
            thdr, cells = read_gol(t / f"{tname}_{it}_{p}.gol")
            assert hdr == thdr == (48 * p, 48 * p + 47, 0, 199), (it, p, hdr, thdr)
            assert (bits == pack(cells)).all() and (it == 20 or cells.any()), (it, p)
    # resume from iteration 10: 15 and 20 come out byte for byte
    b = tmp_path / "b"
    shutil.copytree(a, b)
    for it in (15, 20):
        for p in range(2):
            (b / f"{name}_{it}_{p}.pbm").unlink()
    _run(args + ["--format", "pbm", "--resume", name, "--from", "10"], b)
    for it in (15, 20):
        for p in range(2):
            assert open(b / f"{name}_{it}_{p}.pbm", "rb").read() == open(a / f"{name}_{it}_{p}.pbm", "rb").read()
    # a short file and a malformed header: a message, exit 1
    good = open(a / f"{name}_10_1.pbm", "rb").read()
    for broken, msg in ((good[:-7], "bad body"), (good.replace(b"# gol", b"# lol", 1), "bad header"),
                        (b"P5" + good[2:], "bad header")):
        open(b / f"{name}_10_1.pbm", "wb").write(broken)
        r = _run(args + ["--format", "pbm", "--resume", name, "--from", "10"], b, check=False)
        assert r.returncode == 1 and msg in r.stdout, (msg, r.returncode, r.stdout[-300:])
    r = _run(args + ["--format", "png", "96", "200", "5", "20"], b, check=False)
    assert r.returncode == 1 and "--format must be" in r.stdout


def test_driver_pbm_over_rank_contexts(gh, tmp_path):
    assert os.path.exists(SHIM), "build the shim first (__graft_entry__.build())"
    args = ["--mode", "dead", "--save", "--gpus", "2", "--seed", "11", "96", "200", "10", "10"]
    a, t = tmp_path / "a", tmp_path / "t"
    a.mkdir()
    t.mkdir()
    _run(["--rccl", "--same-device", "--rccl-lib", SHIM, "--format", "pbm"] + args, a)
    _run(["--format", "pbm"] + args, t)
    name, tname = _main_name(a), _main_name(t)
    for it in (0, 10):
        for p in range(2):
            got, want = read_pbm(a / f"{name}_{it}_{p}.pbm"), read_pbm(t / f"{tname}_{it}_{p}.pbm")
            assert got[0] == want[0] and (got[1] == want[1]).all() and want[1].any(), (it, p)
    _run(["--rccl", "--same-device", "--rccl-lib", SHIM, "--format", "pbm", "--mode", "dead", "--save", "--gpus", "2",
          "--resume", name, "--from", "0"], a)
    for p in range(2):
        assert (read_pbm(a / f"{name}_10_{p}.pbm")[1] == read_pbm(t / f"{tname}_10_{p}.pbm")[1]).all()
