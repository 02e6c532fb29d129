"""gol_density* on the GPU.  The master property: in every state of every context
density(th, tw) equals the reference map (tests/density_ref.py) of what
download() returns, and its sum is popcount() — every layout and group width,
partial words and units, tile rows shorter than a row segment and ending
mid-segment, tiles wider than the board, the torus ghost margin at shifts that
are no multiple of 32, MESH_COMPAT's reversed column blocks, SERIAL_COMPAT's
dead last row and column, windows, slabs, rank contexts, pending async maps."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from density_ref import density_ref, tile_cells

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mpi_amd", "bin", "gol")
SHIM = os.path.join(ROOT, "tests", "shim", "libfake_rccl.so")

BIT_BYTE_K = [("bit", 1), ("bit", 3), ("bit", 7), ("bit", 8), ("bit", 16), ("byte", 1), ("byte", 16)]
# a tile shorter than a 64-row block, a tile row that ends mid-block, a tile wider than the
# board, one tile for the whole board
TILES = [(1, 32), (3, 32), (5, 64), (16, 96), (64, 128), (37, 160), (1000, 4096)]


@pytest.fixture(scope="module")
def gh():
    from mpi_amd import golhip
    golhip.load()
    return golhip


def soup(seed, rows, cols, p=0.4):
    return (np.random.default_rng(seed).random((rows, cols)) < p).astype(np.uint8)


def same_as_download(e, tiles, what):
    got = e.download()
    live = e.popcount()
    for th, tw in tiles:
        d, want = e.density(th, tw), density_ref(got, th, tw)
        assert d.dtype == np.uint32 and d.shape == want.shape, (what, th, tw, d.shape, want.shape)
        bad = np.argwhere(d != want)
        assert bad.size == 0, f"{what} tile {th}x{tw}: {len(bad)} tiles differ, first {bad[0]}: " \
                              f"{d[tuple(bad[0])]} want {want[tuple(bad[0])]}"
        assert int(d.sum(dtype=np.uint64)) == live == int(got.sum())
    return got


def block_steps(k):
    return [k, max(1, k - 3), 1, k]   # both ping-pong buffers and a short block are read


# ------------------------------------------------------------------ layouts and shapes
@pytest.mark.parametrize("layout,k", BIT_BYTE_K)
def test_layouts_shapes_and_tiles(gh, layout, k):
    for rows, cols in ((37, 131), (8, 8), (64, 257), (100, 4096)):
        with gh.Engine(rows, cols, layout=layout, tblock_k=k) as e:
            for th, tw in TILES:
                assert not e.density(th, tw).any()   # the empty board
            e.upload(soup(rows + cols, rows, cols))
            got = same_as_download(e, TILES, (layout, k, rows, cols, 0))
            assert got.any()
            for s in block_steps(k):
                e.step(s)
                same_as_download(e, TILES, (layout, k, rows, cols, e.generation))


def test_known_answers(gh):
    b = np.zeros((37, 131), np.uint8)
    b[3, 70] = b[3, 95] = b[4, 96] = b[36, 130] = 1
    want = np.array([[0, 0, 2, 0, 0],
                     [0, 0, 0, 1, 0],
                     [0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 1]], np.uint32)
    for layout, k in (("bit", 1), ("bit", 8), ("byte", 1)):
        with gh.Engine(37, 131, layout=layout, tblock_k=k) as e:
            e.upload(b)
            d = e.density(4, 32)
            assert d.shape == (10, 5) and (d == want).all(), (layout, k, d)
            # a full board: every tile holds its own (clipped) cell count
            e.upload(np.ones((37, 131), np.uint8))
            assert (e.density(4, 32) == np.outer([4] * 9 + [1], [32] * 4 + [3])).all()


# ------------------------------------------------------------------ boundaries
@pytest.mark.parametrize("layout,k", [("bit", 1), ("bit", 3), ("bit", 8), ("bit", 32), ("byte", 16), ("byte", 3)])
def test_torus_ghost_columns_are_not_counted(gh, layout, k):
    for rows, cols in ((64, 64), (40, 131)):
        with gh.Engine(rows, cols, layout=layout, boundary="torus", tblock_k=k) as e:
            # live cells in the first and last two columns: their copies sit in the ghost margins
            b = soup(k, rows, cols)
            b[:, :2] = 1
            b[:, -2:] = 1
            e.upload(b)
            same_as_download(e, [(8, 32), (40, 64)], (layout, k, rows, cols, 0))
            for s in (k, 1):
                e.step(s)
                same_as_download(e, [(8, 32), (40, 64)], (layout, k, rows, cols, e.generation))


@pytest.mark.parametrize("layout", ["bit", "byte"])
@pytest.mark.parametrize("m,n", [(4, 48), (2, 1024)])
def test_mesh_compat_maps_are_in_logical_columns(gh, layout, m, n):
    with gh.Engine(n, n, layout=layout, boundary="mesh_compat", mesh_m=m, tblock_k=2) as e:
        e.upload(soup(m, n, n))
        same_as_download(e, [(5, 32)], (layout, m, n, 0))
        e.step(3)
        got = same_as_download(e, [(5, 32)], (layout, m, n, 3))
        # a window at col0 = 32 across a block seam (n / m columns per block)
        nc = min(n - 32, n // m + 9)
        d = e.density_window(5, 32, 20, nc, 5, 32)
        assert (d == density_ref(got[5:25, 32:32 + nc], 5, 32)).all()


@pytest.mark.parametrize("layout", ["bit", "byte"])
def test_serial_compat_inactive_row_and_column_count_zero(gh, layout):
    with gh.Engine(37, 37, layout=layout, boundary="serial_compat", tblock_k=2) as e:
        e.upload(np.ones((37, 37), np.uint8))   # the last row and column are stored as 0
        got = same_as_download(e, [(4, 32), (37, 64)], (layout, "ones"))
        assert not got[-1].any() and not got[:, -1].any()
        assert (e.density(4, 32) == np.outer([4] * 9 + [0], [32, 4])).all()
        e.step(5)
        same_as_download(e, [(4, 32)], (layout, 5))


# ------------------------------------------------------------------ slabs and ranks
@pytest.mark.parametrize("layout,k", [("bit", 8), ("byte", 4)])
def test_three_slabs_equal_one(gh, layout, k):
    b = soup(9, 64, 200)
    maps = []
    for slabs in (1, 3):
        with gh.Engine(64, 200, n_gpus=slabs, layout=layout, tblock_k=k) as e:
            e.upload(b)
            for s in block_steps(k):
                e.step(s)
            same_as_download(e, [(7, 32), (7, 96)], (layout, k, slabs))   # tiles straddle both seams
            maps.append(e.density(7, 32))
    assert (maps[0] == maps[1]).all()


def test_rank_maps_sum_to_the_board(gh):
    assert os.path.exists(SHIM), "build the shim first (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "density_rank_check.py"), SHIM],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "density ranks ok" in r.stdout


# ------------------------------------------------------------------ windows
@pytest.mark.parametrize("layout,k,boundary", [("bit", 1, "dead"), ("bit", 8, "dead"), ("byte", 1, "dead"),
                                               ("bit", 3, "torus"), ("byte", 5, "torus")])
def test_windows(gh, layout, k, boundary):
    rows, cols = 100, 300
    with gh.Engine(rows, cols, layout=layout, boundary=boundary, tblock_k=k) as e:
        e.upload(soup(3, rows, cols))
        e.step(k)
        got = e.download()
        whole = e.density(7, 32)
        for row0, nrows in ((0, 100), (13, 71), (99, 1)):      # row0 not a multiple of anything
            for col0 in (0, 32, 96):
                for ncols in (300 - col0, 77, 130):            # to the edge; ending mid-tile
                    for th, tw in ((7, 32), (1, 64), (64, 96)):
                        d = e.density_window(row0, col0, nrows, ncols, th, tw)
                        want = density_ref(got[row0:row0 + nrows, col0:col0 + ncols], th, tw)
                        assert d.shape == want.shape and (d == want).all(), (row0, col0, nrows, ncols, th, tw)
        assert e.density_window(rows, 288, 0, 0, 7, 32).shape == (0, 0)
        for bad in ((0, 0, rows + 1, cols, 7, 32), (0, 16, 10, 10, 7, 32), (0, 0, 10, 10, 7, 48), (0, 0, 10, 10, 0, 32)):
            with pytest.raises(gh.GolError) as ex:
                e.density_window(*bad)
            assert ex.value.code == -1
        assert (e.density(7, 32) == whole).all()   # the context stays usable


# ------------------------------------------------------------------ async
@pytest.mark.parametrize("layout,k,slabs,boundary,rows", [("bit", 8, 1, "dead", 700), ("bit", 4, 3, "dead", 100),
                                                          ("byte", 16, 2, "torus", 90)])
def test_async_maps_between_steps(gh, layout, k, slabs, boundary, rows):
    cols = 300
    b = soup(21, rows, cols)
    kw = dict(n_gpus=slabs, layout=layout, boundary=boundary, tblock_k=k)
    with gh.Engine(rows, cols, **kw) as e, gh.Engine(rows, cols, **kw) as ref:
        e.upload(b)
        ref.upload(b)
        for _ in range(3):
            outs, wants = [], []
            for tiles in ((7, 32), (64, 128), (7, 32)):   # three pending at once, no sync in between
                e.step(k)
                outs.append(e.density_async(*tiles))
                ref.step(k)   # the second engine in lockstep: the board at that generation
                wants.append(density_ref(ref.download(), *tiles))
            assert not any(o.any() for o in outs)
            e.sync()      # one synchronising call delivers all three
            for o, w in zip(outs, wants):
                assert o.shape == w.shape and (o == w).all() and w.any(), (layout, k, slabs)


# ------------------------------------------------------------------ bin/gol --density
def read_pgm(path):
    raw = open(path, "rb").read()
    m = re.match(rb"P5\n(\d+) (\d+)\n65535\n", raw)
    assert m, raw[:40]
    tcols, trows = int(m.group(1)), int(m.group(2))
    body = raw[m.end():]
    assert len(body) == 2 * tcols * trows
    return np.frombuffer(body, ">u2").reshape(trows, tcols).astype(np.uint32)


def test_driver_density_pgm(gh, tmp_path):
    for extra, boundary in ((["--mode", "dead"], "dead"), (["--mode", "torus", "--gpus", "2"], "torus")):
        r = subprocess.run([EXE, "--density", "16x32"] + extra + ["100", "200", "5", "10"], cwd=tmp_path, check=True,
                           capture_output=True, text=True, timeout=120)
        name = re.search(r"^0: (\S+)  gens=10 ", r.stdout, re.M).group(1)
        lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("density ")]
        assert [(int(g), f) for _, g, f in lines] == [(5, f"{name}_5.pgm"), (10, f"{name}_10.pgm")], r.stdout
        cells = tile_cells(100, 200, 16, 32).astype(np.uint64)
        with gh.Engine(100, 200, layout="bit", boundary=boundary, tblock_k=1) as e:
            e.initialize_board("stream", 1)
            for gen in (5, 10):
                e.step(gen - e.generation)
                ref = density_ref(e.download(), 16, 32).astype(np.uint64)
                assert ref.any()
                got = read_pgm(os.path.join(tmp_path, f"{name}_{gen}.pgm"))
                assert got.shape == (7, 7) and (got == 65535 * ref // cells).all(), (extra, gen)
    for bad in ("0", "16", "16x", "16x48", "x32", "16x32x", "4294967296x32"):
        r = subprocess.run([EXE, "--density", bad, "--mode", "dead", "100", "200", "5", "10"], cwd=tmp_path,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--density must be" in r.stdout, (bad, r.stdout)


# ------------------------------------------------------------------ schedule
def test_density_schedule_has_no_race_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sched_density_check.py"), "gpu"],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "sched density gpu ok" in r.stdout
