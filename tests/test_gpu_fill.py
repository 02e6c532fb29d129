"""gol_fill_random* on the GPU.  Every comparison is exact equality with the numpy
reference of the definition (tests/fill_ref.py, which computes every plane and
compares X as a number): every layout and group width, thresholds whose plane skip
starts at planes 31, 29, 0 and 0 and the two that bypass the hash, the seam between
two wave items, windows at any column on a board of ones, the torus ghost margin
(refreshed: the next step is right), MESH_COMPAT's reversed column blocks,
SERIAL_COMPAT's dead last row and column, slabs, rank contexts, the digest of the
filled board, a rule's soup, a fill beside the clock probe and bin/gol --soup."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rule_ref  # noqa: E402
import torus_ref  # noqa: E402
from digest_ref import digest_ref  # noqa: E402
from fill_ref import FULL, fill_x  # noqa: E402

EXE = os.path.join(ROOT, "mpi_amd", "bin", "gol")
SHIM = os.path.join(ROOT, "tests", "shim", "libfake_rccl.so")
THRESHOLDS = (1 << 31, 3 << 29, 0x55555555, 1, FULL - 1, 0, FULL)


@pytest.fixture(scope="module")
def gh():
    from mpi_amd import golhip
    golhip.load()
    return golhip


@functools.lru_cache(maxsize=None)
def x_of(seed, rows, cols):
    x = fill_x(seed, rows, cols)   # X(r, c) of the whole board: computed once, shared, never written
    x.setflags(write=False)
    return x


def ref(seed, t, rows, cols):
    return (x_of(seed, rows, cols) < np.uint64(t)).astype(np.uint8)


def ref_window(seed, t, row0, col0, nrows, ncols):
    return (fill_x(seed, nrows, ncols, row0, col0) < np.uint64(t)).astype(np.uint8)


def first_diff(a, b):
    bad = np.argwhere(a != b)
    return f"{len(bad)} differ, first at {bad[0]}: {a[tuple(bad[0])]} want {b[tuple(bad[0])]}"


def filled(e, seed, t, what, serial=False):
    want = ref(seed, t, e.rows, e.cols)
    if serial:
        want[-1] = 0
        want[:, -1] = 0
    got = e.download()
    assert (got == want).all(), f"{what} seed={seed} T={t:#x}: {first_diff(got, want)}"
    return want


# ------------------------------------------------------------------ layouts, depths, thresholds
@pytest.mark.parametrize("layout,k,cols", [("bit", 1, 8300), ("bit", 8, 8300), ("bit", 16, 8300), ("byte", 1, 2100)])
def test_layouts_depths_and_thresholds(gh, layout, k, cols):
    """203 rows (no multiple of 4 or 64) x more than 64 units (an item seam at storage column 8192 resp. 2048)."""
    with gh.Engine(203, cols, layout=layout, tblock_k=k) as e:
        for i, t in enumerate(THRESHOLDS):
            seed = (0, 1, 12345, 2**64 - 1)[i % 4]
            e.fill_random(seed=seed, threshold=t)
            want = filled(e, seed, t, (layout, k))
            assert e.generation == 0 and e.popcount() == int(want.sum())
        e.fill_random(0.375, seed=12345)   # the density form: threshold 3 * 2^29
        filled(e, 12345, 3 << 29, (layout, k, "density"))


# ------------------------------------------------------------------ windows
@pytest.mark.parametrize("layout,k,cols", [("bit", 1, 8300), ("bit", 8, 8300), ("byte", 1, 8300)])
def test_window_fill_changes_exactly_the_window(gh, layout, k, cols):
    rows = 203
    with gh.Engine(rows, cols, layout=layout, tblock_k=k) as e:
        e.upload(np.ones((rows, cols), np.uint8))
        cur = np.ones((rows, cols), np.uint8)
        n = 0
        for col0 in (37, 64, 8191):
            for ncols in (1, 31, 33, 200):
                if col0 + ncols > cols:
                    ncols = cols - col0
                row0, nrows = ((0, rows), (13, 5), (202, 1), (60, 70))[n % 4]
                seed, t = 100 + n, THRESHOLDS[n % 5]
                n += 1
                e.fill_random(seed=seed, threshold=t, window=(row0, col0, nrows, ncols))
                cur[row0:row0 + nrows, col0:col0 + ncols] = ref_window(seed, t, row0, col0, nrows, ncols)
                got = e.download()
                assert (got == cur).all(), (layout, k, row0, col0, nrows, ncols, first_diff(got, cur))


# ------------------------------------------------------------------ boundaries
@pytest.mark.parametrize("layout,k", [("bit", 3), ("bit", 8), ("bit", 16), ("bit", 32), ("byte", 16)])
def test_torus_fill_and_refreshed_ghosts(gh, layout, k):
    for rows, cols in ((64, 64), (40, 131)):
        with gh.Engine(rows, cols, layout=layout, boundary="torus", tblock_k=k) as e:
            e.upload(np.ones((rows, cols), np.uint8))   # ghosts of ones: stale ones would feed the step
            e.fill_random(0.5, seed=k)
            b = filled(e, k, 1 << 31, (layout, k, rows, cols))
            e.step(k)
            got, want = e.download(), torus_ref.run(b, k)
            assert (got == want).all(), (layout, k, rows, cols, first_diff(got, want))
            # a window at the right edge: its cells' ghosts are in the LEFT margin
            e.fill_random(0.375, seed=k + 1, window=(3, cols - 9, rows - 5, 9))
            b = want.copy()
            b[3:rows - 2, cols - 9:] = ref(k + 1, 3 << 29, rows, cols)[3:rows - 2, cols - 9:]
            assert (e.download() == b).all()
            e.step(1)
            got, want = e.download(), torus_ref.run(b, 1)
            assert (got == want).all(), (layout, k, rows, cols, "window", first_diff(got, want))


@pytest.mark.parametrize("layout", ["bit", "byte"])
@pytest.mark.parametrize("m,n", [(4, 48), (2, 1024)])
def test_mesh_compat_fills_logical_columns(gh, layout, m, n):
    with gh.Engine(n, n, layout=layout, boundary="mesh_compat", mesh_m=m, tblock_k=2) as e:
        e.fill_random(1 / 3, seed=m)
        cur = filled(e, m, gh.fill_threshold(1 / 3), (layout, m, n))
        # windows across block seams (n / m columns per block), at odd columns
        for i, (col0, nc) in enumerate(((5, n // m + 9), (n // m - 3, 7), (1, n - 2))):
            e.fill_random(seed=50 + i, threshold=0x55555555, window=(5, col0, 20, nc))
            cur[5:25, col0:col0 + nc] = ref(50 + i, 0x55555555, n, n)[5:25, col0:col0 + nc]
            got = e.download()
            assert (got == cur).all(), (layout, m, n, col0, nc, first_diff(got, cur))


@pytest.mark.parametrize("layout", ["bit", "byte"])
def test_serial_compat_keeps_a_dead_last_row_and_column(gh, layout):
    with gh.Engine(37, 37, layout=layout, boundary="serial_compat", tblock_k=2) as e:
        e.fill_random(1.0)
        got = e.download()
        assert got[:-1, :-1].all() and not got[-1].any() and not got[:, -1].any() and e.popcount() == 36 * 36
        e.fill_random(0.5, seed=3)
        filled(e, 3, 1 << 31, (layout, "serial"), serial=True)
        e.fill_random(1.0, window=(30, 30, 7, 7))   # a window over the corner
        got = e.download()
        assert got[30:36, 30:36].all() and not got[-1].any() and not got[:, -1].any()


# ------------------------------------------------------------------ slabs and ranks
@pytest.mark.parametrize("layout,k", [("bit", 8), ("byte", 4)])
def test_three_slabs(gh, layout, k):
    with gh.Engine(64, 200, n_gpus=3, layout=layout, tblock_k=k) as e:
        e.fill_random(0.375, seed=9)
        cur = filled(e, 9, 3 << 29, (layout, k))
        e.fill_random(0.5, seed=10, window=(10, 37, 45, 101))   # across both seams (rows 22 and 43)
        cur[10:55, 37:138] = ref(10, 1 << 31, 64, 200)[10:55, 37:138]
        got = e.download()
        assert (got == cur).all(), (layout, k, first_diff(got, cur))


def test_rank_parts_tile_the_board(gh):
    assert os.path.exists(SHIM), "build the shim first (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fill_rank_check.py"), SHIM],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "fill ranks ok" in r.stdout


# ------------------------------------------------------------------ digest, rules, the clock probe
@pytest.mark.parametrize("layout,k,boundary,slabs", [("bit", 1, "dead", 1), ("bit", 8, "torus", 3),
                                                     ("byte", 2, "dead", 2)])
def test_digest_of_the_filled_board(gh, layout, k, boundary, slabs):
    """Two independent device paths (fill, digest) against two independent host paths."""
    with gh.Engine(83, 300, layout=layout, boundary=boundary, n_gpus=slabs, tblock_k=k) as e:
        for seed, t in ((5, 1 << 31), (6, 0x55555555), (7, 0)):
            e.fill_random(seed=seed, threshold=t)
            assert e.digest() == digest_ref(ref(seed, t, 83, 300)), (layout, k, boundary, seed, t)
        assert e.digest() == (0, 0)
        e.fill_random(seed=8, threshold=3 << 29, window=(11, 33, 40, 131))
        assert e.digest() == digest_ref(ref(8, 3 << 29, 83, 300)[11:51, 33:164], 11, 33)


def test_day_and_night_soup(gh):
    birth, survive = rule_ref.parse("B3678/S34678")
    with gh.Engine(61, 130, rule="B3678/S34678", boundary="torus", layout="bit", tblock_k=4) as e:
        e.fill_random(0.5, seed=2)
        b = filled(e, 2, 1 << 31, "day & night")
        e.step(8)
        got, want = e.download(), rule_ref.run(b, 8, birth, survive, torus=True)
        assert e.rule == (birth, survive) and e.generation == 8
        assert (got == want).all() and want.any(), first_diff(got, want)


def test_fill_beside_the_clock_probe_and_between_steps(gh):
    """Nothing is allocated or staged: a context that has copied no window fills while the probe runs.
    The generation stays, and the context steps on from the filled board."""
    from oracle import golcpu as g
    with gh.Engine(100, 300, layout="bit", tblock_k=8) as e:
        e.step(8)
        e.clock_start(30000.0)
        try:
            e.fill_random(0.375, seed=4)
            e.fill_random(0.5, seed=6, window=(2, 3, 50, 170))
        finally:
            e.clock_stop()
        assert e.generation == 8
        b = ref(4, 3 << 29, 100, 300)
        b[2:52, 3:173] = ref(6, 1 << 31, 100, 300)[2:52, 3:173]
        assert (e.download() == b).all()
        e.step(11)
        assert e.generation == 19 and (e.download() == g.run(b, 11, g.DEAD)).all()


def test_errors_leave_the_context_usable(gh):
    with gh.Engine(20, 100, layout="bit") as e:
        e.fill_random(0.5, seed=9)
        want = ref(9, 1 << 31, 20, 100)
        for bad in ((0, 0, 21, 100), (0, 0, 20, 101), (-1, 0, 1, 1), (0, -1, 1, 1), (19, 96, 2, 1), (0, 99, 1, 2)):
            with pytest.raises(gh.GolError) as ex:
                e.fill_random(0.5, window=bad)
            assert ex.value.code == -1 and "outside the grid" in str(ex.value)
        with pytest.raises(gh.GolError) as ex:
            e.fill_random(threshold=FULL + 1)
        assert ex.value.code == -1 and "threshold" in str(ex.value)
        e.fill_random(1.0, window=(5, 5, 0, 3))   # empty: nothing written
        e.fill_random(1.0, window=(5, 5, 3, 0))
        assert (e.download() == want).all()


# ------------------------------------------------------------------ bin/gol --soup
def _run(args, cwd, check=True):
    return subprocess.run([EXE] + args, cwd=cwd, check=check, capture_output=True, text=True, timeout=120)


def last_board(d, it, parts, rows):
    """The snapshot of iteration `it`: the parts' PBM rasters, unpacked and stacked."""
    name = [f for f in os.listdir(d) if f.endswith(".gol") and "_" not in f][0][:-4]
    out = []
    for p in range(parts):
        raw = open(d / f"{name}_{it}_{p}.pbm", "rb").read()
        m = re.match(rb"P4\n# gol \d+ \d+ \d+ \d+\n(\d+) (\d+)\n", raw)
        assert m, raw[:60]
        ncols, nrows = int(m.group(1)), int(m.group(2))
        bits = np.frombuffer(raw[m.end():], np.uint8).reshape(nrows, (ncols + 7) // 8)
        out.append(np.unpackbits(bits, axis=1)[:, :ncols])
    b = np.concatenate(out)
    assert b.shape[0] == rows
    return b


def test_driver_soup(gh, tmp_path):
    from oracle import golcpu as g
    b0 = ref(7, 1 << 31, 96, 200)
    want = g.run(b0, 10, g.DEAD)
    args = ["--mode", "dead", "--save", "--gpus", "2", "-k", "3", "--soup", "0.5", "--seed", "7", "--format", "pbm",
            "96", "200", "5", "10"]
    _run(args, tmp_path)
    assert (last_board(tmp_path, 0, 2, 96) == b0).all()
    assert (last_board(tmp_path, 10, 2, 96) == want).all() and want.any()
    # the default seed is 1; the byte layout and the serial mode take the same soup
    d = tmp_path / "serial"
    d.mkdir()
    _run(["--mode", "serial", "--layout", "byte", "--soup", "0.375", "--format", "pbm", "64", "64", "4", "4"], d)
    s0 = ref(1, 3 << 29, 64, 64)
    s0[-1] = 0
    s0[:, -1] = 0
    assert (last_board(d, 0, 1, 64) == s0).all()
    assert (last_board(d, 4, 1, 64) == g.run(s0, 4, g.SERIAL_COMPAT)).all()
    for bad in ("1.5", "-0.1", "nan", "half"):
        r = _run(["--mode", "dead", "--soup", bad, "96", "200", "5", "10"], tmp_path, check=False)
        assert r.returncode == 1 and "--soup must be" in r.stdout, (bad, r.stdout[-300:])


def test_driver_soup_over_rank_contexts(gh, tmp_path):
    from oracle import golcpu as g
    assert os.path.exists(SHIM), "build the shim first (__graft_entry__.build())"
    _run(["--rccl", "--same-device", "--rccl-lib", SHIM, "--mode", "dead", "--save", "--gpus", "2", "--soup", "0.5",
          "--seed", "7", "--format", "pbm", "96", "200", "10", "10"], tmp_path)
    b0 = ref(7, 1 << 31, 96, 200)
    assert (last_board(tmp_path, 0, 2, 96) == b0).all()
    assert (last_board(tmp_path, 10, 2, 96) == g.run(b0, 10, g.DEAD)).all()
