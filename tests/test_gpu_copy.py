"""gol_copy_window / gol_copy on the GPU.  The expected board is always the numpy
statement of the definition applied to the two downloads (exact equality): every
pair of storage forms at column shifts 0, 1, 31, 32, 33 and -97 with either buffer
current, the seam between two wave items, torus ghost margins (never copied as cells,
refreshed: the next step is right), MESH_COMPAT's reversed column blocks,
SERIAL_COMPAT's dead last row and column, different slab counts with seams of both
sides inside the window, one context onto itself, rank contexts, a copy beside the
clock probe, Engine.clone and Engine.period."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torus_ref  # noqa: E402

SHIM = os.path.join(ROOT, "tests", "shim", "libfake_rccl.so")
OPS = ("replace", "or", "xor")


@pytest.fixture(scope="module")
def gh():
    from mpi_amd import golhip
    golhip.load()
    return golhip


def first_diff(a, b):
    bad = np.argwhere(a != b)
    return f"{len(bad)} differ, first at {bad[0]}: {a[tuple(bad[0])]} want {b[tuple(bad[0])]}"


def merged(dst, src, win, at, op, serial=False):
    """The definition: numpy on the two downloads.  win = (row0, col0, nrows, ncols) of src."""
    r0, c0, nr, nc = win
    out = dst.copy()
    s, o = src[r0:r0 + nr, c0:c0 + nc], out[at[0]:at[0] + nr, at[1]:at[1] + nc]
    out[at[0]:at[0] + nr, at[1]:at[1] + nc] = s if op == "replace" else (o | s) if op == "or" else (o ^ s)
    if serial:
        out[-1] = 0
        out[:, -1] = 0
    return out


def copy_and_check(dst, src, db, sb, win, at, op, what, serial=False):
    dst.copy_from(src, win, at, op)
    want = merged(db, sb, win, at, op, serial)
    got = dst.download()
    assert (got == want).all(), (what, win, at, op, first_diff(got, want))
    return want


# ------------------------------------------------------------------ every storage pair
KINDS = (("bit", 1), ("bit", 8), ("byte", 1))
PAIRS = [(s, d, True) for s in KINDS for d in KINDS] + [(("bit", 16), ("bit", 7), False), (("byte", 16), ("bit", 8), False)]
# (srow0, scol0, drow0, dcol0, nrows, ncols) on a 70 x 517 source and a 90 x 700 destination
WINDOWS = ((0, 5, 3, 5, 40, 1),          # shift 0
           (2, 36, 0, 37, 30, 31),       # shift 1
           (5, 100, 7, 131, 50, 33),     # shift 31
           (1, 64, 20, 96, 60, 128),     # shift 32
           (3, 7, 11, 40, 66, 300),      # shift 33
           (10, 200, 0, 103, 13, 128),   # shift -97
           (0, 217, 5, 400, 70, 300),    # ends at the last column of both boards
           (30, 0, 50, 0, 40, 517))      # ends at the last row of both boards


@pytest.mark.parametrize("skind,dkind,all_ops", PAIRS, ids=lambda v: f"{v[0]}{v[1]}" if isinstance(v, tuple) else str(v))
def test_every_storage_pair(gh, skind, dkind, all_ops):
    with gh.Engine(70, 517, layout=skind[0], tblock_k=skind[1]) as src, \
            gh.Engine(90, 700, layout=dkind[0], tblock_k=dkind[1]) as dst:
        src.fill_random(0.5, seed=1)
        dst.fill_random(0.5, seed=2)
        src.step(skind[1])       # one k-step: the source reads from its second buffer
        dst.step(2 * dkind[1])   # two: the destination writes its first
        sb, db = src.download(), dst.download()
        assert sb.any() and db.any()
        gens = src.generation, dst.generation
        for i, (sr, sc, dr, dc, nr, nc) in enumerate(WINDOWS):
            for op in OPS if all_ops else OPS[:1]:
                db = copy_and_check(dst, src, db, sb, (sr, sc, nr, nc), (dr, dc), op, (skind, dkind, i))
        assert (src.download() == sb).all() and (src.generation, dst.generation) == gens


# ------------------------------------------------------------------ the seam between two wave items
BIG = {("bit", 1): 8300, ("bit", 8): 8300, ("byte", 1): 2100}   # more than 64 destination units in a row


@pytest.mark.parametrize("skind,dkind", [(("bit", 1), ("bit", 8)), (("bit", 8), ("bit", 1)), (("bit", 8), ("bit", 8)),
                                         (("bit", 1), ("byte", 1)), (("bit", 8), ("byte", 1)),
                                         (("byte", 1), ("bit", 1)), (("byte", 1), ("bit", 8)),
                                         (("byte", 1), ("byte", 1))],
                         ids=lambda v: f"{v[0]}{v[1]}")
def test_wave_item_seam(gh, skind, dkind):
    scols, dcols = BIG[skind], BIG[dkind]
    with gh.Engine(3, scols, layout=skind[0], tblock_k=skind[1]) as src, \
            gh.Engine(3, dcols, layout=dkind[0], tblock_k=dkind[1]) as dst:
        src.fill_random(0.5, seed=3)
        dst.fill_random(0.5, seed=4)
        sb, db = src.download(), dst.download()
        # destination unit 64 starts at column 8192 (bit) resp. 2048 (byte): every window covers it
        base = 6144 if dcols > scols else 0   # a narrow source: the window sits at the seam (6144 = 48 * 128)
        ncols = min(scols, dcols) - 60
        for i, shift in enumerate((0, 1, 33)):
            win, at = (0, 20, 3, ncols), (0, 20 + base + shift)
            assert at[1] < (8192 if dkind[0] == "bit" else 2048) < at[1] + ncols <= dcols
            db = copy_and_check(dst, src, db, sb, win, at, OPS[i], (skind, dkind, shift))


# ------------------------------------------------------------------ boundaries
@pytest.mark.parametrize("layout,k", [("bit", 8), ("byte", 3)])
def test_torus_source_and_destination(gh, layout, k):
    """Ghost columns are never copied as cells, and the destination's are refreshed: its next k-step is the
    torus step of the numpy board."""
    other = ("byte", 1) if layout == "bit" else ("bit", 8)
    with gh.Engine(50, 131, layout=layout, boundary="torus", tblock_k=k) as t, \
            gh.Engine(60, 200, layout=other[0], tblock_k=other[1]) as flat:
        t.fill_random(0.5, seed=5)
        flat.fill_random(0.5, seed=6)
        t.step(k)
        tb, fb = t.download(), flat.download()
        # torus as source: windows at both edges of its rows (next to the ghost margins)
        fb = copy_and_check(flat, t, fb, tb, (0, 0, 50, 131), (5, 33), "replace", (layout, k, "whole"))
        fb = copy_and_check(flat, t, fb, tb, (3, 100, 40, 31), (0, 0), "xor", (layout, k, "right edge"))
        fb = copy_and_check(flat, t, fb, tb, (3, 0, 40, 9), (20, 191), "or", (layout, k, "left edge"))
        # torus as destination: windows that write its first and last columns
        for win, at, op in (((1, 7, 45, 131), (2, 0), "replace"), ((0, 150, 50, 9), (0, 122), "xor"),
                            ((10, 0, 30, 5), (15, 0), "or")):
            # (the ghosts hold tb's edge columns: stale ones would feed the step)
            tb2 =copy_and_check(t, flat, tb, fb, win, at, op, (layout, k, "dst"))
            t.step(k)
            got, want = t.download(), torus_ref.run(tb2, k)
            assert (got == want).all(), (layout, k, win, at, first_diff(got, want))
            tb = want
        # torus to torus, the same storage
        with gh.Engine(50, 131, layout=layout, boundary="torus", tblock_k=k) as t2:
            t2.copy_from(t)
            assert (t2.download() == tb).all() and t2.digest() == t.digest()
            t2.step(k)
            assert (t2.download() == torus_ref.run(tb, k)).all()


@pytest.mark.parametrize("layout", ["bit", "byte"])
@pytest.mark.parametrize("m,n", [(4, 48), (2, 1024)])
def test_mesh_compat_source_and_destination(gh, layout, m, n):
    other = "byte" if layout == "bit" else "bit"
    with gh.Engine(n, n, layout=layout, boundary="mesh_compat", mesh_m=m, tblock_k=2) as mesh, \
            gh.Engine(n + 5, n + 70, layout=other, tblock_k=8) as flat:
        mesh.fill_random(0.5, seed=7)
        flat.fill_random(0.5, seed=8)
        mb, fb = mesh.download(), flat.download()
        L = n // m   # columns per block
        # windows across block seams, at odd columns
        wins = ((5, L + 9), (L - 3, 7), (1, n - 2))
        for i, (c0, nc) in enumerate(wins):
            fb = copy_and_check(flat, mesh, fb, mb, (3, c0, 20, nc), (i, 37 + i), OPS[i], (layout, m, n, "src", c0, nc))
        for i, (c0, nc) in enumerate(wins):
            mb = copy_and_check(mesh, flat, mb, fb, (i, 33 + i, 20, nc), (7, c0), OPS[2 - i], (layout, m, n, "dst", c0, nc))
        # mesh to mesh: the runs of both sides are paired
        with gh.Engine(n, n, layout=other, boundary="mesh_compat", mesh_m=m, tblock_k=2) as mesh2:
            m2 = mesh2.download()
            m2 = copy_and_check(mesh2, mesh, m2, mb, (0, 0, n, n), (0, 0), "replace", (layout, m, n, "whole"))
            copy_and_check(mesh2, mesh, m2, mb, (2, 3, 30, n - L - 1), (5, L - 2), "xor", (layout, m, n, "shifted"))


@pytest.mark.parametrize("layout", ["bit", "byte"])
def test_serial_compat_keeps_a_dead_last_row_and_column(gh, layout):
    with gh.Engine(37, 37, layout="bit" if layout == "byte" else "byte") as ones, \
            gh.Engine(37, 37, layout=layout, boundary="serial_compat", tblock_k=2) as e:
        ones.upload(np.ones((37, 37), np.uint8))
        e.fill_random(0.5, seed=9)
        b = e.download()
        assert not b[-1].any() and not b[:, -1].any()
        e.copy_from(ones, op="or")   # the whole board
        got = e.download()
        assert got[:-1, :-1].all() and not got[-1].any() and not got[:, -1].any() and e.popcount() == 36 * 36
        for op in ("xor", "replace"):
            e.copy_from(ones, (0, 0, 7, 7), (30, 30), op)   # a window over the corner
            got = e.download()
            assert not got[-1].any() and not got[:, -1].any()
            assert got[30:36, 30:36].all() == (op == "replace") and got[30:36, 30:36].any() == (op == "replace")


# ------------------------------------------------------------------ slabs
@pytest.mark.parametrize("dslabs", [2, 1])
@pytest.mark.parametrize("slayout,dlayout,k", [("bit", "byte", 4), ("byte", "bit", 8)])
def test_slabs_of_both_sides_inside_the_window(gh, dslabs, slayout, dlayout, k):
    from oracle import golcpu as g
    with gh.Engine(64, 200, n_gpus=3, layout=slayout, tblock_k=2) as src, \
            gh.Engine(70, 260, n_gpus=dslabs, layout=dlayout, tblock_k=k) as dst:   # seams: 22, 43 | 35
        src.fill_random(0.5, seed=10)
        dst.fill_random(0.375, seed=11)
        src.step(2)
        sb, db = src.download(), dst.download()
        # source seams at destination rows 26 and 47, the destination's seam at source row 31
        db = copy_and_check(dst, src, db, sb, (5, 3, 55, 190), (9, 33), "replace", (dslabs, slayout, dlayout))
        db = copy_and_check(dst, src, db, sb, (0, 0, 64, 200), (6, 60), "xor", (dslabs, slayout, dlayout))
        db = copy_and_check(dst, src, db, sb, (21, 0, 3, 200), (34, 1), "or", (dslabs, slayout, dlayout))
        dst.step(k)
        got, want = dst.download(), g.run(db, k, g.DEAD)
        assert (got == want).all() and want.any(), first_diff(got, want)


# ------------------------------------------------------------------ one context
@pytest.mark.parametrize("layout,k,slabs", [("bit", 1, 1), ("bit", 8, 2), ("byte", 1, 1)])
def test_window_tiled_within_one_board(gh, layout, k, slabs):
    with gh.Engine(60, 300, layout=layout, tblock_k=k, n_gpus=slabs) as e:
        e.fill_random(0.5, seed=12)
        e.step(k)
        b = e.download()
        assert b.any()
        # 20 x 45 from (3, 5): columns 5 .. 49; the tiles start where the window's last storage word goes on
        for at, op in (((3, 50), "replace"), ((3, 95), "or"), ((3, 141), "xor"), ((23, 49), "replace")):
            b = copy_and_check(e, e, b, b, (3, 5, 20, 45), at, op, (layout, k, slabs))
        for at in ((3, 5), (3, 49), (22, 49), (0, 0)):
            with pytest.raises(gh.GolError) as ex:
                e.copy_from(e, (3, 5, 20, 45), at)
            assert ex.value.code == -1 and "overlap" in str(ex.value)
            assert (e.download() == b).all()


# ------------------------------------------------------------------ ranks, the clock probe
def test_rank_contexts_tile_the_source_board(gh):
    assert os.path.exists(SHIM), "build the shim first (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "copy_rank_check.py"), SHIM],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "copy ranks ok" in r.stdout


def test_copy_beside_the_clock_probe(gh):
    """Nothing is allocated or staged: two contexts that have copied no window copy while a probe runs on one."""
    with gh.Engine(100, 300, layout="bit", tblock_k=8) as a, gh.Engine(120, 310, layout="byte", tblock_k=2) as b:
        a.fill_random(0.5, seed=13)
        b.fill_random(0.5, seed=14)
        a.step(8)
        ab, bb = a.download(), b.download()
        a.clock_start(30000.0)
        try:
            b.copy_from(a, (2, 3, 90, 290), (11, 7), "xor")     # the probe on the source
            a.copy_from(b, (0, 0, 50, 170), (40, 129), "or")    # ... and on the destination
        finally:
            a.clock_stop()
        bb = merged(bb, ab, (2, 3, 90, 290), (11, 7), "xor")
        ab = merged(ab, bb, (0, 0, 50, 170), (40, 129), "or")
        assert (b.download() == bb).all() and (a.download() == ab).all() and a.generation == 8


# ------------------------------------------------------------------ clone and period
def test_clone_at_another_layout_and_depth(gh):
    with gh.Engine(83, 300, layout="bit", tblock_k=16, n_gpus=2) as e:
        e.fill_random(0.4, seed=15)
        e.step(16)
        b, d = e.download(), e.digest()
        for kw in (dict(), dict(layout="byte", tblock_k=3, n_gpus=1), dict(tblock_k=7), dict(boundary="torus", tblock_k=8)):
            with e.clone(**kw) as c:
                assert c.generation == 0 and c.digest() == d and (c.download() == b).all(), kw
        assert e.generation == 16 and e.digest() == d


def test_clone_carries_the_rule_or_raises(gh):
    with gh.Engine(40, 100, layout="bit", tblock_k=4, rule="B36/S23") as e:
        e.fill_random(0.5, seed=16)
        with e.clone(tblock_k=7, boundary="torus") as c:
            assert c.rule == e.rule and c.digest() == e.digest()
        with pytest.raises(gh.GolError) as ex:
            e.clone(tblock_k=8)
        assert ex.value.code == -5


def test_period_of_blinker_and_pulsar(gh):
    b = np.zeros((40, 40), np.uint8)
    arm = (2, 3, 4, 8, 9, 10)
    for i in (0, 5, 7, 12):   # the pulsar (period 3), corner at (2, 2)
        for j in arm:
            b[2 + i, 2 + j] = 1
            b[2 + j, 2 + i] = 1
    b[30, 29:32] = 1          # a blinker (period 2)
    for kw in (dict(layout="bit", tblock_k=8), dict(layout="byte", tblock_k=4, n_gpus=2)):
        with gh.Engine(40, 40, **kw) as e:
            e.upload(b)
            e.step(3)
            d = e.digest()
            assert e.period(10) == 6 and e.period(10, batch=4) == 6 and e.period(5) is None
            assert e.generation == 3 and e.digest() == d
