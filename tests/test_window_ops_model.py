"""tests/window_ops_model.py pinned on the CPU: the model's fill, digest, packed rows,
density and merge against the per-cell definitions, and the plan tables of the sweep of
the device-side window calls (tests/window_ops_sweep.py) on every board of the kinds
table: tiles, thresholds, shifts, copy sources, the density pass and the digest tiling.
The GPU test and the CPU script take all of it from the same helper, so they cannot
thin anything without this file failing.  (The sweep sorts the window list by class
before it writes; the copy plan is pinned on the sorted list.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digest_ref  # noqa: E402
import fill_ref  # noqa: E402
import window_ops_model as wm  # noqa: E402

BOARDS = sorted({b for kind in wm.KINDS for b in kind[3]})


def test_the_base_model_is_unchanged():
    import window_model
    for name in ("KINDS", "COL0", "NCOLS", "SLABS", "windows", "write", "step", "text", "seams", "slab_counts", "soup"):
        assert getattr(wm, name) is getattr(window_model, name), name


# ------------------------------------------------------------------ the device-side window calls
def test_fill_is_the_per_cell_definition():
    w = (3, 29, 4, 37)   # a nonzero origin, across a word seam
    for seed, T in ((11, 1 << 31), (12, 3 << 29), (13, 0x55555555), (14, 1 << 32), (15, 0)):
        m = np.zeros((9, 70), np.uint8)
        assert wm.fill(m, w, seed, T, "dead") is m
        want = np.zeros((9, 70), np.uint8)
        want[3:7, 29:66] = fill_ref.fill_cells(seed, T, 4, 37, 3, 29)
        assert (m == want).all(), (seed, T)
        assert bool(m.any()) == (T > 0) and (T < 1 << 32 or int(m.sum()) == 4 * 37)
    s = np.ones((5, 6), np.uint8)
    wm.fill(s, (0, 0, 5, 6), 1, 1 << 32, "serial_compat")
    assert s[:4, :5].all() and not s[4].any() and not s[:, 5].any()


def test_digest_is_the_per_cell_definition():
    m = wm.soup(5, 9, 70)
    for w in ((3, 29, 4, 37), (0, 0, 9, 70), (8, 69, 1, 1), (2, 31, 5, 2)):
        assert wm.digest(m, w) == digest_ref.digest_cells(wm.cut(m, w), w[0], w[1]), w
    assert wm.digest(m, (0, 0, 9, 70)) != wm.digest(m, (0, 0, 9, 69))
    assert digest_ref.add(wm.digest(m, (0, 0, 9, 33)), wm.digest(m, (0, 33, 9, 37))) == wm.digest(m, (0, 0, 9, 70))


def test_bits_pad_bits_are_zero():
    cells = np.ones((2, 11), np.uint8)
    cells[1, 8] = 0
    got = wm.bits(cells)
    assert got.dtype == np.uint8 and got.tolist() == [[0xFF, 0xE0], [0xFF, 0x60]]
    assert wm.bits(np.array([[2, 0, 0x80]], np.uint8)).tolist() == [[0xA0]]   # any nonzero byte is a live cell


def test_density_is_the_tile_sum():
    m = wm.soup(6, 9, 200)
    got = wm.density(m, (2, 32, 7, 100), 3, 64)
    assert got.shape == (3, 2) and got.dtype == np.uint32
    assert got[0, 0] == m[2:5, 32:96].sum() and got[2, 1] == m[8:9, 96:132].sum() and got.sum() == m[2:9, 32:132].sum()


def test_merge():
    d0 = np.array([[1, 1, 0], [0, 1, 0], [0, 0, 1]], np.uint8)
    s = np.array([[1, 0, 1], [1, 1, 0], [0, 1, 1]], np.uint8)
    want = {"replace": [[1, 1, 0], [0, 1, 0], [0, 1, 1]],      # rows 1..2, columns 1..2 <- src rows 0..1, columns 0..1
            "or": [[1, 1, 0], [0, 1, 0], [0, 1, 1]],
            "xor": [[1, 1, 0], [0, 0, 0], [0, 1, 0]]}
    for op in wm.OPS:
        d = d0.copy()
        assert wm.merge(d, (1, 1, 2, 2), s, (0, 0), op, "dead") is d
        assert d.tolist() == want[op], op
    for op, rows in (("replace", [[1, 0, 0], [1, 1, 0], [0, 0, 0]]), ("or", [[1, 1, 0], [1, 1, 0], [0, 0, 0]]),
                     ("xor", [[0, 1, 0], [1, 0, 0], [0, 0, 0]])):
        d = d0.copy()
        wm.merge(d, (0, 0, 3, 3), s, (0, 0), op, "serial_compat")   # the dead last row and column under every op
        assert d.tolist() == rows, op
    assert (s == [[1, 0, 1], [1, 1, 0], [0, 1, 1]]).all()


def test_plan_tables():
    assert set(wm.THRESHOLDS) == {0, 1 << 32, 1 << 31, 3 << 29, 0x55555555, 1} and len(wm.THRESHOLDS) == 6
    assert {s for s in wm.SHIFTS if s >= 0} == {0, 1, 31, 32, 33, 97}
    assert {-s for s in wm.SHIFTS if s < 0} == {1, 31, 32, 33, 97} and len(wm.SHIFTS) == 11
    assert all(tr >= 1 and tc >= 32 and tc % 32 == 0 for tr, tc in wm.TILES)
    assert any(tr == 1 for tr, _ in wm.TILES) and {tc for _, tc in wm.TILES} >= {32, 64, 96, 128}
    assert any(tc > max(b[1] for b in BOARDS) for _, tc in wm.TILES)   # a tile wider than any window
    # the foreign copy source of every kind: never its own storage form, every entry in use,
    # and legal on every board of the kind in 3 slabs (a torus needs rows / slabs >= k and cols >= k)
    used = set()
    for ki, (layout, k, _, boards) in enumerate(wm.KINDS):
        f = wm.foreign_kind(ki)
        used.add(f)
        assert f in wm.FOREIGN and wm.storage_form(*f[:2]) != wm.storage_form(layout, k), ki
        assert all(rows // 3 >= f[1] and cols >= f[1] for rows, cols, _ in boards), ki
    assert used == set(wm.FOREIGN) and len(set(wm.FOREIGN)) == 4
    assert {wm.storage_form(*f[:2]) for f in wm.FOREIGN} == {"bit2", "bit4", "byte"}
    assert {wm.fill_plan(i)[1] for i in range(6)} == set(wm.THRESHOLDS)
    assert len({wm.fill_plan(i)[0] for i in range(150)}) == 150


def _ordered(rows, cols, m):
    wins = wm.windows(rows, cols, wm.seams(rows), m)
    return wins, sorted(wins, key=lambda w: -w[0])


@pytest.mark.parametrize("rows,cols,m", BOARDS)
def test_density_and_fill_plans(rows, cols, m):
    wins, order = _ordered(rows, cols, m)
    ok = [(i, w[1:]) for i, w in enumerate(wins) if wm.density_ok(w[1:])]
    no = [w[1:] for w in wins if not wm.density_ok(w[1:])]
    assert {w[1] for _, w in ok} == {c for c in wm.COL0 if c % 32 == 0 and c < cols}
    assert no and all(w[1] % 32 for w in no) and {w[1] for w in no} >= {c for c in wm.COL0 if c % 32 and c < cols}
    assert {wm.tile_plan(i) for i, _ in ok} == set(wm.TILES)
    assert {wm.tile_plan(i) for i in range(6)} == set(wm.TILES)            # the async pass: one per row class
    assert {wm.fill_plan(i)[1] for i in range(len(order))} == set(wm.THRESHOLDS)
    seam_rows = wm.seams(rows)
    tiled = [(w, wm.tile_plan(i)) for i, w in ok]
    assert any(tr == 1 and nr > 1 for (_, _, nr, _), (tr, _) in tiled)                       # a 1-row tile
    assert any(nr > tr and nr % tr for (_, _, nr, _), (tr, _) in tiled)                      # a clipped last tile row
    assert any(nc > tc and nc % tc for (_, _, _, nc), (_, tc) in tiled)                      # ... and tile column
    assert any(tc > nc for (_, _, _, nc), (_, tc) in tiled)                             # a tile wider than its window
    # a tile row with rows of two slabs in it, and a slab seam on a tile seam's wrong side
    assert any(tr > 1 and (s - r0) % tr and r0 < s < r0 + nr for (r0, _, nr, _), (tr, _) in tiled for s in seam_rows)
    # the tiling the digests are added over: it covers the board, at least 3 of its pieces are list windows
    t = wm.tiling(wins, rows, cols)
    body = {w[1:] for w in wins}
    assert [w[1] for w, _ in t] == [0] + [w[1] + w[3] for w, _ in t[:-1]] and t[-1][0][1] + t[-1][0][3] == cols
    assert all(w[0] == 0 and w[2] == rows for w, _ in t) and all((w in body) == listed for w, listed in t)
    assert sum(listed for _, listed in t) >= 3 and all(listed for _, listed in t[:-1])


@pytest.mark.parametrize("slabs", wm.SLABS)
@pytest.mark.parametrize("rows,cols,m", BOARDS)
def test_copy_plan(rows, cols, m, slabs):
    _, order = _ordered(rows, cols, m)
    plan = list(zip([w[1:] for w in order], wm.copy_plan(order, rows, cols, slabs)))
    assert plan == list(zip([w[1:] for w in order], wm.copy_plan(order, rows, cols, slabs))) and len(plan) == len(order)
    fits, shifts, ops = set(), set(), {op: 0 for op in wm.OPS}
    for (row0, col0, nrows, ncols), (sources, srow0, scol0, op) in plan:
        assert sources == ("same", "foreign")
        assert 0 <= srow0 <= rows - nrows and 0 <= scol0 <= cols - ncols
        assert slabs == 1 or srow0 == row0     # several slabs: source and destination line up slab for slab
        fits |= {s for s in wm.SHIFTS if 0 <= col0 + s <= cols - ncols}
        shifts.add(scol0 - col0)
        ops[op] += 1
    assert shifts >= fits and fits >= {0, 1, 31, 32, 33, -1, -31, -32, -33}, sorted(fits - shifts)
    assert cols < 131 or fits == set(wm.SHIFTS)
    assert all(5 * n >= len(plan) for n in ops.values()), ops
    assert any(scol0 == 0 and col0 for (_, col0, _, _), (_, _, scol0, _) in plan)
    assert any(scol0 + w[3] == cols and w[1] + w[3] < cols for w, (_, _, scol0, _) in plan)
    if slabs == 1:
        assert any(srow0 != w[0] for w, (_, srow0, _, _) in plan)
        assert {srow0 - w[0] for w, (_, srow0, _, _) in plan} >= {1, -1}
    # every op at a shift that is no multiple of 32, and at one that is (a copy of whole storage words)
    aligned = {(op, (scol0 - w[1]) % 32 == 0) for w, (_, _, scol0, op) in plan}
    assert aligned == {(op, a) for op in wm.OPS for a in (0, 1)}
    if m > 1:
        # a source window that crosses a block seam inside ONE destination run: the source runs then
        # start `off` > 0 columns into the destination run
        L, crossing = cols // m, 0
        for (_, col0, _, ncols), (_, _, scol0, _) in plan:
            a = col0
            while a < col0 + ncols:
                b = min(col0 + ncols, (a // L + 1) * L)
                lo, hi = a + scol0 - col0, b + scol0 - col0    # the run's source columns [lo, hi)
                crossing += any(lo < x < hi for x in range(L, cols, L))
                a = b
        assert crossing >= 10, crossing
