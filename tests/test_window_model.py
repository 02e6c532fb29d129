"""tests/window_model.py pinned on the CPU: the model's text against the oracle's, its
stepper against the reference's own boards (tests/golden), and the properties of the
window list that tests/test_gpu_window_io.py sweeps, for every board of its kinds table
— the residue classes of both window edges, the 1-cell, 1-row and 1-column windows, the
slab-seam crossings, the last row and column.  The GPU test takes its windows from the
same helper, so it cannot thin them without this file failing."""
import os
import sys

import numpy as np
import pytest

from oracle import golcpu as g

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torus_ref  # noqa: E402
import window_model as wm  # noqa: E402

BOARDS = sorted({b for kind in wm.KINDS for b in kind[3]})


def test_kinds_table():
    assert len(wm.KINDS) == 14 and len({wm.kind_id(k) for k in wm.KINDS}) == 14
    assert BOARDS == [(37, 37, 1), (40, 131, 1), (40, 300, 1), (48, 48, 4), (52, 300, 1), (96, 96, 3),
                      (100, 131, 1), (100, 300, 1)]
    assert {k[2] for k in wm.KINDS} == {"dead", "torus", "serial_compat", "mesh_compat"}
    # bit layout: 2-word groups (k < 8) and 4-word groups (k >= 8) under every boundary that has both
    for boundary in ("dead", "torus", "mesh_compat"):
        depths = [k for layout, k, b, _ in wm.KINDS if layout == "bit" and b == boundary]
        assert min(depths) < 8 <= max(depths), boundary
        assert any(layout == "byte" and b == boundary for layout, _, b, _ in wm.KINDS)


def test_three_slab_pass_drops_no_kind():
    """A slab thinner than tblock_k is GOL_EINVAL; the table's boards are tall enough that the
    3-slab pass runs for every kind (100 rows at k = 32, 52 at k = 16)."""
    dropped = [(wm.kind_id(kind), rows) for kind in wm.KINDS for rows, _, _ in kind[3]
               if wm.slab_counts(rows, kind[1]) != [1, 3]]
    assert dropped == []
    assert wm.slab_counts(40, 16) == [1] and wm.slab_counts(48, 16) == [1, 3]


def test_text_is_the_oracles_text_body():
    for shape in ((1, 1), (1, 7), (5, 1), (13, 33)):
        b = wm.soup(shape[0] * 100 + shape[1], *shape)
        assert wm.text(b) == g.text_body(b), shape
    assert wm.text(np.array([[0, 1], [1, 0]], np.uint8)) == b"0\t1\t\n1\t0\t\n"


def test_write():
    m = np.zeros((5, 6), np.uint8)
    wm.write(m, 1, 2, np.array([[1, 0], [2, 0x80], [0xFF, 0]], np.uint8), "dead")
    want = np.zeros((5, 6), np.uint8)
    want[1, 2] = want[2, 2] = want[2, 3] = want[3, 2] = 1
    assert (m == want).all() and m.dtype == np.uint8
    s = np.zeros((5, 6), np.uint8)
    wm.write(s, 2, 3, np.ones((3, 3), np.uint8), "serial_compat")
    want = np.zeros((5, 6), np.uint8)
    want[2:4, 3:5] = 1
    assert (s == want).all()


def _golden_small(golden):
    d, cases = golden
    for name, case in sorted(cases.items()):
        if "all" not in case["files"]:
            continue
        n, bpb = case["n"], case["bytes_per_board"]
        blob = open(os.path.join(d, case["files"]["all"]), "rb").read()
        yield name, case, [(gen, g.unpack(blob[i * bpb:(i + 1) * bpb], n, n)) for i, gen in enumerate(case["all_gens"])]


def test_step_matches_the_golden_small_cases(golden):
    seen = set()
    for name, case, boards in _golden_small(golden):
        seen.add(case["mode"])
        (gen0, cur), rest = boards[0], boards[1:]
        assert rest, name
        for gen, want in rest:
            cur, gen0 = wm.step(cur, gen - gen0, case["mode"], case["mesh_m"]), gen
            assert (cur == want).all(), (name, gen)
    assert seen == {"dead", "serial_compat", "mesh_compat"}


def test_step_on_a_torus():
    b = torus_ref.glider(9, 11, 7, 9)    # its box wraps both edges
    assert (wm.step(b, 4, "torus") == torus_ref.glider(9, 11, 8, 10)).all()
    s = wm.soup(3, 12, 17)
    assert (wm.step(s, 3, "torus") == torus_ref.run(s, 3)).all()
    assert (wm.step(s, 3, "torus") != wm.step(s, 3, "dead")).any()


@pytest.mark.parametrize("rows,cols,m", BOARDS)
def test_window_list(rows, cols, m):
    seam_rows = wm.seams(rows)
    assert len(seam_rows) == 2 and 2 <= seam_rows[0] < seam_rows[1] <= rows - 2
    wins = wm.windows(rows, cols, seam_rows, m)
    body = [w[1:] for w in wins]
    assert len(set(body)) == len(body)
    classes = wm.row_classes(rows, seam_rows)
    assert len(classes) == 5 and all(0 <= r0 and r0 + nr <= rows and nr >= 1 for r0, nr in classes)
    for cls, row0, col0, nrows, ncols in wins:
        assert 0 <= row0 and 0 <= col0 and nrows >= 1 and ncols >= 1, (row0, col0, nrows, ncols)
        assert row0 + nrows <= rows and col0 + ncols <= cols, (row0, col0, nrows, ncols)
        assert 0 <= cls <= len(classes) and (cls == len(classes) or (row0, nrows) == classes[cls])
    # every row class holds windows (the async check keeps one class pending at a time)
    assert {w[0] for w in wins} == set(range(len(classes) + 1))
    # every col0 of the list that lies on the board, and every width that fits somewhere, occurs
    assert {w[2] for w in wins if w[0] < len(classes)} == {c for c in wm.COL0 if c < cols}
    assert {w[4] for w in wins} >= {n for n in wm.NCOLS if n is not None and n <= cols}
    # ... and so does every residue class of both edges that the list reaches on this board
    starts, ends = {w[2] % 32 for w in wins}, {(w[2] + w[4]) % 32 for w in wins}
    assert starts >= {c % 32 for c in wm.COL0 if c < cols}
    assert ends >= {(c + n) % 32 for c in wm.COL0 for n in wm.NCOLS if n is not None and c + n <= cols} | {cols % 32}
    if cols >= 131:
        assert starts >= {0, 1, 31} and ends >= {0, 1, 2, 3, 30, 31}
        # both sides of the 64-column (2-word) and 128-column (4-word) group seams
        assert {w[2] for w in wins} >= {63, 64, 65, 127, 128, 129}
    else:
        assert starts >= {0, 1, 31} and ends >= {0, 1, 2}
    # a window inside one word, one crossing a word seam and one crossing a 128-column group seam
    assert any(c0 // 32 == (c0 + nc - 1) // 32 and nc > 1 for _, _, c0, _, nc in wins)
    assert any(c0 // 32 != (c0 + nc - 1) // 32 for _, _, c0, _, nc in wins)
    assert cols < 131 or any(c0 // 128 != (c0 + nc - 1) // 128 and c0 % 32 for _, _, c0, _, nc in wins)
    # the shapes
    assert (0, 0, 1, 1) in body and (rows - 1, cols - 1, 1, 1) in body and (0, 0, rows, cols) in body
    assert any(nr == 1 and nc > 1 for _, _, _, nr, nc in wins)          # a single row
    assert any(nc == 1 and nr == rows for _, _, _, nr, nc in wins)      # a single column, all rows
    assert any(nc == 1 and nr == 1 and c0 not in (0, cols - 1) for _, _, c0, nr, nc in wins)
    for s in seam_rows:   # a short window and a tall one across every slab seam
        assert any(r0 < s < r0 + nr and nr == 4 for _, r0, _, nr, _ in wins), s
        assert any(r0 < s < r0 + nr and nr == rows for _, r0, _, nr, _ in wins), s
    assert any(r0 < seam_rows[0] and r0 + nr > seam_rows[1] for _, r0, _, nr, _ in wins)
    assert sum(c0 + nc == cols for _, _, c0, _, nc in wins) >= len([c for c in wm.COL0 if c < cols])
    assert any(r0 + nr == rows and nr > 1 for _, r0, _, nr, _ in wins)
    assert any(r0 + nr == rows and c0 + nc == cols and c0 % 32 for _, r0, c0, nr, nc in wins)
    # a window that ends at the last column and holds its three rightmost columns (the pad-bit write)
    assert any(c0 + nc == cols and nc >= 3 for _, _, c0, _, nc in wins)
    # mesh boards: the block-seam windows, and runs on both sides of every block seam
    if m > 1:
        L = cols // m
        for w in wm.mesh_seam_windows(cols, m):
            assert w in body and w[1] + w[3] <= cols and w[0] + w[2] <= rows
        for seam in range(L, cols, L):
            assert any(c0 < seam < c0 + nc for _, _, c0, _, nc in wins), seam
        assert any((c0 + nc - 1) // L - c0 // L == m - 1 for _, _, c0, _, nc in wins)   # every block in one window
    assert len(wins) <= 12 * 12 + 6
