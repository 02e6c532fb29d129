"""A numpy model of the logical board behind the byte-window and snapshot-text calls
(gol_upload_window, gol_download_window[_async], gol_format_text, gol_parse_text), the
storage kinds they are swept over and the deterministic window list of the sweep
(tests/test_gpu_window_io.py).  tests/test_window_model.py pins all of it on the CPU:
the GPU test cannot thin the list without that test failing.

A model is a uint8 array of 0/1, shape (rows, cols), in LOGICAL coordinates: no ghost
column, column group, reversed mesh block or halo row exists here."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import torus_ref  # noqa: E402
from oracle import golcpu as g  # noqa: E402

MODE = {"dead": g.DEAD, "serial_compat": g.SERIAL_COMPAT, "mesh_compat": g.MESH_COMPAT}

# (layout, tblock_k, boundary, boards); a board is (rows, cols, mesh_m)
KINDS = [
    ("bit", 3, "dead", ((40, 300, 1),)),        # 2-word groups, ragged last word
    ("bit", 8, "dead", ((40, 300, 1),)),        # 4-word groups
    ("bit", 32, "dead", ((100, 300, 1),)),      # halo depth 32 in the storage row offset
    ("byte", 1, "dead", ((40, 300, 1),)),
    ("byte", 16, "dead", ((52, 300, 1),)),
    ("bit", 3, "torus", ((40, 300, 1),)),       # ghost margin 3: every group is misaligned against logical columns
    ("bit", 8, "torus", ((40, 131, 1),)),
    ("bit", 32, "torus", ((100, 131, 1),)),
    ("byte", 5, "torus", ((40, 131, 1),)),      # ghosts off a dword boundary
    ("bit", 2, "serial_compat", ((37, 37, 1), (40, 300, 1))),    # active_cols
    ("byte", 2, "serial_compat", ((37, 37, 1), (40, 300, 1))),   # enforce_inactive
    ("bit", 2, "mesh_compat", ((96, 96, 3), (48, 48, 4))),       # reversed column blocks of 32 and of 12 columns
    ("bit", 8, "mesh_compat", ((96, 96, 3), (48, 48, 4))),
    ("byte", 2, "mesh_compat", ((96, 96, 3), (48, 48, 4))),
]

COL0 = (0, 1, 31, 32, 33, 63, 64, 65, 95, 127, 128, 129)
NCOLS = (1, 2, 31, 32, 33, 63, 64, 65, 97, 128, 129, None)   # None: to the last column
SLABS = (1, 3)


def kind_id(kind):
    return f"{kind[0]}-k{kind[1]}-{kind[2]}"


def seams(rows, world=3):
    """First rows of slabs 1 .. world-1 of the library's slab plan (host only)."""
    from mpi_amd import golhip
    return [golhip.slab_plan(rows, world, r)[0] for r in range(1, world)]


def slab_counts(rows, k):
    """The slab counts a board of `rows` rows is swept at: 3 slabs only where each holds
    tblock_k rows (thinner slabs are GOL_EINVAL by contract)."""
    return [n for n in SLABS if n == 1 or rows // n >= k]


def soup(seed, rows, cols, p=0.4):
    return (np.random.default_rng(seed).random((rows, cols)) < p).astype(np.uint8)


# ------------------------------------------------------------------ the model
def write(model, row0, col0, cells, boundary):
    """The window's cells replace the model's (any nonzero byte is a live cell);
    SERIAL_COMPAT keeps its last row and column dead."""
    cells = np.asarray(cells)
    model[row0:row0 + cells.shape[0], col0:col0 + cells.shape[1]] = cells != 0
    if boundary == "serial_compat":
        model[-1, :] = 0
        model[:, -1] = 0
    return model


def text(cells):
    """The `.gol` part-file body of a window: "0\\t" or "1\\t" per cell, "\\n" per row."""
    return b"".join(b"".join(b"1\t" if v else b"0\t" for v in row) + b"\n" for row in np.asarray(cells))


def step(model, gens, boundary, mesh_m=1):
    if boundary == "torus":
        return torus_ref.run(model, gens)
    return g.run(model, gens, MODE[boundary], mesh_m)


# ------------------------------------------------------------------ the window list
def row_classes(rows, seam_rows):
    """The row ranges the column windows rotate through: all rows, 5 rows from row 13,
    the two rows either side of each slab seam, the last row alone."""
    return [(0, rows), (13, 5)] + [(s - 2, 4) for s in seam_rows] + [(rows - 1, 1)]


def mesh_seam_windows(n, m):
    """The three block-seam windows of test_gpu_bits.py::test_mesh_compat_rows_are_in_logical_columns."""
    return [(5, col0, 20, nc) for col0, nc in ((5, n // m + 9), (n // m - 3, 7), (1, n - 2))]


def windows(rows, cols, seam_rows, mesh_m=1):
    """[(cls, row0, col0, nrows, ncols)]: COL0 x NCOLS clipped to the board (empty and
    repeated results dropped), each paired with the next of row_classes (cls: its index);
    then, as class len(row_classes), the whole board, cell (0, 0), the last cell and, on
    mesh boards, the block-seam windows."""
    classes = row_classes(rows, seam_rows)
    out, seen, n = [], set(), 0
    for col0 in COL0:
        for nc in NCOLS:
            cls = n % len(classes)
            n += 1
            nc = cols - col0 if nc is None else min(nc, cols - col0)
            if nc <= 0:
                continue
            row0, nrows = classes[cls]
            w = (row0, col0, nrows, nc)
            if w not in seen:
                seen.add(w)
                out.append((cls,) + w)
    extra = [(0, 0, rows, cols), (0, 0, 1, 1), (rows - 1, cols - 1, 1, 1)]
    if mesh_m > 1:
        extra += mesh_seam_windows(cols, mesh_m)
    for w in extra:
        if w not in seen:
            seen.add(w)
            out.append((len(classes),) + w)
    return out
