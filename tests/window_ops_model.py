"""The numpy model of the device-side window calls (gol_download_bits_window[_async],
gol_upload_bits_window, gol_digest_window, gol_density_window, gol_fill_random_window,
gol_copy_window) on top of tests/window_model.py, whose names (KINDS, windows, write,
step, text, ...) are all available here unchanged, and the plan tables of their sweep
(tests/window_ops_sweep.py): tiles, thresholds, column shifts, copy sources.
tests/test_window_ops_model.py pins all of it on the CPU: the GPU test cannot thin a
table without that test failing.

A model is a uint8 array of 0/1, shape (rows, cols), in LOGICAL coordinates; a window w
is (row0, col0, nrows, ncols)."""
import numpy as np

from window_model import *  # noqa: F401,F403  (sys.path: tests/ and the repository root, set there too)
from window_model import KINDS, write

import density_ref
import digest_ref
import fill_ref

# ------------------------------------------------------------------ the device-side window calls
# (gol_download_bits_window / gol_upload_bits_window, gol_digest_window, gol_density_window,
# gol_fill_random_window, gol_copy_window); a window w is (row0, col0, nrows, ncols)
OPS = ("replace", "or", "xor")


def cut(model, w):
    row0, col0, nrows, ncols = w
    return model[row0:row0 + nrows, col0:col0 + ncols]


def bits(cells):
    """The packed rows of a window: ceil(ncols / 8) bytes per row, MSB first, pad bits 0."""
    return np.packbits(np.asarray(cells) != 0, axis=1)


def digest(model, w):
    return digest_ref.digest_ref(cut(model, w), w[0], w[1])


def density(model, w, tile_rows, tile_cols):
    return density_ref.density_ref(cut(model, w), tile_rows, tile_cols)


def fill(model, w, seed, T, boundary):
    """gol_fill_random_window: the window's cells take the formula on their global coordinates."""
    return write(model, w[0], w[1], fill_ref.fill_ref(seed, T, w[2], w[3], w[0], w[1]), boundary)


def merge(dst_model, dw, src_model, sw, op, boundary):
    """gol_copy_window: window dw of dst becomes op(itself, the window of dw's size at sw[:2] of src)."""
    old = cut(dst_model, dw)
    src = cut(src_model, (sw[0], sw[1], dw[2], dw[3]))
    assert src.shape == old.shape == (dw[2], dw[3]), (dw, sw)
    new = {"replace": src, "or": old | src, "xor": old ^ src}[op]
    return write(dst_model, dw[0], dw[1], new, boundary)


# the plan tables of the sweep
TILES = ((1, 32), (3, 64), (7, 96), (16, 128), (64, 1024))   # (tile_rows, tile_cols)
THRESHOLDS = (0, 1 << 32, 1 << 31, 3 << 29, 0x55555555, 1)   # none, all, one plane, three planes, all 32 planes, 2^-32
SHIFTS = (0, 1, 31, 32, 33, 97, -1, -31, -32, -33, -97)      # source column - destination column
ROW_SHIFTS = (0, 1, -1, 7, -9)
FOREIGN = (("bit", 3, "dead"), ("bit", 8, "torus"), ("byte", 5, "torus"), ("byte", 1, "dead"))
SOURCES = ("same", "foreign")


def storage_form(layout, k):
    return "byte" if layout == "byte" else "bit4" if k >= 8 else "bit2"


def foreign_kind(ki):
    """(layout, tblock_k, boundary) of the foreign copy source of KINDS[ki]: FOREIGN in rotation,
    skipping the entries of the destination's own storage form."""
    own = storage_form(*KINDS[ki][:2])
    return next(f for f in (FOREIGN[(ki + j) % len(FOREIGN)] for j in range(len(FOREIGN)))
                if storage_form(*f[:2]) != own)


def tile_plan(i):
    return TILES[i % len(TILES)]


def fill_plan(i):
    """(seed, threshold) of the fill at window i."""
    return 0x9000 + 7 * i, THRESHOLDS[i % len(THRESHOLDS)]


def density_ok(w):
    """gol_density_window takes col0 at a multiple of 32 only; the other windows are refusals."""
    return w[1] % 32 == 0


def copy_plan(order, rows, cols, slabs):
    """[(sources, srow0, scol0, op)]: for every window of `order` (the list as the writers take
    it) the sources to copy from in turn, the source window's corner and the op.  The column
    shift is the entry of SHIFTS used least so far among those that keep the source window on
    the board (0 always does; ties go round the table), so the large shifts are reached on
    the 37- and 48-column boards too, where they fit four or five windows only; every eighth
    window has its source flush against the last column or column 0 instead, at whatever
    shift that takes.  Rows shift in one slab only (several slabs line up slab for slab);
    the op rotates."""
    used = {s: 0 for s in SHIFTS}
    out = []
    for i, (_, row0, col0, nrows, ncols) in enumerate(order):
        if i % 8 == 7:
            scol0 = 0 if (i // 8) % 2 else cols - ncols
        else:
            fitting = [s for s in SHIFTS if 0 <= col0 + s <= cols - ncols]
            s = min(fitting, key=lambda s: (used[s], (SHIFTS.index(s) - i) % len(SHIFTS)))
            used[s] += 1
            scol0 = col0 + s
        srow0 = row0
        if slabs == 1:
            srow0 = (row0 + ROW_SHIFTS[(i // 3) % len(ROW_SHIFTS)]) % (rows - nrows + 1)
        out.append((SOURCES, srow0, scol0, OPS[i % len(OPS)]))
    return out


def tiling(wins, rows, cols):
    """[(w, listed)]: windows `rows` rows tall that tile the board side by side: from
    column 0 the narrowest window of the list that starts where the last one ended; where
    the list has none, the rest of the board closes the tiling (listed: False)."""
    tall = {}
    for _, row0, col0, nrows, ncols in wins:
        if row0 == 0 and nrows == rows and ncols < cols:
            tall[col0] = min(ncols, tall.get(col0, cols))
    out, c0 = [], 0
    while c0 < cols:
        nc, listed = (tall[c0], True) if c0 in tall else (cols - c0, False)
        out.append(((0, c0, rows, nc), listed))
        c0 += nc
    return out
