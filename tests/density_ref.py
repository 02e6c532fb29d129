"""numpy reference of the density map (include/golhip.h, gol_density*): pad the
board to whole tiles, reshape, sum.  counts[i, j] = live cells of tile (i, j),
tiles of tile_rows × tile_cols cells counted from the board's (window's) origin,
the last tile row and tile column clipped.  An offset window is a slice of the
board: density_ref(board[r0:r0 + nr, c0:c0 + nc], th, tw)."""
import numpy as np


def density_dims(nrows, ncols, tile_rows, tile_cols):
    return -(-nrows // tile_rows), -(-ncols // tile_cols)


def density_ref(board, tile_rows, tile_cols=None):
    tile_cols = tile_rows if tile_cols is None else tile_cols
    b = (np.asarray(board) != 0)
    nrows, ncols = b.shape
    trows, tcols = density_dims(nrows, ncols, tile_rows, tile_cols)
    padded = np.zeros((trows * tile_rows, tcols * tile_cols), np.uint32)
    padded[:nrows, :ncols] = b
    return padded.reshape(trows, tile_rows, tcols, tile_cols).sum(axis=(1, 3), dtype=np.uint32)


def tile_cells(nrows, ncols, tile_rows, tile_cols):
    """Cells of every (clipped) tile: what a count is out of."""
    return density_ref(np.ones((nrows, ncols), np.uint8), tile_rows, tile_cols)
