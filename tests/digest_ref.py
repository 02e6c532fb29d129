"""numpy reference of the board digest (include/golhip.h, gol_digest*), word-level:

    sm = splitmix64's output function, all arithmetic mod 2^64
    A_i(r) = sm(4r + i) | 1,  B_i(w) = sm(4w + 2 + i) | 1,  i = 0, 1
    digest_i = sum_r A_i(r) * sum_w B_i(w) * W(r, w)

with W(r, w) the row's canonical 32-column word (bit j = column 32w + j) and
GLOBAL coordinates: a window's digest takes its origin (row0, col0) along.
"""
import numpy as np

MASK = (1 << 64) - 1


def sm(x):
    """splitmix64 on a uint64 array (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        z = np.asarray(x, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def weights_a(i, r0, n):
    return sm(np.uint64(4) * np.arange(r0, r0 + n, dtype=np.uint64) + np.uint64(i)) | np.uint64(1)


def weights_b(i, w0, n):
    return sm(np.uint64(4) * np.arange(w0, w0 + n, dtype=np.uint64) + np.uint64(2 + i)) | np.uint64(1)


def digest_ref(board, row0=0, col0=0):
    """(lane 0, lane 1) of a 0/1 board whose cell [0, 0] is global cell (row0, col0)."""
    b = np.asarray(board) != 0
    nrows, ncols = b.shape
    if nrows == 0 or ncols == 0:
        return 0, 0
    w0, w1 = col0 >> 5, (col0 + ncols - 1) >> 5
    nw = w1 - w0 + 1
    lin = np.zeros((nrows, nw * 32), np.uint64)
    lin[:, col0 - 32 * w0: col0 - 32 * w0 + ncols] = b
    words = (lin.reshape(nrows, nw, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)
    out = []
    with np.errstate(over="ignore"):
        for i in (0, 1):
            rowsum = (words * weights_b(i, w0, nw)).sum(axis=1, dtype=np.uint64)
            out.append(int((rowsum * weights_a(i, row0, nrows)).sum(dtype=np.uint64)))
    return out[0], out[1]


def digest_cells(board, row0=0, col0=0):
    """The per-cell definition, in Python integers (slow: small boards only)."""
    def s(x):
        z = (x + 0x9E3779B97F4A7C15) & MASK
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        return z ^ (z >> 31)

    d = [0, 0]
    for r, c in zip(*np.nonzero(np.asarray(board))):
        gr, gc = int(r) + row0, int(c) + col0
        for i in (0, 1):
            d[i] = (d[i] + (s(4 * gr + i) | 1) * (s(4 * (gc >> 5) + 2 + i) | 1) * (1 << (gc & 31))) & MASK
    return d[0], d[1]


def add(*parts):
    """Sum of digests (of disjoint windows), mod 2^64 per lane."""
    return tuple(sum(p[i] for p in parts) & MASK for i in (0, 1))
