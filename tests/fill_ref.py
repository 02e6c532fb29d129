"""numpy reference of the random fill (include/golhip.h, gol_fill_random*), word-level:

    sm = splitmix64's output function (digest_ref.sm), all arithmetic mod 2^64
    K        = sm(seed)
    h(r,w,j) = sm( sm(K + r) + 16*w + j )      r = global row, w = global column >> 5, j = 0..15
    plane 2j (r,w) = low 32 bits of h(r,w,j),  plane 2j+1 (r,w) = high 32 bits
    X(r,c)   = sum_i 2^i * bit (c & 31) of plane i (r, c >> 5)
    cell (r,c) is live  iff  X(r,c) < T        0 <= T <= 2^32

with GLOBAL coordinates: a window takes its origin (row0, col0) along.  Every plane
is computed and X is compared as a number: the plane skip and the bit-sliced
comparison of the device code are not used here.
"""
import numpy as np

from digest_ref import MASK, sm

FULL = 1 << 32


def fill_x(seed, nrows, ncols, row0=0, col0=0):
    """X(r, c) of the window as a uint64 array of shape (nrows, ncols)."""
    w0 = col0 >> 5
    nw = ((col0 + ncols - 1) >> 5) - w0 + 1 if ncols else 0
    with np.errstate(over="ignore"):
        K = sm(np.uint64(seed & MASK))
        R = sm(K + np.arange(row0, row0 + nrows, dtype=np.uint64))                       # (nrows,)
        base = R[:, None] + np.uint64(16) * np.arange(w0, w0 + nw, dtype=np.uint64)      # (nrows, nw)
        x = np.zeros((nrows, nw, 32), np.uint64)
        col = np.arange(32, dtype=np.uint64)
        for j in range(16):
            h = sm(base + np.uint64(j))
            lo, hi = h & np.uint64(0xFFFFFFFF), h >> np.uint64(32)
            x |= ((lo[:, :, None] >> col) & np.uint64(1)) << np.uint64(2 * j)
            x |= ((hi[:, :, None] >> col) & np.uint64(1)) << np.uint64(2 * j + 1)
    off = col0 - 32 * w0
    return x.reshape(nrows, nw * 32)[:, off:off + ncols]


def fill_ref(seed, threshold, nrows, ncols, row0=0, col0=0):
    """The 0/1 window (uint8) whose cell [0, 0] is global cell (row0, col0)."""
    assert 0 <= threshold <= FULL
    return (fill_x(seed, nrows, ncols, row0, col0) < np.uint64(threshold)).astype(np.uint8)


def fill_cells(seed, threshold, nrows, ncols, row0=0, col0=0):
    """The per-cell definition, in Python integers (slow: small boards only)."""
    def s(x):
        z = (x + 0x9E3779B97F4A7C15) & MASK
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        return z ^ (z >> 31)

    K = s(seed & MASK)
    out = np.zeros((nrows, ncols), np.uint8)
    for r in range(nrows):
        R = s((K + row0 + r) & MASK)
        for c in range(ncols):
            gc = col0 + c
            x = 0
            for i in range(32):
                h = s((R + 16 * (gc >> 5) + (i >> 1)) & MASK)
                plane = h >> 32 if i & 1 else h & 0xFFFFFFFF
                x |= ((plane >> (gc & 31)) & 1) << i
            out[r, c] = x < threshold
    return out


def threshold_of(p):
    """round(p * 2^32) as gol_fill_threshold computes it (llround: halves away from zero)."""
    return int(np.floor(p * 4294967296.0 + 0.5))
