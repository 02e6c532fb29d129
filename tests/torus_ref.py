"""A numpy reference for the periodic board (GOL_TORUS): B3/S23 with the
neighbour sum taken by np.roll, so row -1 is row rows-1 and column -1 is column
cols-1.  tests/test_torus_ref.py pins it to the pinned oracle (oracle/golcpu)."""
import numpy as np


def step(b: np.ndarray) -> np.ndarray:
    b = b.astype(np.uint8)
    n = np.zeros(b.shape, np.uint8)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if dr or dc:
                n += np.roll(np.roll(b, dr, 0), dc, 1)
    return ((n == 3) | ((b == 1) & (n == 2))).astype(np.uint8)


def run(b: np.ndarray, gens: int) -> np.ndarray:
    b = (np.asarray(b) != 0).astype(np.uint8)
    for _ in range(gens):
        b = step(b)
    return b


def glider(rows: int, cols: int, r0: int, c0: int) -> np.ndarray:
    """A glider (heading down-right, one cell diagonally every 4 generations)
    with its 3x3 box at (r0, c0), wrapped onto the rows x cols torus."""
    b = np.zeros((rows, cols), np.uint8)
    for dr, dc in ((0, 1), (1, 2), (2, 0), (2, 1), (2, 2)):
        b[(r0 + dr) % rows, (c0 + dc) % cols] = 1
    return b
