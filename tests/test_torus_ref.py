"""tests/torus_ref.py (the numpy torus stepper the GPU torus tests compare
against) pinned to the pinned oracle, not to the code under test.

A torus is its own infinite periodic tiling.  The centre tile of a 3x3 tiling
stepped with the oracle's DEAD boundary equals the torus as long as the error
of the tiling's clipped edge, which moves one cell per generation, has not
crossed the outer ring of tiles: g <= min(rows, cols), exactly.  Longer runs
take a (2t+1)^2 tiling, t = ceil(g / min(rows, cols))."""
import numpy as np
import pytest

import torus_ref
from oracle import golcpu as g


def centre_of_tiling(b, gens, t=1):
    r, c = b.shape
    return g.run_dead_fast(np.tile(b, (2 * t + 1, 2 * t + 1)), gens)[t * r:(t + 1) * r, t * c:(t + 1) * c]


@pytest.mark.parametrize("rows,cols", [(8, 8), (16, 37), (33, 16), (17, 17), (40, 130)])
def test_numpy_torus_equals_the_oracle_on_a_tiling(rows, cols):
    rng = np.random.default_rng(rows * 1000 + cols)
    b = (rng.random((rows, cols)) < 0.4).astype(np.uint8)
    m = min(rows, cols)
    for gens in (1, m // 2, m):
        assert (centre_of_tiling(b, gens) == torus_ref.run(b, gens)).all(), gens
    # past the 3x3 bound: a wider tiling
    gens = 2 * m + 3
    assert (centre_of_tiling(b, gens, t=-(-gens // m)) == torus_ref.run(b, gens)).all()


def test_glider_returns_on_the_torus_and_not_on_the_dead_board():
    b = torus_ref.glider(16, 16, 3, 5)
    # one cell diagonally per 4 generations: 64 generations = 16 cells = once around
    assert (torus_ref.run(b, 64) == b).all()
    assert int(torus_ref.run(b, 32).sum()) == 5
    assert not (g.run_dead_fast(b, 64) == b).all()
