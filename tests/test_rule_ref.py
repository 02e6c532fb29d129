"""Pins tests/rule_ref.py, the reference of the life-like-rule tests: to the
pinned oracle and the torus reference at B3/S23, and to facts about other rules
that follow from the rules themselves."""
import numpy as np
import pytest

import rule_ref
import torus_ref
from oracle import golcpu as g


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (41, 130), (64, 64)])
def test_life_dead_equals_oracle(shape):
    b = (np.random.default_rng(3).random(shape) < 0.45).astype(np.uint8)
    for gens in (1, 2, 9):
        assert (rule_ref.run(b, gens, *rule_ref.LIFE) == g.run(b, gens, g.DEAD)).all()


@pytest.mark.parametrize("shape", [(3, 3), (5, 7), (41, 130)])
def test_life_torus_equals_torus_ref(shape):
    b = (np.random.default_rng(4).random(shape) < 0.45).astype(np.uint8)
    for gens in (1, 2, 9):
        assert (rule_ref.run(b, gens, *rule_ref.LIFE, torus=True) == torus_ref.run(b, gens)).all()


def test_parse():
    assert rule_ref.parse("B3/S23") == rule_ref.LIFE
    assert rule_ref.parse("b36/s23") == (0b1001000, 0b1100)
    assert rule_ref.parse("B2/S") == (0b100, 0)


REPLICATOR = ["..OOO", ".O..O", "O...O", "O..O.", "OOO.."]


def test_highlife_replicator():
    """HighLife (B36/S23): the replicator copies itself along its diagonal every 12
    generations, the copies cancelling like rule 90: 1, 2, 2, 4 replicators at
    generations 0, 12, 24, 36, each a translate of the first by a multiple of 2 cells along it
    (the population in between, from the first replicator alone, is recorded here)."""
    birth, survive = rule_ref.parse("B36/S23")
    rep = np.array([[ch == "O" for ch in row] for row in REPLICATOR], np.uint8)
    assert rep.sum() == 12
    n = 81
    b = np.zeros((n, n), np.uint8)
    b[38:43, 38:43] = rep

    def copies(shifts):
        want = np.zeros_like(b)
        for s in shifts:   # the copy 2·s cells down the main diagonal
            want[38 + 2 * s:43 + 2 * s, 38 + 2 * s:43 + 2 * s] ^= rep
        return want

    pops = [int(rule_ref.run(b, t, birth, survive).sum()) for t in range(13)]
    assert pops == [12, 20, 17, 30, 20, 28, 34, 38, 26, 17, 16, 22, 24]
    assert (rule_ref.run(b, 12, birth, survive) == copies([-1, 1])).all()
    assert (rule_ref.run(b, 24, birth, survive) == copies([-2, 2])).all()
    assert (rule_ref.run(b, 36, birth, survive) == copies([-3, -1, 1, 3])).all()
    # ... and in Life itself the same cells do nothing of the kind
    assert not (rule_ref.run(b, 12, *rule_ref.LIFE) == copies([-1, 1])).all()


def test_seeds_domino():
    """Seeds (B2/S): every live cell dies; a dead cell with exactly two live neighbours is
    born.  A domino's only such cells are the two above and the two below it."""
    birth, survive = rule_ref.parse("B2/S")
    b = np.zeros((7, 8), np.uint8)
    b[3, 3] = b[3, 4] = 1
    want = np.zeros_like(b)
    want[2, 3] = want[2, 4] = want[4, 3] = want[4, 4] = 1
    assert (rule_ref.run(b, 1, birth, survive) == want).all()
    # at the edge of a dead-boundary board the row outside stays dead: only the pair inside is born
    e = np.zeros((3, 6), np.uint8)
    e[0, 2] = e[0, 3] = 1
    want = np.zeros_like(e)
    want[1, 2] = want[1, 3] = 1
    assert (rule_ref.run(e, 1, birth, survive) == want).all()
    # on a torus of 3 rows the pair above wraps to the last row
    want[2, 2] = want[2, 3] = 1
    assert (rule_ref.run(e, 1, birth, survive, torus=True) == want).all()


@pytest.mark.parametrize("torus", [False, True])
def test_fredkin_replicates_a_single_cell(torus):
    """B1357/S1357: a cell is alive next iff it has an odd number of live neighbours — linear
    over GF(2), so after 2^j generations any pattern is the XOR of its 8 translates by 2^j."""
    birth, survive = rule_ref.parse("B1357/S1357")
    b = np.zeros((33, 35), np.uint8)
    b[16, 17] = 1
    for t in (1, 2, 4, 8):
        want = np.zeros_like(b)
        for dr in (-t, 0, t):
            for dc in (-t, 0, t):
                if dr or dc:
                    want[16 + dr, 17 + dc] ^= 1
        assert (rule_ref.run(b, t, birth, survive, torus=torus) == want).all()


def test_pairs_visited_sees_all_18_on_a_random_board():
    b = (np.random.default_rng(7).random((41, 130)) < 0.5).astype(np.uint8)
    for rule in ("B3/S23", "B1/S8", "B2/S"):
        for torus in (False, True):
            assert len(rule_ref.pairs_visited(b, 3, *rule_ref.parse(rule), torus=torus)) == 18
