"""The numpy reference of the board digest (tests/digest_ref.py): pinned to the
known answers of the digest's definition, checked against the per-cell loop, and
the properties the header documents (additivity, single-word differences)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digest_ref as dr  # noqa: E402


def _one(rows, cols, r, c):
    b = np.zeros((rows, cols), np.uint8)
    b[r, c] = 1
    return b


def test_splitmix_zero():
    assert int(dr.sm(np.uint64(0))) == 0xE220A8397B1DCDAF


def test_known_answers():
    assert dr.digest_ref(_one(5, 5, 0, 0)) == (0x30DFCFAC066B1A81, 0x8BD9E2C2A0C0ADAD)
    assert dr.digest_ref(_one(8, 100, 3, 70)) == (0xCE34D829B13D1840, 0xA18D6F5A3F8398C0)
    b = np.random.default_rng(1).random((37, 131)) < 0.33
    assert dr.digest_ref(b) == (0xAEDA039A1005E57F, 0x694F44CC75A22755)
    assert dr.digest_cells(b) == (0xAEDA039A1005E57F, 0x694F44CC75A22755)


def test_empty_board():
    assert dr.digest_ref(np.zeros((37, 131), np.uint8)) == (0, 0)
    assert dr.digest_ref(np.zeros((0, 5), np.uint8)) == (0, 0)


def test_against_per_cell_loop():
    rng = np.random.default_rng(7)
    for shape in ((1, 1), (9, 70), (37, 131), (64, 257), (3, 32), (5, 33)):
        b = (rng.random(shape) < 0.4).astype(np.uint8)
        assert dr.digest_ref(b) == dr.digest_cells(b), shape
        # a window away from the origin carries its global coordinates
        assert dr.digest_ref(b, 1000, 77) == dr.digest_cells(b, 1000, 77), shape


def test_additive_over_a_split_that_cuts_a_word():
    b = (np.random.default_rng(3).random((37, 131)) < 0.33).astype(np.uint8)
    tiles = [dr.digest_ref(b[0:10, 0:50], 0, 0), dr.digest_ref(b[0:10, 50:131], 0, 50),
             dr.digest_ref(b[10:37, :], 10, 0)]
    assert dr.add(*tiles) == dr.digest_ref(b)


def test_every_single_cell_flip_changes_both_lanes():
    b = (np.random.default_rng(5).random((9, 70)) < 0.5).astype(np.uint8)
    d = dr.digest_ref(b)
    for r in range(9):
        for c in range(70):
            f = b.copy()
            f[r, c] ^= 1
            e = dr.digest_ref(f)
            assert e[0] != d[0] and e[1] != d[1], (r, c)
