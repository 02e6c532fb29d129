"""A numpy reference for life-like (outer-totalistic, B/S notation) rules on a
dead-boundary or periodic board.  Bit n of `birth`: a dead cell with n live
neighbours (of 8) is born; bit n of `survive`: a live cell with n live
neighbours stays alive.  Outside a dead-boundary board every cell is dead at
every generation (it does not evolve).  tests/test_rule_ref.py pins it to the
pinned oracle (oracle/golcpu), to tests/torus_ref.py and to hand-checked facts."""
import numpy as np

LIFE = (1 << 3, (1 << 2) | (1 << 3))


def parse(text: str) -> tuple[int, int]:
    """(birth, survive) of "B36/S23" (this file's own reading, letters first form only)."""
    b, s = text.upper().split("/")
    assert b[0] == "B" and s[0] == "S", text
    return sum(1 << int(d) for d in b[1:]), sum(1 << int(d) for d in s[1:])


def neighbours(b: np.ndarray, torus: bool) -> np.ndarray:
    p = b if torus else np.pad(b, 1)
    n = np.zeros(p.shape, np.uint8)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if dr or dc:
                n += np.roll(np.roll(p, dr, 0), dc, 1)
    return n if torus else n[1:-1, 1:-1]


def step(b: np.ndarray, birth: int, survive: int, torus: bool = False) -> np.ndarray:
    n = neighbours(b, torus).astype(np.uint32)
    return np.where(b == 1, (np.uint32(survive) >> n) & 1, (np.uint32(birth) >> n) & 1).astype(np.uint8)


def run(board: np.ndarray, gens: int, birth: int, survive: int, torus: bool = False) -> np.ndarray:
    b = (np.asarray(board) != 0).astype(np.uint8)
    for _ in range(gens):
        b = step(b, birth, survive, torus)
    return b


def pairs_visited(board: np.ndarray, gens: int, birth: int, survive: int, torus: bool = False) -> set:
    """The (alive, neighbours) pairs that occur while `board` runs `gens` generations."""
    b = (np.asarray(board) != 0).astype(np.uint8)
    seen = set()
    for _ in range(gens):
        n = neighbours(b, torus)
        seen |= {(int(v) // 9, int(v) % 9) for v in np.unique(b.astype(np.int32) * 9 + n)}
        b = step(b, birth, survive, torus)
    return seen
