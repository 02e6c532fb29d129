"""Life-like rules (gol_set_rule) on the GPU: the rule-generic bit kernel,
bit-exact — boards and popcounts — against tests/rule_ref.py (the numpy
stepper that tests/test_rule_ref.py pins to the oracle).

What can go wrong, and what the shapes are chosen for:
 - the stage: every (alive, neighbours) pair must occur, so every reference run
   on a board of at least 41 x 130 cells is checked to visit all 18;
 - B1 rules (B1/S8, B1357/S1357): a cell born outside the grid, in a pad column
   or in a row outside a slab's live rows feeds back into the board within one
   generation — the column mask and the per-row validity of the EDGE path;
 - columns: 2-word groups, 64 columns per lane, strips of 64 lanes storing 62:
   64, 65, 127, 130, 4100 (two strips, ragged last word), 8100 (three strips);
 - rows: 41..70, and >= 200 with 16-row chunks so the non-EDGE instantiation
   runs beside the EDGE one;
 - depths 1..7, generation counts that are no multiple of K, a short block
   followed by a full one; 1, 2, 3 slabs (thin, uneven), overlap, interior
   split; the torus' ghost columns at every position of a group.
"""
import os
import subprocess

import numpy as np
import pytest

import rule_ref
from oracle import golcpu as g

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mpi_amd", "bin", "gol")

NAMED = ["B3/S23", "B36/S23", "B3678/S34678", "B2/S", "B1357/S1357", "B3/S012345678", "B1/S8", "B45678/S2345"]


def random_rules():
    rng = np.random.default_rng(2026)
    return [(int(rng.integers(0, 512)) & ~1, int(rng.integers(0, 512))) for _ in range(4)]


RULES = [rule_ref.parse(t) for t in NAMED] + random_rules()
IDS = NAMED + ["random%d" % i for i in range(4)]
SHARP = [rule_ref.parse(t) for t in ("B1/S8", "B1357/S1357", "B36/S23")]


@pytest.fixture(scope="module")
def gh():
    from mpi_amd import golhip
    golhip.load()
    return golhip


def rand_board(rows, cols, seed=7):
    return (np.random.default_rng(seed).random((rows, cols)) < 0.5).astype(np.uint8)


def reference(b, segments, torus):
    """The board after running `segments` = [(rule, generations), ...]; on boards of at
    least 41 x 130 cells the run must have met all 18 (alive, neighbours) pairs."""
    seen = set()
    for (birth, survive), gens in segments:
        if b.shape[0] >= 41 and b.shape[1] >= 130:
            seen |= rule_ref.pairs_visited(b, gens, birth, survive, torus)
        b = rule_ref.run(b, gens, birth, survive, torus)
    if seen or (b.shape[0] >= 41 and b.shape[1] >= 130):
        assert len(seen) == 18, (b.shape, segments, sorted(seen))
    return b


def run_gpu(gh, b, rule, steps, k, slabs=1, torus=False, options=(), rule_kernel=1):
    rows, cols = b.shape
    with gh.Engine(rows, cols, n_gpus=slabs, layout="bit", boundary="torus" if torus else "dead", tblock_k=k,
                   rule=rule) as e:
        e.set_option(gh.OPT_RULE_KERNEL, rule_kernel)
        for opt, v in options:
            e.set_option(opt, v)
        e.upload(b)
        for s in steps:
            e.step(s)
        return e.download(), e.popcount()


def check(gh, b, rule, steps, k, slabs=1, torus=False, options=(), ref=None):
    ref = reference(b, [(rule, sum(steps))], torus) if ref is None else ref
    got, live = run_gpu(gh, b, rule, steps, k, slabs, torus, options)
    rr, cc = np.nonzero(got != ref)
    assert rr.size == 0, (f"{b.shape} rule={rule} k={k} slabs={slabs} torus={torus} steps={steps} options={options}: "
                          f"{rr.size} cells differ, columns {np.unique(cc)[:12]} rows {np.unique(rr)[:12]}")
    assert live == int(ref.sum()), (b.shape, rule, k, slabs, live, int(ref.sum()))
    return ref


# ------------------------------------------------------------------ rules x depths, one strip
@pytest.mark.parametrize("rule", RULES, ids=IDS)
def test_every_rule_at_every_depth(gh, rule):
    for k in range(1, 8):
        steps = [k, 2 * k + 3, 1]   # full blocks, a short last block, a single generation
        check(gh, rand_board(41 + 4 * k, 130, k), rule, steps, k)
        check(gh, rand_board(41 + k, (64, 65, 127)[k % 3], k), rule, steps, k)
        if k >= 4:   # a short block followed by a full one
            check(gh, rand_board(50, 130, 20 + k), rule, [k - 3, k], k)


# ------------------------------------------------------------------ identity with the tuned kernels
@pytest.mark.parametrize("k", range(1, 8))
def test_life_through_the_generic_kernel_is_the_default_kernels_board(gh, k):
    b = rand_board(70, 4100, k)
    steps = [k, 2 * k + 3, 1]
    want = g.run(b, sum(steps), g.DEAD)
    tuned, live0 = run_gpu(gh, b, "B3/S23", steps, k, rule_kernel=0)
    generic, live1 = run_gpu(gh, b, "B3/S23", steps, k, rule_kernel=1)
    assert (tuned == want).all() and (generic == want).all() and (generic == tuned).all()
    assert live0 == live1 == int(want.sum())
    assert (want == reference(b, [(rule_ref.LIFE, sum(steps))], False)).all()


# ------------------------------------------------------------------ strips
@pytest.mark.parametrize("cols", [4100, 8100])
@pytest.mark.parametrize("rule", RULES[:8], ids=NAMED)
def test_strips(gh, rule, cols):
    for k, rows in ((1, 41), (4, 57), (7, 70)):
        check(gh, rand_board(rows, cols, k), rule, [2 * k + 3], k)


# ------------------------------------------------------------------ EDGE beside non-EDGE
@pytest.mark.parametrize("k", [1, 2, 3, 5, 7])
def test_short_chunks_run_the_interior_instantiation(gh, k):
    """230 rows in 16-row chunks: chunks whose light cone stays inside the live rows, in
    strips whose words are all inside the grid (the first of 4100 columns' two), skip the
    column masks and the row checks; their neighbours do not."""
    b = rand_board(230, 4100, 40 + k)
    for rule in SHARP:
        ref = check(gh, b, rule, [k, k + 1] if k > 1 else [3], k, options=[(gh.OPT_CHUNK_ROWS, 16)])
        check(gh, b, rule, [k, k + 1] if k > 1 else [3], k, ref=ref)   # the default chunk policy


# ------------------------------------------------------------------ slabs
@pytest.mark.parametrize("k", [1, 2, 5, 7])
def test_slabs(gh, k):
    steps = [k, k - 1, 2 * k] if k > 1 else [3]
    for rows in (3 * k + 1, 41 + k, 6 * k + 41):   # thin (K <= H <= 2K with 2 or 3 slabs), uneven
        b = rand_board(rows, 130, rows)
        for rule in SHARP:
            ref = None
            for slabs in (1, 2, 3):
                if slabs > 1 and rows // slabs < k:
                    continue   # GOL_EINVAL: a slab holds at least K rows
                for overlap in (1, 0):
                    ref = check(gh, b, rule, steps, k, slabs, options=[(gh.OPT_OVERLAP, overlap)], ref=ref)


@pytest.mark.parametrize("slabs", [1, 2])
@pytest.mark.parametrize("split", [1, 2])
def test_interior_split(gh, slabs, split):
    k = 3
    rows = slabs * (2 * 32 * k + 2 * k) + 3
    b = rand_board(rows, 130, rows)
    rule = rule_ref.parse("B1/S8")
    ref = check(gh, b, rule, [k, k - 1, 2 * k], k, slabs, options=[(gh.OPT_INTERIOR_SPLIT, split)])
    check(gh, b, rule, [k, k - 1, 2 * k], k, slabs, torus=False, options=[(gh.OPT_INTERIOR_SPLIT, split),
                                                                          (gh.OPT_OVERLAP, 0)], ref=ref)
    with gh.Engine(rows, 130, n_gpus=slabs, layout="bit", tblock_k=k, rule=rule) as e:
        e.set_option(gh.OPT_INTERIOR_SPLIT, split)
        e.upload(b)
        e.step(2 * k)
        e.sync()
        _, launches = e.kernel_time()
    assert launches == 2 * split * slabs   # `split` interior parts per slab and k-step


# ------------------------------------------------------------------ torus
@pytest.mark.parametrize("rule", RULES[:8], ids=NAMED)
def test_torus_ghosts_at_every_group_position(gh, rule):
    for k in (1, 3, 4, 7):
        steps = [k, 2 * k + 3, 1]
        for cols in sorted({k, 64 - k, 64, 65, 128 - k, 1000}):
            b = rand_board(41 + k, cols, cols + k)
            ref = check(gh, b, rule, steps, k, 1, torus=True)
            check(gh, b, rule, steps, k, 3, torus=True, ref=ref)


@pytest.mark.parametrize("rule", SHARP)
def test_torus_wide(gh, rule):
    for k in (2, 7):
        check(gh, rand_board(44, 4100, k), rule, [k, k + 2], k, 3, torus=True)


# ------------------------------------------------------------------ the rule changed in flight
@pytest.mark.parametrize("torus", [False, True])
@pytest.mark.parametrize("k", [1, 4, 7])
def test_rule_changed_between_steps(gh, k, torus):
    b = rand_board(47, 130, k)
    life, fredkin, seeds = rule_ref.LIFE, rule_ref.parse("B1357/S1357"), rule_ref.parse("B2/S")
    plan = [(life, k + 2), (fredkin, 2 * k + 1), (life, 3), (seeds, k), (life, 2)]
    want = reference(b, plan, torus)
    with gh.Engine(47, 130, n_gpus=2, layout="bit", boundary="torus" if torus else "dead", tblock_k=k) as e:
        e.upload(b)
        for rule, gens in plan:
            e.set_rule(rule)
            assert e.rule == rule
            e.step(gens)   # no sync in between: set_rule itself holds from the next step
        got, live = e.download(), e.popcount()
    assert (got == want).all() and live == int(want.sum())


# ------------------------------------------------------------------ limits, on a real device
@pytest.mark.parametrize("kw", [dict(layout="byte", tblock_k=4), dict(layout="bit", tblock_k=8),
                                dict(layout="bit", tblock_k=16), dict(layout="bit", boundary="serial_compat", tblock_k=4)])
def test_unsupported_contexts_refuse_and_stay_usable(gh, kw):
    b = rand_board(64, 64, 5)
    with gh.Engine(64, 64, **kw) as e:
        e.upload(b)
        e.step(3)
        for call in (lambda: e.set_rule("B36/S23"), lambda: e.set_option(gh.OPT_RULE_KERNEL, 1)):
            with pytest.raises(gh.GolError) as ex:
                call()
            assert ex.value.code == -5
        e.set_rule("B3/S23")
        e.step(6)
        got = e.download()
    mode = g.SERIAL_COMPAT if kw.get("boundary") == "serial_compat" else g.DEAD
    assert (got == g.run(b, 9, mode)).all()


# ------------------------------------------------------------------ driver
@pytest.mark.parametrize("mode,extra", [("dead", ["-k", "3"]), ("torus", ["-k", "5", "--gpus", "2"])])
def test_driver_rule_against_the_binding(gh, tmp_path, mode, extra):
    rows, cols = 64, 96
    subprocess.run([EXE, "--mode", mode, "--rule", "B36/S23", "--save"] + extra + [str(rows), str(cols), "7", "14"],
                   cwd=tmp_path, check=True, capture_output=True, text=True, timeout=120)
    name = [f for f in os.listdir(tmp_path) if f.endswith(".gol") and "_" not in f][0][:-4]
    parts = 2 if "--gpus" in extra else 1
    k = int(extra[1])
    with gh.Engine(rows, cols, layout="bit", boundary=mode, tblock_k=k, rule="B36/S23") as e:
        e.initialize_board("stream", 1)
        b0 = e.download()
        for it in (0, 7, 14):
            if it:
                e.step(7)
            board = e.download()
            assert (board == rule_ref.run(b0, it, *rule_ref.parse("B36/S23"), torus=mode == "torus")).all()
            for p in range(parts):
                path = tmp_path / f"{name}_{it}_{p}.gol"
                r0, c0, nr, nc, off = gh.part_geometry(str(path))
                assert open(path, "rb").read()[off:] == g.text_body(board[r0:r0 + nr, c0:c0 + nc]), (it, p)


@pytest.mark.parametrize("args,names", [(["--mode", "serial"], "--mode dead or torus"),
                                        (["--mode", "dead", "--layout", "byte"], "--layout bit"),
                                        (["--mode", "dead", "-k", "8"], "tblock_k = 1 .. 7"),
                                        (["--mode", "dead", "--rule", "B3S23"], "B/S notation")])
def test_driver_names_the_limit(tmp_path, args, names):
    r = subprocess.run([EXE, "--rule", "B36/S23"] + args + ["64", "64", "4", "8"], cwd=tmp_path, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and names in r.stdout + r.stderr, r.stdout + r.stderr
