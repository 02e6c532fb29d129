"""Compiled life-like rules on the GPU: the rules of golhip.compiled_rules() on
the kernels compiled for them (bit_crule_kernel), bit-exact — boards and
popcounts — against tests/rule_ref.py and, where noted, against the same run
through the rule-generic kernel (OPT_RULE_KERNEL = 1).  Every run asserts
Engine.rule_path first: a dispatch that fell back to the generic kernel would
pass every parity check.

The pipeline, the strips and the EDGE split are the rule-generic kernel's, so
the shapes are tests/test_gpu_rule.py's (its docstring says what each is for):
 - the stage: every (alive, neighbours) pair must occur, so every reference run
   on a board of at least 41 x 130 cells is checked to visit all 18;
 - Replicator (B1357/S1357) is the list's B1 rule: a cell born outside the grid,
   in a pad column or in a row outside a slab's live rows feeds back into the
   board within one generation;
 - columns 64, 65, 127, 130, 4100 (two strips), 8100 (three); rows 41..70, and
   230 with 16-row chunks for the non-EDGE instantiation; depths 1..7, short
   blocks; 1, 2, 3 slabs, overlap, interior split; the torus' ghost columns.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import rule_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mpi_amd", "bin", "gol")

LISTED = ["B36/S23", "B3678/S34678", "B2/S", "B3/S012345678", "B1357/S1357", "B36/S125", "B3/S12345", "B37/S23",
          "B38/S23", "B35678/S5678", "B368/S245", "B4678/S35678"]
HIGHLIFE, DAYNIGHT, SEEDS, REPLICATOR = (rule_ref.parse(t) for t in ("B36/S23", "B3678/S34678", "B2/S", "B1357/S1357"))
UNLISTED = rule_ref.parse("B1/S8")


@pytest.fixture(scope="module")
def gh():
    from mpi_amd import golhip
    golhip.load()
    return golhip


@functools.lru_cache(maxsize=None)
def rand_board(rows, cols, seed=7):
    b = (np.random.default_rng(seed).random((rows, cols)) < 0.5).astype(np.uint8)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def reference(rows, cols, seed, rule, gens, torus):
    """rand_board(rows, cols, seed) after `gens` generations of `rule`; on boards of at least
    41 x 130 cells the run must have met all 18 (alive, neighbours) pairs."""
    b = rand_board(rows, cols, seed)
    if rows >= 41 and cols >= 130:
        seen = rule_ref.pairs_visited(b, gens, *rule, torus)
        assert len(seen) == 18, ((rows, cols), rule, sorted(seen))
    ref = rule_ref.run(b, gens, *rule, torus)
    ref.setflags(write=False)
    return ref


def run_gpu(gh, b, rule, steps, k, path, slabs=1, torus=False, options=()):
    rows, cols = b.shape
    with gh.Engine(rows, cols, n_gpus=slabs, layout="bit", boundary="torus" if torus else "dead", tblock_k=k,
                   rule=rule) as e:
        if path == "generic":
            e.set_option(gh.OPT_RULE_KERNEL, 1)
        for opt, v in options:
            e.set_option(opt, v)
        assert e.rule_path == path, (e.rule_path, path, rule, k)
        e.upload(b)
        for s in steps:
            e.step(s)
        assert e.rule_path == path
        return e.download(), e.popcount()


def check(gh, shape, seed, rule, steps, k, slabs=1, torus=False, options=(), generic=False):
    b = rand_board(*shape, seed)
    ref = reference(*shape, seed, rule, sum(steps), torus)
    for path in ("compiled", "generic") if generic else ("compiled",):
        got, live = run_gpu(gh, b, rule, steps, k, path, slabs, torus, options)
        rr, cc = np.nonzero(got != ref)
        assert rr.size == 0, (f"{path} {shape} rule={rule} k={k} slabs={slabs} torus={torus} steps={steps} "
                              f"options={options}: {rr.size} cells differ, columns {np.unique(cc)[:12]} "
                              f"rows {np.unique(rr)[:12]}")
        assert live == int(ref.sum()), (path, shape, rule, k, slabs, live, int(ref.sum()))


def test_the_list_is_the_one_the_tests_name(gh):
    assert [(b, s) for _, b, s in gh.compiled_rules()] == [rule_ref.parse(t) for t in LISTED]


# ------------------------------------------------------------------ rules x depths, one strip
@pytest.mark.parametrize("k", range(1, 8))
@pytest.mark.parametrize("text", LISTED)
def test_every_listed_rule_at_every_depth(gh, text, k):
    """compiled == generic == reference."""
    rule = rule_ref.parse(text)
    steps = [k, 2 * k + 3, 1]   # full blocks, a short last block, a single generation
    check(gh, (41 + 4 * k, 130), k, rule, steps, k, generic=True)
    check(gh, (41 + k, (64, 65, 127)[k % 3]), k, rule, steps, k, generic=True)


# ------------------------------------------------------------------ strips
@pytest.mark.parametrize("cols", [4100, 8100])
@pytest.mark.parametrize("rule", [HIGHLIFE, REPLICATOR, DAYNIGHT], ids=["highlife", "replicator", "daynight"])
def test_strips(gh, rule, cols):
    for k, rows in ((1, 41), (4, 57), (7, 70)):
        check(gh, (rows, cols), k, rule, [2 * k + 3], k)


# ------------------------------------------------------------------ EDGE beside non-EDGE
@pytest.mark.parametrize("k", [1, 2, 3, 5, 7])
@pytest.mark.parametrize("rule", [REPLICATOR, HIGHLIFE], ids=["replicator", "highlife"])
def test_short_chunks_run_the_interior_instantiation(gh, rule, k):
    """230 rows in 16-row chunks: chunks whose light cone stays inside the live rows, in
    strips whose words are all inside the grid, skip the column masks and the row checks."""
    steps = [k, k + 1] if k > 1 else [3]
    check(gh, (230, 4100), 40 + k, rule, steps, k, options=((gh.OPT_CHUNK_ROWS, 16),))
    check(gh, (230, 4100), 40 + k, rule, steps, k)   # the default chunk policy


# ------------------------------------------------------------------ slabs
@pytest.mark.parametrize("k", [1, 2, 5, 7])
@pytest.mark.parametrize("rule", [REPLICATOR, SEEDS], ids=["replicator", "seeds"])
def test_slabs(gh, rule, k):
    steps = [k, k - 1, 2 * k] if k > 1 else [3]
    for rows in (3 * k + 1, 41 + k, 6 * k + 41):   # thin (K <= H <= 2K with 2 or 3 slabs), uneven
        for slabs in (1, 2, 3):
            if slabs > 1 and rows // slabs < k:
                continue   # GOL_EINVAL: a slab holds at least K rows
            for overlap in (1, 0):
                check(gh, (rows, 130), rows, rule, steps, k, slabs, options=((gh.OPT_OVERLAP, overlap),))


@pytest.mark.parametrize("slabs", [1, 2])
@pytest.mark.parametrize("split", [1, 2])
def test_interior_split(gh, slabs, split):
    k = 3
    rows = slabs * (2 * 32 * k + 2 * k) + 3
    steps = [k, k - 1, 2 * k]
    check(gh, (rows, 130), rows, REPLICATOR, steps, k, slabs, options=((gh.OPT_INTERIOR_SPLIT, split),))
    check(gh, (rows, 130), rows, REPLICATOR, steps, k, slabs,
          options=((gh.OPT_INTERIOR_SPLIT, split), (gh.OPT_OVERLAP, 0)))
    with gh.Engine(rows, 130, n_gpus=slabs, layout="bit", tblock_k=k, rule=REPLICATOR) as e:
        e.set_option(gh.OPT_INTERIOR_SPLIT, split)
        assert e.rule_path == "compiled"
        e.upload(rand_board(rows, 130, rows))
        e.step(2 * k)
        e.sync()
        _, launches = e.kernel_time()
    assert launches == 2 * split * slabs   # `split` interior parts per slab and k-step


# ------------------------------------------------------------------ torus
@pytest.mark.parametrize("k", [1, 3, 4, 7])
@pytest.mark.parametrize("rule", [REPLICATOR, DAYNIGHT], ids=["replicator", "daynight"])
def test_torus_ghosts_at_every_group_position(gh, rule, k):
    steps = [k, 2 * k + 3, 1]
    for cols in sorted({k, 64 - k, 64, 65, 128 - k, 1000}):
        for slabs in (1, 3):
            check(gh, (41 + k, cols), cols + k, rule, steps, k, slabs, torus=True)


# ------------------------------------------------------------------ the rule changed in flight
@pytest.mark.parametrize("torus", [False, True])
@pytest.mark.parametrize("k", [1, 4, 7])
def test_rule_changed_between_steps(gh, k, torus):
    b = rand_board(47, 130, k)
    plan = [(rule_ref.LIFE, k + 2, "tuned"), (HIGHLIFE, 2 * k + 1, "compiled"), (UNLISTED, 3, "generic"),
            (SEEDS, k, "compiled"), (rule_ref.LIFE, 2, "tuned")]
    want, seen = b, set()
    for rule, gens, _ in plan:
        seen |= rule_ref.pairs_visited(want, gens, *rule, torus)
        want = rule_ref.run(want, gens, *rule, torus)
    assert len(seen) == 18
    with gh.Engine(47, 130, n_gpus=2, layout="bit", boundary="torus" if torus else "dead", tblock_k=k) as e:
        e.upload(b)
        for rule, gens, path in plan:
            e.set_rule(rule)
            assert e.rule == rule and e.rule_path == path
            e.step(gens)   # no sync in between: set_rule itself holds from the next step
        got, live = e.download(), e.popcount()
    assert (got == want).all() and live == int(want.sum())


# ------------------------------------------------------------------ the options, on a real device
@pytest.mark.parametrize("k", [2, 7])
def test_either_option_gives_the_generic_kernel_and_the_same_board(gh, k):
    shape, steps = (41 + 4 * k, 130), [k, 2 * k + 3, 1]
    b, ref = rand_board(*shape, k), reference(*shape, k, DAYNIGHT, sum(steps), False)
    for options, path in (((), "compiled"), (((gh.OPT_RULE_COMPILED, 0),), "generic"),
                          (((gh.OPT_RULE_KERNEL, 1),), "generic"),
                          (((gh.OPT_RULE_KERNEL, 1), (gh.OPT_RULE_COMPILED, 0)), "generic"),
                          (((gh.OPT_RULE_COMPILED, 0), (gh.OPT_RULE_COMPILED, 1)), "compiled")):
        with gh.Engine(*shape, layout="bit", tblock_k=k, rule=DAYNIGHT) as e:
            for opt, v in options:
                e.set_option(opt, v)
                assert e.get_option(opt) == v
            assert e.rule_path == path, (options, e.rule_path)
            e.upload(b)
            for s in steps:
                e.step(s)
            got, live = e.download(), e.popcount()
        assert (got == ref).all() and live == int(ref.sum()), options


@pytest.mark.parametrize("kw", [dict(layout="byte", tblock_k=4), dict(layout="bit", tblock_k=8),
                                dict(layout="bit", tblock_k=16), dict(layout="bit", boundary="serial_compat", tblock_k=4)])
def test_unsupported_contexts_refuse_listed_rules_and_stay_usable(gh, kw):
    from oracle import golcpu as g
    b = rand_board(64, 64, 5)
    with gh.Engine(64, 64, **kw) as e:
        e.upload(b)
        e.step(3)
        for text in ("B36/S23", "B1357/S1357"):
            with pytest.raises(gh.GolError) as ex:
                e.set_rule(text)
            assert ex.value.code == -5
        e.set_option(gh.OPT_RULE_COMPILED, 0)   # local state: accepted everywhere, and nothing changes
        e.set_option(gh.OPT_RULE_COMPILED, 1)
        assert e.rule_path == "tuned" and e.rule == rule_ref.LIFE
        e.step(6)
        got = e.download()
    mode = g.SERIAL_COMPAT if kw.get("boundary") == "serial_compat" else g.DEAD
    assert (got == g.run(b, 9, mode)).all()


# ------------------------------------------------------------------ driver
def test_driver_rule_kernel_switch_writes_identical_parts(gh, tmp_path):
    outs = {}
    for name, extra in (("auto", []), ("generic", ["--rule-kernel", "generic"])):
        d = tmp_path / name
        d.mkdir()
        subprocess.run([EXE, "--mode", "dead", "--rule", "B36/S23", "--save", "-k", "3"] + extra +
                       ["64", "96", "7", "14"], cwd=d, check=True, capture_output=True, text=True, timeout=120)
        # <date>_<generation>_<part>.gol: the parts, keyed without the run's date
        outs[name] = {f.split("_", 1)[1]: open(d / f, "rb").read() for f in sorted(os.listdir(d))
                      if f.endswith(".gol") and "_" in f}
    assert sorted(outs["auto"]) == ["0_0.gol", "14_0.gol", "7_0.gol"] and outs["auto"] == outs["generic"]
    with gh.Engine(64, 96, layout="bit", tblock_k=3, rule="B36/S23") as e:
        e.initialize_board("stream", 1)
        b0 = e.download()
        e.step(14)
        board = e.download()
    assert (board == rule_ref.run(b0, 14, *HIGHLIFE)).all()
    from oracle import golcpu as g
    assert outs["auto"]["14_0.gol"].endswith(g.text_body(board))
    r = subprocess.run([EXE, "--mode", "dead", "--rule", "B36/S23", "--rule-kernel", "fast", "64", "64", "4", "8"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--rule-kernel" in r.stdout + r.stderr
