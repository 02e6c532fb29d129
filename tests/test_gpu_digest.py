"""gol_digest* on the GPU.  The master property: in every state of every context
digest() equals the reference digest (tests/digest_ref.py) of what download()
returns — every layout and group width, partial words and groups, the torus
ghost margin at shifts that are no multiple of 32, MESH_COMPAT's reversed
column blocks, SERIAL_COMPAT's dead last row and column, windows, slabs, rank
contexts — and therefore equal boards give equal digests whatever the
configuration that computed them."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from digest_ref import add, digest_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mpi_amd", "bin", "gol")
SHIM = os.path.join(ROOT, "tests", "shim", "libfake_rccl.so")
ESTATE = -6

BIT_BYTE_K = [("bit", 1), ("bit", 3), ("bit", 7), ("bit", 8), ("bit", 16), ("byte", 1), ("byte", 16)]


@pytest.fixture(scope="module")
def gh():
    from mpi_amd import golhip
    golhip.load()
    return golhip


def soup(seed, rows, cols, p=0.4):
    return (np.random.default_rng(seed).random((rows, cols)) < p).astype(np.uint8)


def same_as_download(e, what):
    got = e.download()
    d, want = e.digest(), digest_ref(got)
    assert d == want, f"{what}: digest {d[0]:016x}{d[1]:016x}, reference of the download {want[0]:016x}{want[1]:016x}"
    return got, d


def block_steps(k):
    return [k, max(1, k - 3), 1, k]   # both ping-pong buffers and a short block are read


# ------------------------------------------------------------------ layouts and shapes
@pytest.mark.parametrize("layout,k", BIT_BYTE_K)
def test_layouts_and_shapes(gh, layout, k):
    for rows, cols in ((37, 131), (8, 8), (64, 257), (100, 4096)):
        with gh.Engine(rows, cols, layout=layout, tblock_k=k) as e:
            assert e.digest() == (0, 0)   # the empty board
            e.upload(soup(rows + cols, rows, cols))
            got, d = same_as_download(e, (layout, k, rows, cols, 0))
            assert got.any() and d != (0, 0)
            for s in block_steps(k):
                e.step(s)
                same_as_download(e, (layout, k, rows, cols, e.generation))


def test_known_answers(gh):
    for layout, k in (("bit", 1), ("bit", 8), ("byte", 1)):
        with gh.Engine(37, 131, layout=layout, tblock_k=k) as e:
            e.upload(np.random.default_rng(1).random((37, 131)) < 0.33)
            assert e.digest() == (0xAEDA039A1005E57F, 0x694F44CC75A22755)
            b = np.zeros((37, 131), np.uint8)
            b[3, 70] = 1
            e.upload(b)
            assert e.digest() == (0xCE34D829B13D1840, 0xA18D6F5A3F8398C0)


# ------------------------------------------------------------------ boundaries
@pytest.mark.parametrize("layout,k", [("bit", 1), ("bit", 3), ("bit", 8), ("bit", 32), ("byte", 16), ("byte", 3)])
def test_torus_ghost_columns_are_not_counted(gh, layout, k):
    for rows, cols in ((64, 64), (40, 131)):
        with gh.Engine(rows, cols, layout=layout, boundary="torus", tblock_k=k) as e:
            # live cells in the first and last columns: their copies sit in the ghost margins
            b = soup(k, rows, cols)
            b[:, :2] = 1
            b[:, -2:] = 1
            e.upload(b)
            same_as_download(e, (layout, k, rows, cols, 0))
            for s in (k, 1):
                e.step(s)
                got, _ = same_as_download(e, (layout, k, rows, cols, e.generation))
            assert e.popcount() == int(got.sum())


@pytest.mark.parametrize("layout", ["bit", "byte"])
@pytest.mark.parametrize("m,n", [(4, 48), (2, 1024)])
def test_mesh_compat_column_runs(gh, layout, m, n):
    with gh.Engine(n, n, layout=layout, boundary="mesh_compat", mesh_m=m, tblock_k=2) as e:
        e.upload(soup(m, n, n))
        same_as_download(e, (layout, m, n, 0))
        e.step(3)
        got, _ = same_as_download(e, (layout, m, n, 3))
        # a window across a block seam (perm_L = n / m columns per block)
        L = n // m
        assert e.digest_window(5, L - 7, 20, 19) == digest_ref(got[5:25, L - 7:L + 12], 5, L - 7)


@pytest.mark.parametrize("layout", ["bit", "byte"])
def test_serial_compat_inactive_row_and_column(gh, layout):
    with gh.Engine(37, 37, layout=layout, boundary="serial_compat", tblock_k=2) as e:
        e.initialize_board("serial", gh.SERIAL_SEED)
        same_as_download(e, (layout, 0))
        e.upload(np.ones((37, 37), np.uint8))   # the last row and column are stored as 0
        got, _ = same_as_download(e, (layout, "ones"))
        assert not got[-1].any() and not got[:, -1].any()
        e.step(5)
        same_as_download(e, (layout, 5))


# ------------------------------------------------------------------ windows
@pytest.mark.parametrize("layout,k,boundary", [("bit", 1, "dead"), ("bit", 8, "dead"), ("byte", 1, "dead"),
                                               ("bit", 3, "torus"), ("byte", 5, "torus")])
def test_windows_and_tiling(gh, layout, k, boundary):
    rows, cols = 100, 300
    rng = np.random.default_rng(17 + k)
    with gh.Engine(rows, cols, layout=layout, boundary=boundary, tblock_k=k) as e:
        e.upload(soup(3, rows, cols))
        e.step(k)
        got, whole = same_as_download(e, (layout, k, boundary))
        # a 5×5 grid of windows at random cuts: each equals the reference, and they tile the board
        rcut = [0] + sorted(rng.choice(np.arange(1, rows), 4, replace=False).tolist()) + [rows]
        ccut = [0] + sorted(rng.choice(np.arange(1, cols), 4, replace=False).tolist()) + [cols]
        parts = []
        for r0, r1 in zip(rcut[:-1], rcut[1:]):
            for c0, c1 in zip(ccut[:-1], ccut[1:]):
                d = e.digest_window(r0, c0, r1 - r0, c1 - c0)
                assert d == digest_ref(got[r0:r1, c0:c1], r0, c0), (r0, c0, r1, c1)
                parts.append(d)
        assert add(*parts) == whole
        assert e.digest_window(rows, cols, 0, 0) == (0, 0)
        with pytest.raises(gh.GolError) as ex:
            e.digest_window(0, 0, rows + 1, cols)
        assert ex.value.code == -1
        assert e.digest() == whole   # the context stays usable


# ------------------------------------------------------------------ slabs and ranks
@pytest.mark.parametrize("layout,k,boundary", [("bit", 8, "dead"), ("bit", 2, "torus"), ("byte", 4, "dead")])
def test_three_slabs_equal_one(gh, layout, k, boundary):
    b = soup(9, 100, 257)
    ds = []
    for slabs in (1, 3):
        with gh.Engine(100, 257, n_gpus=slabs, layout=layout, boundary=boundary, tblock_k=k) as e:
            e.upload(b)
            for s in block_steps(k):
                e.step(s)
            ds.append(same_as_download(e, (layout, k, boundary, slabs))[1])
    assert ds[0] == ds[1]


def test_rank_parts_sum_to_the_board(gh):
    assert os.path.exists(SHIM), "build the shim first (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "digest_rank_check.py"), SHIM],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "digest ranks ok" in r.stdout


# ------------------------------------------------------------------ the point of the feature
def test_cross_configuration_equality(gh):
    n, gens = 2048, 96
    configs = [("bit", 1, 1), ("bit", 8, 1), ("bit", 16, 1), ("byte", 1, 1), ("byte", 16, 1), ("bit", 16, 3)]
    ds, ref = [], None
    for layout, k, slabs in configs:
        with gh.Engine(n, n, n_gpus=slabs, layout=layout, tblock_k=k) as e:
            e.initialize_board("stream", 1)
            e.step(gens)
            ds.append(e.digest())
            if ref is None:
                ref = digest_ref(e.download())
    assert ds[0] == ref and ref != (0, 0)
    assert all(d == ds[0] for d in ds), list(zip(configs, ds))


# ------------------------------------------------------------------ async
@pytest.mark.parametrize("layout,k,slabs,boundary,rows", [("bit", 8, 1, "dead", 700), ("bit", 4, 3, "dead", 100),
                                                          ("byte", 16, 2, "torus", 90)])
def test_async_digest_behind_every_step(gh, layout, k, slabs, boundary, rows):
    cols = 300
    b = soup(21, rows, cols)
    kw = dict(n_gpus=slabs, layout=layout, boundary=boundary, tblock_k=k)
    with gh.Engine(rows, cols, **kw) as e:
        e.upload(b)
        outs = []
        for _ in range(40):   # no sync in between
            e.step(k)
            outs.append(e.digest_async())
        e.sync()
    with gh.Engine(rows, cols, **kw) as e:
        e.upload(b)
        for i in range(40):
            e.step(k)
            assert (int(outs[i][0]), int(outs[i][1])) == digest_ref(e.download()), (layout, k, slabs, i)


def test_pending_limit_is_estate_and_the_context_stays_usable(gh):
    b = soup(5, 50, 70)
    with gh.Engine(50, 70, layout="bit", tblock_k=2) as e:
        e.upload(b)
        outs = [e.digest_async() for _ in range(1024)]
        with pytest.raises(gh.GolError) as ex:
            e.digest_async()
        assert ex.value.code == ESTATE
        e.step(2)
        got, d = same_as_download(e, "after the refused request")
        want0 = digest_ref(b)
        assert all((int(o[0]), int(o[1])) == want0 for o in outs)
        o = e.digest_async()
        e.sync()
        assert (int(o[0]), int(o[1])) == d


# ------------------------------------------------------------------ find_repeat
def board_at(gh, b, gens, **kw):
    with gh.Engine(b.shape[0], b.shape[1], **kw) as e:
        e.upload(b)
        e.step(gens)
        return e.download()


def test_find_repeat_blinker_and_block(gh):
    b = np.zeros((20, 30), np.uint8)
    b[5, 4:7] = 1       # blinker
    b[12:14, 20:22] = 1  # block
    with gh.Engine(20, 30, layout="bit", tblock_k=1) as e:
        e.upload(b)
        assert e.find_repeat(100, every=1) == (0, 2)


def test_find_repeat_glider_on_a_torus(gh):
    b = np.zeros((64, 64), np.uint8)
    b[1, 2] = b[2, 3] = b[3, 1] = b[3, 2] = b[3, 3] = 1
    kw = dict(layout="bit", boundary="torus", tblock_k=8)
    with gh.Engine(64, 64, **kw) as e:
        e.upload(b)
        rep = e.find_repeat(1024)   # every = tblock_k = 8
    assert rep == (0, 256)
    assert (board_at(gh, b, rep[1], **kw) == b).all()


def test_find_repeat_highlife_soup(gh):
    b = soup(HIGHLIFE_SEED, 32, 32, 0.35)
    kw = dict(layout="bit", boundary="torus", tblock_k=4, rule="B36/S23")
    with gh.Engine(32, 32, **kw) as e:
        e.upload(b)
        rep = e.find_repeat(HIGHLIFE_MAX)
    assert rep is not None and rep[0] < rep[1] and (rep[1] - rep[0]) % 4 == 0
    first, again = board_at(gh, b, rep[0], **kw), board_at(gh, b, rep[1], **kw)
    assert (first == again).all()


# this B36/S23 soup (32×32 torus, density 0.35) is in a cycle from generation 228 on at the
# latest (a numpy stepper, checked every 4 generations, when the test was written)
HIGHLIFE_SEED, HIGHLIFE_MAX = 0, 4000


# ------------------------------------------------------------------ bin/gol --digest
def driver(args, cwd):
    r = subprocess.run([EXE] + args, cwd=cwd, check=True, capture_output=True, text=True, timeout=120)
    return r.stdout


def test_driver_digest(gh, tmp_path):
    args = ["--mode", "dead", "-k", "4", "64", "96", "12", "30"]
    plain = driver(args, tmp_path)
    with_flag = driver(["--digest"] + args, tmp_path)
    two_slabs = driver(["--digest", "--gpus", "2"] + args, tmp_path)
    want = {}
    with gh.Engine(64, 96, layout="bit", tblock_k=4) as e:
        e.initialize_board("stream", 1)
        for gen in (0, 12, 24, 30):
            e.step(gen - e.generation)
            d = e.digest()
            want[gen] = f"{d[0]:016x}{d[1]:016x}"
    for out in (with_flag, two_slabs):
        lines = [ln.split() for ln in out.splitlines() if ln.startswith("digest ")]
        assert [(int(g), h) for _, g, h in lines] == sorted(want.items()), out

    # without the flag: no digest line, and the flag adds nothing but its lines
    def fixed(out):   # the run's name is a timestamp, the device time varies
        out = re.sub(r"\d{4}-\d\d-\d\d-\d\d-\d\d-\d\d", "NAME", out)
        return re.sub(r"device [\d.]+ ms  [\d.]+ GCUPS", "device T ms  G GCUPS", out)

    assert "digest" not in plain
    assert fixed(plain) == fixed("".join(ln + "\n" for ln in with_flag.splitlines() if not ln.startswith("digest ")))


# ------------------------------------------------------------------ schedule
def test_digest_schedules_have_no_race_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sched_digest_check.py"), "gpu"],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "sched digest gpu ok" in r.stdout
