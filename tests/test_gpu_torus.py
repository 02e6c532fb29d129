"""GOL_TORUS on the GPU, bit-exact against tests/torus_ref.py (the numpy torus
stepper that tests/test_torus_ref.py pins to the oracle).

The torus runs the unchanged dead-boundary kernels on rows widened by K ghost
columns per side; launch_wrap_cols refreshes the ghosts after every launch and
the K-row halo exchange is closed into a ring.  What can go wrong, and what
the shapes below are chosen for:
 - bit layout: the ghosts are bit fields inside the interleaved G-word groups
   (64 columns for k <= 7, 128 above); the column counts put them at every
   position relative to a group, straddling one, and in the same group as
   their sources;
 - byte layout: ghosts off a dword boundary;
 - the ring: one slab exchanging with itself, two slabs with the same
   neighbour on both sides, thin (H <= 2K) and uneven slabs, overlap on/off,
   the split interior, a short block followed by a full one ("grow").
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import torus_ref
from oracle import golcpu as g

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mpi_amd", "bin", "gol")
SHIM = os.path.join(ROOT, "tests", "shim", "libfake_rccl.so")


@pytest.fixture(scope="module")
def gh():
    from mpi_amd import golhip
    golhip.load()
    return golhip


def rand_board(seed, rows, cols, p=0.4):
    return (np.random.default_rng(seed).random((rows, cols)) < p).astype(np.uint8)


def run_torus(gh, b, steps, layout, k, slabs=1, options=()):
    """The board and the popcount after gol_step(s) for s in steps."""
    rows, cols = b.shape
    with gh.Engine(rows, cols, n_gpus=slabs, layout=layout, boundary="torus", tblock_k=k) as e:
        for opt, v in options:
            e.set_option(opt, v)
        e.upload(b)
        for s in steps:
            e.step(s)
        return e.download(), e.popcount()


def check(gh, b, steps, layout, k, slabs=1, options=(), ref=None):
    ref = torus_ref.run(b, sum(steps)) if ref is None else ref
    got, live = run_torus(gh, b, steps, layout, k, slabs, options)
    rr, cc = np.nonzero(got != ref)
    assert rr.size == 0, (f"{b.shape} {layout} k={k} slabs={slabs} steps={steps} options={options}: {rr.size} cells "
                          f"differ, columns {np.unique(cc)[:12]} rows {np.unique(rr)[:12]}")
    assert live == int(ref.sum()), (b.shape, layout, k, slabs, live, int(ref.sum()))
    return ref


def bit_cols(k):
    c = [k, 64 - k, 64, 65, 128 - 2 * k, 128 - k, 127, 128, 129, 256 - k - 1, 1000]
    return sorted({x for x in c if x >= k})


# ------------------------------------------------------------------ 5. bit layout, one slab
@pytest.mark.parametrize("k", [1, 3, 7, 8, 16, 32])
def test_bit_one_slab_ghosts_at_every_group_position(gh, k):
    gens = 3 * k + (k - 1)   # three full blocks and a short last one
    for cols in bit_cols(k):
        for rows in (k, 2 * k + 1, 37 + k):
            b = rand_board(1000 * k + cols + rows, rows, cols)
            check(gh, b, [gens], "bit", k)
            if k >= 4:   # a short block followed by full ones: the exchange's grow dependency
                check(gh, b, [k - 3, 2 * k], "bit", k)


# ------------------------------------------------------------------ 6. strips
@pytest.mark.parametrize("rows,cols,k", [(48, 16200, 8), (48, 16200, 16), (40, 8000, 5)])
def test_bit_strips(gh, rows, cols, k):
    b = rand_board(cols + k, rows, cols)
    check(gh, b, [2 * k + 3], "bit", k)


# ------------------------------------------------------------------ 7. slabs
@pytest.mark.parametrize("k", [3, 8, 16])
@pytest.mark.parametrize("layout", ["bit", "byte"])
def test_slab_ring(gh, layout, k):
    for rows in (3 * k + 1, 7 * k, 20 * k + 3):
        b = rand_board(rows + k, rows, 200)
        steps = [k, k - 1, k, 2 * k] if k > 1 else [3]
        ref = torus_ref.run(b, sum(steps))
        for slabs in (2, 3, 5):
            if rows // slabs < k:
                continue   # GOL_EINVAL by the size constraint (tests/test_torus_cpu.py)
            for overlap in (1, 0):
                check(gh, b, steps, layout, k, slabs, [(gh.OPT_OVERLAP, overlap)], ref)


@pytest.mark.parametrize("k", [8, 16])
@pytest.mark.parametrize("slabs", [1, 2])
def test_bit_split_interior(gh, k, slabs):
    rows = slabs * (2 * 32 * k + 2 * k) + (3 if slabs == 1 else 0)
    b = rand_board(rows, rows, 200)
    check(gh, b, [k, k - 3, 2 * k], "bit", k, slabs, [(gh.OPT_INTERIOR_SPLIT, 2)])
    with gh.Engine(rows, 200, n_gpus=slabs, layout="bit", boundary="torus", tblock_k=k) as e:
        e.set_option(gh.OPT_INTERIOR_SPLIT, 2)
        e.upload(b)
        e.step(2 * k)
        e.sync()
        _, launches = e.kernel_time()
    assert launches == 2 * 2 * slabs   # two interior parts per slab and k-step: the split really ran


# ------------------------------------------------------------------ 8. byte layout
@pytest.mark.parametrize("k,core", [(1, None), (5, None), (8, None), (32, None), (48, None), (16, 4)])
def test_byte_layout(gh, k, core):
    options = [] if core is None else [(gh.OPT_BYTE_CORE, core)]
    gens = [k, k - 1] if k > 1 else [3]
    for cols in sorted({c for c in (k, 63, 64, 65, 255, 256, 257, 5000) if c >= k}):
        rows = 3 * k + 2
        b = rand_board(7 * k + cols, rows, cols)
        ref = check(gh, b, gens, "byte", k, 1, options)
        check(gh, b, gens, "byte", k, 3, options, ref)


# ------------------------------------------------------------------ 9. gliders
@pytest.mark.parametrize("layout", ["bit", "byte"])
@pytest.mark.parametrize("slabs", [1, 3])
def test_glider_crosses_the_corner_and_returns(gh, layout, slabs):
    rows, cols = 24, 40
    b = torus_ref.glider(rows, cols, rows - 2, cols - 1)   # its box lies across all four corners
    assert b[0].any() and b[-1].any() and b[:, 0].any() and b[:, -1].any()
    with gh.Engine(rows, cols, n_gpus=slabs, layout=layout, boundary="torus", tblock_k=8) as e:
        e.upload(b)
        e.step(240)
        assert e.popcount() == 5
        e.step(240)   # one cell diagonally per 4 generations: 120 cells, a multiple of 24 and of 40
        assert (e.download() == b).all()


# ------------------------------------------------------------------ 10. I/O
@pytest.mark.parametrize("layout,k", [("bit", 1), ("bit", 8), ("bit", 32), ("byte", 5), ("byte", 16)])
@pytest.mark.parametrize("slabs", [1, 3])
def test_init_stream_has_the_dead_boards_cells(gh, layout, k, slabs):
    rows, cols, seed = 101, 333, 5
    want = g.init_dead(rows, cols, seed)
    with gh.Engine(rows, cols, n_gpus=slabs, layout=layout, boundary="torus", tblock_k=k) as e:
        e.initialize_board("stream", seed)
        assert (e.download() == want).all()
        assert e.popcount() == int(want.sum())
        e.step(k + 2)
        assert (e.download() == torus_ref.run(want, k + 2)).all()
        with pytest.raises(gh.GolError) as ex:
            e.initialize_board("serial", seed)
        assert ex.value.code == -5


@pytest.mark.parametrize("layout,k", [("bit", 8), ("bit", 3), ("byte", 8)])
def test_windows_text_and_parse(gh, layout, k):
    rows, cols = 67, 389
    b = rand_board(17, rows, cols)
    with gh.Engine(rows, cols, n_gpus=2, layout=layout, boundary="torus", tblock_k=k) as e:
        e.upload(b)
        # windows touching column 0 and column cols-1 (they do not wrap), then steps from them
        left, right = rand_board(18, 30, 9), rand_board(19, 41, 11)
        e.upload_window(20, 0, left)
        e.upload_window(5, cols - 11, right)
        b[20:50, 0:9] = left
        b[5:46, cols - 11:] = right
        assert (e.download() == b).all()
        e.step(k + 3)
        ref = torus_ref.run(b, k + 3)
        assert (e.download_window(0, 0, rows, 7) == ref[:, :7]).all()
        assert (e.download_window(3, cols - 5, 60, 5) == ref[3:63, cols - 5:]).all()
        assert e.format_text(0, 0, rows, cols) == g.text_body(ref)
        assert e.format_text(9, cols - 40, 50, 40) == g.text_body(ref[9:59, cols - 40:])
        # parse round trip, then the generations continue from the parsed board
        b2 = rand_board(20, rows, cols)
        e.parse_text(0, 0, rows, cols, g.text_body(b2))
        assert (e.download() == b2).all()
        w = rand_board(21, 30, 50)
        e.parse_text(10, 0, 30, 50, g.text_body(w))
        b2[10:40, 0:50] = w
        e.step(2 * k + 1)
        ref2 = torus_ref.run(b2, 2 * k + 1)
        assert (e.download() == ref2).all()
        assert e.popcount() == int(ref2.sum())


@pytest.mark.parametrize("extra", [["--gpus", "2", "-k", "8"], ["--layout", "byte", "-k", "4"]])
def test_driver_torus_snapshots(gh, tmp_path, extra):
    rows, cols = 64, 96
    subprocess.run([EXE, "--mode", "torus", "--save"] + extra + [str(rows), str(cols), "12", "24"], cwd=tmp_path,
                   check=True, capture_output=True, text=True, timeout=120)
    name = [f for f in os.listdir(tmp_path) if f.endswith(".gol") and "_" not in f][0][:-4]
    parts = 2 if "--gpus" in extra else 1
    b0 = g.init_dead(rows, cols, 1)
    for it in (0, 12, 24):
        ref = torus_ref.run(b0, it)
        for p in range(parts):
            path = tmp_path / f"{name}_{it}_{p}.gol"
            r0, c0, nr, nc, off = gh.part_geometry(str(path))
            assert open(path, "rb").read()[off:] == g.text_body(ref[r0:r0 + nr, c0:c0 + nc]), (it, p)


# ------------------------------------------------------------------ 11. RCCL ranks
def test_rccl_ring_over_shim():
    assert os.path.exists(SHIM), "build the shim first (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rccl_torus_check.py"), SHIM],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "rccl torus ok" in r.stdout and "rccl torus sched ok" in r.stdout
