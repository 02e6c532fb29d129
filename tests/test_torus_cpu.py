"""GOL_TORUS without a GPU: what gol_create accepts (validate() runs before any
device is touched, so libgolhip.so answers on a machine with no GPU), and the
torus step schedule — the halo ring, the wrap behind every stencil launch —
recorded over the host-only HIP stand-in and race-checked (tests/
sched_torus_check.py)."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "fake_hip", "libgolhip_fakehip.so")
SHIM = os.path.join(ROOT, "tests", "fake_hip", "libfake_rccl_host.so")
EINVAL, EHIP = -1, -2
BIT, BYTE, TORUS = 1, 0, 3


@pytest.fixture(scope="module")
def lib():
    from mpi_amd import golhip
    return golhip.load()


def create(lib, rows, cols, slabs, layout, boundary, k):
    ctx = ctypes.c_void_p()
    rc = lib.gol_create(ctypes.byref(ctx), rows, cols, slabs, layout, boundary, 1, k)
    if rc == 0:
        lib.gol_destroy(ctx)
    return rc


def test_binding_names_the_torus():
    from mpi_amd import golhip
    assert golhip.BOUNDARY["torus"] == TORUS
    assert "#define GOL_TORUS 3" in open(os.path.join(ROOT, "include", "golhip.h")).read()


@pytest.mark.parametrize("rows,cols,slabs,layout,k,names", [
    (64, 7, 1, BIT, 8, "cols >= tblock_k"),        # cols < K
    (64, 15, 1, BIT, 16, "cols >= tblock_k"),
    (7, 64, 1, BIT, 8, "at least tblock_k=8 rows"),   # rows < K: the single slab sends K rows to itself
    (47, 64, 1, BYTE, 48, "at least tblock_k=48 rows"),
    (23, 64, 3, BIT, 8, "at least tblock_k=8 rows"),  # a slab thinner than K
    (31, 64, 2, BYTE, 16, "at least tblock_k=16 rows"),
])
def test_torus_size_constraints_are_einval_before_any_device(lib, capfd, rows, cols, slabs, layout, k, names):
    assert create(lib, rows, cols, slabs, layout, TORUS, k) == EINVAL
    assert names in capfd.readouterr().err


def test_torus_is_a_known_boundary_and_4_is_not(lib, capfd):
    # a valid torus passes validate(): GOL_OK with a GPU, GOL_EHIP ("no HIP device") without
    assert create(lib, 64, 64, 1, BIT, TORUS, 8) in (0, EHIP)
    assert create(lib, 8, 8, 1, BIT, TORUS, 8) in (0, EHIP)      # rows = cols = K: the smallest board
    assert create(lib, 48, 64, 3, BYTE, TORUS, 16) in (0, EHIP)  # slabs of exactly K rows
    capfd.readouterr()
    assert create(lib, 64, 64, 1, BIT, 4, 8) == EINVAL
    assert "bad boundary" in capfd.readouterr().err


def test_torus_row_width_limit_counts_the_ghost_columns(lib, capfd):
    # byte rows: (cols + 2K)·(2K + 8) must stay below 2^28; cols alone would pass at K = 64
    k = 64
    cols = (1 << 28) // (2 * k + 8) - 2 * k + 1
    assert cols * (2 * k + 8) < (1 << 28) <= (cols + 2 * k) * (2 * k + 8)
    assert create(lib, 64, cols, 1, BYTE, TORUS, k) == -5
    assert "too wide" in capfd.readouterr().err


needs_fake = pytest.mark.skipif(not os.path.exists(LIB),
                                reason="build the host-only runtime first (__graft_entry__.build())")


@needs_fake
def test_torus_schedules_have_no_race_cpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sched_torus_check.py")],
                       env=dict(os.environ, GOL_LIB=LIB), capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "sched torus ok" in r.stdout


@needs_fake
def test_torus_rank_schedules_have_no_race_cpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sched_torus_check.py")],
                       env=dict(os.environ, GOL_LIB=LIB, GOL_RCCL_SHIM=SHIM), capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "sched torus rccl ok" in r.stdout


@needs_fake
def test_torus_init_modes_cpu():
    """GOL_INIT_STREAM is accepted on a torus, the reference-shaped modes are GOL_EUNSUPPORTED."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from mpi_amd import golhip as gh\n"
            "for layout in ('bit', 'byte'):\n"
            "    with gh.Engine(64, 64, layout=layout, boundary='torus', tblock_k=4) as e:\n"
            "        e.initialize_board('stream', 1)\n"
            "        for mode in ('serial', 'mesh'):\n"
            "            try:\n"
            "                e.initialize_board(mode, 1)\n"
            "            except gh.GolError as ex:\n"
            "                assert ex.code == -5, ex\n"
            "            else:\n"
            "                raise SystemExit('init mode accepted: ' + mode)\n"
            "print('torus init modes ok')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GOL_LIB=LIB), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "torus init modes ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
