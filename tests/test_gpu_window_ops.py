"""The device-side window calls — gol_download_bits_window[_async], gol_upload_bits_window,
gol_digest_window / gol_digest_async, gol_density_window / gol_density_async,
gol_fill_random_window, gol_copy_window — swept over every storage form and column
alignment against one numpy model of the logical board (tests/window_model.py with the
operations and plan tables of tests/window_ops_model.py, pinned on the CPU by
tests/test_window_model.py and tests/test_window_ops_model.py).  The body is tests/window_ops_sweep.py,
which tests/test_window_ops_cpu.py also runs over the host-only HIP stand-in.

Per storage kind (layout x group width x boundary, 1 and 3 slabs): the board is filled
by seed and stepped [k, max(1, k - 3), 1]; after each step the packed download, the
digest and the density map (tiles rotating through 1-row tiles, clipped tile rows and
columns, tiles wider than the window, 32 to 128 columns) are compared with the model
at every window of the list — windows off a multiple of 32 columns must be refused by
the density call with the caller's block untouched —, digests of a tiling add up to
the board's, every map holds the live count, the C ABI runs with ld beyond the row,
and the packed windows of a row class are pending with a digest and a map while a
k-step is enqueued behind them.  Then every writer replaces every window: fills with
seeds and thresholds rotating (none, all, one, three and all 32 planes, 2^-32), packed
uploads with every pad bit set, copies from a second context of the same kind and
from a foreign one (other layout or group width) at shifts 0, +-1, +-31, +-32, +-33,
+-97 under REPLACE / OR / XOR.  After every write the whole board (packed and byte
download, popcount) must be the model's, the sources unchanged; each pass ends with
writes to column 0, the last column and a full row and 2k + 1 generations: a stale
torus ghost, a live pad or inactive bit or a halo row left behind changes those.

What a defect would turn red first (read from the code, not tried on a device;
windows are (row0, col0, nrows, ncols)).  The kernels' own lane / unit / row-segment
distribution:
  gol_bits.hip   `if (lane > 0) P[0] |= carry` dropped in get_bits_kernel: a unit's top packed word
                 never reaches its right neighbour: bit-k3-dead, download_bits_window (0, 1, 40, 97) of
                 the first reader pass: packed bits 96 .. travel in unit 0's carry word
                 `in + ra * ipitch` without `ra` in put_bits_kernel (the second 64-row segment reads the
                 first one's packed rows): bit-k32-dead, upload_bits_window (0, 0, 100, 300), rows 64 .. 99
                 atomicOr of a run's first / last word as a plain store: bit-k2-mesh_compat 96 / m = 3,
                 download_bits_window at col0 = 1 (two runs of one window share a packed word)
  gol_kernels.hip  `grow0 + rs + lane` as `grow0 + lane` in digest_kernel (A_i of the second block of 64
                 rows): bit-k32-dead, digest_window (0, 0, 100, 1) of the first reader pass
                 `ok == key` dropped from density_kernel's segmented reduction (lanes of other tiles
                 added in): bit-k3-dead, density(16, 128) of the whole board: units 0, 1, 2 are tiles 0, 1, 2
                 `trow_off + r` as `r` in density_kernel: every kind in 3 slabs, density_window of an
                 all-rows window at tiles (3, 64): the second slab's rows start mid-tile
  gol_fill.hip   `grow0 + ra + i0 + k` without `ra`: bit-k32-dead, the same-kind copy source's whole-board
                 fill (rows 64 .. 99 repeat rows 0 .. 35)
                 `carry` false at a shifted run: bit-k3-torus (ghost margin 3), the same fill: the columns of
                 every unit that its last canonical word holds
  gol_copy.hip   `read` without `op == kCopyReplace`'s negation, i.e. covered units never read: the first
                 OR or XOR copy that covers a whole destination unit (128 columns of a bit row, 32 of a byte row)
                 `(sr0 + ra) * spitch` without `ra`: bit-k32-dead, the whole-board REPLACE that opens the
                 copy pass, rows 64 .. 99
The runtime's window -> slab piece -> column run code (gol_runtime.cpp; each of these was
built into the host-only stand-in and turned tests/test_window_ops_cpu.py red there first):
  gol_copy_window   `dpc + off` as `dpc`: bit-k2-mesh_compat 96 / m = 3 from its same-kind source,
                    copy (5, 5, 20, 41) <- (5, 6) OR: a source block seam inside one destination run
                    `srow` from d->hk: bit-k3-dead <- bit-k8-torus, the whole-board REPLACE
  gol_fill_random_window  the window's row0 for the piece's r0: bit-k3-dead in 3 slabs, the source fill
                    the window's col0 for the run's lc: bit-k2-mesh_compat, the source fill
  window_async      packed: `lc - col0` as 0 (every run lands at packed bit 0): bit-k2-mesh_compat
  digest_enqueue    row0 for r0: bit-k3-dead in 3 slabs, digest_window (0, 0, 40, 1);
                    col0 for lc: bit-k2-mesh_compat, digest_window (0, 0, 96, 63)
  density_enqueue   col0 for lc: bit-k2-mesh_compat, density_window (0, 0, 96, 63) at tiles (1, 32);
                    one slab's part delivered: bit-k3-dead in 3 slabs, density_window (0, 0, 40, 1)
Not reached on these boards (at most 300 columns, so one item of 64 units per row): the
hand-over between two wave items along a row (get_bits_kernel's lane 0 / lane 63 words);
tests/test_gpu_bits.py, test_gpu_fill.py and test_gpu_copy.py keep their 8300- and
2100-column boards for that."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import window_ops_model as wm  # noqa: E402
import window_ops_sweep  # noqa: E402


@pytest.fixture(scope="module")
def gh():
    from mpi_amd import golhip
    golhip.load()
    return golhip


@pytest.mark.parametrize("kind", wm.KINDS, ids=wm.kind_id)
def test_window_ops_sweep(gh, kind):
    for board in kind[3]:
        for slabs in wm.slab_counts(board[0], kind[1]):
            window_ops_sweep.sweep(gh, kind, board, slabs, stepping=True)
