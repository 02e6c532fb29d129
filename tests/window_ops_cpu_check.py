#!/usr/bin/env python3
"""The runtime's side of the device-side window calls over the host-only HIP stand-in (no
GPU): tests/window_ops_sweep.py without stepping, for all 14 storage kinds of
tests/window_model.py in 1 and 3 slabs.  The stand-in's fill, copy, packed-bit, digest
and density launchers run the row routines of the shared headers on host memory for
byte boards and for both group widths of bit boards, and none of these calls needs a
byte upload or download, so the window -> slab piece -> column run code of
gol_runtime.cpp is checked here for bit-layout boards too: torus ghost margins,
MESH_COMPAT's reversed blocks on both sides of a copy, SERIAL_COMPAT's dead line, slab
seams inside a window.  Run by tests/test_window_ops_cpu.py in a subprocess:

    GOL_LIB=tests/fake_hip/libgolhip_fakehip.so python tests/window_ops_cpu_check.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from mpi_amd import golhip as gh  # noqa: E402
import window_ops_model as wm  # noqa: E402
import window_ops_sweep  # noqa: E402

if __name__ == "__main__":
    gh.load()
    boards = 0
    for kind in wm.KINDS:
        for board in kind[3]:
            for slabs in wm.slab_counts(board[0], kind[1]):
                window_ops_sweep.sweep(gh, kind, board, slabs, stepping=False)
                boards += 1
    print(f"window ops cpu ok {boards}")
