"""The device-side window calls (packed bits, digest, density, random fill, board-to-board
copy) swept over every storage kind of tests/window_model.py on the host-only HIP
stand-in: tests/window_ops_cpu_check.py runs the sweep body of the GPU test
(tests/window_ops_sweep.py) without stepping, bit-layout boards included."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "fake_hip", "libgolhip_fakehip.so")

sys.path.insert(0, os.path.join(ROOT, "tests"))
import window_ops_model as wm  # noqa: E402


def run_script(name, **env):
    assert os.path.exists(LIB), "build the host-only runtime first (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", name)], env=dict(os.environ, GOL_LIB=LIB, **env),
                       capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_window_ops_sweep_cpu():
    boards = sum(len(wm.slab_counts(rows, kind[1])) for kind in wm.KINDS for rows, _, _ in kind[3])
    assert boards == 38   # 14 kinds, 19 boards, 1 and 3 slabs
    assert f"window ops cpu ok {boards}" in run_script("window_ops_cpu_check.py").splitlines()
