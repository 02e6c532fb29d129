#!/usr/bin/env python3
"""What the rule-generic kernel costs: B3/S23 through the rule-generic kernel
(GOL_OPT_RULE_KERNEL = 1) against B3/S23 on the tuned kernels (the reference
for this number) on one GPU — same build, same shape, one process, the boards
taking turns after a settle phase.  A third board runs HighLife (B36/S23), as a
check that the rule's content does not matter.  Further boards run HighLife and
Day & Night on their compiled kernels (GOL_OPT_RULE_COMPILED = 1, the default)
beside the same rules on the rule-generic kernel.

    python tools/rule_cost.py [--spec N:K ...] [--rounds 4] [--window-s 0.4] [--out FILE]

Per spec (bit layout, N x N, dead boundary): the boards are seeded alike
(srand(1) row-major) and stepped for a settle phase (the clock ramp of a GPU
that idled); then, per round and per board, one timed window
(device ms between events, gol_sync) and right after it the same window again
beside the clock probe (the probe's wave takes registers on one SIMD, so the
timed window runs without it, as in bench.py).  One JSON line per window, then
one summary line per spec: median ms per k-step of every board, the ratios to
the tuned board, of each compiled board to the tuned board and to the generic
board of its rule, the clocks.  A measurement, not a gate.
"""
import argparse
import json
import os
import statistics
import sys
import time

# every board's streams and the probe's want hardware queues of their own (see bench.py)
if int(os.environ.get("GPU_MAX_HW_QUEUES", "4") or 4) < 24:
    os.environ["GPU_MAX_HW_QUEUES"] = "24"

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_amd import golhip as gh  # noqa: E402

PROBE_MAX_MS = 20000.0
# board: (rule, GOL_OPT_RULE_KERNEL); GOL_OPT_RULE_COMPILED stays at its default, 1
BOARDS = {"tuned": ("B3/S23", 0), "generic": ("B3/S23", 1), "highlife": ("B36/S23", 1),
          "daynight": ("B3678/S34678", 1), "highlife_compiled": ("B36/S23", 0),
          "daynight_compiled": ("B3678/S34678", 0)}
COMPILED = {"highlife_compiled": "highlife", "daynight_compiled": "daynight"}   # and its generic board


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--spec", action="append", help="N:K (default: 131072:1 131072:2 131072:4 131072:7)")
    p.add_argument("--rounds", type=int, default=4, help="alternations of the boards (at least 3)")
    p.add_argument("--window-s", type=float, default=0.4, help="seconds of steps per timed window")
    p.add_argument("--settle-s", type=float, default=1.0)
    p.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = p.parse_args()
    specs = a.spec or ["131072:1", "131072:2", "131072:4", "131072:7"]
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for sp in specs:
        n, k = (int(x) for x in sp.split(":"))
        boards = {}
        for b, (rule, generic) in BOARDS.items():
            e = gh.Engine(n, n, layout="bit", tblock_k=k, rule=rule)
            e.set_option(gh.OPT_RULE_KERNEL, generic)
            e.initialize_board("stream", 1)
            e.sync()
            want = "compiled" if b in COMPILED else "generic" if generic else "tuned"
            assert e.rule_path == want, (b, e.rule_path)
            boards[b] = e
        # calibration block (on the tuned board), then the settle phase shared by the boards
        t = time.perf_counter()
        boards["tuned"].step(10 * k)
        boards["tuned"].sync()
        per_step = (time.perf_counter() - t) / 10
        for b, e in boards.items():   # (the same generations on every board)
            if b != "tuned":
                e.step(10 * k)
        steps = max(4, int(a.window_s / per_step))
        settle = max(0, int(a.settle_s / per_step / len(boards)))
        for e in boards.values():
            e.step(settle * k)
        for e in boards.values():
            e.sync()
        ms = {b: [] for b in boards}
        mhz = {b: [] for b in boards}
        for rnd in range(max(3, a.rounds)):
            for b, e in boards.items():
                w = steps
                e.step(w * k)
                dev_ms = e.sync()
                e.clock_start(PROBE_MAX_MS)
                e.step(w * k)
                e.sync()
                clk = e.clock_stop()[0]
                ms[b].append(dev_ms / w)
                mhz[b].append(clk)
                emit({"spec": sp, "board": b, "rule": BOARDS[b][0], "rule_kernel": BOARDS[b][1],
                      "rule_path": e.rule_path, "round": rnd,
                      "k_steps": w, "ms_per_k_step": round(dev_ms / w, 5),
                      "gcups": round(n * n * k * w / dev_ms / 1e6, 1), "sclk_mhz_next_window": round(clk, 1)})
        live = {b: e.popcount() for b, e in boards.items()}
        for e in boards.values():
            e.close()
        med = {b: statistics.median(v) for b, v in ms.items()}
        emit({"spec": sp, "summary": True, "ms_per_k_step": {b: round(v, 5) for b, v in med.items()},
              "gcups": {b: round(n * n * k / v / 1e6, 1) for b, v in med.items()},
              "generic_over_tuned": round(med["generic"] / med["tuned"], 4),
              "highlife_over_generic": round(med["highlife"] / med["generic"], 4),
              "compiled_over_tuned": {b: round(med[b] / med["tuned"], 4) for b in COMPILED},
              "compiled_over_generic": {b: round(med[b] / med[g], 4) for b, g in COMPILED.items()},
              "spread": {b: [round(min(v), 5), round(max(v), 5)] for b, v in ms.items()},
              "sclk_mhz": {b: round(statistics.median(v), 1) for b, v in mhz.items()},
              "live_cells": live, "generic_live_equals_tuned": live["generic"] == live["tuned"],
              "version": gh.version()})
    if out:
        out.close()


if __name__ == "__main__":
    main()
