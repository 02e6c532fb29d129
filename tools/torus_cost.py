#!/usr/bin/env python3
"""What the periodic boundary costs: the GOL_TORUS k-step against the GOL_DEAD
k-step (the reference for this number) on one GPU — same build, same shape, one
process, the two boards taking turns after a settle phase.

    python tools/torus_cost.py [--spec LAYOUT:N:K[:TCOLS] ...] [--rounds 4] [--window-s 0.4] [--out FILE]

Both boards are N x N unless TCOLS gives the torus board's columns: N - 2K makes
its stored row (TCOLS + 2K ghost columns) as wide as the dead board's, so both
run the same strip geometry (rates are per cell of each board's own size).

Per spec: both boards are seeded alike (srand(1) row-major) and stepped for a
settle phase (the clock ramp of a GPU that idled); then, per
round and per board, one timed window (device ms between events, gol_sync)
and right after it the same window again beside the clock probe (the probe's
wave takes registers on one SIMD, so the timed window runs without it, as in
bench.py).  One JSON line per window, then one summary line per spec: median
ms per k-step of either board, their ratio, the clocks.  A measurement, not a
gate.
"""
import argparse
import json
import os
import statistics
import sys
import time

# both boards' streams and the probe's want hardware queues of their own (see bench.py)
if int(os.environ.get("GPU_MAX_HW_QUEUES", "4") or 4) < 24:
    os.environ["GPU_MAX_HW_QUEUES"] = "24"

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_amd import golhip as gh  # noqa: E402

PROBE_MAX_MS = 20000.0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--spec", action="append", help="LAYOUT:N:K[:TCOLS] (default: bit:131072:16 bit:131072:1 byte:32768:48)")
    p.add_argument("--rounds", type=int, default=4, help="alternations of the two boards (at least 3)")
    p.add_argument("--window-s", type=float, default=0.4, help="seconds of steps per timed window")
    p.add_argument("--settle-s", type=float, default=1.0)
    p.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = p.parse_args()
    specs = a.spec or ["bit:131072:16", "bit:131072:1", "byte:32768:48"]
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for sp in specs:
        layout, n, k, *tc = sp.split(":")
        n, k = int(n), int(k)
        cols = {"dead": n, "torus": int(tc[0]) if tc else n}
        boards = {}
        for b in ("dead", "torus"):
            e = gh.Engine(n, cols[b], layout=layout, boundary=b, tblock_k=k)
            e.initialize_board("stream", 1)
            e.sync()
            boards[b] = e
        # calibration block, then the settle phase shared by the two boards
        t = time.perf_counter()
        for e in boards.values():
            e.step(10 * k)
        for e in boards.values():
            e.sync()
        per_step = (time.perf_counter() - t) / 20
        steps = max(4, int(a.window_s / per_step))
        settle = max(0, int(a.settle_s / per_step / 2))
        for e in boards.values():
            e.step(settle * k)
        for e in boards.values():
            e.sync()
        ms = {b: [] for b in boards}
        mhz = {b: [] for b in boards}
        launches = {}
        for rnd in range(max(3, a.rounds)):
            for b, e in boards.items():
                e.kernel_time(reset=True)
                e.step(steps * k)
                dev_ms = e.sync()
                _, nl = e.kernel_time(reset=True)
                e.clock_start(PROBE_MAX_MS)
                e.step(steps * k)
                e.sync()
                clk = e.clock_stop()[0]
                ms[b].append(dev_ms / steps)
                mhz[b].append(clk)
                launches[b] = nl / steps
                emit({"spec": sp, "board": b, "round": rnd, "k_steps": steps, "ms_per_k_step": round(dev_ms / steps, 5),
                      "gcups": round(n * cols[b] * k * steps / dev_ms / 1e6, 1), "interior_launches_per_k_step": nl / steps,
                      "sclk_mhz_next_window": round(clk, 1)})
        live = {b: e.popcount() for b, e in boards.items()}
        for e in boards.values():
            e.close()
        md, mt = statistics.median(ms["dead"]), statistics.median(ms["torus"])
        emit({"spec": sp, "summary": True, "dead_ms_per_k_step": round(md, 5), "torus_ms_per_k_step": round(mt, 5),
              "torus_over_dead": round(mt / md, 4),
              "spread": {b: [round(min(v), 5), round(max(v), 5)] for b, v in ms.items()},
              "sclk_mhz": {b: round(statistics.median(v), 1) for b, v in mhz.items()},
              "interior_launches_per_k_step": launches,
              "live_cells": live, "settle_k_steps_per_board": settle + 10, "version": gh.version()})
    if out:
        out.close()


if __name__ == "__main__":
    main()
