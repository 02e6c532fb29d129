#!/usr/bin/env python3
"""What the board digest costs (gol_digest*, include/golhip.h) on one GPU: ms per
gol_digest of a whole board, and the k-step with and without a gol_digest_async
behind every k-step — one process, the boards taking turns after a settle phase,
the clock recorded.

    python tools/digest_cost.py [--spec LAYOUT:N:K ...] [--rounds 4] [--window-s 0.3] [--out FILE]

Default specs: bit:131072:16 (4-word groups), bit:131072:1 (2-word groups) and
byte:32768:1.  The yardstick is the k = 1 step of the same board on the same
build (it reads and writes the board once; the digest reads it once): the
summary of a k = 1 spec carries digest_over_step.  Per spec the board is seeded
(srand(1) row-major), stepped through a settle phase (the clock ramp of a GPU
that idled), then per round: a timed window of k-steps (device ms
between events, gol_sync), the same window with a digest_async behind every
k-step, `digests` back-to-back gol_digest calls (host wall clock: each call
synchronises, so a launch-and-sync round trip is inside the figure), and the
plain window again beside the clock probe (as bench.py: the timed windows run
without the probe's wave).  One JSON line per round, one summary line per spec.
A measurement, not a gate.
"""
import argparse
import json
import os
import statistics
import sys
import time

# the board's streams and the probe's want hardware queues of their own (see bench.py)
if int(os.environ.get("GPU_MAX_HW_QUEUES", "4") or 4) < 24:
    os.environ["GPU_MAX_HW_QUEUES"] = "24"

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_amd import golhip as gh  # noqa: E402

PROBE_MAX_MS = 20000.0
MAX_PENDING = 1000   # digests pending per sync (the library allows 1024)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--spec", action="append", help="LAYOUT:N:K (default: bit:131072:16 bit:131072:1 byte:32768:1)")
    p.add_argument("--rounds", type=int, default=4, help="rounds per board (at least 3)")
    p.add_argument("--window-s", type=float, default=0.3, help="seconds of steps per timed window")
    p.add_argument("--settle-s", type=float, default=1.0)
    p.add_argument("--digests", type=int, default=20, help="back-to-back gol_digest calls per round")
    p.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = p.parse_args()
    specs = a.spec or ["bit:131072:16", "bit:131072:1", "byte:32768:1"]
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    boards = {}
    for sp in specs:
        layout, n, k = sp.split(":")
        n, k = int(n), int(k)
        e = gh.Engine(n, n, layout=layout, tblock_k=k)
        e.initialize_board("stream", 1)
        first = e.digest()   # (allocates the digest slots: nothing is allocated beside the probe)
        t = time.perf_counter()
        e.step(10 * k)
        e.sync()
        per_step = (time.perf_counter() - t) / 10
        e.step(max(0, int(a.settle_s / per_step)) * k)
        e.sync()
        boards[sp] = (e, n, k, min(MAX_PENDING, max(4, int(a.window_s / per_step))), first)
    rec = {sp: [] for sp in specs}
    for rnd in range(max(3, a.rounds)):
        for sp, (e, n, k, w, _) in boards.items():   # the boards take turns
            e.step(w * k)
            plain = e.sync() / w
            for _ in range(w):
                e.step(k)
                e.digest_async()
            with_digest = e.sync() / w
            t = time.perf_counter()
            for _ in range(a.digests):
                d = e.digest()
            digest_ms = (time.perf_counter() - t) * 1e3 / a.digests
            e.clock_start(PROBE_MAX_MS)
            e.step(w * k)
            e.sync()
            clk = e.clock_stop()[0]
            r = {"spec": sp, "round": rnd, "k_steps": w, "ms_per_k_step": round(plain, 5),
                 "ms_per_k_step_with_digest": round(with_digest, 5), "ms_per_digest": round(digest_ms, 5),
                 "digest_gb_per_s": round(n * n / (8 if sp.startswith("bit") else 1) / digest_ms / 1e6, 1),
                 "sclk_mhz_next_window": round(clk, 1), "digest": f"{d[0]:016x}{d[1]:016x}"}
            rec[sp].append(r)
            emit(r)
    for sp, (e, n, k, w, first) in boards.items():
        med = {f: statistics.median(r[f] for r in rec[sp])
               for f in ("ms_per_k_step", "ms_per_k_step_with_digest", "ms_per_digest", "sclk_mhz_next_window")}
        s = {"spec": sp, "summary": True, **{f: round(v, 5) for f, v in med.items()},
             "digest_behind_step_ms": round(med["ms_per_k_step_with_digest"] - med["ms_per_k_step"], 5),
             "digest_gb_per_s": round(n * n / (8 if sp.startswith("bit") else 1) / med["ms_per_digest"] / 1e6, 1),
             "spread_ms_per_digest": [min(r["ms_per_digest"] for r in rec[sp]), max(r["ms_per_digest"] for r in rec[sp])],
             "digest_generation_0": f"{first[0]:016x}{first[1]:016x}", "generation": e.generation,
             "version": gh.version()}
        if k == 1:   # the yardstick: this board's own k = 1 step
            s["digest_over_step"] = round(med["ms_per_digest"] / med["ms_per_k_step"], 4)
        emit(s)
        e.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
