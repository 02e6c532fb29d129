#!/usr/bin/env python3
"""What the density map costs (gol_density*, include/golhip.h) on one GPU: ms per
whole-board map at tiles of 128 x 128 and 1024 x 1024, measured beside gol_digest
and the k = 1 step of the same board and build — one process, the boards taking
turns after a settle phase, the clock recorded.

    python tools/density_cost.py [--spec LAYOUT:N:K ...] [--rounds 3] [--window-s 0.2] [--out FILE]

Default specs: bit:131072:16 (4-word groups), bit:131072:1 (2-word groups) and
byte:32768:1; the default --out is profiles/density_cost.jsonl.  Per spec the
board is seeded (srand(1) row-major) and stepped through a settle phase (the
clock ramp of a GPU that idled), then per round:
  * a timed window of k-steps (device ms between events, gol_sync);
  * the same window with a digest_async, then with a density_async of each tile
    size, behind every k-step: the difference to the plain window is what the
    reduction costs ON THE DEVICE behind a step (launch, memset and the D2H copy
    of the part included, no host wait).  At most --pending maps are pending at
    once (each holds a pooled staging pair of trows x tcols x 4 bytes), so these
    windows are cut to that many k-steps;
  * back-to-back synchronising calls, gol_digest and gol_density per tile size
    (host wall clock per call: launch, sync, and for the map the D2H copy and the
    host's delivery of trows x tcols counts are inside the figure);
  * the plain window again beside the clock probe (as bench.py: the timed
    windows run without the probe's wave).
One JSON line per round, one summary line per spec.  A measurement, not a gate.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpi_amd import golhip as gh  # noqa: E402

PROBE_MAX_MS = 20000.0
TILES = (128, 1024)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--spec", action="append", help="LAYOUT:N:K (default: bit:131072:16 bit:131072:1 byte:32768:1)")
    p.add_argument("--rounds", type=int, default=3, help="rounds per board (at least 3)")
    p.add_argument("--window-s", type=float, default=0.2, help="seconds of steps per timed window")
    p.add_argument("--settle-s", type=float, default=1.0)
    p.add_argument("--calls", type=int, default=20, help="back-to-back synchronising calls per round and kind")
    p.add_argument("--pending", type=int, default=48, help="maps pending per sync at most")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_cost.jsonl"),
                   help="append the JSON lines to this file as well ('' for none)")
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
        e.digest()   # (allocates the digest slots: nothing is allocated beside the probe)
        t = time.perf_counter()
        e.step(10 * k)
        e.sync()
        per_step = (time.perf_counter() - t) / 10
        w = max(4, int(a.window_s / per_step))
        wd = min(w, a.pending)
        for tile in TILES:   # pools the parts' staging: no allocation inside a timed window
            for _ in range(wd):
                e.density_async(tile)
            e.sync()
        first = e.density(TILES[0])
        # the maps agree with each other and with gol_popcount at this size too
        f = TILES[1] // TILES[0]
        coarse = first.astype("uint64").reshape(first.shape[0] // f, f, first.shape[1] // f, f).sum(axis=(1, 3))
        if (coarse != e.density(TILES[1])).any() or int(first.sum(dtype="uint64")) != e.popcount():
            raise SystemExit(f"{sp}: the {TILES[0]} map, the {TILES[1]} map and gol_popcount disagree")
        e.step(max(0, int(a.settle_s / per_step)) * k)
        e.sync()
        boards[sp] = (e, n, k, w, wd, int(first.sum(dtype="uint64")))
    rec = {sp: [] for sp in specs}
    for rnd in range(max(3, a.rounds)):
        for sp, (e, n, k, w, wd, _) in boards.items():   # the boards take turns
            e.step(w * k)
            plain = e.sync() / w
            e.step(wd * k)
            plain_short = e.sync() / wd
            for _ in range(wd):
                e.step(k)
                e.digest_async()
            r = {"spec": sp, "round": rnd, "k_steps": w, "k_steps_with_reduction": wd, "ms_per_k_step": round(plain, 5),
                 "ms_per_k_step_short_window": round(plain_short, 5),
                 "ms_per_k_step_with_digest": round(e.sync() / wd, 5)}
            for tile in TILES:
                for _ in range(wd):
                    e.step(k)
                    e.density_async(tile)
                r[f"ms_per_k_step_with_density_{tile}"] = round(e.sync() / wd, 5)
            t = time.perf_counter()
            for _ in range(a.calls):
                e.digest()
            r["ms_per_digest"] = round((time.perf_counter() - t) * 1e3 / a.calls, 5)
            for tile in TILES:
                t = time.perf_counter()
                for _ in range(a.calls):
                    d = e.density(tile)
                r[f"ms_per_density_{tile}"] = round((time.perf_counter() - t) * 1e3 / a.calls, 5)
            e.clock_start(PROBE_MAX_MS)
            e.step(w * k)
            e.sync()
            r["sclk_mhz_next_window"] = round(e.clock_stop()[0], 1)
            r["live"] = int(d.sum(dtype="uint64"))
            rec[sp].append(r)
            emit(r)
    for sp, (e, n, k, w, wd, live0) in boards.items():
        fields = [f for f in rec[sp][0] if f.startswith("ms_") or f.startswith("sclk")]
        med = {f: statistics.median(r[f] for r in rec[sp]) for f in fields}
        nbytes = n * n / (8 if sp.startswith("bit") else 1)
        s = {"spec": sp, "summary": True, **{f: round(v, 5) for f, v in med.items()},
             "digest_behind_step_ms": round(med["ms_per_k_step_with_digest"] - med["ms_per_k_step_short_window"], 5)}
        for tile in TILES:
            behind = med[f"ms_per_k_step_with_density_{tile}"] - med["ms_per_k_step_short_window"]
            s[f"density_{tile}_behind_step_ms"] = round(behind, 5)
            s[f"density_{tile}_behind_step_gb_per_s"] = round(nbytes / behind / 1e6, 1) if behind > 0 else None
            s[f"spread_ms_per_density_{tile}"] = [min(r[f"ms_per_density_{tile}"] for r in rec[sp]),
                                                   max(r[f"ms_per_density_{tile}"] for r in rec[sp])]
        s.update({"live_generation_0": live0, "generation": e.generation, "version": gh.version()})
        if k == 1:   # the yardstick: this board's own k = 1 step
            s["digest_over_step"] = round(med["ms_per_digest"] / med["ms_per_k_step"], 4)
            for tile in TILES:
                s[f"density_{tile}_over_step"] = round(med[f"ms_per_density_{tile}"] / med["ms_per_k_step"], 4)
        emit(s)
        e.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
