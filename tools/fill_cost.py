#!/usr/bin/env python3
"""What a whole-board gol_fill_random costs (include/golhip.h) on one GPU, measured
beside gol_init_glibc(GOL_INIT_STREAM), a packed gol_upload_bits and single
generations of the same board and build — one process, the boards taking turns
after a settle phase, the clock recorded.

    python tools/fill_cost.py [--spec LAYOUT:N:K ...] [--rounds 3] [--out FILE]

Default specs: bit:131072:16 (4-word groups), bit:131072:1 (2-word groups) and
byte:32768:1; the default --out is profiles/fill_cost.jsonl.  Per spec the board is
filled and stepped through a settle phase (the clock ramp of a GPU that idled,
DESIGN.md §5), then per round:
  * per threshold 2^31, 3·2^29 and 0x55555555 (1, 3 and 32 planes: 1, 2 and 16 sm
    per 32 cells) and for the two constant fills, --calls back-to-back gol_fill_random
    calls beside the clock probe (the fill allocates nothing): host wall clock per
    call — every call synchronises, so this is the kernel plus one launch and one
    stream sync — and the shader clock over those calls;
  * a timed window of single generations (gol_step(1) each; device ms between
    events, gol_sync): the k = 1 yardstick of this board;
  * one gol_init_glibc(GOL_INIT_STREAM) and one gol_upload_bits of the board's own
    packed rows (host wall clock).
Every fill is verified by gol_popcount against n·T / 2^32 within 5 sigma, and the
three boards of a square size must agree on the digest of the same (seed, T).  One
JSON line per round, one summary line per spec.  A measurement, not a gate.
"""
import argparse
import json
import math
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
FILLS = (("t_2p31", 1 << 31), ("t_3_2p29", 3 << 29), ("t_55555555", 0x55555555), ("t_0", 0), ("t_2p32", 1 << 32))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--spec", action="append", help="LAYOUT:N:K (default: bit:131072:16 bit:131072:1 byte:32768:1)")
    p.add_argument("--rounds", type=int, default=3, help="rounds per board (at least 3)")
    p.add_argument("--window-s", type=float, default=0.2, help="seconds of steps per timed window")
    p.add_argument("--settle-s", type=float, default=1.0)
    p.add_argument("--calls", type=int, default=10, help="back-to-back fills per round and threshold")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill_cost.jsonl"),
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

    def wall(fn, calls):
        t = time.perf_counter()
        for _ in range(calls):
            fn()
        return round((time.perf_counter() - t) * 1e3 / calls, 5)

    boards, digests = {}, {}
    for sp in specs:
        layout, n, k = sp.split(":")
        n, k = int(n), int(k)
        e = gh.Engine(n, n, layout=layout, tblock_k=k)
        for name, t in FILLS:   # every fill is checked once: the live count, and the digest across the boards
            e.fill_random(seed=1, threshold=t)
            live, pr = e.popcount(), t / 2**32
            if abs(live - n * n * pr) > 5 * math.sqrt(n * n * pr * (1 - pr)) + 1:
                raise SystemExit(f"{sp} {name}: {live} live cells, expected about {n * n * pr:.0f}")
            if digests.setdefault((n, name), e.digest()) != e.digest():
                raise SystemExit(f"{sp} {name}: this board's digest differs from another layout's")
        e.fill_random(0.375, seed=1)
        t0 = time.perf_counter()
        e.step(10)
        e.sync()
        per_gen = (time.perf_counter() - t0) / 10
        w = max(4, int(a.window_s / per_gen))
        bits = e.download_bits()   # (pools the staging of the packed upload)
        e.upload_bits(bits)
        e.step(max(k, int(a.settle_s / per_gen) // k * k))
        e.sync()
        boards[sp] = (e, n, k, w, bits)
    rec = {sp: [] for sp in specs}
    for rnd in range(max(3, a.rounds)):
        for sp, (e, n, k, w, bits) in boards.items():   # the boards take turns
            r = {"spec": sp, "round": rnd, "generations": w, "calls": a.calls}
            for _ in range(w):
                e.step(1)
            r["ms_per_generation_k1"] = round(e.sync() / w, 5)
            for name, t in FILLS:
                e.clock_start(PROBE_MAX_MS)
                r["ms_per_fill_" + name] = wall(lambda: e.fill_random(seed=rnd, threshold=t), a.calls)
                r["sclk_mhz_fill_" + name] = round(e.clock_stop()[0], 1)
            r["ms_per_init_glibc_stream"] = wall(lambda: e.initialize_board("stream", 1), 1)
            r["ms_per_upload_bits"] = wall(lambda: e.upload_bits(bits), 1)
            rec[sp].append(r)
            emit(r)
    for sp, (e, n, k, w, bits) in boards.items():
        fields = [f for f in rec[sp][0] if f.startswith("ms_") or f.startswith("sclk")]
        med = {f: statistics.median(r[f] for r in rec[sp]) for f in fields}
        board_bytes = n * n // (8 if sp.startswith("bit") else 1)
        s = {"spec": sp, "summary": True, **{f: round(v, 5) for f, v in med.items()}, "board_bytes": board_bytes,
             "version": gh.version()}
        for name, _ in FILLS:
            ms = med["ms_per_fill_" + name]
            s["gb_per_s_written_" + name] = round(board_bytes / ms / 1e6, 1)
            s["fill_over_generation_" + name] = round(ms / med["ms_per_generation_k1"], 3)
            s["spread_ms_per_fill_" + name] = [min(r["ms_per_fill_" + name] for r in rec[sp]),
                                               max(r["ms_per_fill_" + name] for r in rec[sp])]
        emit(s)
        e.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
