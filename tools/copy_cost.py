#!/usr/bin/env python3
"""What a whole-board gol_copy_window costs (include/golhip.h) on one GPU, measured
beside single generations, gol_digest and the packed download + upload of the same
boards in the same run — one process, the cases taking turns after a settle phase,
the clock probe's figure beside every line.

    python tools/copy_cost.py [--n 131072] [--byte-n 32768] [--rounds 3] [--out FILE]

Boards: A and B, bit n x n at tblock_k = 16 (4-word groups); C, bit n x n at
tblock_k = 1 (2-word groups); D, byte m x m; E, bit m x m at tblock_k = 16.  Per
round, --calls back-to-back calls each (host wall clock per call: every call
synchronises, so this is the kernel plus one launch and the stream syncs), with the
probe running on the destination:
  * g4_g4_replace       A -> B, the whole board, aligned (the storage words are merged as they are)
  * g2_g4_replace       C -> B, the whole board
  * g4_g4_shift1        A -> B, (n - 1) columns moved one column to the right
  * g4_g4_or            A -> B, the whole board, OR
  * byte_bit_replace    D -> E, the whole board
and beside them a timed window of single generations of B and E (device ms between
events), gol_digest of B, and one gol_download_bits + gol_upload_bits of B: the host
route that the copy replaces.  Every copy is verified by the digests of the two boards
(equal after REPLACE).  One JSON line per round, one summary line.  A measurement,
not a gate.  The default --out is profiles/copy_cost.jsonl.
"""
import argparse
import json
import os
import statistics
import sys
import time

# the boards' streams and the probe's want hardware queues of their own (see bench.py)
if int(os.environ.get("GPU_MAX_HW_QUEUES", "4") or 4) < 24:
    os.environ["GPU_MAX_HW_QUEUES"] = "24"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpi_amd import golhip as gh  # noqa: E402

PROBE_MAX_MS = 20000.0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=131072, help="side of the bit boards")
    p.add_argument("--byte-n", type=int, default=32768, help="side of the byte board and its bit destination")
    p.add_argument("--rounds", type=int, default=3, help="rounds (at least 3)")
    p.add_argument("--window-s", type=float, default=0.2, help="seconds of steps per timed window")
    p.add_argument("--settle-s", type=float, default=1.0)
    p.add_argument("--calls", type=int, default=10, help="back-to-back calls per round and case")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "copy_cost.jsonl"),
                   help="append the JSON lines to this file as well ('' for none)")
    a = p.parse_args()
    n, m = a.n, a.byte_n
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

    A = gh.Engine(n, n, layout="bit", tblock_k=16)
    B = gh.Engine(n, n, layout="bit", tblock_k=16)
    C = gh.Engine(n, n, layout="bit", tblock_k=1)
    D = gh.Engine(m, m, layout="byte", tblock_k=1)
    E = gh.Engine(m, m, layout="bit", tblock_k=16)
    A.fill_random(0.375, seed=1)
    C.fill_random(0.375, seed=2)
    D.fill_random(0.375, seed=3)
    B.fill_random(0.5, seed=4)
    E.fill_random(0.5, seed=5)
    da, dc, dd = A.digest(), C.digest(), D.digest()
    B.digest()   # (allocates its digest slots before any probe runs)
    E.digest()
    # (window, at, op) per case; the digest the destination must have afterwards, where it is known
    cases = (("g4_g4_replace", A, B, None, (0, 0), "replace", da),
             ("g2_g4_replace", C, B, None, (0, 0), "replace", dc),
             ("g4_g4_shift1", A, B, (0, 0, n, n - 1), (0, 1), "replace", None),
             ("g4_g4_or", A, B, None, (0, 0), "or", None),
             ("byte_bit_replace", D, E, None, (0, 0), "replace", dd))
    for name, src, dst, win, at, op, want in cases:   # every case is checked once
        dst.copy_from(src, win, at, op)
        if want is not None and dst.digest() != want:
            raise SystemExit(f"{name}: the destination's digest differs from the source's")
    # the shifted copy, copied back one column to the left into C, must be A's columns 0 .. n - 2 again
    B.copy_from(A, (0, 0, n, n - 1), (0, 1))
    C.copy_from(B, (0, 1, n, n - 1), (0, 0))
    if C.digest_window(0, 0, n, n - 1) != A.digest_window(0, 0, n, n - 1):
        raise SystemExit("g4_g4_shift1: the shifted copy, copied back, differs from the source")
    C.fill_random(0.375, seed=2)
    # settle: steps of B and E past the clock ramp of a GPU that idled
    gens = {}
    for e, key in ((B, "n"), (E, "m")):
        t0 = time.perf_counter()
        e.step(10)
        e.sync()
        per_gen = (time.perf_counter() - t0) / 10
        gens[key] = max(4, int(a.window_s / per_gen))
        e.step(max(16, int(a.settle_s / per_gen) // 16 * 16))
        e.sync()
    bits = B.download_bits()   # (pools the staging of the packed route)
    B.upload_bits(bits)
    rec = []
    for rnd in range(max(3, a.rounds)):
        r = {"round": rnd, "calls": a.calls, "n": n, "byte_n": m}
        for e, key, tag in ((B, "n", "bit_n"), (E, "m", "bit_m")):
            for _ in range(gens[key]):
                e.step(1)
            r[f"ms_per_generation_k1_{tag}"] = round(e.sync() / gens[key], 5)
        for name, src, dst, win, at, op, _ in cases:   # the cases take turns
            dst.clock_start(PROBE_MAX_MS)
            r["ms_per_copy_" + name] = wall(lambda: dst.copy_from(src, win, at, op), a.calls)
            r["sclk_mhz_copy_" + name] = round(dst.clock_stop()[0], 1)
        B.clock_start(PROBE_MAX_MS)
        r["ms_per_digest_bit_n"] = wall(B.digest, a.calls)
        r["sclk_mhz_digest_bit_n"] = round(B.clock_stop()[0], 1)
        r["ms_per_download_bits"] = wall(lambda: B.download_bits(), 1)
        r["ms_per_upload_bits"] = wall(lambda: B.upload_bits(bits), 1)
        rec.append(r)
        emit(r)
    fields = [f for f in rec[0] if f.startswith("ms_") or f.startswith("sclk")]
    med = {f: statistics.median(r[f] for r in rec) for f in fields}
    s = {"summary": True, "n": n, "byte_n": m, **{f: round(v, 5) for f, v in med.items()}, "version": gh.version()}
    # bytes a case moves: the source board read, the destination board written (and read, where it is merged)
    bit_n, bit_m, byte_m = n * n // 8, m * m // 8, m * m
    moved = {"g4_g4_replace": 2 * bit_n, "g2_g4_replace": 2 * bit_n, "g4_g4_shift1": 2 * bit_n, "g4_g4_or": 3 * bit_n,
             "byte_bit_replace": byte_m + bit_m}
    for name, src, dst, *_ in cases:
        ms = med["ms_per_copy_" + name]
        gen = med["ms_per_generation_k1_bit_n" if dst is B else "ms_per_generation_k1_bit_m"]
        s["gb_per_s_" + name] = round(moved[name] / ms / 1e6, 1)
        s["copy_over_generation_" + name] = round(ms / gen, 3)
        s["spread_ms_per_copy_" + name] = [min(r["ms_per_copy_" + name] for r in rec),
                                           max(r["ms_per_copy_" + name] for r in rec)]
    s["gb_per_s_generation_k1_bit_n"] = round(2 * bit_n / med["ms_per_generation_k1_bit_n"] / 1e6, 1)
    s["host_route_over_copy"] = round((med["ms_per_download_bits"] + med["ms_per_upload_bits"]) /
                                      med["ms_per_copy_g4_g4_replace"], 1)
    emit(s)
    for e in (A, B, C, D, E):
        e.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
