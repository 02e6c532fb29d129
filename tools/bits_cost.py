#!/usr/bin/env python3
"""What 1-bit-per-cell board I/O costs (gol_download_bits* / gol_upload_bits*,
include/golhip.h) on one GPU, measured beside gol_digest and the k = 1 step of the
same board and build — one process, the boards taking turns after a settle phase,
the clock recorded.

    python tools/bits_cost.py [--spec LAYOUT:N:K ...] [--rounds 3] [--out FILE]

Default specs: bit:131072:16 (4-word groups), bit:131072:1 (2-word groups) and
byte:32768:1; the default --out is profiles/bits_cost.jsonl.  Per spec the board
is seeded (srand(1) row-major) and stepped through a settle phase (the clock ramp
of a GPU that idled), then per round:
  * a timed window of k-steps (device ms between events, gol_sync), and this
    board's k = 1 yardstick where k = 1;
  * the same window with a whole-board gol_download_bits_window_async behind every
    k-step: the difference to the plain window is what the packed copy costs ON
    THE DEVICE behind a step — the staging memset, the pack kernel and the D2H copy
    of the packed rows on the compute stream, no host wait.  Each pending copy
    holds a pooled staging pair of the packed board's size, so these windows are
    --pending k-steps long;
  * back-to-back synchronising calls: gol_digest, gol_download_bits (kernel, D2H
    copy and the host's delivery, in 64-MiB row blocks) and gol_upload_bits (host
    wall clock per call);
  * a byte-per-cell gol_download_window of a 16384² window and the packed download
    of the same window (host wall clock per call);
  * the plain window again beside the clock probe (as bench.py: the timed windows
    run without the probe's wave).
The packed board is verified on the host with a byte-popcount table against
gol_popcount, and the upload by the digest of the board it leaves.  One JSON line
per round, one summary line per spec.  A measurement, not a gate.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

# the board's streams and the probe's want hardware queues of their own (see bench.py)
if int(os.environ.get("GPU_MAX_HW_QUEUES", "4") or 4) < 24:
    os.environ["GPU_MAX_HW_QUEUES"] = "24"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpi_amd import golhip as gh  # noqa: E402

PROBE_MAX_MS = 20000.0
WIN = 16384
POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def popcount_packed(bits):
    total = 0
    for a in range(0, bits.shape[0], 4096):   # row blocks: the table lookup makes a copy
        total += int(POP8[bits[a:a + 4096]].sum(dtype=np.uint64))
    return total


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--spec", action="append", help="LAYOUT:N:K (default: bit:131072:16 bit:131072:1 byte:32768:1)")
    p.add_argument("--rounds", type=int, default=3, help="rounds per board (at least 3)")
    p.add_argument("--window-s", type=float, default=0.2, help="seconds of steps per plain timed window")
    p.add_argument("--settle-s", type=float, default=1.0)
    p.add_argument("--calls", type=int, default=3, help="back-to-back synchronising calls per round and kind")
    p.add_argument("--pending", type=int, default=2, help="packed copies pending per sync")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "bits_cost.jsonl"),
                   help="append the JSON lines to this file as well ('' for none)")
    p.add_argument("--trace-run", action="store_true",
                   help="no timing: per board a few whole-board packed downloads and uploads, for a kernel trace "
                        "(rocprofv3 --kernel-trace --stats -- python tools/bits_cost.py --trace-run): the kernels "
                        "alone, get_bits_kernel<G> / put_bits_kernel<G>, G = 4, 2, 0 for the default specs")
    a = p.parse_args()
    specs = a.spec or ["bit:131072:16", "bit:131072:1", "byte:32768:1"]
    if a.trace_run:
        for sp in specs:
            layout, n, k = sp.split(":")
            n, k = int(n), int(k)
            with gh.Engine(n, n, layout=layout, tblock_k=k) as e:
                e.initialize_board("stream", 1)
                e.step(4 * k)
                for _ in range(5):
                    bits = e.download_bits_window_async(0, 0, n, n)   # one launch for the whole board
                    e.sync()
                for _ in range(5):
                    e.upload_bits_window(0, 0, n, bits[:min(n, 4096)])   # (one 64-MiB row block: one launch)
        return
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
        win = min(WIN, n)
        keep = [e.download_bits_window_async(0, 0, n, n) for _ in range(a.pending)]   # pools the staging
        e.sync()
        live = e.popcount()
        if popcount_packed(keep[0]) != live or (keep[0] != keep[-1]).any():
            raise SystemExit(f"{sp}: popcount of the packed board and gol_popcount disagree")
        bits = e.download_bits()   # (pools the 64-MiB blocks of the synchronising form)
        if (bits != keep[0]).any():
            raise SystemExit(f"{sp}: the synchronising and the async packed download disagree")
        d0 = e.digest()
        e.upload_bits(bits)
        if e.digest() != d0 or e.popcount() != live:
            raise SystemExit(f"{sp}: the board after gol_upload_bits of its own rows has another digest")
        e.download_window(0, 0, win, win)
        e.download_bits_window(0, 0, win, win)
        del keep
        e.step(max(0, int(a.settle_s / per_step)) * k)
        e.sync()
        boards[sp] = (e, n, k, w, win, bits, live)
    rec = {sp: [] for sp in specs}
    for rnd in range(max(3, a.rounds)):
        for sp, (e, n, k, w, win, bits, _) in boards.items():   # the boards take turns
            e.step(w * k)
            plain = e.sync() / w
            e.step(a.pending * k)
            plain_short = e.sync() / a.pending
            keep = []
            for _ in range(a.pending):
                e.step(k)
                keep.append(e.download_bits_window_async(0, 0, n, n))
            r = {"spec": sp, "round": rnd, "k_steps": w, "k_steps_with_copy": a.pending,
                 "ms_per_k_step": round(plain, 5), "ms_per_k_step_short_window": round(plain_short, 5),
                 "ms_per_k_step_with_bits_async": round(e.sync() / a.pending, 5)}
            del keep

            def wall(fn, calls=a.calls):
                t = time.perf_counter()
                for _ in range(calls):
                    fn()
                return round((time.perf_counter() - t) * 1e3 / calls, 5)

            r["ms_per_digest"] = wall(e.digest, 20)
            r["ms_per_download_bits"] = wall(e.download_bits)
            r["ms_per_download_bits_window_16384"] = wall(lambda: e.download_bits_window(0, 0, win, win))
            r["ms_per_download_window_16384"] = wall(lambda: e.download_window(0, 0, win, win))
            cur = e.download_bits()
            r["ms_per_upload_bits"] = wall(lambda: e.upload_bits(cur))
            e.clock_start(PROBE_MAX_MS)
            e.step(w * k)
            e.sync()
            r["sclk_mhz_next_window"] = round(e.clock_stop()[0], 1)
            rec[sp].append(r)
            emit(r)
    for sp, (e, n, k, w, win, bits, live0) in boards.items():
        fields = [f for f in rec[sp][0] if f.startswith("ms_") or f.startswith("sclk")]
        med = {f: statistics.median(r[f] for r in rec[sp]) for f in fields}
        board_bytes = n * n / (8 if sp.startswith("bit") else 1)
        behind = med["ms_per_k_step_with_bits_async"] - med["ms_per_k_step_short_window"]
        s = {"spec": sp, "summary": True, **{f: round(v, 5) for f, v in med.items()},
             "bits_async_behind_step_ms": round(behind, 5),
             "board_bytes": int(board_bytes), "packed_bytes": n * gh.bits_row_bytes(n),
             "download_bits_gb_per_s_packed": round(n * gh.bits_row_bytes(n) / med["ms_per_download_bits"] / 1e6, 2),
             "upload_bits_gb_per_s_packed": round(n * gh.bits_row_bytes(n) / med["ms_per_upload_bits"] / 1e6, 2),
             "window_bytes_over_packed": round(med["ms_per_download_window_16384"] /
                                               med["ms_per_download_bits_window_16384"], 3),
             "spread_ms_per_download_bits": [min(r["ms_per_download_bits"] for r in rec[sp]),
                                             max(r["ms_per_download_bits"] for r in rec[sp])],
             "live_generation_0": live0, "generation": e.generation, "version": gh.version()}
        if k == 1:   # the yardstick: this board's own k = 1 step
            s["bits_async_over_step"] = round(behind / med["ms_per_k_step"], 4)
            s["digest_over_step"] = round(med["ms_per_digest"] / med["ms_per_k_step"], 4)
        emit(s)
        e.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
