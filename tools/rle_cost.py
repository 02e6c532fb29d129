#!/usr/bin/env python3
"""What writing a board as RLE costs (gol_write_rle / gol_rle_bytes, include/golhip.h)
on one GPU, beside the packed download of the same window (gol_download_bits_window:
the first half of any route through the host) — one process, the boards taking turns,
the clock recorded.

    python tools/rle_cost.py [--n 131072] [--rounds 3] [--block-mib 64] [--out FILE]

Three bit boards of n x n cells (k = 16):
  gun     a single Gosper gun after 600 generations, the whole board
  aged    the srand(1) soup aged 1000 generations, the whole board
  fresh   the srand(1) soup as seeded, a window of n / 4 x n / 4 (the text stays near a
          gigabyte at n = 131072)
Per round and board, each call synchronising (host wall clock):
  ms_write_rle       gol_write_rle of the window to /dev/null: packed staging, row pass,
                     row scan, write pass, the copy of the text and the host's write()
  ms_rle_bytes       gol_rle_bytes: the two counting passes, nothing but the record crosses PCIe
  ms_download_bits   gol_download_bits_window into host memory
and once per board the bytes written.  Before the rounds a short window of steps runs
beside the clock probe (its reading is recorded).  The default --out is
profiles/rle_cost.jsonl.  One JSON line per round, one summary line per board.  A
measurement, not a gate.
"""
import argparse
import json
import os
import statistics
import sys
import time

if int(os.environ.get("GPU_MAX_HW_QUEUES", "4") or 4) < 24:
    os.environ["GPU_MAX_HW_QUEUES"] = "24"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpi_amd import golhip as gh  # noqa: E402

GUN = (b"x = 36, y = 9, rule = B3/S23\n"
       b"24bo$22bobo$12b2o6b2o12b2o$11bo3bo4b2o12b2o$2o8bo5bo3b2o$2o8bo3bob2o4bobo$10bo5bo7bo$11bo3bo$12b2o!\n")
PROBE_MAX_MS = 20000.0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=131072)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--block-mib", type=int, default=64, help="GOL_OPT_TEXT_BLOCK_BYTES in MiB (the default is 64)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "rle_cost.jsonl"),
                   help="append the JSON lines to this file as well ('' for none)")
    a = p.parse_args()
    n, k = a.n, 16
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    boards = {}
    for name in ("gun", "aged", "fresh"):
        e = gh.Engine(n, n, layout="bit", tblock_k=k)
        e.set_option(gh.OPT_TEXT_BLOCK_BYTES, a.block_mib << 20)
        win = (0, 0, n, n)
        if name == "gun":
            e.parse_rle(GUN, at=(n // 2, n // 2))
            e.step(600)
        else:
            e.initialize_board("stream", 1)
            if name == "aged":
                e.step(1000)
            else:
                win = (0, 0, n // 4, n // 4)
        e.sync()
        e.clock_start(PROBE_MAX_MS)
        e.step(4 * k)
        e.sync()
        mhz = round(e.clock_stop()[0], 1)
        boards[name] = (e, win, mhz, e.popcount(), e.generation)
    null = os.open("/dev/null", os.O_WRONLY)
    rec = {b: [] for b in boards}
    for rnd in range(a.rounds):
        for name, (e, win, mhz, live, gen) in boards.items():   # the boards take turns
            def wall(fn):
                t = time.perf_counter()
                v = fn()
                return round((time.perf_counter() - t) * 1e3, 3), v

            r = {"board": name, "round": rnd, "n": n, "window": list(win), "block_mib": a.block_mib}
            r["ms_write_rle"], _ = wall(lambda: e._chk(e.lib.gol_write_rle(e._c, *win, null), "gol_write_rle"))
            r["ms_rle_bytes"], r["rle_bytes"] = wall(lambda: e.rle_bytes(win))
            r["ms_download_bits"], bits = wall(lambda: e.download_bits_window(*win))
            r["packed_bytes"] = int(bits.size)
            del bits
            rec[name].append(r)
            emit(r)
    for name, (e, win, mhz, live, gen) in boards.items():
        s = {"board": name, "summary": True, "n": n, "window": list(win), "block_mib": a.block_mib,
             "generation": gen, "live": live, "sclk_mhz_step_window": mhz,
             "rle_bytes": rec[name][0]["rle_bytes"], "packed_bytes": rec[name][0]["packed_bytes"],
             **{f: statistics.median(r[f] for r in rec[name]) for f in ("ms_write_rle", "ms_rle_bytes", "ms_download_bits")},
             "spread_ms_write_rle": [min(r["ms_write_rle"] for r in rec[name]), max(r["ms_write_rle"] for r in rec[name])],
             "version": gh.version()}
        emit(s)
        e.close()
    os.close(null)
    if out:
        out.close()


if __name__ == "__main__":
    main()
