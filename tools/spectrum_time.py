#!/usr/bin/env python3
"""Time of kgma_genome_kmer_count (the library's hipEvents around the rows' memset and the launch, kgma_get_spectrum_stats) on a
synthetic genome of four equal records (--bases in all) held on one MI355X.  Cases:

  whole_k{1,4,6,7,8,10}   every whole record as one range, flags == 0
  bins1000_k{1,2}         api.composition_track: BY_START bins of 1000 starts, SKIP_N
  n_run_k6                the whole records at k = 6, flags == 0, after a stretch of --n-run residues of the second record was poked
                          to N (every k-mer of the stretch is T...T: the contention case)

Per case: median / min / max of --reps calls after --warmup, bases per second, and the fraction of the device copy rate for the
1 byte per base that is read (COPY_RATE: the 6.29 TB/s the README and DESIGN.md quote; not re-derived here).

The route the library had to the same numbers before this call -- Genome.fetch_batch of the ranges, then
Context.kmer_count_batch -- is timed in the same run (wall clock: it crosses the link twice) on a record of --parent-bases
residues, for the whole record at every k above and for the bins at k = 1 and 2; the new call is timed on that same record too,
and the two results are compared value for value.  Run it under a time limit of its own
(`timeout -k 10 900 python tools/spectrum_time.py ...`).

usage: python tools/spectrum_time.py [--bases 400e6] [--parent-bases 16e6] [--n-run 64e6] [--reps 7] [--warmup 2]
                                     [--out profiles/spectrum_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmergma.jl_amd")]

from kmergma_amd import _lib, api  # noqa: E402

COPY_RATE = 6.29e12          # bytes per second, measured device copy (README.md)
FORMS = ("wg", "wave", "global")
WHOLE_KS = (1, 4, 6, 7, 8, 10)


def spread(ms):
    return {"min_ms": round(min(ms), 4), "median_ms": round(float(np.median(ms)), 4), "max_ms": round(max(ms), 4)}


def timed(ctx, call, reps, warmup, bases):
    ms = []
    for it in range(warmup + reps):
        call()
        st = ctx.spectrum_stats()
        if it >= warmup:
            ms.append(st["count_ms"])
    med = float(np.median(ms)) * 1e-3
    return dict(spread(ms), form=FORMS[st["form"]], span=st["span"], n_workgroups=st["n_workgroups"], n_ranges=st["n_ranges"],
                n_positions=st["n_positions"], Gbases_per_s=round(bases / med / 1e9, 2), fraction_of_copy_rate=round(bases / med / COPY_RATE, 4))


def wall(call, reps):
    out, sec = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        sec.append(time.perf_counter() - t0)
    return out, float(np.median(sec))


def parent_route(ctx, n_bases, reps, warmup):
    """fetch_batch + kmer_count_batch against the new call, on one record of n_bases residues."""
    g = ctx.genome_synthetic([n_bases], 79)
    rows = {"bases": n_bases, "clock": "wall, median of %d (the parent's route crosses the link; the new call's count_ms is beside it)" % max(1, reps // 2)}
    bins = [(0, lo, min(1000, n_bases - lo + 1)) for lo in range(1, n_bases + 1, 1000)]
    for name, k, ranges in [(f"whole_k{k}", k, [(0, 1, n_bases)]) for k in WHOLE_KS] + [(f"bins1000_k{k}", k, bins) for k in (1, 2)]:
        contig, lo, hi = [r[0] for r in ranges], [r[1] for r in ranges], [r[1] + r[2] - 1 for r in ranges]
        old, old_s = wall(lambda: ctx.kmer_count_batch(g.fetch_batch(ranges), k), max(1, reps // 2))
        (new, _), new_s = wall(lambda: ctx.genome_kmer_count(g, k, contig, lo, hi), max(1, reps // 2))
        dev = timed(ctx, lambda: ctx.genome_kmer_count(g, k, contig, lo, hi), reps, warmup, n_bases)
        rows[name] = {"parent_route_s": round(old_s, 4), "new_call_wall_s": round(new_s, 4), "new_call_count_ms": dev["median_ms"], "form": dev["form"],
                      "equal": bool(np.array_equal(new, old.astype(np.int64))), "parent_over_new_wall": round(old_s / new_s, 1)}
        print(json.dumps({name: rows[name]}), flush=True)
    g.free()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", default="400e6")
    ap.add_argument("--parent-bases", default="16e6")
    ap.add_argument("--n-run", default="64e6")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n, n_run, R, W = int(float(args.bases)), int(float(args.n_run)), args.reps, args.warmup
    ctx = _lib.Context(0)
    lens = [n // 4] * 4
    n = sum(lens)
    g = ctx.genome_synthetic(lens, 77)
    whole = ([0, 1, 2, 3], [1] * 4, lens)
    rows = {"records": 4, "bases": n, "copy_rate_bytes_per_s": COPY_RATE}
    for k in WHOLE_KS:
        rows[f"whole_k{k}"] = timed(ctx, lambda: ctx.genome_kmer_count(g, k, *whole), R, W, n)
        print(json.dumps({f"whole_k{k}": rows[f"whole_k{k}"]}), flush=True)
    for k in (1, 2):
        rows[f"bins1000_k{k}"] = timed(ctx, lambda: api.composition_track(g, 1000, k, ctx=ctx), R, W, n)
        print(json.dumps({f"bins1000_k{k}": rows[f"bins1000_k{k}"]}), flush=True)
    if n_run > 0:
        n_run = min(n_run, lens[1])
        at = (lens[1] - n_run) // 2 + 1
        for lo in range(0, n_run, 1 << 24):
            g.poke(1, at + lo, b"N" * min(1 << 24, n_run - lo))
        rows["n_run_k6"] = dict(timed(ctx, lambda: ctx.genome_kmer_count(g, 6, *whole), R, W, n), n_run=n_run)
        counts, _ = ctx.genome_kmer_count(g, 6, *whole)
        rows["n_run_k6"]["count_of_the_all_T_kmer"] = int(counts[1, -1])
        print(json.dumps({"n_run_k6": rows["n_run_k6"]}), flush=True)
    g.free()
    n_parent = int(float(args.parent_bases))
    if n_parent > 0:
        rows["parent_route"] = parent_route(ctx, n_parent, R, W)
    ctx.close()
    out = {"tool": "tools/spectrum_time.py", "reps": R, "warmup": W, "genome": rows}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
