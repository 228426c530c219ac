#!/usr/bin/env python3
"""Time of gene assignment (kgma_assign_ranges) against the only device route to the same score matrix before it existed:
kgma_align_hits_device called once per reference (a trace byte per cell to HBM and a traceback per pair, of which only the score
is kept).

Workload: a resident genome of H = 1024 loci, each a fixture gene (tests/data/Alp_V_ref.fasta, taken in turn) with 5 % of its
residues substituted, planted in random sequence; a query is the gene with 50 residues of flank on either side.  References:
R = 84 (the fixture) and R = 512 (copies of the fixture genes with 3 % substituted).  Both routes run on the same inputs in one
process, alternating, after one warm-up call each; every call ends in a stream synchronise, so the host clock around it is the
whole call.  Of the new call the score pass and the trace pass are also timed on the device (kgma_assign_stats, hipEvents).  The
two score matrices must be equal.

usage: python tools/assign_time.py [--hits 1024] [--reps 3] [--out profiles/assign_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmergma.jl_amd")]

from kmergma_amd import _lib, fasta  # noqa: E402

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
FLANK = 50
SLOT = 1000          # residues of genome per locus


def substituted(rng, seq: bytes, rate: float) -> bytes:
    a = np.frombuffer(seq.upper(), dtype=np.uint8).copy()
    hit = rng.random(a.size) < rate
    a[hit] = BASES[rng.integers(0, 4, size=int(hit.sum()))]
    return a.tobytes()


def spread(ms):
    return {"min_ms": round(min(ms), 3), "median_ms": round(float(np.median(ms)), 3), "max_ms": round(max(ms), 3), "runs": len(ms)}


def clocked(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hits", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rng = np.random.default_rng(84)
    genes = [r.sequence for r in fasta.read_fasta(os.path.join(ROOT, "tests", "data", "Alp_V_ref.fasta"))]
    assert max(map(len, genes)) + 2 * FLANK + 100 < SLOT
    H = args.hits
    rec = BASES[rng.integers(0, 4, size=H * SLOT)].copy()
    lo, hi = np.zeros(H, dtype=np.int64), np.zeros(H, dtype=np.int64)
    for i in range(H):
        g = substituted(rng, genes[i % len(genes)], 0.05)
        p = i * SLOT + 100 + int(rng.integers(0, 50))
        rec[p:p + len(g)] = np.frombuffer(g, dtype=np.uint8)
        lo[i], hi[i] = p + 1 - FLANK, p + len(g) + FLANK
    contig = np.zeros(H, dtype=np.int32)
    ref_sets = {"R84": genes, "R512": [substituted(rng, genes[j % len(genes)], 0.03) for j in range(512)]}
    ctx = _lib.Context(0)
    genome = ctx.genome_from_host([rec.tobytes()])
    out = {"tool": "tools/assign_time.py", "hits": H, "flank": FLANK, "reps": args.reps, "gap_open": -69, "gap_extend": -1,
           "timing": "host clock around calls that end in a stream synchronise; score / trace pass: kgma_assign_stats (hipEvents); "
                     "routes alternating after one warm-up call each",
           "baseline": "kgma_align_hits_device once per reference (align_kernel: trace bytes and a traceback for every pair)"}
    for name, refs in ref_sets.items():
        def new():
            return ctx.assign_ranges(genome, refs, contig, lo, hi, -69, -1, 1)

        def old():
            return np.stack([ctx.align_hits_device(genome, r, -69, -1, contig, lo, hi)[2] for r in refs], axis=1)

        (_, S), base = new(), old()                      # warm-up, and the check
        assert np.array_equal(S.astype(np.int64), base), "the two routes disagree"
        call, score, trace, base_call = [], [], [], []
        for _ in range(args.reps):
            ms, _r = clocked(new)
            st = ctx.assign_stats()
            call.append(ms); score.append(st["score_ms"]); trace.append(st["trace_ms"])
            ms, _r = clocked(old)
            base_call.append(ms)
        cells = st["n_cells"]
        out[name] = {"refs": len(refs), "pairs": st["n_pairs"], "cells": cells, "score_launches": st["n_score_launches"],
                     "score_pass": spread(score), "trace_pass": spread(trace), "assign_call": spread(call), "baseline_calls": spread(base_call),
                     "gcups_score_pass": round(cells / (float(np.median(score)) * 1e6), 2),
                     "baseline_over_assign_call": round(float(np.median(base_call) / np.median(call)), 2),
                     "baseline_over_score_pass": round(float(np.median(base_call) / np.median(score)), 2),
                     "slowest_assign_call_beats_fastest_baseline": bool(max(call) < min(base_call)),
                     "scores_equal": True}
    genome.free()
    ctx.close()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
