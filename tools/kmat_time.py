#!/usr/bin/env python3
"""Time of gene assignment with the k-mer prescreen (kgma_assign_ranges_screened, n_near = 8 at k = 6) against the unscreened
call (kgma_assign_ranges), on tools/assign_time.py's workload: a resident genome of H = 1024 loci, each a fixture gene
(tests/data/Alp_V_ref.fasta, taken in turn) with 5 % of its residues substituted, planted in random sequence, a query being the
gene with 50 residues of flank either side; references R = 84 (the fixture) and R = 512 (copies of the fixture genes with 3 %
substituted).

Both routes run on the same inputs in one process, alternating, after one warm-up call each; every call ends in a stream
synchronise, so the host clock around it is the whole call.  Of the screened call the matrix launches, the select launch, the
score pass and the trace pass are also timed on the device (kgma_kmat_stats, kgma_assign_stats: hipEvents).  Recorded too: for how
many of the loci the two routes name the same best reference.

Every reference set is one step: a child process of its own under its own time limit; the first step that fails or runs out of
time ends the run (nothing further is started on the GPU).

usage: python tools/kmat_time.py [--hits 1024] [--reps 5] [--step-timeout 240] [--out profiles/kmat_time.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmergma.jl_amd"), os.path.join(ROOT, "tools")]

FLANK = 50
SLOT = 1000          # residues of genome per locus
N_NEAR, SCREEN_K = 8, 6
STEPS = ("R84", "R512")


def spread(ms):
    return {"min_ms": round(min(ms), 3), "median_ms": round(float(np.median(ms)), 3), "max_ms": round(max(ms), 3), "runs": len(ms)}


def clocked(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def step(name, H, reps):
    """One reference set, in this process: returns its entry of the result."""
    from assign_time import BASES, substituted
    from kmergma_amd import _lib, fasta

    rng = np.random.default_rng(84)
    genes = [r.sequence for r in fasta.read_fasta(os.path.join(ROOT, "tests", "data", "Alp_V_ref.fasta"))]
    rec = BASES[rng.integers(0, 4, size=H * SLOT)].copy()
    lo, hi = np.zeros(H, dtype=np.int64), np.zeros(H, dtype=np.int64)
    for i in range(H):
        g = substituted(rng, genes[i % len(genes)], 0.05)
        p = i * SLOT + 100 + int(rng.integers(0, 50))
        rec[p:p + len(g)] = np.frombuffer(g, dtype=np.uint8)
        lo[i], hi[i] = p + 1 - FLANK, p + len(g) + FLANK
    contig = np.zeros(H, dtype=np.int32)
    r512 = [substituted(rng, genes[j % len(genes)], 0.03) for j in range(512)]
    refs = genes if name == "R84" else r512
    ctx = _lib.Context(0)
    genome = ctx.genome_from_host([rec.tobytes()])

    def plain():
        return ctx.assign_ranges(genome, refs, contig, lo, hi, -69, -1, 1)

    def screened():
        return ctx.assign_ranges_screened(genome, refs, contig, lo, hi, -69, -1, 1, SCREEN_K, N_NEAR)

    (full, S), (fast, cand, _s) = plain(), screened()          # warm-up, and the comparison
    same_ref = int((full["ref"][:, 0] == fast["ref"][:, 0]).sum())
    same_score = int((full["score"][:, 0] == fast["score"][:, 0]).sum())
    winner_rank = [int(np.flatnonzero(cand[q] == full["ref"][q, 0])[0]) if full["ref"][q, 0] in cand[q] else -1 for q in range(H)]
    t_plain, t_fast, kmat, select, score, trace, plain_score = [], [], [], [], [], [], []
    for _ in range(reps):
        ms, _r = clocked(plain)
        t_plain.append(ms); plain_score.append(ctx.assign_stats()["score_ms"])
        ms, _r = clocked(screened)
        t_fast.append(ms)
        ks, st = ctx.kmat_stats(), ctx.assign_stats()
        kmat.append(ks["kmat_ms"]); select.append(ks["select_ms"]); score.append(st["score_ms"]); trace.append(st["trace_ms"])
    genome.free()
    ctx.close()
    ratio = float(np.median(t_plain) / np.median(t_fast))
    return {"refs": len(refs), "hits": H, "n_near": N_NEAR, "screen_k": SCREEN_K, "kmat_pairs": ks["n_pairs"], "scored_pairs": st["n_pairs"],
            "kmat_form": ks["form"], "kmat_tile": ks["tile"], "kmat_chunks": ks["chunks"],
            "unscreened_call": spread(t_plain), "unscreened_score_pass": spread(plain_score), "screened_call": spread(t_fast),
            "kmat_ms": spread(kmat), "select_ms": spread(select), "screened_score_pass": spread(score), "screened_trace_pass": spread(trace),
            "unscreened_over_screened_call": round(ratio, 2),
            "slowest_screened_call_beats_fastest_unscreened": bool(max(t_fast) < min(t_plain)),
            "same_best_reference": same_ref, "same_best_score": same_score,
            "full_winner_among_candidates": int(sum(r >= 0 for r in winner_rank)), "worst_winner_rank": int(max(winner_rank))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hits", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--step", choices=STEPS, default=None)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.reps < 3:
        ap.error("at least three repetitions")
    if args.step:                                   # a child: one reference set
        print(json.dumps(step(args.step, args.hits, args.reps)), flush=True)
        return 0
    out = {"tool": "tools/kmat_time.py", "hits": args.hits, "flank": FLANK, "reps": args.reps, "gap_open": -69, "gap_extend": -1,
           "timing": "host clock around calls that end in a stream synchronise; kmat / select / score / trace: hipEvents "
                     "(kgma_kmat_stats, kgma_assign_stats); routes alternating after one warm-up call each",
           "baseline": "kgma_assign_ranges (unscreened: every locus against every reference), unchanged by the prescreen"}
    for name in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--hits", str(args.hits), "--reps", str(args.reps)],
                               stdout=subprocess.PIPE, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"step {name} ran past {args.step_timeout} s: stopping", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"step {name} failed with status {p.returncode}: stopping", file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
        out[name] = json.loads(p.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
