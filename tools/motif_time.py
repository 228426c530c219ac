#!/usr/bin/env python3
"""Time of kgma_motif_match (the library's hipEvents around the launches of the call) on synthetic genomes held on one MI355X:
the 25 records of GRCh38's lengths and, by default, 100 records of 1 Gb (100 Gb: the residue text, the 2-bit copy and the bit
planes, 150 GB, fit the device together).  Cases, each planted a few times so that it has matches:

  a  HumanRSSD (16 informative positions), 1 mismatch, plus strand
  b  the same on both strands: two motifs, one pass
  c  one 16-symbol A/C/G/T motif, no mismatch
  d  eight RSS-shaped motifs (heptamer, 23 N, nonamer), 2 mismatches

and, re-timed in the same run on the same genome, case c's motif as kgma_exact_match: through exact_2bit_kernel (0.25 B per
base) and under KGMA_EXACT_ASCII=1 through the residue-text kernel (1 B per base).

Per case: median / min / max of --reps calls after --warmup, Gbp/s, and the fraction of the 0.25 B per base model at the
6.29 TB/s measured-copy figure the project uses.  The first motif call on a genome also makes its bit-plane copy; that
call is one of the warm-ups.

usage: python tools/motif_time.py [--genomes grch38,100g] [--reps 7] [--warmup 2] [--out profiles/motif_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmergma.jl_amd")]

from kmergma_amd import _lib, api, fasta, workloads  # noqa: E402

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
COPY_BPS = 6.29e12


def spread(ms):
    return {"min_ms": round(min(ms), 4), "median_ms": round(float(np.median(ms)), 4), "max_ms": round(max(ms), 4)}


def row(ms, st, n, what, bytes_per_base):
    rate = st["bases_scanned"] / (np.median(ms) * 1e-3)
    return dict(spread(ms), **what, matches=n, n_launches=st["n_launches"], Gbp_per_s=round(rate / 1e9, 1),
                bytes_per_base=bytes_per_base, fraction_of_byte_model=round(bytes_per_base * rate / COPY_BPS, 4))


def run_motif(ctx, g, motifs, ds, reps, warmup):
    ms = []
    for it in range(warmup + reps):
        ctx.motif_match(g, motifs, ds)
        st = ctx.stats()
        if it >= warmup:
            ms.append(st["scan_ms"])
    informative = [sum(1 for ch in m.upper() if ch != ord("N")) for m in motifs]
    return row(ms, st, int(ctx.motif_matches().size), dict(motifs=len(motifs), informative=informative, max_mismatch=list(ds)), 0.25)


def run_exact(ctx, g, queries, bytes_per_base, reps, warmup, ascii_only=False):
    if ascii_only:
        os.environ["KGMA_EXACT_ASCII"] = "1"
    try:
        ms = []
        for it in range(warmup + reps):
            ctx.exact_match(g, queries)
            st = ctx.stats()
            if it >= warmup:
                ms.append(st["scan_ms"])
        n = int(ctx.matches().size)
    finally:
        os.environ.pop("KGMA_EXACT_ASCII", None)
    return row(ms, st, n, dict(queries=len(queries)), bytes_per_base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", default="grch38,100g")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    rssd = api.HumanRSSD
    qc = BASES[rng.integers(0, 4, size=16)].tobytes()
    eight = [BASES[rng.integers(0, 4, size=7)].tobytes() + b"N" * 23 + BASES[rng.integers(0, 4, size=9)].tobytes() for _ in range(8)]
    out = {"tool": "tools/motif_time.py", "copy_TBps": COPY_BPS / 1e12, "reps": args.reps, "warmup": args.warmup, "genomes": {}}
    ctx = _lib.Context(0)
    for name in args.genomes.split(","):
        lens = [1_000_000_000] * 100 if name == "100g" else list(workloads.GRCH38_LENS) if name == "grch38" else [int(float(name))]
        g = ctx.genome_synthetic(lens, 77)
        big = [c for c, L in enumerate(lens) if L > 100_000]
        inst = lambda m: bytes(BASES[rng.integers(0, 4)] if ch == ord("N") else ch for ch in m)
        for i, q in enumerate([rssd, fasta.reverse_complement(rssd), qc] + eight):
            for j in range(3):
                c = big[(7 * i + j) % len(big)]
                g.poke(c, 20_000 + 1_000 * i + 400 * j if j else lens[c] - len(q) + 1 - 1_000 * i, inst(q))
        g.repack()
        rows = {"records": len(lens), "bases": int(sum(lens))}
        rows["a_rssd_d1_plus"] = run_motif(ctx, g, [rssd], [1], args.reps, args.warmup)
        rows["b_rssd_d1_both"] = run_motif(ctx, g, [rssd, fasta.reverse_complement(rssd)], [1, 1], args.reps, args.warmup)
        rows["c_16_acgt_d0"] = run_motif(ctx, g, [qc], [0], args.reps, args.warmup)
        rows["d_eight_rss_d2"] = run_motif(ctx, g, eight, [2] * 8, args.reps, args.warmup)
        rows["c_as_exact_2bit_kernel"] = run_exact(ctx, g, [qc], 0.25, args.reps, args.warmup)
        rows["c_as_exact_text_kernel"] = run_exact(ctx, g, [qc], 1.0, args.reps, args.warmup, ascii_only=True)
        a, t2, tx = rows["a_rssd_d1_plus"], rows["c_as_exact_2bit_kernel"], rows["c_as_exact_text_kernel"]
        rows["a_over_text_kernel"] = round(tx["median_ms"] / a["median_ms"], 3)          # > 1: the motif search is the faster one
        rows["a_over_2bit_kernel"] = round(t2["median_ms"] / a["median_ms"], 3)
        rows["a_faster_than_text_kernel_beyond_spread"] = bool(a["max_ms"] < tx["min_ms"])
        out["genomes"][name] = rows
        print(name, json.dumps(rows), flush=True)
        g.free()
        if args.out:                                            # (after every genome: a later one may not fit the device)
            with open(args.out, "w") as fh:
                json.dump(out, fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
