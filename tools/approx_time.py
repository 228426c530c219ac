#!/usr/bin/env python3
"""Time of kgma_approx_match (the library's hipEvents around the search launch and around the start kernel) on a synthetic genome
held on one MI355X: the 25 records of GRCh38's lengths.  Cases, each planted a few times so that it has hits:

  a  HumanRSSD, 1 edit, plus strand
  b  the same on both strands: two queries, one pass
  c  one 16-symbol A/C/G/T query at 0 and at 2 edits -- under the one-word form the library chooses for it and, with
     KGMA_APPROX_WORDS=2, under the two-word form (the comparison that decides whether the one-word form is kept)
  d  eight RSS-shaped queries (heptamer, 23 N, nonamer), 2 edits
  e  a 64-symbol query, 3 edits

and, re-timed in the same run on the same genome, kgma_motif_match for cases a, b and d with max_mismatch = the edits: the
nearest call the library had, which answers a subset (no inserted or deleted base).

Per case: median / min / max of --reps calls after --warmup, Gbp/s per query, and the time per query beside the 3 ms that the
operation count alone gives at this size (about 1 Tbp/s per query: an estimate).  Run it under a time
limit of its own (`timeout -k 10 600 python tools/approx_time.py ...`).

usage: python tools/approx_time.py [--genome grch38] [--reps 7] [--warmup 2] [--out profiles/approx_time.json]
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


def spread(ms):
    return {"min_ms": round(min(ms), 4), "median_ms": round(float(np.median(ms)), 4), "max_ms": round(max(ms), 4)}


def run_approx(ctx, g, queries, eds, reps, warmup, two_words=False):
    if two_words:
        os.environ["KGMA_APPROX_WORDS"] = "2"
    try:
        search, starts = [], []
        for it in range(warmup + reps):
            ctx.approx_match(g, queries, eds, True)
            st = ctx.approx_stats()
            if it >= warmup:
                search.append(st["search_ms"])
                starts.append(st["starts_ms"])
    finally:
        os.environ.pop("KGMA_APPROX_WORDS", None)
    bases = ctx.stats()["bases_scanned"]
    med = float(np.median(search))
    return dict(spread(search), queries=len(queries), symbols=[len(q) for q in queries], max_edits=list(eds), words=st["words"],
                n_launches=st["n_launches"], n_ends=st["n_ends"], n_hits=st["n_hits"], starts_median_ms=round(float(np.median(starts)), 4),
                ms_per_query=round(med / len(queries), 4), Gbp_per_s_per_query=round(bases * len(queries) / (med * 1e-3) / 1e9, 1))


def run_motif(ctx, g, motifs, ds, reps, warmup):
    ms = []
    for it in range(warmup + reps):
        ctx.motif_match(g, motifs, ds)
        st = ctx.stats()
        if it >= warmup:
            ms.append(st["scan_ms"])
    return dict(spread(ms), motifs=len(motifs), max_mismatch=list(ds), matches=int(ctx.motif_matches().size), n_launches=st["n_launches"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", default="grch38")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    rssd, rc = api.HumanRSSD, fasta.reverse_complement(api.HumanRSSD)
    qc = BASES[rng.integers(0, 4, size=16)].tobytes()
    eight = [BASES[rng.integers(0, 4, size=7)].tobytes() + b"N" * 23 + BASES[rng.integers(0, 4, size=9)].tobytes() for _ in range(8)]
    q64 = BASES[rng.integers(0, 4, size=64)].tobytes()
    lens = list(workloads.GRCH38_LENS) if args.genome == "grch38" else [int(float(args.genome))]
    ctx = _lib.Context(0)
    g = ctx.genome_synthetic(lens, 77)
    big = [c for c, L in enumerate(lens) if L > 100_000]
    inst = lambda m: bytes(BASES[rng.integers(0, 4)] if ch == ord("N") else ch for ch in m)
    for i, q in enumerate([rssd, rc, qc, q64] + eight):
        for j in range(3):
            c = big[(7 * i + j) % len(big)]
            text = inst(q)
            if j == 2:
                text = text[:5] + text[6:]                       # one base deleted
            g.poke(c, 20_000 + 1_000 * i + 400 * j if j else lens[c] - len(q) + 1 - 1_000 * i, text)
    g.repack()
    rows = {"records": len(lens), "bases": int(sum(lens)), "estimate_ms_per_query": round(sum(lens) / 1e12 * 1e3, 2)}
    R, W = args.reps, args.warmup
    rows["a_rssd_e1_plus"] = run_approx(ctx, g, [rssd], [1], R, W)
    rows["b_rssd_e1_both"] = run_approx(ctx, g, [rssd, rc], [1, 1], R, W)
    for e in (0, 2):
        one, two = run_approx(ctx, g, [qc], [e], R, W), run_approx(ctx, g, [qc], [e], R, W, two_words=True)
        rows[f"c_16_acgt_e{e}"], rows[f"c_16_acgt_e{e}_two_words"] = one, two
        rows[f"c_e{e}_one_word_over_two"] = round(one["median_ms"] / two["median_ms"], 3)
        rows[f"c_e{e}_one_word_faster_beyond_spread"] = bool(one["max_ms"] < two["min_ms"])
    rows["d_eight_rss_e2"] = run_approx(ctx, g, eight, [2] * 8, R, W)
    rows["e_64_acgt_e3"] = run_approx(ctx, g, [q64], [3], R, W)
    rows["a_as_motif_match"] = run_motif(ctx, g, [rssd], [1], R, W)
    rows["b_as_motif_match"] = run_motif(ctx, g, [rssd, rc], [1, 1], R, W)
    rows["d_as_motif_match"] = run_motif(ctx, g, eight, [2] * 8, R, W)
    for k in "abd":
        a = next(v for n, v in rows.items() if n.startswith(k + "_") and "motif" not in n)
        rows[f"{k}_over_motif_match"] = round(a["median_ms"] / rows[f"{k}_as_motif_match"]["median_ms"], 2)
    out = {"tool": "tools/approx_time.py", "reps": R, "warmup": W, "genomes": {args.genome: rows}}
    print(json.dumps(rows), flush=True)
    g.free()
    ctx.close()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
