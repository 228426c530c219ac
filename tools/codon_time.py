#!/usr/bin/env python3
"""Time of kgma_codon_match (the library's hipEvents around the search launch) on a synthetic genome held on one MI355X: the 25
records of GRCh38's lengths, tools/pwm_time.py's genome.  Per m in 8, 21 and 64: a dense amino-acid profile of m rows (no
constant row), folded by the standard code, at its exact p <= 1e-9 threshold (prot_threshold), on the plus strand (one codon
matrix) and on both strands (two, one pass), each planted a few times so that it has hits.

The yardstick, taken in the same run on the same genome, is kgma_pwm_match with a dense matrix of the same number of rows at
p <= 1e-9 (at 8 rows, where no score is that rare, at its highest score): per m the ratio codon / pwm of the medians.  A codon
row costs one byte read and one table read; the position-weight-matrix kernel folds two rows into one such pair, so at equal rows
the codon kernel makes twice the reads.  Each case also reports Gbp/s per matrix and the share of the device copy rate for the
1 byte per base that is read (COPY_RATE: the 6.29 TB/s the README and DESIGN.md quote; not re-derived here).

Run it under a time limit of its own (`timeout -k 10 600 python tools/codon_time.py ...`).

usage: python tools/codon_time.py [--genome grch38] [--reps 7] [--warmup 2] [--out profiles/codon_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmergma.jl_amd")]

from kmergma_amd import _lib, api, workloads  # noqa: E402

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
COPY_RATE = 6.29e12          # bytes per second, measured device copy (README.md)
ROWS = (8, 21, 64)
PVALUE = 1e-9


def spread(ms):
    return {"min_ms": round(min(ms), 4), "median_ms": round(float(np.median(ms)), 4), "max_ms": round(max(ms), 4)}


def run(ctx, g, match, stats, mats, thr, reps, warmup):
    ms = []
    for it in range(warmup + reps):
        match(g, mats, thr)
        st = stats()
        if it >= warmup:
            ms.append(st["search_ms"])
    bases = ctx.stats()["bases_scanned"]
    med = float(np.median(ms))
    return dict(spread(ms), matrices=len(mats), rows=[len(W) for W in mats], thresholds=[int(t) for t in thr], n_launches=st["n_launches"],
                n_hits=st["n_hits"], ms_per_matrix=round(med / len(mats), 4), Gbp_per_s_per_matrix=round(bases * len(mats) / (med * 1e-3) / 1e9, 1),
                fraction_of_copy_rate=round(bases / (med * 1e-3) / COPY_RATE, 4))


def codon_site(W) -> bytes:
    return b"".join(bytes([b"ACGT"[c >> 4], b"ACGT"[(c >> 2) & 3], b"ACGT"[c & 3]]) for c in np.asarray(W)[:, :64].argmax(axis=1).tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", default="grch38")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    profiles, pwms = {}, {}
    for m in ROWS:
        P = rng.integers(-300, 301, size=(m, 21))
        P[np.arange(m), rng.integers(0, 20, size=m)] = 320            # (no constant row)
        P[:, 20] = -400                                               # the stop
        W = rng.integers(-300, 301, size=(m, 4))
        W[np.arange(m), rng.integers(0, 4, size=m)] = 320
        profiles[m], pwms[m] = P, W
    lens = list(workloads.GRCH38_LENS) if args.genome == "grch38" else [int(float(args.genome))]
    ctx = _lib.Context(0)
    g = ctx.genome_synthetic(lens, 77)
    big = [c for c, L in enumerate(lens) if L > 100_000]
    planted = []
    for m in ROWS:
        planted += [codon_site(api.prot_fold(profiles[m])), codon_site(api.prot_fold(profiles[m], minus=True)),
                    BASES[pwms[m].argmax(axis=1)].tobytes()]
    for i, text in enumerate(planted):
        for j in range(3):
            c = big[(7 * i + j) % len(big)]
            g.poke(c, 20_000 + 1_000 * i + 400 * j if j else lens[c] - len(text) + 1 - 1_000 * i, text)
    g.repack()
    rows = {"records": len(lens), "bases": int(sum(lens)), "copy_rate_bytes_per_s": COPY_RATE, "pvalue": PVALUE}
    R, Wm = args.reps, args.warmup
    for m in ROWS:
        P, W = profiles[m], pwms[m]
        t = api.prot_threshold(P, PVALUE)
        plus, minus = api.prot_fold(P), api.prot_fold(P, minus=True)
        rows[f"codon_{m}_plus"] = run(ctx, g, ctx.codon_match, ctx.codon_stats, [plus], [t], R, Wm)
        rows[f"codon_{m}_both"] = run(ctx, g, ctx.codon_match, ctx.codon_stats, [plus, minus], [t, t], R, Wm)
        # (4^8 sequences are too few for a score as rare as PVALUE: the highest score then, 47 k expected hits, one launch)
        tw = min(api.pwm_threshold(W, PVALUE), int(W.max(axis=1).sum()))
        rows[f"pwm_{m}_plus"] = run(ctx, g, ctx.pwm_match, ctx.pwm_stats, [W], [tw], R, Wm)
        rows[f"pwm_{m}_both"] = run(ctx, g, ctx.pwm_match, ctx.pwm_stats, [W, api.pwm_revcomp(W)], [tw, tw], R, Wm)
        for s in ("plus", "both"):
            rows[f"codon_over_pwm_{m}_{s}"] = round(rows[f"codon_{m}_{s}"]["median_ms"] / rows[f"pwm_{m}_{s}"]["median_ms"], 2)
        rows[f"codon_{m}_ns_per_start_and_row"] = round(rows[f"codon_{m}_plus"]["median_ms"] * 1e6 / (rows["bases"] * m), 6)
        print(json.dumps({k: v for k, v in rows.items() if f"_{m}_" in k}), flush=True)
    g.free()
    ctx.close()
    out = {"tool": "tools/codon_time.py", "reps": R, "warmup": Wm, "genomes": {args.genome: rows}}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
