#!/usr/bin/env python3
"""Time of kgma_pwm_match (the library's hipEvents around the search launch) on a synthetic genome held on one MI355X: the 25
records of GRCh38's lengths, tools/approx_time.py's genome.  Cases, each planted a few times so that it has hits:

  a  the RSS matrix of the seven sites of tests/golden/pwm.json at its p <= 1e-6 threshold, plus strand
  b  the same on both strands: two matrices, one pass
  c  eight RSS-shaped matrices (log-odds of a few random sites: 7 rows, 23 constant rows, 9 rows) at p <= 1e-6
  d  a dense 16-row matrix, no constant row, at p <= 1e-6
  e  a dense 64-row matrix, no constant row, at p <= 1e-8

and, re-timed in the same run on the same genome, the nearest calls the library had: kgma_motif_match and kgma_approx_match of
HumanRSSD at 1 mismatch / 1 edit.  The host baseline is the numpy oracle (tests/pwm_oracle.py) for case a on one record of
--oracle-bases residues, in slices, which also checks that device and oracle report the same hits there.

Per case: median / min / max of --reps calls after --warmup, the time per matrix and Gbp/s per matrix.  Run it under a time
limit of its own (`timeout -k 10 900 python tools/pwm_time.py ...`).

usage: python tools/pwm_time.py [--genome grch38] [--reps 7] [--warmup 2] [--oracle-bases 400e6] [--out profiles/pwm_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmergma.jl_amd")]

from kmergma_amd import _lib, api, workloads  # noqa: E402
from tests import pwm_oracle as po  # noqa: E402

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def spread(ms):
    return {"min_ms": round(min(ms), 4), "median_ms": round(float(np.median(ms)), 4), "max_ms": round(max(ms), 4)}


def folded_pairs(W) -> int:
    """Table reads per start: the rows that are not constant, each taken with the row behind it (kgma_pwm.cpp)."""
    n, r = 0, 0
    while r < len(W):
        if len(set(W[r].tolist())) == 1:
            r += 1
        else:
            n, r = n + 1, r + 2
    return n


def run_pwm(ctx, g, mats, thr, reps, warmup):
    ms = []
    for it in range(warmup + reps):
        ctx.pwm_match(g, mats, thr)
        st = ctx.pwm_stats()
        if it >= warmup:
            ms.append(st["search_ms"])
    bases = ctx.stats()["bases_scanned"]
    med = float(np.median(ms))
    return dict(spread(ms), matrices=len(mats), rows=[len(W) for W in mats], pairs=[folded_pairs(W) for W in mats], thresholds=list(thr),
                n_launches=st["n_launches"], n_hits=st["n_hits"], ms_per_matrix=round(med / len(mats), 4),
                Gbp_per_s_per_matrix=round(bases * len(mats) / (med * 1e-3) / 1e9, 1))


def run_other(ctx, g, call, fetch, reps, warmup):
    ms = []
    for it in range(warmup + reps):
        call()
        st = ctx.stats()
        if it >= warmup:
            ms.append(st["scan_ms"])
    return dict(spread(ms), matches=int(fetch().size), n_launches=st["n_launches"])


def oracle_baseline(ctx, W, thr, n_bases, site):
    """Case a on one record of n_bases residues: the device call and the numpy oracle, in slices of 16 Mb that overlap by m - 1."""
    g = ctx.genome_synthetic([n_bases], 78)
    for at in (12_345, n_bases // 2, n_bases - len(W) + 1):
        g.poke(0, at, site)
    g.repack()
    ctx.pwm_match(g, [W], [thr])
    got = [(s, k) for _, _, s, k, _ in ctx.pwm_matches().tolist()]
    ms = ctx.pwm_stats()["search_ms"]
    t0 = time.perf_counter()
    want, step, m = [], 1 << 24, len(W)
    for lo in range(0, n_bases - m + 1, step):
        hi = min(n_bases, lo + step + m - 1)
        want += [(lo + s, k) for s, k in po.find(W, g.fetch(0, lo + 1, hi - lo), thr)]
    sec = time.perf_counter() - t0
    g.free()
    return {"bases": n_bases, "device_ms": round(ms, 4), "oracle_s": round(sec, 2), "oracle_includes_fetching_the_text": True,
            "hits": len(want), "device_equals_oracle": got == want, "oracle_over_device": round(sec * 1e3 / ms, 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", default="grch38")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--oracle-bases", default="400e6")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    with open(os.path.join(ROOT, "tests", "golden", "pwm.json")) as f:
        gold = json.load(f)
    rss = api.pwm_from_sequences(gold["sites"])
    t_rss = api.pwm_threshold(rss, 1e-6)
    assert rss.tolist() == gold["matrix"] and t_rss == gold["thresholds"]["1e-6"]

    def rss_shaped():
        site = BASES[rng.integers(0, 4, size=39)].tobytes()
        sites = [site] + [bytes(BASES[rng.integers(0, 4)] if rng.random() < 0.15 else ch for ch in site) for _ in range(6)]
        W = api.pwm_from_sequences(sites)
        W[7:30] = 0                                               # the spacer: 23 constant rows
        return W

    eight = [rss_shaped() for _ in range(8)]
    d16 = rng.integers(-300, 301, size=(16, 4))
    d64 = rng.integers(-300, 301, size=(64, 4))
    for W in (d16, d64):
        W[np.arange(len(W)), rng.integers(0, 4, size=len(W))] = 320        # (no constant row)
    lens = list(workloads.GRCH38_LENS) if args.genome == "grch38" else [int(float(args.genome))]
    ctx = _lib.Context(0)
    g = ctx.genome_synthetic(lens, 77)
    big = [c for c, L in enumerate(lens) if L > 100_000]
    best = lambda W: BASES[np.asarray(W).argmax(axis=1)].tobytes()
    planted = [gold["sites"][0].encode(), po.revcomp_text(gold["sites"][1].encode()), best(d16), best(d64)] + [best(W) for W in eight]
    for i, text in enumerate(planted):
        for j in range(3):
            c = big[(7 * i + j) % len(big)]
            g.poke(c, 20_000 + 1_000 * i + 400 * j if j else lens[c] - len(text) + 1 - 1_000 * i, text)
    g.repack()
    rows = {"records": len(lens), "bases": int(sum(lens))}
    R, Wm = args.reps, args.warmup
    rows["a_rss_plus"] = run_pwm(ctx, g, [rss], [t_rss], R, Wm)
    rows["b_rss_both"] = run_pwm(ctx, g, [rss, api.pwm_revcomp(rss)], [t_rss, t_rss], R, Wm)
    rows["c_eight_rss_shaped"] = run_pwm(ctx, g, eight, [api.pwm_threshold(W, 1e-6) for W in eight], R, Wm)
    rows["d_dense_16"] = run_pwm(ctx, g, [d16], [api.pwm_threshold(d16, 1e-6)], R, Wm)
    rows["e_dense_64"] = run_pwm(ctx, g, [d64], [api.pwm_threshold(d64, 1e-8)], R, Wm)
    rows["motif_match_rssd_1"] = run_other(ctx, g, lambda: ctx.motif_match(g, [api.HumanRSSD], [1]), ctx.motif_matches, R, Wm)
    rows["approx_match_rssd_1"] = run_other(ctx, g, lambda: ctx.approx_match(g, [api.HumanRSSD], [1], True), ctx.approx_matches, R, Wm)
    rows["a_over_motif_match"] = round(rows["a_rss_plus"]["median_ms"] / rows["motif_match_rssd_1"]["median_ms"], 2)
    rows["a_over_approx_match"] = round(rows["a_rss_plus"]["median_ms"] / rows["approx_match_rssd_1"]["median_ms"], 2)
    for k in ("a_rss_plus", "d_dense_16", "e_dense_64", "c_eight_rss_shaped"):
        v = rows[k]
        rows[k + "_ns_per_start_and_pair"] = round(v["median_ms"] * 1e6 / (rows["bases"] * sum(v["pairs"])), 6)
    print(json.dumps(rows), flush=True)
    g.free()
    n_oracle = int(float(args.oracle_bases))
    if n_oracle > 0:
        rows["oracle_one_record"] = oracle_baseline(ctx, rss, t_rss, n_oracle, gold["sites"][0].encode())
        print(json.dumps(rows["oracle_one_record"]), flush=True)
    ctx.close()
    out = {"tool": "tools/pwm_time.py", "reps": R, "warmup": Wm, "genomes": {args.genome: rows}}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
