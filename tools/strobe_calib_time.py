#!/usr/bin/env python3
"""Time of kgma_strobe_window_dists against the only route to the same numbers before it existed: one whole-genome
kgma_strobe_scan with KGMA_F_RETURN_DISTS (8 bytes per window of the genome on the device), then kgma_get_dists.

Workload: one synthetic 400 Mb record (kgma_genome_synthetic), a strobemer reference of 7 mutated copies of a random gene
(s = 2, w_min = 3, w_max = 5, q = 5, W = 289) and 100 000 windows drawn by api.sample_window_starts(lens, W + 1, ...), the draw
api.estimate_strobe_threshold_from_genome makes.  The two sides alternate in one process after warm-up calls of the same shape.
Each call ends in a stream synchronise, so the host clock around it is the whole call (uploads, kernel, downloads); the kernels
alone are kgma_stats.scan_ms (hipEvents).  The download of the scan's distance array is timed apart.  No target is set: the file
shows by how much the call is cheaper than the route it replaces.  The sampled windows' distances must equal the scan's, bit for bit.

usage: python tools/strobe_calib_time.py [--mb 400] [--windows 100000] [--reps 7] [--warmup 2] [--out profiles/strobe_calib_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmergma.jl_amd")]

from kmergma_amd import _lib, api, refprep  # noqa: E402
from kmergma_amd.fasta import Record  # noqa: E402

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
CFG = (2, 3, 5, 5)
W = 289


def family(rng, L, n_refs=7, rate=0.03):
    base = BASES[rng.integers(0, 4, size=L)].copy()
    recs = []
    for i in range(n_refs):
        a = base.copy()
        hit = rng.random(L) < rate
        a[hit] = BASES[rng.integers(0, 4, size=int(hit.sum()))]
        recs.append(Record(f"g{i}", a.tobytes()))
    return recs


def spread(ms):
    return {"min_ms": round(min(ms), 3), "median_ms": round(float(np.median(ms)), 3), "max_ms": round(max(ms), 3), "runs": len(ms)}


def clocked(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=400.0)
    ap.add_argument("--windows", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n = int(args.mb * 1e6)
    RV, Wr, _cons, (_S, N) = refprep.gen_ref_ws_cons_strobe(family(np.random.default_rng(1), W), *CFG, return_int=True)
    assert Wr == W
    contig, start = api.sample_window_starts([n], W + 1, args.windows, 42)
    ctx = _lib.Context(0)
    ctx.set_strobe_ref(*CFG, RV, W, 1.0, N)
    g = ctx.genome_synthetic([n], 77)
    call, kernel, scan_call, scan_kernel, fetch = [], [], [], [], []
    names = {}
    for it in range(args.warmup + args.reps):
        ms, (_D, dist) = clocked(lambda: ctx.strobe_window_dists(g, contig, start))
        k_ms = ctx.stats()["scan_ms"]
        names["window_dists"] = ctx.kernel_name()
        s_ms, _ = clocked(lambda: ctx.strobe_scan(g, 50, _lib.F_RETURN_DISTS, None))
        sk_ms = ctx.stats()["scan_ms"]
        names["scan"] = ctx.kernel_name()
        if it >= args.warmup:
            call.append(ms); kernel.append(k_ms); scan_call.append(s_ms); scan_kernel.append(sk_ms)
        if it in (0, args.warmup + args.reps - 1):
            f_ms, d = clocked(lambda: ctx.dists(1))
            fetch.append(f_ms)
            assert d.size == n - W - 1
            assert np.array_equal(dist[start > 1], d[start[start > 1] - 2]), "the two routes disagree"
            del d
    g.free()
    ctx.close()
    out = {"tool": "tools/strobe_calib_time.py", "bases": n, "W": W, "cfg": CFG, "windows": int(contig.size), "warmup": args.warmup,
           "timing": "host clock around calls that end in a stream synchronise; kernels: kgma_stats.scan_ms (hipEvents); sides alternating",
           "strobe_window_dists": {"kernel_name": names["window_dists"], "call": spread(call), "kernel": spread(kernel)},
           "strobe_scan_return_dists": {"kernel_name": names["scan"], "call": spread(scan_call), "kernel": spread(scan_kernel),
                                        "get_dists": spread(fetch), "device_bytes_of_dists": 8 * (n - W - 1)},
           "agree_bit_for_bit": True}
    out["scan_call_over_window_dists_call"] = round(float(np.median(scan_call) / np.median(call)), 1)
    out["scan_call_plus_get_dists_over_window_dists_call"] = round(float((np.median(scan_call) + np.median(fetch)) / np.median(call)), 1)
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
