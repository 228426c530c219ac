"""The distance landscape on the device against what the parent commit offers for the same answers, in one run:
kgma_dist_bins and kgma_dist_sweep (device ms by hipEvents, kgma_get_landscape_stats; median (min .. max) of 9 calls after 2
warm-ups; GB/s of the 8 bytes per value they read, as a share of the device copy rate) against kgma_get_dists to the host plus the
NumPy reduction of tests/landscape_ref.py (wall clock; the transfer 3 times, the reductions once -- they take seconds).
usage: python tools/landscape_time.py [--genomes 400m,grch38] [--baseline 400m] [--out profiles/landscape_time.json]

The genome: synthetic records (kgma_genome_synthetic) with a mutated reference gene every ~400 kb, scanned by the single engine
(k = 6, the alpaca IGHV fixture, W = 289) with the distances kept.  Sweeps: 64, 512 and 4096 thresholds halfway between lattice
points from 0 up to the random-sequence mean (api.default_sweep_thresholds: nearly every window lies above the largest, the kernel's
short cut), and 4096 thresholds from 0 up to twice that mean (`wide`: every window is searched and counted, most of them in a few
buckets).  Where the baseline runs, the device results are compared with it before anything is reported."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmergma.jl_amd")]

from kmergma_amd import _lib, api, fasta, refprep, workloads  # noqa: E402
from tests import landscape_ref as lr  # noqa: E402

COPY_TBS = 6.29                      # measured device copy, TB/s
BINS = (289, 1000)
K, WARM, REPS = 6, 2, 9


def stats(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)), calls=len(ms))


def rate(n_values, ms):
    gbs = 8.0 * n_values / (ms["median"] * 1e-3) / 1e9
    return dict(GBs=gbs, share_of_copy=gbs / (COPY_TBS * 1e3))


def timed(call, field, ctx):
    out = []
    for rep in range(WARM + REPS):
        call()
        if rep >= WARM:
            st = ctx.landscape_stats()
            out.append(sum(st[f] for f in field))
    return stats(out)


def wall(call, reps):
    out, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = call()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", default="400m,grch38")
    ap.add_argument("--baseline", default="400m")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ref_path = os.path.join(ROOT, "tests", "data", "Alp_V_ref.fasta")
    RV, W, _cons, (_S, N) = refprep.gen_ref_ws_cons(ref_path, K, return_int=True)
    genes = [r.sequence.upper() for r in fasta.read_fasta(ref_path)]
    ctx = api.default_context()
    ctx.set_refs(K, [RV], [W], [30.0], [N])
    sweeps = {str(n): api.default_sweep_thresholds(ctx, RV, W, n) for n in (64, 512, 4096)}
    top = float(sweeps["4096"][-1])
    sweeps["4096-wide"] = (np.unique(np.round(np.linspace(0, 2 * top * ctx.kfv_scale(1), 4096))) + 0.5) / ctx.kfv_scale(1)
    res = dict(k=K, windowsize=int(W), copy_TBs=COPY_TBS, warmups=WARM, genomes={})
    for name in args.genomes.split(","):
        lens = {"400m": [400_000_000], "grch38": list(workloads.GRCH38_LENS)}[name]
        rng = np.random.default_rng(5)
        gene = max(genes, key=len)
        plants = [(c, int(p)) for c, L in enumerate(lens) for p in range(200_000, L - 1000, 400_000)]
        a = np.frombuffer(gene, dtype=np.uint8).copy()
        hit = rng.random(a.size) < 0.04
        a[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(hit.sum()))]
        g = ctx.genome_synthetic(lens, 77, a.tobytes(), plants)
        try:
            ctx.set_refs(K, [RV], [W], [30.0], [N])
            ctx.scan_device(g, _lib.MODE_SINGLE, _lib.F_RETURN_DISTS)
            offset = ctx.dist_layout()
            n = int(offset[-1])
            r = dict(bases=int(sum(lens)), records=len(lens), values=n, dist_bytes=8 * n, scan_ms=ctx.stats()["scan_ms"], bins={}, sweep={})
            print("%s: %d values (%.2f GB of distances)" % (name, n, 8 * n / 1e9), flush=True)
            for width in BINS:
                ms = timed(lambda: ctx.dist_bins(1, width), ("bins_ms", "combine_ms"), ctx)
                k_ms = timed(lambda: ctx.dist_bins(1, width), ("bins_ms",), ctx)
                r["bins"][str(width)] = dict(device_ms=ms, bins_kernel_ms=k_ms, n_bins=ctx.landscape_stats()["n_bins"], **rate(n, ms))
                print("bins %5d: %8.3f ms (%.3f .. %.3f) = %.0f GB/s = %.2f of copy" % (
                    width, ms["median"], ms["min"], ms["max"], r["bins"][str(width)]["GBs"], r["bins"][str(width)]["share_of_copy"]), flush=True)
            for key, thr in sweeps.items():
                ms = timed(lambda: ctx.dist_sweep(thr, 1), ("sweep_ms",), ctx)
                below, dips = ctx.dist_sweep(thr, 1)
                r["sweep"][key] = dict(n_thr=int(thr.size), device_ms=ms, windows_below_last=int(below[-1]), dips_below_last=int(dips[-1]),
                                       **rate(n, ms))
                print("sweep %9s: %8.3f ms (%.3f .. %.3f) = %.0f GB/s = %.2f of copy; %d windows, %d dips under the last" % (
                    key, ms["median"], ms["min"], ms["max"], r["sweep"][key]["GBs"], r["sweep"][key]["share_of_copy"], below[-1], dips[-1]),
                      flush=True)
            if name in args.baseline.split(","):
                get_ms, d = wall(lambda: ctx.dists(1), 3)
                b = dict(get_dists_ms=get_ms, bins={}, sweep={})
                for width in BINS:
                    ms, (m, am, _o) = wall(lambda: lr.bins(d, offset, width), 1)
                    bmin, barg, _ = ctx.dist_bins(1, width)
                    assert np.array_equal(bmin.view(np.uint64), m.view(np.uint64)) and np.array_equal(barg, am), width
                    b["bins"][str(width)] = ms
                for key in ("64", "4096", "4096-wide"):
                    ms, (wb, db) = wall(lambda: lr.sweep(d, offset, sweeps[key]), 1)
                    below, dips = ctx.dist_sweep(sweeps[key], 1)
                    assert np.array_equal(below, wb) and np.array_equal(dips, db), key
                    b["sweep"][key] = ms
                r["baseline"] = b
                print("baseline: get_dists %.0f ms; NumPy bins %s ms; NumPy sweeps %s ms; device results equal the model's" % (
                    get_ms["median"], {k: round(v["median"]) for k, v in b["bins"].items()},
                    {k: round(v["median"]) for k, v in b["sweep"].items()}), flush=True)
                del d
            res["genomes"][name] = r
        finally:
            g.free()
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
