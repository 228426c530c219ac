#!/usr/bin/env python3
"""Scan and chain time (the library's hipEvents) of k = 1 and k >= 11 on one synthetic record (400 Mb by default): one KFV of a
family of 7 mutated copies of a random gene, W = 289 and 3000, the generic kernel's 32-bit counter form (k = 1) and wide hash
form (k >= 11, the KFV given through kgma_set_refs_sparse: no 4^k table anywhere).

usage: python tools/large_k_time.py [--mb 400] [--reps 5] [--ks 1,11,12,13,15] [--ws 289,3000] [--out rows.json]
"""
import argparse
import json
import os
import sys
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmergma.jl_amd")]

from kmergma_amd import _lib  # noqa: E402

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def kmers(codes, k):
    n = codes.size - k + 1
    v = np.zeros(n, dtype=np.int64)
    for j in range(k):
        v = (v << 2) | codes[j:j + n]
    return v


def family(rng, L, k, n_refs=7):
    """The family's KFV as its non-zero entries: natural k-mer values, S / N."""
    base = rng.integers(0, 4, size=L)
    cnt = Counter()
    for _ in range(n_refs):
        a = base.copy()
        hit = rng.random(L) < 0.03
        a[hit] = rng.integers(0, 4, size=int(hit.sum()))
        cnt.update(kmers(a, k).tolist())
    keys = np.asarray(sorted(cnt), dtype=np.uint32)
    S = np.asarray([cnt[x] for x in sorted(cnt)], dtype=np.float64)
    return keys, S / n_refs, n_refs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=400.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="1,11,12,13,15")
    ap.add_argument("--ws", default="289,3000")
    ap.add_argument("--no-chain", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n = int(args.mb * 1e6)
    ctx = _lib.Context(0)
    g = ctx.genome_synthetic([n], 77)
    rng = np.random.default_rng(1)
    rows = []
    for k in [int(x) for x in args.ks.split(",")]:
        for W in [int(x) for x in args.ws.split(",")]:
            keys, vals, N = family(rng, W, k)
            ctx.set_refs_sparse(k, [keys], [vals], [W], [1.0], [N])
            ctx.scan_device(g, _lib.MODE_SINGLE, 0)
            ms = []
            for _ in range(args.reps):
                ctx.scan_device(g, _lib.MODE_SINGLE, 0)
                ms.append(ctx.stats()["scan_ms"])
            row = {"k": k, "W": W, "nnz": int(keys.size), "kernel": ctx.kernel_name(), "scan_ms": round(min(ms), 4),
                   "Gbp_per_s": round(n / min(ms) / 1e6, 1)}
            if not args.no_chain:
                nwin = n - W + 1
                cms = []
                try:
                    for _ in range(max(2, args.reps // 2)):
                        g.chain_values(0, 1, [(nwin, nwin)])
                        cms.append(ctx.stats()["chain_device_ms"])
                    row["chain_ms"] = round(min(cms), 4)
                    row["chain_Gbp_per_s"] = round(n / min(cms) / 1e6, 1)
                except _lib.KgmaError as e:                     # (recorded, not fatal: the scan rows still count)
                    row["chain_error"] = str(e)
            rows.append(row)
            print(json.dumps(row), flush=True)
    g.free()
    ctx.close()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"tool": "tools/large_k_time.py", "bases": n, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
