#!/usr/bin/env python3
"""Scan time (the library's hipEvents) of the strobemer engine on one synthetic record (400 Mb by default), s = 2, w 3..5, q = 5,
W = 289, and -- alternating with it, in the same process -- of the nearest existing path: the generic kernel (KGMA_KERNEL=generic)
at k = 4, W = 289, which walks the same 256-bin count table.  Both references come from one family of 7 mutated copies of a random
gene.  The yardsticks are that kernel and the CPU oracle's rate (tests/strobe_oracle.py on --oracle-kb residues), never the code
under test.

usage: python tools/strobe_time.py [--mb 400] [--reps 7] [--warmup 2] [--oracle-kb 300] [--out rows.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmergma.jl_amd")]

from kmergma_amd import _lib, refprep  # noqa: E402
from kmergma_amd.fasta import Record  # noqa: E402

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
CFG = (2, 3, 5, 5)


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
    return {"min_ms": round(min(ms), 4), "median_ms": round(float(np.median(ms)), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=400.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--oracle-kb", type=float, default=300.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n = int(args.mb * 1e6)
    W = 289
    rng = np.random.default_rng(1)
    recs = family(rng, W)
    sRV, sW, _, (_, sN) = refprep.gen_ref_ws_cons_strobe(recs, *CFG, return_int=True)
    kRV, kW, _, (_, kN) = refprep.gen_ref_ws_cons(recs, 4, return_int=True)
    assert sW == kW == W
    ctx = _lib.Context(0)
    g = ctx.genome_synthetic([n], 77)
    t_strobe, t_gen, names = [], [], {}
    for it in range(args.warmup + args.reps):
        ctx.set_strobe_ref(*CFG, sRV, W, 1.0, sN)
        os.environ.pop("KGMA_KERNEL", None)
        ctx.scan_device(g, _lib.MODE_STROBE, 0)
        a = ctx.stats()["scan_ms"]
        names["strobe"] = ctx.kernel_name()
        ctx.set_refs(4, [kRV], [W], [1.0], [kN])
        os.environ["KGMA_KERNEL"] = "generic"
        ctx.scan_device(g, _lib.MODE_SINGLE, 0)
        b = ctx.stats()["scan_ms"]
        names["generic"] = ctx.kernel_name()
        os.environ.pop("KGMA_KERNEL", None)
        if it >= args.warmup:
            t_strobe.append(a); t_gen.append(b)
    g.free()
    ctx.close()
    out = {"tool": "tools/strobe_time.py", "bases": n, "W": W, "strobe": dict(kernel=names["strobe"], cfg=CFG, **spread(t_strobe)),
           "generic_k4": dict(kernel=names["generic"], **spread(t_gen))}
    out["strobe"]["Gbp_per_s"] = round(n / np.median(t_strobe) / 1e6, 1)
    out["generic_k4"]["Gbp_per_s"] = round(n / np.median(t_gen) / 1e6, 1)
    out["ratio_strobe_over_generic"] = round(float(np.median(t_strobe) / np.median(t_gen)), 3)
    if args.oracle_kb > 0:
        from tests import strobe_oracle as so
        S = np.rint(sRV * sN).astype(np.int64)
        seq = BASES[rng.integers(0, 4, size=int(args.oracle_kb * 1e3))].tobytes()
        t0 = time.perf_counter()
        so.scan_record(seq, sRV, S, sN, *CFG, W, 1.0, 50)
        dt = time.perf_counter() - t0
        out["cpu_oracle"] = {"residues": len(seq), "seconds": round(dt, 3), "Mbp_per_s": round(len(seq) / dt / 1e6, 3)}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
