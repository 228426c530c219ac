#!/usr/bin/env python3
"""Time of kgma_exact_match (the library's hipEvents around the call: uploads of the queries, the launches, the download of the
matches) on synthetic genomes held on one MI355X: by default 100 records of 1 Gb (100 Gb: the residue text and the 2-bit copy,
125 GB, fit the device together) and the 25 records of GRCh38's lengths.  Cases, each planted a few times so that it has matches:

  a  one 289-symbol A/C/G/T query                       2-bit prefilter, 0.25 B per base
  b  the 84 genes of the fixture in one batch           2-bit prefilter
  c  one 8-symbol query (about bases / 65536 matches)   2-bit prefilter
  d  one 40-symbol query that holds an N                residue-text kernel, 1 B per base
  e  case a under KGMA_EXACT_ASCII=1                    residue-text kernel

Per case: median / min / max of --reps calls after --warmup, Gbp/s, and the fraction of the kernel's own byte model at the
6.29 TB/s measured-copy figure the project uses.  The CPU figure beside them is one core of Python's bytes.find of
query a over chr22-size random bytes.

usage: python tools/exact_time.py [--genomes 100g,grch38] [--reps 7] [--warmup 2] [--out profiles/exact_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmergma.jl_amd")]

from kmergma_amd import _lib, fasta, workloads  # noqa: E402

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
COPY_BPS = 6.29e12


def spread(ms):
    return {"min_ms": round(min(ms), 4), "median_ms": round(float(np.median(ms)), 4), "max_ms": round(max(ms), 4)}


def run_case(ctx, g, queries, bytes_per_base, reps, warmup, ascii_only=False):
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
    bases = st["bases_scanned"]
    rate = bases / (np.median(ms) * 1e-3)
    return dict(spread(ms), queries=len(queries), matches=n, n_launches=st["n_launches"], Gbp_per_s=round(rate / 1e9, 1),
                bytes_per_base=bytes_per_base, fraction_of_byte_model=round(bytes_per_base * rate / COPY_BPS, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", default="100g,grch38")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    genes = [r.sequence for r in fasta.read_fasta(os.path.join(ROOT, "tests", "data", "Alp_V_ref.fasta"))]
    qa = BASES[rng.integers(0, 4, size=289)].tobytes()
    qc = BASES[rng.integers(0, 4, size=8)].tobytes()
    qd = bytearray(BASES[rng.integers(0, 4, size=40)].tobytes()); qd[20] = ord("N"); qd = bytes(qd)
    out = {"tool": "tools/exact_time.py", "copy_TBps": COPY_BPS / 1e12, "reps": args.reps, "warmup": args.warmup, "genomes": {}}
    ctx = _lib.Context(0)
    for name in args.genomes.split(","):
        lens = [1_000_000_000] * 100 if name == "100g" else list(workloads.GRCH38_LENS) if name == "grch38" else [int(float(name))]
        g = ctx.genome_synthetic(lens, 77)
        big = [c for c, L in enumerate(lens) if L > 100_000]
        for i, q in enumerate([qa, qd] + genes[:8]):
            for j in range(3):
                c = big[(7 * i + j) % len(big)]
                g.poke(c, 20_000 + 1_000 * i + 400 * j if j else lens[c] - len(q) + 1 - 1_000 * i, q)
        g.repack()
        rows = {"records": len(lens), "bases": int(sum(lens))}
        rows["a_289_acgt"] = run_case(ctx, g, [qa], 0.25, args.reps, args.warmup)
        rows["b_84_genes"] = run_case(ctx, g, genes, 0.25, args.reps, args.warmup)
        rows["c_8_symbols"] = run_case(ctx, g, [qc], 0.25, args.reps, args.warmup)
        rows["d_with_N"] = run_case(ctx, g, [qd], 1.0, args.reps, args.warmup)
        rows["e_289_acgt_text_kernel"] = run_case(ctx, g, [qa], 1.0, args.reps, args.warmup, ascii_only=True)
        a, e = rows["a_289_acgt"], rows["e_289_acgt_text_kernel"]
        rows["prefilter_over_text_kernel"] = round(e["median_ms"] / a["median_ms"], 3)
        # (the stage-2 condition: the prefilter's slowest run against the text kernel's fastest)
        rows["prefilter_gain_beyond_spread"] = bool(a["max_ms"] < e["min_ms"])
        out["genomes"][name] = rows
        print(name, json.dumps(rows), flush=True)
        g.free()
    ctx.close()
    seq = BASES[rng.integers(0, 4, size=workloads.CHR22_LEN)].tobytes()
    t0 = time.perf_counter()
    seq.find(qa)
    dt = time.perf_counter() - t0
    out["cpu_bytes_find"] = {"residues": len(seq), "seconds": round(dt, 4), "Gbp_per_s": round(len(seq) / dt / 1e9, 3)}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
