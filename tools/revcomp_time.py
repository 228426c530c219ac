#!/usr/bin/env python3
"""Time of revcomp_kernel alone (kgma_genome_revcomp_into: the launch and its 64-byte tail memset, nothing else) against a
device-to-device hipMemcpyAsync of the same residue text, both between hipEvents on kgma_stream, on synthetic genomes held on
one MI355X.  The copy is the floor for 1 byte read + 1 byte written per base.

Genomes: `400m` one record of 400 000 000 bases (a multiple of 16: every chunk's source bytes are aligned, one load per chunk),
`400m+7` one record of 400 000 007 bases (misaligned by 7: two loads per chunk and the byte shift), `grch38` the 25 records of
GRCh38's lengths (3.1 Gb, mixed).  Per genome: --warmup untimed rounds, then --reps rounds that alternate one kernel and one
copy, so both see the same machine; median / min / max of each, their ratio, and GB/s counted as 2 x ascii_bytes (read + write).
The result of the kernel is checked once per genome against the host map on sampled ranges.

usage: python tools/revcomp_time.py [--genomes 400m,400m+7,grch38] [--reps 25] [--warmup 3] [--out profiles/revcomp_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmergma.jl_amd")]

from kmergma_amd import _lib, fasta, workloads  # noqa: E402

HBM_PEAK_BPS = 8.0e12       # spec
COPY_BPS = 6.29e12          # the measured-copy figure the project uses
D2D = 3                     # hipMemcpyDeviceToDevice


def hip():
    h = C.CDLL("libamdhip64.so")
    h.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    h.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    h.hipEventSynchronize.argtypes = [C.c_void_p]
    h.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    h.hipEventDestroy.argtypes = [C.c_void_p]
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipFree.argtypes = [C.c_void_p]
    h.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    h.hipStreamSynchronize.argtypes = [C.c_void_p]
    return h


def check(st, what):
    if st != 0:
        raise RuntimeError(f"{what} failed with HIP status {st}")


def ascii_bytes(lens):
    """genome_layout (kgma_api.cpp): every record's residues rounded up to 32 bytes + 32, and 64 tail bytes."""
    return sum(((L + 31) & ~31) + 32 for L in lens) + 64


def spread(ms):
    return {"min_ms": round(min(ms), 4), "median_ms": round(float(np.median(ms)), 4), "max_ms": round(max(ms), 4)}


def verify(g, r, lens, rng):
    for c in sorted(set([0, len(lens) - 1] + rng.integers(0, len(lens), size=4).tolist())):
        L = lens[c]
        for lo in sorted(set([1, max(1, L - 4999)] + rng.integers(1, max(2, L - 5000), size=4).tolist())):
            n = min(5000, L - lo + 1)
            want = fasta.reverse_complement(g.fetch(c, lo, n))
            assert r.fetch(c, L - (lo + n - 1) + 1, n) == want, f"record {c}, source range {lo}:{lo + n - 1}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", default="400m,400m+7,grch38")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: at least 20 timed runs")
    h = hip()
    ctx = _lib.Context(0)
    st = C.c_void_p(ctx.stream)
    ev = [C.c_void_p() for _ in range(2)]
    for e in ev:
        check(h.hipEventCreate(C.byref(e)), "hipEventCreate")
    out = {"tool": "tools/revcomp_time.py", "reps": args.reps, "warmup": args.warmup, "hbm_peak_TBps": HBM_PEAK_BPS / 1e12,
           "copy_TBps": COPY_BPS / 1e12, "genomes": {}}
    rng = np.random.default_rng(7)

    def timed(fn):
        check(h.hipEventRecord(ev[0], st), "hipEventRecord")
        fn()
        check(h.hipEventRecord(ev[1], st), "hipEventRecord")
        check(h.hipEventSynchronize(ev[1]), "hipEventSynchronize")
        ms = C.c_float(0)
        check(h.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]), "hipEventElapsedTime")
        return float(ms.value)

    for name in args.genomes.split(","):
        lens = {"400m": [400_000_000], "400m+7": [400_000_007], "grch38": list(workloads.GRCH38_LENS)}.get(name) or [int(float(name))]
        nbytes = ascii_bytes(lens)
        g = ctx.genome_synthetic(lens, 77)
        r = g.revcomp()
        check(h.hipStreamSynchronize(st), "hipStreamSynchronize")
        verify(g, r, lens, rng)
        a, b = C.c_void_p(), C.c_void_p()
        check(h.hipMalloc(C.byref(a), nbytes), "hipMalloc")
        check(h.hipMalloc(C.byref(b), nbytes), "hipMalloc")
        check(h.hipMemsetAsync(a, 0x41, nbytes, st), "hipMemsetAsync")
        kern = lambda: g.revcomp_into(r)
        copy = lambda: check(h.hipMemcpyAsync(b, a, nbytes, D2D, st), "hipMemcpyAsync")
        k_ms, c_ms = [], []
        for it in range(args.warmup + args.reps):
            tk, tc = timed(kern), timed(copy)
            if it >= args.warmup:
                k_ms.append(tk); c_ms.append(tc)
        verify(g, r, lens, rng)
        km, cm = float(np.median(k_ms)), float(np.median(c_ms))
        row = {"records": len(lens), "bases": int(sum(lens)), "ascii_bytes": nbytes, "kernel": spread(k_ms), "copy": spread(c_ms),
               "kernel_over_copy": round(km / cm, 4), "kernel_GBps": round(2 * nbytes / (km * 1e-3) / 1e9, 1),
               "copy_GBps": round(2 * nbytes / (cm * 1e-3) / 1e9, 1),
               "kernel_fraction_of_hbm_peak": round(2 * nbytes / (km * 1e-3) / HBM_PEAK_BPS, 4),
               "kernel_Gbp_per_s": round(sum(lens) / (km * 1e-3) / 1e9, 1),
               # does the run-to-run spread explain the difference?  (the kernel's fastest run against the copy's slowest)
               "difference_beyond_spread": bool(min(k_ms) > max(c_ms) or max(k_ms) < min(c_ms))}
        out["genomes"][name] = row
        print(name, json.dumps(row), flush=True)
        check(h.hipFree(a), "hipFree"); check(h.hipFree(b), "hipFree")
        r.free(); g.free()
    for e in ev:
        h.hipEventDestroy(e)
    ctx.close()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
