#!/usr/bin/env python3
"""Time of kgma_window_dists against the only route the library offered to the same numbers before it existed:
kgma_genome_fetch_batch (the windows' residues to the host) followed by kgma_kmer_dist_batch (back to the device).

Workload: one synthetic 400 Mb record (kgma_genome_synthetic), the fixture KFV (tests/data/Alp_V_ref.fasta, k = 6, W = 289) and
10^6 windows drawn by api.sample_window_starts.  Both sides are timed with hipEvents on kgma_stream around the WHOLE call(s) --
uploads, kernels, downloads: each call ends in a stream synchronise -- after warm-up calls of the same shape; the new call's
kernel alone is kgma_stats.scan_ms.  Every measurement runs in a fresh child process, and the two sides alternate (--rounds) so
that a drift of the machine shows as spread, not as a difference.  `--old-lib PATH` names the build of libkgma.so that runs the
old route (the parent commit's build; default: this tree's library, whose two functions are the same code).  The children leave
their first distances in the result, and the two routes must agree to 1e-9 (the old route sums Float64 squares over 4^k bins, the
new one divides an exact integer).

Also recorded, without a condition: kgma_mutation_dists for the 84 fixture genes x 81 rates (0:0.0125:1) x 42 trials.

usage: python tools/window_dists_time.py [--old-lib PATH] [--bases 400000000] [--windows 1000000] [--rounds 2]
                                         [--out profiles/window_dists_time.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmergma.jl_amd")]

from kmergma_amd import _lib, api, fasta, refprep  # noqa: E402

REF = os.path.join(ROOT, "tests", "data", "Alp_V_ref.fasta")
K = 6
SEED = 77


class Events:
    def __init__(self, stream):
        h = self.h = C.CDLL("libamdhip64.so")
        h.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        h.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        h.hipEventSynchronize.argtypes = [C.c_void_p]
        h.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.st = C.c_void_p(stream)
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            self.check(h.hipEventCreate(C.byref(e)))

    @staticmethod
    def check(st):
        if st != 0:
            raise RuntimeError(f"HIP status {st}")

    def timed(self, fn):
        self.check(self.h.hipEventRecord(self.ev[0], self.st))
        fn()
        self.check(self.h.hipEventRecord(self.ev[1], self.st))
        self.check(self.h.hipEventSynchronize(self.ev[1]))
        ms = C.c_float(0)
        self.check(self.h.hipEventElapsedTime(C.byref(ms), self.ev[0], self.ev[1]))
        return float(ms.value)


def spread(ms):
    return {"min_ms": round(min(ms), 3), "median_ms": round(float(np.median(ms)), 3), "max_ms": round(max(ms), 3), "runs": len(ms)}


def workload(args):
    RV, W, _cons, (_S, N) = refprep.gen_ref_ws_cons(REF, K, return_int=True)
    contig, start = api.sample_window_starts([args.bases], W, args.windows, 42)
    return RV, W, N, contig, start


def role_new(args):
    """kgma_window_dists (and kgma_mutation_dists) on this tree's library."""
    RV, W, N, contig, start = workload(args)
    ctx = _lib.Context(0)
    ev = Events(ctx.stream)
    ctx.set_refs(K, [RV], [W], [30.0], [N])
    g = ctx.genome_synthetic([args.bases], SEED)
    call, kernel, res = [], [], None
    for it in range(args.warmup + args.reps):
        ms = ev.timed(lambda: ctx.window_dists(g, 1, contig, start))
        if it >= args.warmup:
            call.append(ms)
            kernel.append(ctx.stats()["scan_ms"])
    _D, res = ctx.window_dists(g, 1, contig, start)
    out = {"call": spread(call), "kernel": spread(kernel), "kernel_name": ctx.kernel_name(), "windows": int(contig.size),
           "first": res[:1000].tolist(), "sum": float(res.sum())}
    g.free()
    genes = [r.sequence for r in fasta.read_fasta(REF)]
    rates = np.arange(0, 1 + 1e-9, 0.0125)
    mcall, mkernel = [], []
    for it in range(args.warmup + args.reps):
        ms = ev.timed(lambda: ctx.mutation_dists(genes, 1, rates, 42, 42))
        if it >= args.warmup:
            mcall.append(ms)
            mkernel.append(ctx.stats()["scan_ms"])
    out["mutation"] = {"sequences": len(genes), "rates": int(rates.size), "trials": 42, "distances": len(genes) * int(rates.size) * 42,
                       "call": spread(mcall), "kernel": spread(mkernel), "kernel_name": ctx.kernel_name()}
    ctx.close()
    return out


def role_route(args):
    """kgma_genome_fetch_batch + kgma_kmer_dist_batch through a binding of its own: the library may be a build that lacks the
    calibration entry points."""
    RV, W, _N, contig, start = workload(args)
    L = C.CDLL(args.lib)
    vp, i32, i64, u64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double
    P = C.POINTER
    L.kgma_create.argtypes = [C.c_int, P(vp)]
    L.kgma_destroy.argtypes = [vp]
    L.kgma_destroy.restype = None
    L.kgma_last_error.restype = C.c_char_p
    L.kgma_last_error.argtypes = [vp]
    L.kgma_stream.argtypes = [vp]
    L.kgma_stream.restype = vp
    L.kgma_genome_synthetic.argtypes = [vp, P(i64), i64, u64, C.c_char_p, i64, P(i64), P(i64), i64, P(vp)]
    L.kgma_genome_fetch_batch.argtypes = [vp, vp, i64, P(i64), P(i64), P(i64), C.c_char_p, i64]
    L.kgma_kmer_dist_batch.argtypes = [vp, i32, P(dbl), C.c_char_p, P(i64), i64, P(dbl)]
    L.kgma_genome_free.argtypes = [vp, vp]
    L.kgma_genome_free.restype = None
    ctx = vp()

    def ok(st):
        if st != 0:
            raise RuntimeError(f"libkgma status {st}: {L.kgma_last_error(ctx).decode()}")

    ok(L.kgma_create(0, C.byref(ctx)))
    ev = Events(L.kgma_stream(ctx))
    lens = np.asarray([args.bases], dtype=np.int64)
    g = vp()
    ok(L.kgma_genome_synthetic(ctx, lens.ctypes.data_as(P(i64)), 1, u64(SEED), None, 0, None, None, 0, C.byref(g)))
    n = int(contig.size)
    c64 = contig.astype(np.int64)
    ln = np.full(n, W, dtype=np.int64)
    off = np.arange(n + 1, dtype=np.int64) * W
    buf = C.create_string_buffer(n * W)
    ref = np.ascontiguousarray(RV, dtype=np.float64)
    dist = np.zeros(n, dtype=np.float64)

    def route():
        ok(L.kgma_genome_fetch_batch(ctx, g, n, c64.ctypes.data_as(P(i64)), start.ctypes.data_as(P(i64)), ln.ctypes.data_as(P(i64)), buf, n * W))
        ok(L.kgma_kmer_dist_batch(ctx, K, ref.ctypes.data_as(P(dbl)), buf, off.ctypes.data_as(P(i64)), n, dist.ctypes.data_as(P(dbl))))

    call = []
    for it in range(args.warmup + args.reps):
        ms = ev.timed(route)
        if it >= args.warmup:
            call.append(ms)
    out = {"call": spread(call), "windows": n, "bytes_each_way": n * W, "lib": os.path.basename(os.path.dirname(os.path.abspath(args.lib))) or ".",
           "has_window_dists": hasattr(L, "kgma_window_dists"), "first": dist[:1000].tolist(), "sum": float(dist.sum())}
    L.kgma_genome_free(ctx, g)
    L.kgma_destroy(ctx)
    return out


def child(role, args, lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--role", role, "--bases", str(args.bases), "--windows", str(args.windows),
           "--reps", str(args.reps), "--warmup", str(args.warmup)]
    if lib:
        cmd += ["--lib", lib]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)
    if p.returncode != 0:
        raise SystemExit(f"{role}: child ended with status {p.returncode}")          # nothing further is started
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--role", default="")
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    ap.add_argument("--old-lib", default="")
    ap.add_argument("--bases", type=int, default=400_000_000)
    ap.add_argument("--windows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.role:
        print(json.dumps(role_new(args) if args.role == "new" else role_route(args)), flush=True)
        return
    old = args.old_lib or _lib.LIB_PATH
    out = {"tool": "tools/window_dists_time.py", "bases": args.bases, "k": K, "reps_per_round": args.reps, "warmup": args.warmup,
           "timing": "hipEvents on kgma_stream around the whole call(s), fresh process per measurement, sides alternating",
           "old_route_lib": "the parent commit's build" if args.old_lib else "this build", "rounds": []}
    for _ in range(args.rounds):
        r = child("route", args, old)
        w = child("new", args)
        a, b = np.asarray(r.pop("first")), np.asarray(w.pop("first"))
        assert np.all(np.abs(a - b) <= 1e-9 * b), "the two routes disagree"
        assert abs(r["sum"] - w["sum"]) <= 1e-9 * w["sum"]
        out["rounds"].append({"fetch_batch_plus_kmer_dist_batch": r, "window_dists": w})
        print(json.dumps(out["rounds"][-1]), flush=True)
    old_ms = [x["fetch_batch_plus_kmer_dist_batch"]["call"] for x in out["rounds"]]
    new_ms = [x["window_dists"]["call"] for x in out["rounds"]]
    out["old_route_median_ms"] = round(float(np.median([x["median_ms"] for x in old_ms])), 3)
    out["window_dists_median_ms"] = round(float(np.median([x["median_ms"] for x in new_ms])), 3)
    out["speedup"] = round(out["old_route_median_ms"] / out["window_dists_median_ms"], 2)
    # the issue's condition, on the spreads: the new call's slowest run against the old route's fastest
    out["not_slower_beyond_spread"] = bool(max(x["max_ms"] for x in new_ms) <= min(x["min_ms"] for x in old_ms))
    out["mutation_dists"] = out["rounds"][-1]["window_dists"]["mutation"]
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
