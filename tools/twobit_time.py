"""Ingest of one genome as FASTA text and as UCSC .2bit, from the page cache to the resident packed genome, in one run:
kgma_genome_from_fasta_file against kgma_genome_from_2bit_file end to end (median (min .. max) of 7 calls after 2 warm-ups),
twobit_unpack_kernel alone (hipEvents; GB/s of the 1.25 bytes it moves per base), and findGenes on both files.
usage: python tools/twobit_time.py [--mb 400] [--out profiles/twobit_time.json]

The genome: 24 records of random bases with a mutated reference gene every ~400 kb (tools/e2e_time.py), a few runs of N per
record and soft-mask blocks of 100 ... 700 bases every 100 ... 700 bases (about half the genome, as a mammalian assembly's).  It is
written once as FASTA (60-column lines, N and lower case in the text) and once as .2bit by the test writer (tests/twobit_ref.py)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmergma.jl_amd")]

from kmergma_amd import _lib, api, fasta  # noqa: E402
from tests import twobit_ref as tb  # noqa: E402

COPY_TBS = 6.29                      # measured device copy, TB/s


def make_record(rng, per, genes):
    B = np.frombuffer(b"ACGT", dtype=np.uint8)
    a = B[rng.integers(0, 4, size=per)].copy()
    for _ in range(max(1, per // 400_000)):                            # a mutated gene every ~400 kb
        g = np.frombuffer(genes[int(rng.integers(0, len(genes)))], dtype=np.uint8).copy()
        hit = rng.random(g.size) < 0.04
        g[hit] = B[rng.integers(0, 4, size=int(hit.sum()))]
        p = int(rng.integers(0, per - g.size))
        a[p:p + g.size] = g
    for _ in range(3):                                                 # a few runs of N
        p = int(rng.integers(0, per - 60_000))
        a[p:p + int(rng.integers(100, 50_000))] = ord("N")
    steps = rng.integers(100, 700, size=per // 400 * 2 + 16)           # gap, block, gap, block, ...
    edges = np.cumsum(steps)
    edges = edges[edges < per]
    toggle = np.zeros(per + 1, dtype=np.int8)
    toggle[edges] = 1
    a[(np.cumsum(toggle[:per]) & 1).astype(bool)] |= 0x20
    return a


def stats(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)), calls=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=400)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ref_path = os.path.join(ROOT, "tests", "data", "Alp_V_ref.fasta")
    genes = [r.sequence.upper() for r in fasta.read_fasta(ref_path)]
    rng = np.random.default_rng(11)
    n_rec = 24
    per = args.mb * 1_000_000 // n_rec // 60 * 60
    tmp = tempfile.mkdtemp(dir="/tmp")
    fa, p2 = os.path.join(tmp, "genome.fasta"), os.path.join(tmp, "genome.2bit")
    bodies, n_blocks, m_blocks = [], 0, 0
    with open(fa, "wb") as f:
        for r in range(n_rec):
            a = make_record(rng, per, genes)
            f.write(b">chr%d\n" % (r + 1))
            f.write(b"\n".join(x.tobytes() for x in a.reshape(-1, 60)) + b"\n")
            bodies.append(tb.pack_record(a.tobytes()))
    names = [b"chr%d" % (r + 1) for r in range(n_rec)]
    with open(p2, "wb") as f:                                          # (tb.twobit_bytes, without a second copy of the bodies)
        pos = 16 + sum(1 + len(n) + 4 for n in names)
        f.write(np.asarray([tb.SIGNATURE, 0, n_rec, 0], dtype="<u4").tobytes())
        for n, b in zip(names, bodies):
            f.write(bytes([len(n)]) + n + np.asarray([pos], dtype="<u4").tobytes())
            pos += len(b)
        for b in bodies:
            f.write(b)
    del bodies
    info = _lib.twobit_inspect(p2)
    total = info["total_bases"]
    res = dict(bases=total, records=n_rec, fasta_bytes=os.path.getsize(fa), twobit_bytes=os.path.getsize(p2),
               n_blocks=info["n_blocks"], mask_blocks=info["mask_blocks"], warmups=2)
    print("genome: %d bases, %d N blocks, %d mask blocks; FASTA %d bytes, .2bit %d bytes" % (
        total, info["n_blocks"], info["mask_blocks"], res["fasta_bytes"], res["twobit_bytes"]), flush=True)
    try:
        ctx = api.default_context()
        # the two ingests give the same genome (checked on a sample of every record before anything is timed)
        ga, gb = ctx.genome_from_fasta(fa), ctx.genome_from_2bit(p2)
        assert ga.n_contigs == gb.n_contigs == n_rec and ga.total_bases == gb.total_bases == total
        for c in range(n_rec):
            for pos in (1, per // 2, per - 99_999):
                assert ga.fetch(c, pos, 100_000) == gb.fetch(c, pos, 100_000), (c, pos)
        ga.free(); gb.free()
        times = {"fasta": [], "twobit": []}
        kernel = []
        for rep in range(9):                                           # alternating, 2 warm-ups each
            for key, path in (("fasta", fa), ("twobit", p2)):
                t0 = time.perf_counter()
                g = ctx.genome_from_path(path)
                g.fetch(0, 1, 10)                                      # waits for the pack
                dt = (time.perf_counter() - t0) * 1e3
                if key == "twobit":
                    k_ms = ctx.twobit_unpack_ms()
                g.free()
                if rep >= 2:
                    times[key].append(dt)
                    if key == "twobit":
                        kernel.append(k_ms)
        res["ingest_fasta_ms"] = stats(times["fasta"])
        res["ingest_twobit_ms"] = stats(times["twobit"])
        res["unpack_kernel_ms"] = stats(kernel)
        res["unpack_kernel_GBs"] = 1.25 * total / (res["unpack_kernel_ms"]["median"] * 1e-3) / 1e9
        res["unpack_kernel_share_of_copy"] = res["unpack_kernel_GBs"] / (COPY_TBS * 1e3)
        res["twobit_slowest_below_fasta_fastest"] = res["ingest_twobit_ms"]["max"] < res["ingest_fasta_ms"]["min"]
        for key, path in (("fasta", fa), ("twobit", p2)):
            ms, n_hits = [], 0
            for rep in range(9):
                t0 = time.perf_counter()
                out = api.findGenes(genome_path=path, ref_path=ref_path, KmerDistThr=30, verbose=False, ctx=ctx)
                dt = (time.perf_counter() - t0) * 1e3
                n_hits = len(out[0])
                if rep >= 2:
                    ms.append(dt)
            res["findGenes_%s_ms" % key] = stats(ms)
            res["findGenes_%s_hits" % key] = n_hits
        for k in ("ingest_fasta_ms", "ingest_twobit_ms", "unpack_kernel_ms", "findGenes_fasta_ms", "findGenes_twobit_ms"):
            print("%-22s %8.2f ms (%.2f .. %.2f)" % (k, res[k]["median"], res[k]["min"], res[k]["max"]), flush=True)
        print("unpack kernel: %.0f GB/s of 1.25 B per base = %.2f of the %.2f TB/s copy" % (
            res["unpack_kernel_GBs"], res["unpack_kernel_share_of_copy"], COPY_TBS), flush=True)
        print("slowest .2bit ingest below fastest FASTA ingest:", res["twobit_slowest_below_fasta_fastest"], flush=True)
        print(json.dumps(res), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
    finally:
        os.unlink(fa); os.unlink(p2); os.rmdir(tmp)


if __name__ == "__main__":
    main()
