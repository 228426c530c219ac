"""Threshold calibration through the api: estimate_threshold_from_genome recomputed in Python from the oracle's exact D, the
off-lattice rule seen by a real scan (kgma_stats.n_at_threshold), and api.window_dists on every kind of genome input."""
import math
import os

import numpy as np
import pytest

from kmergma_amd import _lib, api, fasta
from tests import calib_ref as cr
from tests import twobit_ref as tb
from tests.conftest import DATA

pytestmark = pytest.mark.gpu

LOCI = os.path.join(DATA, "Loci.fasta")
REF = os.path.join(DATA, "Alp_V_ref.fasta")
N_SAMPLES = 5000
# the quantile (with buffer = 0) whose estimate is a lattice point that 16 tested windows of Loci.fasta attain: picked from the
# oracle's D list on the CPU, and checked against it in test_lattice_threshold_is_at_threshold
LATTICE_QUANTILE = 0.01


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def loci_D(alp_ref, loci):
    """(sequences, the oracle's [D1] + Dout per record, scale): computed once."""
    seqs = [r.sequence for r in loci]
    return seqs, cr.oracle_D(seqs, alp_ref["S"], alp_ref["N"], 6, alp_ref["ws"]), 2.0 * 6 * alp_ref["N"] * alp_ref["N"]


def sampled(seqs, D, scale, W, seed=42):
    c, s = api.sample_window_starts([len(x) for x in seqs], W, N_SAMPLES, seed)
    assert c.size == N_SAMPLES
    return [D[ci][si - 1] / scale for ci, si in zip(c.tolist(), s.tolist())]


def test_estimator_mean_and_quantile(ctx, alp_ref, loci_D):
    seqs, D, scale = loci_D
    RV, W, N = alp_ref["RV"], alp_ref["ws"], alp_ref["N"]
    d = sampled(seqs, D, scale, W)
    mean = math.fsum(d) / len(d) - 8
    assert api.estimate_threshold_from_genome(LOCI, RV, W, 6, n_samples=N_SAMPLES, off_lattice=False, n_refs=N, ctx=ctx) == mean
    assert ctx.kfv_scale(1) == scale
    got = api.estimate_threshold_from_genome(LOCI, RV, W, 6, n_samples=N_SAMPLES, n_refs=N, ctx=ctx)
    assert got == (math.floor(mean * scale) + 0.5) / scale and abs(got - mean) <= 1 / scale
    q = sorted(d)[math.ceil(0.01 * len(d)) - 1] - 8
    assert api.estimate_threshold_from_genome(LOCI, RV, W, 6, n_samples=N_SAMPLES, quantile=0.01, off_lattice=False, n_refs=N, ctx=ctx) == q
    assert api.estimate_threshold_from_genome(LOCI, RV, W, 6, n_samples=N_SAMPLES, quantile=0.01, n_refs=N, ctx=ctx) == (math.floor(q * scale) + 0.5) / scale
    assert api.estimate_threshold_from_genome(LOCI, RV, W, 6, n_samples=N_SAMPLES, quantile=1.0, buffer=0, off_lattice=False, n_refs=N, ctx=ctx) == max(d)
    # another seed, another buffer; an open genome instead of a path
    d7 = sampled(seqs, D, scale, W, seed=7)
    g = ctx.genome_from_path(LOCI)
    try:
        assert api.estimate_threshold_from_genome(g, RV, W, 6, n_samples=N_SAMPLES, seed=7, buffer=2.5, off_lattice=False, n_refs=N, ctx=ctx) \
            == math.fsum(d7) / len(d7) - 2.5
        assert g.n_contigs == len(seqs)                                      # it stays open
    finally:
        g.free()
    # more samples than windows: every window once
    small = [seqs[0][:1000]]
    gs = ctx.genome_from_host(small)
    try:
        every = [x / scale for x in cr.window_D(small[0], alp_ref["S"], N, 6, W)]
        assert api.estimate_threshold_from_genome(gs, RV, W, 6, n_samples=N_SAMPLES, off_lattice=False, n_refs=N, ctx=ctx) == math.fsum(every) / len(every) - 8
    finally:
        gs.free()


def test_estimator_cluster_lists(ctx, alp_clusters, loci):
    seqs = [r.sequence for r in loci]
    cl = alp_clusters
    got = api.estimate_threshold_from_genome(LOCI, cl["KFVs"], cl["ws"], 6, n_samples=400, seed=3, buffer=7, n_refs=cl["N"], ctx=ctx)
    assert isinstance(got, list) and len(got) == 5
    for j in range(5):
        W, S, N = cl["ws"][j], cl["S"][j], cl["N"][j]
        scale = 2.0 * 6 * N * N
        c, s = api.sample_window_starts([len(x) for x in seqs], W, 400, 3)
        d = [cr.D(seqs[ci][si - 1:si - 1 + W], S, N, 6) / scale for ci, si in zip(c.tolist(), s.tolist())]
        assert got[j] == api.off_lattice_threshold(math.fsum(d) / len(d) - 7, scale), j


def test_off_lattice_threshold_is_never_at_threshold(ctx, alp_ref):
    thr = api.estimate_threshold_from_genome(LOCI, alp_ref["RV"], alp_ref["ws"], 6, n_samples=N_SAMPLES, quantile=LATTICE_QUANTILE,
                                             buffer=0, n_refs=alp_ref["N"], ctx=ctx)
    hits = api.findGenes(genome_path=LOCI, ref_path=REF, KmerDistThr=thr, do_align=False, verbose=False, ctx=ctx)[0]
    assert len(hits) >= 7
    assert ctx.stats()["n_at_threshold"] == 0


def test_lattice_threshold_is_at_threshold(ctx, alp_ref, loci_D):
    seqs, D, scale = loci_D
    est = api.estimate_threshold_from_genome(LOCI, alp_ref["RV"], alp_ref["ws"], 6, n_samples=N_SAMPLES, quantile=LATTICE_QUANTILE,
                                             buffer=0, off_lattice=False, n_refs=alp_ref["N"], ctx=ctx)
    m = math.floor(est * scale)
    # the pick, against the oracle: windows the scan tests (2 ... of every record) lie exactly at the lattice point below
    at = sum(1 for rec in D for x in rec[1:] if x == m)
    assert at >= 1
    api.findGenes(genome_path=LOCI, ref_path=REF, KmerDistThr=m / scale, do_align=False, verbose=False, ctx=ctx)
    n_att = ctx.stats()["n_at_threshold"]
    print("windows at the lattice point:", at, "n_at_threshold:", n_att)
    assert n_att == at


def test_api_window_dists_inputs(ctx, alp_ref, loci, loci_D, tmp_path):
    seqs, D, scale = loci_D
    RV, W, N = alp_ref["RV"], alp_ref["ws"], alp_ref["N"]
    contig = [3, 0, 0, 2, 1]
    start = [len(seqs[3]) - W + 1, 1, 20380, 5, 777]
    want = [D[c][s - 1] for c, s in zip(contig, start)]
    Dp, dp = api.window_dists(LOCI, RV, W, 6, contig, start, n_refs=N, ctx=ctx)                    # a FASTA path
    assert Dp.tolist() == want and np.array_equal(dp, Dp / scale)
    p2 = str(tmp_path / "loci.2bit")
    tb.write_twobit(p2, [(r.description.split()[0], r.sequence) for r in loci])
    D2, d2 = api.window_dists(p2, RV, W, 6, contig, start, n_refs=N, ctx=ctx)                      # a .2bit path
    assert D2.tolist() == want and np.array_equal(d2, dp)
    g = ctx.genome_from_path(LOCI)
    try:
        Dg, _ = api.window_dists(g, RV, W, 6, contig, start, n_refs=N, ctx=ctx)                    # an open genome
        assert Dg.tolist() == want
        # the minus strand: the reverse-complemented windows, in the reversed genome's own coordinates
        rc = g.revcomp()
        try:
            Dr, _ = api.window_dists(rc, RV, W, 6, contig, start, n_refs=N, ctx=ctx)
        finally:
            rc.free()
        rcs = [fasta.reverse_complement(s) for s in seqs]
        assert Dr.tolist() == [cr.D(rcs[c][s - 1:s - 1 + W], alp_ref["S"], N, 6) for c, s in zip(contig, start)]
        assert Dr.tolist() != want
    finally:
        g.free()
    with pytest.raises(TypeError):
        api.window_dists([b"ACGT"], RV, W, 6, [0], [1], ctx=ctx)
