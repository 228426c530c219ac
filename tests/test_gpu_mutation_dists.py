"""kgma_mutation_dists on the device: the distance of mutated copies that are never materialised, against the host mirror of
the mutation rule (api.mutate_seq, itself held to tests/calib_ref.py in test_calib_host.py) and the plain-Python D of
tests/calib_ref.py: sequence lengths around k and the workgroup's stride, the ends of the rate range, both kernel forms, the
Float64 form within (4^k + 4) 2^-53 of the exact rational value, the errors, and what a result may depend on."""
import os
from fractions import Fraction

import numpy as np
import pytest

from kmergma_amd import _lib, api, fasta
from tests import calib_ref as cr
from tests.conftest import DATA
from tests.helpers import random_dna
from tests.test_gpu_window_dists import form, random_table, status

pytestmark = pytest.mark.gpu

RATES = [0.0, 2.0 ** -53, 0.0125, 0.5, 1.0]
SEED = 9


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def lengths(k):
    return [0, 1, k - 1, k, k + 1, 64 + k - 1, 300, 5000]


def mixed_case(rng, n):
    a = bytearray(random_dna(rng, n))
    for i in np.flatnonzero(rng.random(n) < 0.2).tolist():
        a[i] |= 0x20
    return bytes(a)


@pytest.mark.parametrize("k", [6, 8])
def test_exact_against_host_mirror(ctx, k):
    rng = np.random.default_rng([90, k])
    seqs = [mixed_case(rng, n) for n in lengths(k)]
    N = 11
    S = random_table(rng, k, seqs, N)
    sumS2 = cr.sum_sq(S)
    ctx.set_refs(k, [S / float(N)], [k + 1], [1.0], [N])
    D, dist = ctx.mutation_dists(seqs, 1, RATES, 3, SEED)
    assert ctx.kernel_name() == form(k, source="mutation")
    st = ctx.stats()
    assert st["n_launches"] == 1 and st["scan_ms"] > 0
    assert D.shape == dist.shape == (len(seqs), len(RATES), 3)
    for i, s in enumerate(seqs):
        for r, rate in enumerate(RATES):
            for t in range(3):
                m = api.mutate_seq(s, rate, seed=SEED, stream=(i, r, t))
                assert int(D[i, r, t]) == cr.D(m, S, N, k, sumS2), (i, r, t)
    assert np.array_equal(dist, D.astype(np.float64) / ctx.kfv_scale(1))
    # a sequence shorter than k counts nothing
    assert set(D[:3].ravel().tolist()) == {sumS2}
    # the rates do what they say on the 5000-residue sequence: none, (almost surely) none, some, all positions substituted
    assert len(set(D[7, 0].tolist())) == 1 and D[7, 0, 0] == cr.D(seqs[7], S, N, k, sumS2)
    assert len(set(D[7, 3].tolist())) == 3
    if k == 8:
        # again in the same context: the per-workgroup table was left all-zero
        D2, _ = ctx.mutation_dists(seqs[::-1], 1, [0.0], 1, SEED)
        assert D2[:, 0, 0].tolist() == [cr.D(s, S, N, k, sumS2) for s in seqs[::-1]]


def test_rate_zero_equals_window_dists(ctx, alp_ref):
    """The fixture's own genes of one length W, each laid into a genome as a record of its own: at rate 0 every trial is the
    distance of that record's only window."""
    genes = [r.sequence for r in fasta.read_fasta(os.path.join(DATA, "Alp_V_ref.fasta"))]
    W = 288
    genes = [g for g in genes if len(g) == W]
    assert len(genes) >= 60
    ctx.set_refs(6, [alp_ref["RV"]], [W], [30.0], [alp_ref["N"]])
    g = ctx.genome_from_host(genes)
    try:
        Dw, dw = ctx.window_dists(g, 1, list(range(len(genes))), [1] * len(genes))
    finally:
        g.free()
    D, d = ctx.mutation_dists(genes, 1, [0.0, 0.3, 0.0], 4, 42)
    for r in (0, 2):
        for t in range(4):
            assert np.array_equal(D[:, r, t], Dw) and np.array_equal(d[:, r, t], dw)
    assert Dw.tolist() == [cr.D(s, alp_ref["S"], alp_ref["N"], 6) for s in genes]
    # a diverged copy lies farther from the family than the gene itself, on average
    assert d[:, 1].mean() > d[:, 0].mean() + 5


@pytest.mark.parametrize("k", [3, 6, 8])
def test_float_form(ctx, alp_ref, k):
    rng = np.random.default_rng([91, k])
    if k == 6:
        ref = alp_ref["RV"] * (np.pi / 3)
    else:
        ref = np.zeros(4 ** k)
        at = rng.integers(0, 4 ** k, size=min(4 ** k, 2000))
        ref[at] = rng.random(at.size) * 4
    seqs = [random_dna(rng, n) for n in (300, 2, 97)]
    rates = [0.0, 0.1]
    ctx.set_refs(k, [ref], [k + 1], [1.0], None)
    assert ctx.kfv_is_float(1)
    D, dist = ctx.mutation_dists(seqs, 1, rates, 2, SEED)
    assert ctx.kernel_name() == form(k, fp=True, source="mutation")
    scale = ctx.kfv_scale(1)
    sumR2 = cr.sum_ref2(ref)
    bound = Fraction(4 ** k + 4, 2 ** 53)
    worst = Fraction(0)
    for i, s in enumerate(seqs):
        for r, rate in enumerate(rates):
            for t in range(2):
                exact = cr.float_dist(api.mutate_seq(s, rate, seed=SEED, stream=(i, r, t)), ref, k, sumR2)
                got = float(dist[i, r, t])
                err = abs(Fraction(got) - exact) / exact
                worst = max(worst, err)
                assert err <= bound, (i, r, t, float(err))
                assert int(D[i, r, t]) == int(Fraction(got * scale) + Fraction(1, 2))
    print("k", k, "worst relative error", float(worst), "bound", float(bound))


def test_errors(alp_ref):
    ctx = _lib.Context(0)
    try:
        seqs = [b"ACGTACGTAC", b"ACNTACGTAC", b"ACGTACGTAX"]
        assert status(lambda: ctx.mutation_dists(seqs[:1], 1, [0.1], 1, 1))[0] == _lib.KGMA_E_STATE
        ctx.set_refs(6, [alp_ref["RV"]], [alp_ref["ws"]], [30.0], [alp_ref["N"]])
        st, msg = status(lambda: ctx.mutation_dists(seqs, 1, [0.0], 1, 1))
        assert st == _lib.KGMA_E_BADBASE and "sequence 1 position 3" in msg          # an N, at rate 0 too
        st, msg = status(lambda: ctx.mutation_dists([seqs[0], seqs[2]], 1, [0.5], 2, 1))
        assert st == _lib.KGMA_E_BADBASE and "sequence 1 position 10" in msg
        for bad in (1.5, float("nan"), -0.1, float("inf")):
            st, msg = status(lambda: ctx.mutation_dists(seqs[:1], 1, [0.2, bad], 1, 1))
            assert st == _lib.KGMA_E_ARG and "rates[1]" in msg
        assert status(lambda: ctx.mutation_dists(seqs[:1], 1, [0.2], 0, 1))[0] == _lib.KGMA_E_ARG
        assert status(lambda: ctx.mutation_dists(seqs[:1], 1, [], 1, 1))[0] == _lib.KGMA_E_ARG
        assert status(lambda: ctx.mutation_dists(seqs[:1], 2, [0.2], 1, 1))[0] == _lib.KGMA_E_ARG
        D, _ = ctx.mutation_dists([], 1, [0.2], 1, 1)
        assert D.shape == (0, 1, 1)
        # the context is still in service
        D, _ = ctx.mutation_dists(seqs[:1], 1, [0.0], 1, 1)
        assert D.tolist() == [[[cr.D(seqs[0], alp_ref["S"], alp_ref["N"], 6)]]]
    finally:
        ctx.close()


def test_what_a_result_depends_on(ctx, alp_ref):
    """Context.mutation_dists' docstring: entry [i, r, t] is a function of (seed, i, r, t, sequence i, rates[r]) alone -- not of
    the sequences, rates or trials that follow; the INDEX r is part of the key, so the same rate at another index redraws."""
    rng = np.random.default_rng(92)
    seqs = [random_dna(rng, n) for n in (400, 289, 150, 600)]
    ctx.set_refs(6, [alp_ref["RV"]], [alp_ref["ws"]], [30.0], [alp_ref["N"]])
    full, _ = ctx.mutation_dists(seqs, 1, [0.1, 0.5], 3, 5)
    part, _ = ctx.mutation_dists(seqs[:2], 1, [0.1, 0.5], 3, 5)
    assert np.array_equal(part, full[:2])
    fewer, _ = ctx.mutation_dists(seqs, 1, [0.1], 2, 5)
    assert np.array_equal(fewer, full[:, :1, :2])
    swapped, _ = ctx.mutation_dists(seqs, 1, [0.5, 0.1], 3, 5)
    assert not np.array_equal(swapped[:, 0], full[:, 1]) and not np.array_equal(swapped[:, 1], full[:, 0])
    S, N = alp_ref["S"], alp_ref["N"]
    for i, s in enumerate(seqs):
        for t in range(3):
            assert int(swapped[i, 0, t]) == cr.D(api.mutate_seq(s, 0.5, seed=5, stream=(i, 0, t)), S, N, 6)
            assert int(full[i, 1, t]) == cr.D(api.mutate_seq(s, 0.5, seed=5, stream=(i, 1, t)), S, N, 6)
    other_seed, _ = ctx.mutation_dists(seqs, 1, [0.1, 0.5], 3, 6)
    assert not np.array_equal(other_seed, full)
    # a rate of 0 never substitutes, at whatever index
    zero, _ = ctx.mutation_dists(seqs, 1, [0.3, 0.0], 2, 5)
    assert zero[:, 1, 0].tolist() == zero[:, 1, 1].tolist() == [cr.D(s, S, N, 6) for s in seqs]


def test_api_mutation_dists(ctx, alp_ref):
    path = os.path.join(DATA, "Alp_V_ref.fasta")
    genes = [r.sequence for r in fasta.read_fasta(path)]
    rates = [0.0, 0.05, 0.4]
    d = api.mutation_dists(path, alp_ref["RV"], 6, rates=rates, n_trials=2, seed=3, n_refs=alp_ref["N"], ctx=ctx)
    assert d.shape == (len(genes), 3, 2)
    scale = ctx.kfv_scale(1)
    for i in (0, 17, 83):
        for r in range(3):
            assert d[i, r, 1] == cr.D(api.mutate_seq(genes[i], rates[r], seed=3, stream=(i, r, 1)), alp_ref["S"], alp_ref["N"], 6) / scale
    d2 = api.mutation_dists(genes[:3], alp_ref["RV"], 6, rates=rates, n_trials=2, seed=3, n_refs=alp_ref["N"], ctx=ctx)
    assert np.array_equal(d2, d[:3])
    g = api.gen_sub_vs_ref(2, 0.25, k=6, RKV=path, ctx=ctx)
    assert g.shape == (len(genes), 5, 2)
    assert np.array_equal(g[:, 0, 0], d[:, 0, 0])                          # rate 0: the genes themselves
