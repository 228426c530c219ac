"""kgma_window_dists on the device: the distance of arbitrary windows of a resident genome, against the exact-integer oracle
(every window of Loci.fasta, and the distances a KGMA_F_RETURN_DISTS scan reports) and against the plain-Python reference
tests/calib_ref.py: both kernel forms (counters in LDS, k <= 7; per-workgroup global table, k = 8 ... 10), window lengths around
the workgroup's strides up to 65 535 k-mers, the top of the int64 range, record edges and odd lists, cluster references, Float64
KFVs within (4^k + 4) 2^-53 of the exact rational value, every error status, and the call's side effects."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from kmergma_amd import _lib, refprep
from tests import calib_ref as cr
from tests import range_cases as rc
from tests.conftest import DATA
from tests.helpers import random_dna

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def form(k, fp=False, source="window"):
    return f"calib_kernel<{source},{'lds' if k <= 7 else 'global'},{'f64' if fp else 'int'}>"


def all_windows(records, W):
    c, s = [], []
    for i, r in enumerate(records):
        n = len(r) - W + 1
        if n > 0:
            c += [i] * n
            s += range(1, n + 1)
    return np.asarray(c, dtype=np.int32), np.asarray(s, dtype=np.int64)


def random_table(rng, k, records, N, smax=40, extra=64):
    """An S table (natural order) that is non-zero on about half of the records' own k-mers and on a few others."""
    S = np.zeros(4 ** k, dtype=np.int64)
    own = np.unique(np.asarray([v for r in records for v in cr.kmers(r, k)], dtype=np.int64))
    pick = own[rng.random(own.size) < 0.5] if own.size > 1 else own
    S[pick] = rng.integers(1, smax, size=pick.size)
    other = rng.integers(0, 4 ** k, size=extra)
    S[other] = rng.integers(1, smax, size=extra)
    return S


def check_int(ctx, records, S, N, k, W, contig=None, start=None, g=None):
    """set_refs + one call over the given (default: all) windows; D against calib_ref, dist == D / scale bit for bit."""
    ctx.set_refs(k, [S / float(N)], [W], [1.0], [N])
    assert not ctx.kfv_is_float(1)
    own = g is None
    g = g or ctx.genome_from_host(records)
    try:
        if contig is None:
            contig, start = all_windows(records, W)
        D, dist = ctx.window_dists(g, 1, contig, start)
        assert ctx.kernel_name() == form(k)
    finally:
        if own:
            g.free()
    want = {i: cr.window_D(r, S, N, k, W) for i, r in enumerate(records) if i in set(np.asarray(contig).tolist())}
    wantD = [want[c][s - 1] for c, s in zip(np.asarray(contig).tolist(), np.asarray(start).tolist())]
    assert D.tolist() == wantD
    assert np.array_equal(dist, D.astype(np.float64) / ctx.kfv_scale(1))
    return D


# ---- exactness on the fixture ---------------------------------------------------------------------------------------------------

def test_every_window_of_loci(ctx, alp_ref, loci):
    seqs = [r.sequence for r in loci]
    W, S, N = alp_ref["ws"], alp_ref["S"], alp_ref["N"]
    want = cr.oracle_D(seqs, S, N, 6, W)
    ctx.set_refs(6, [alp_ref["RV"]], [W], [30.0], [N])
    g = ctx.genome_from_host(seqs)
    try:
        contig, start = all_windows(seqs, W)
        assert contig.size == sum(len(w) for w in want) == 484127 + len(seqs)
        D, dist = ctx.window_dists(g, 1, contig, start)                      # one call
        assert ctx.kernel_name() == form(6)
        st = ctx.stats()
        assert st["n_launches"] == 1 and st["scan_ms"] > 0
        assert np.array_equal(D, np.concatenate([np.asarray(w, dtype=np.int64) for w in want]))
        scale = ctx.kfv_scale(1)
        assert scale == 2 * 6 * N * N
        assert np.array_equal(dist, D.astype(np.float64) / scale)
        # the windows 2 ... L - W + 1 of every record: what a KGMA_F_RETURN_DISTS scan reports
        ctx.scan(g, _lib.MODE_SINGLE, 50, 0, _lib.F_RETURN_DISTS, None)
        d = ctx.dists(1)
        assert d.size == 484127
        assert np.array_equal(d, dist[start > 1])
    finally:
        g.free()


def test_scan_results_survive(ctx, alp_ref, loci):
    seqs = [r.sequence for r in loci]
    ctx.set_refs(6, [alp_ref["RV"]], [alp_ref["ws"]], [30.0], [alp_ref["N"]])
    g = ctx.genome_from_host(seqs)
    try:
        ctx.scan(g, _lib.MODE_SINGLE, 50, 0, _lib.F_RETURN_DISTS, None)
        hits, d, st0 = ctx.hits(), ctx.dists(1).copy(), ctx.stats()
        assert len(hits) == 7
        ctx.window_dists(g, 1, [0, 1, 3], [1, 100, 5])
        assert ctx.hits() == hits
        assert np.array_equal(ctx.dists(1), d)
        st1 = ctx.stats()
        assert {f for f in st0 if st0[f] != st1[f]} <= {"scan_ms", "n_launches"}
        # and the references and thresholds: the same scan gives the same hits
        ctx.scan(g, _lib.MODE_SINGLE, 50, 0, 0, None)
        assert ctx.hits() == hits
    finally:
        g.free()


# ---- the kernel forms ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,W", [(1, 2), (2, 40), (4, 101), (5, 155), (7, 157), (8, 158), (10, 160)])
def test_kernel_forms(ctx, k, W):
    rng = np.random.default_rng([77, k])
    rec = [random_dna(rng, 3000)]
    N = 13
    S = random_table(rng, k, rec, N)
    D1 = check_int(ctx, rec, S, N, k, W)
    assert len(set(D1.tolist())) > (100 if k > 2 else 2)
    if k >= 8:
        # the same context again, other windows first: the per-workgroup table was left all-zero
        g = ctx.genome_from_host(rec)
        try:
            c, s = all_windows(rec, W)
            D2, _ = ctx.window_dists(g, 1, c[::-1].copy(), s[::-1].copy())
            assert ctx.kernel_name() == form(k)
            assert np.array_equal(D2[::-1], D1)
            D3, _ = ctx.window_dists(g, 1, c[:5], s[:5])                    # fewer windows than workgroups before
            assert np.array_equal(D3, D1[:5])
        finally:
            g.free()


# ---- window lengths around the workgroup's strides ----------------------------------------------------------------------------

@pytest.mark.parametrize("nk", [2, 63, 64, 65, 255, 256, 257, 1000])
def test_window_lengths(ctx, nk):
    k = 6
    W = nk + k - 1
    rng = np.random.default_rng([78, nk])
    rec = [random_dna(rng, W + 300), random_dna(rng, W)]
    check_int(ctx, rec, random_table(rng, k, rec, 9), 9, k, W)


def test_longest_window_poly_a(ctx):
    """65 535 k-mers, every count in one bin (and a random record of the same size beside it)."""
    k, nk = 6, 65535
    W = nk + k - 1
    rng = np.random.default_rng(79)
    rec = [b"A" * (W + 3), random_dna(rng, W + 2)]
    N = 7
    S = random_table(rng, k, [rec[1][:4000]], N)
    S[0] = 31
    D = check_int(ctx, rec, S, N, k, W)
    assert D[0] == cr.sum_sq(S) - 31 * 31 + (31 - N * nk) ** 2
    assert len(D) == 4 + 3


def test_top_of_the_int64_range(ctx):
    """tests/range_cases.py, family `copies` at the largest N kgma_set_refs accepts (d61, edge-): inside the run of C every window
    is at dmax = sum S^2 + N^2 nk^2, the largest D of the device path, just below 2^61."""
    k, nk = 6, 100
    W = nk + k - 1
    N = rc.edge_N("d61", k, W, "copies")[0]
    ref = rc.ref_of("copies", k, W, N)
    rec = [ref["base"] + b"C" * (W + 40) + ref["base"][:50]]
    D = check_int(ctx, rec, ref["S"], N, k, W)
    dmax = rc.dmax(ref["S"], N, nk)
    assert 2 ** 60 < dmax < 2 ** 61
    assert int(D.max()) == dmax and int(D[0]) == 0


# ---- record edges and lists ---------------------------------------------------------------------------------------------------

def test_record_edges_and_lists(ctx):
    k, W = 6, 120
    rng = np.random.default_rng(80)
    a = bytearray(random_dna(rng, 1000))
    a[100:160] = bytes(a[100:160]).lower()
    a[300:420] = b"N" * 120
    a[500:503] = b"nnn"
    recs = [random_dna(rng, W), bytes(a), random_dna(rng, 50), random_dna(rng, 500)]
    N = 5
    S = random_table(rng, k, recs, N)
    S[4 ** k - 1] = 17                                                       # T...T: what the runs of N count as
    g = ctx.genome_from_host(recs)
    try:
        L = [len(r) for r in recs]
        edges_c = [0, 1, 1, 3, 3]
        edges_s = [1, 1, L[1] - W + 1, 1, L[3] - W + 1]
        check_int(ctx, recs, S, N, k, W, edges_c, edges_s, g=g)
        # lower case and runs of N (as T), window by window through them
        check_int(ctx, recs, S, N, k, W, [1] * 500, list(range(1, 501)), g=g)
        # duplicates, descending
        dup_c = [3, 3, 3, 1, 1, 1, 0, 0]
        dup_s = [381, 381, 7, 881, 300, 300, 1, 1]
        D = check_int(ctx, recs, S, N, k, W, dup_c, dup_s, g=g)
        assert D[0] == D[1] and D[4] == D[5] and D[6] == D[7]
        check_int(ctx, recs, S, N, k, W, [1], [333], g=g)                    # n = 1
        D0, d0 = ctx.window_dists(g, 1, [], [])                              # n = 0
        assert D0.size == 0 and d0.size == 0 and ctx.stats()["n_launches"] == 0
    finally:
        g.free()


# ---- cluster references: kfv selects the table and W --------------------------------------------------------------------------

def test_cluster_references(ctx, alp_clusters, loci):
    from kmergma_amd import api
    seqs = [r.sequence for r in loci]
    cl = alp_clusters
    assert len(cl["ws"]) == 5 and len(set(cl["ws"])) == 3
    ctx.set_refs(6, cl["KFVs"], cl["ws"], [30.0] * 5, cl["N"])
    g = ctx.genome_from_host(seqs)
    try:
        for j in range(5):
            W = cl["ws"][j]
            c, s = api.sample_window_starts([len(x) for x in seqs], W, 150, 100 + j)
            D, dist = ctx.window_dists(g, j + 1, c, s)
            want = [cr.D(seqs[ci][si - 1:si - 1 + W], cl["S"][j], cl["N"][j], 6) for ci, si in zip(c.tolist(), s.tolist())]
            assert D.tolist() == want, j
            assert np.array_equal(dist, D.astype(np.float64) / ctx.kfv_scale(j + 1))
    finally:
        g.free()


# ---- Float64 KFVs ---------------------------------------------------------------------------------------------------------------

def check_float(ctx, rec, ref, k, W, contig, start, twice=False):
    ctx.set_refs(k, [ref], [W], [1.0], None)
    assert ctx.kfv_is_float(1)
    g = ctx.genome_from_host(rec)
    try:
        D, dist = ctx.window_dists(g, 1, contig, start)
        assert ctx.kernel_name() == form(k, fp=True)
        if twice:
            D2, dist2 = ctx.window_dists(g, 1, contig, start)
            assert np.array_equal(dist2, dist) and np.array_equal(D2, D)
    finally:
        g.free()
    scale = ctx.kfv_scale(1)
    sumR2 = cr.sum_ref2(ref)
    bound = Fraction(4 ** k + 4, 2 ** 53)        # two roundings per term, 4^k - 1 additions of non-negative terms, one scaling
    worst = Fraction(0)
    for i, (c, s) in enumerate(zip(contig, start)):
        exact = cr.float_dist(rec[c][s - 1:s - 1 + W], ref, k, sumR2)
        err = abs(Fraction(float(dist[i])) - exact) / exact
        worst = max(worst, err)
        assert err <= bound, (i, float(err), float(bound))
        assert int(D[i]) == math.floor(Fraction(float(dist[i]) * scale) + Fraction(1, 2))
    print("k", k, "worst relative error", float(worst), "bound", float(bound))


def test_float_kfv_fixture(ctx, alp_ref, alp_locus):
    rec = [r.sequence for r in alp_locus]
    W = alp_ref["ws"]
    rng = np.random.default_rng(81)
    start = sorted(rng.integers(1, len(rec[0]) - W + 2, size=40).tolist()) + [1, len(rec[0]) - W + 1]
    check_float(ctx, rec, alp_ref["RV"] * (math.pi / 3), 6, W, [0] * len(start), start)


def test_float_kfv_random_table(ctx):
    rng = np.random.default_rng(82)
    rec = [random_dna(rng, 400), random_dna(rng, 77)]
    c, s = all_windows(rec, 50)
    check_float(ctx, rec, rng.random(64) * 5, 3, 50, c.tolist(), s.tolist())


def test_float_kfv_global_table(ctx):
    rng = np.random.default_rng(83)
    rec = [random_dna(rng, 1200)]
    ref = np.zeros(4 ** 8)
    ref[rng.integers(0, 4 ** 8, size=3000)] = rng.random(3000) * 3
    ref[np.asarray(cr.kmers(rec[0], 8))[::3]] = math.e / 2
    start = list(range(1, 1200 - 300 + 2, 37))
    check_float(ctx, rec, ref, 8, 300, [0] * len(start), start, twice=True)


# ---- errors -----------------------------------------------------------------------------------------------------------------------

def status(fn):
    with pytest.raises(_lib.KgmaError) as e:
        fn()
    return e.value.status, e.value.message


def test_errors():
    ctx = _lib.Context(0)
    try:
        rng = np.random.default_rng(84)
        k, W, N = 6, 100, 3
        recs = [random_dna(rng, 300), random_dna(rng, 99), random_dna(rng, 200) + b"X" + random_dna(rng, 200)]
        g = ctx.genome_from_host(recs)
        # before kgma_set_refs
        assert status(lambda: ctx.window_dists(g, 1, [0], [1]))[0] == _lib.KGMA_E_STATE
        S = random_table(rng, k, recs[:1], N)
        ctx.set_refs(k, [S / float(N)], [W], [1.0], [N])
        for kfv in (0, 2, -1):
            assert status(lambda: ctx.window_dists(g, kfv, [0], [1]))[0] == _lib.KGMA_E_ARG
        for c in (-1, 3):
            st, msg = status(lambda: ctx.window_dists(g, 1, [0, 0, c], [1, 2, 1]))
            assert st == _lib.KGMA_E_ARG and "window 2" in msg
        for c, s in ((0, 0), (0, 202), (1, 1), (0, -5)):                     # outside the record; a record shorter than W
            st, msg = status(lambda: ctx.window_dists(g, 1, [0, c], [201, s]))
            assert st == _lib.KGMA_E_ARG and "window 1" in msg
        # a bad residue inside a requested window: record 2, position 201
        for s in (102, 150, 201):
            st, msg = status(lambda: ctx.window_dists(g, 1, [0, 2, 2], [5, s, 1]))
            assert st == _lib.KGMA_E_BADBASE and "record 2 position 201" in msg
        assert isinstance(pytest.raises(KeyError, lambda: ctx.window_dists(g, 1, [2], [150])).value, _lib.BadBaseError)
        # outside every requested window it is no error
        D, _ = ctx.window_dists(g, 1, [2, 2, 0], [101, 202, 7])
        assert D.tolist() == [cr.D(recs[2][100:200], S, N, k), cr.D(recs[2][201:301], S, N, k), cr.D(recs[0][6:106], S, N, k)]
        # k = 11: the references are kept sparse
        ctx.set_refs_sparse(11, [np.asarray([5, 77, 4000000])], [np.asarray([1.0, 2.0, 1.0])], [W], [1.0], [1])
        st, msg = status(lambda: ctx.window_dists(g, 1, [0], [1]))
        assert st == _lib.KGMA_E_UNSUPPORTED and "k = 11" in msg
        # a strobemer context
        RV, Ws, _cons, (_S, Ns) = refprep.gen_ref_ws_cons_strobe(os.path.join(DATA, "Alp_V_ref.fasta"), 2, 3, 5, 5, return_int=True)
        ctx.set_strobe_ref(2, 3, 5, 5, RV, Ws, 30.0, Ns)
        assert status(lambda: ctx.window_dists(g, 1, [0], [1]))[0] == _lib.KGMA_E_STATE
        # and kgma_set_refs puts the context back in service
        ctx.set_refs(k, [S / float(N)], [W], [1.0], [N])
        D, _ = ctx.window_dists(g, 1, [0], [7])
        assert D.tolist() == [cr.D(recs[0][6:106], S, N, k)]
        g.free()
    finally:
        ctx.close()
