"""kgma_strobe_window_dists / kgma_strobe_mutation_dists on the device (strobe_calib_kernel) and their Python mirror.  Everything is
compared exactly -- integers ==, doubles bit for bit -- against the strobemer scan (an independent kernel: strobe_kernel's
first-window D and KGMA_F_RETURN_DISTS distances) and against the plain-Python model tests/strobe_calib_ref.py, whose cases
tests/test_strobe_calib_host.py holds to the oracle.  Inputs: tests/strobe_calib_cases.py."""
import os

import numpy as np
import pytest

from kmergma_amd import _lib, api, fasta, refprep
from tests import strobe_calib_cases as cc
from tests import strobe_calib_ref as scr
from tests import strobe_cases as sc
from tests import strobe_oracle as so
from tests.conftest import DATA
from tests.helpers import random_dna

pytestmark = pytest.mark.gpu

REF = os.path.join(DATA, "Alp_V_ref.fasta")
LOCI = os.path.join(DATA, "Loci.fasta")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def form(s, source="window"):
    return f"strobe_calib_kernel<{source},{s}>"


def set_ref(ctx, ref, thr=0.0):
    ctx.set_strobe_ref(*ref["cfg"], ref["RV"], ref["W"], thr, ref["N"])
    scale = ctx.kfv_scale(1)
    assert scale == 2.0 * ref["k"] * ref["N"] * ref["N"] == float(sc.scale_of(ref))     # the engine's scale, exactly
    return scale


def status(fn):
    with pytest.raises(_lib.KgmaError) as e:
        fn()
    return e.value.status, e.value.message


def check(ctx, g, seqs, ref, contig, start, want=None):
    """One call over the given windows: D against the host model (or `want`), dist == D / scale bit for bit."""
    scale = ctx.kfv_scale(1)
    D, dist = ctx.strobe_window_dists(g, contig, start)
    assert ctx.kernel_name() == form(ref["cfg"][0])
    if want is None:
        want = [scr.window_D(seqs[c], ref["S"], ref["N"], ref["cfg"], ref["W"], q) for c, q in zip(contig, start)]
    assert D.tolist() == want
    assert np.array_equal(dist, D.astype(np.float64) / scale)
    return D


# ---- 1. parity with the scan, an independent kernel -------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg,W", cc.parity_sets(), ids=lambda v: str(v))
def test_parity_with_the_scan(ctx, cfg, W):
    c = cc.parity_case(cfg, W)
    seqs, ref = c["seqs"], c["ref"]
    set_ref(ctx, ref)
    g = ctx.genome_from_host(seqs)
    try:
        ctx.strobe_scan(g, 50, _lib.F_RETURN_DISTS, None)
        assert ctx.kernel_name() == f"strobe_kernel<{cfg[0]}>"
        first, d = ctx.first_window(1).copy(), ctx.dists(1).copy()
        contig, start = cc.all_starts(seqs, W)                                    # EVERY valid start of every record
        assert len(start) == (1300 - W) + 1 + 1 and d.size == 1300 - W - 1
        D, dist = ctx.strobe_window_dists(g, contig, start)
        assert ctx.kernel_name() == form(cfg[0])
        st = ctx.stats()
        assert st["n_launches"] == 1 and st["scan_ms"] > 0
    finally:
        g.free()
    s = np.asarray(start)
    assert D[s == 1].tolist() == first.tolist()
    assert np.array_equal(dist[s > 1], d)                                         # step q - 1 <-> start q, bit for bit
    # the host model as ONE sweep of the reference's update per record: window_D would run window_counts_direct from the record's
    # start for each of the ~1250 starts (quadratic); test_strobe_calib_host.py holds the sweep to window_D, and the two lines
    # above hold every start to the scan kernel independently
    want = [x for seq in seqs for x in scr.all_window_D(seq, ref["S"], ref["N"], cfg, W)]
    assert D.tolist() == want
    assert np.array_equal(dist, D.astype(np.float64) / float(sc.scale_of(ref)))


# ---- 2. item counts around the kernel's strides -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n_items", cc.STRIDE_ITEMS)
def test_item_counts(ctx, n_items):
    c = cc.stride_case(n_items)
    set_ref(ctx, c["ref"])
    g = ctx.genome_from_host(c["seqs"])
    try:
        check(ctx, g, c["seqs"], c["ref"], c["contig"], c["start"])
    finally:
        g.free()


# ---- 3. the 32-bit / 64-bit edge ----------------------------------------------------------------------------------------------------

def test_one_bin_of_65535(ctx):
    c = cc.onebin_case()
    ref = c["ref"]
    set_ref(ctx, ref)
    g = ctx.genome_from_host(c["seqs"])
    try:
        n = cc.ONEBIN_ITEMS
        want = sum(int(x) ** 2 for x in ref["S"]) - 31 * 31 + (31 - ref["N"] * n) ** 2
        check(ctx, g, c["seqs"], ref, c["contig"], c["start"], want=[want] * 3)
    finally:
        g.free()


def test_largest_N_and_largest_entry(ctx):
    cfg = cc.STRIDE_CFG
    c = sc.top_cell(cfg, sc.top_edge_N(cfg)[0])
    seq = c["seqs"][0]
    L, W = len(seq), c["W"]
    set_ref(ctx, c["ref"])
    g = ctx.genome_from_host(c["seqs"])
    try:
        start = [1, 2, 3, c["at"] - 1, c["at"], c["at"] + 1, c["at"] + 2, c["at"] + 200, L - W]
        want = [c["first_D"][0] if q == 1 else int(c["D"][q - 2]) for q in start]
        D = check(ctx, g, c["seqs"], c["ref"], [0] * len(start), start, want=want)
        assert int(D[0]) == c["dmax"] > 0.999 * 2 ** 61
    finally:
        g.free()
    e = sc.entry_cell()
    set_ref(ctx, e["ref"])
    g = ctx.genome_from_host(e["seqs"])
    try:
        assert len(e["seqs"][3]) < e["W"]
        contig, start = cc.all_starts(e["seqs"], e["W"])
        want = [x for seq in e["seqs"] if len(seq) >= e["W"] for x in scr.all_window_D(seq, e["ref"]["S"], 1, e["cfg"], e["W"])]
        D = check(ctx, g, e["seqs"], e["ref"], contig, start, want=want)
        assert {e["one"], e["two"]} <= set(D.tolist()) and int(D.max()) <= e["dmax"]
    finally:
        g.free()


# ---- 4. list handling -----------------------------------------------------------------------------------------------------------------

def test_lists_records_and_strands(ctx):
    c = cc.list_case()
    seqs, ref, W = c["seqs"], c["ref"], c["W"]
    set_ref(ctx, ref)
    g = ctx.genome_from_host(seqs)
    try:
        L = [len(x) for x in seqs]
        # unsorted, with duplicates, in every record (the permanent item is the window's own record's)
        contig = [2, 0, 1, 1, 2, 0, 0, 1, 2, 2]
        start = [L[2] - W, 700, 1, 100, 1, 1, 700, L[1] - W, 2, L[2] - W]
        D = check(ctx, g, seqs, ref, contig, start)
        assert D[0] == D[9] and D[1] == D[6]
        # lower case and runs of N (as T), window by window through them
        check(ctx, g, seqs, ref, [0] * 560, list(range(1, 561)), want=scr.all_window_D(seqs[0], ref["S"], ref["N"], ref["cfg"], W)[:560])
        check(ctx, g, seqs, ref, [1], [33])                                       # n = 1
        D0, d0 = ctx.strobe_window_dists(g, [], [])                               # n = 0
        assert D0.size == 0 and d0.size == 0 and ctx.stats()["n_launches"] == 0
        # the minus strand: a reverse-complement genome in its own coordinates
        rc = g.revcomp()
        try:
            comp = bytes.maketrans(b"ACGTNacgtn", b"TGCANtgcan")
            rseqs = [x.translate(comp)[::-1] for x in seqs]
            check(ctx, rc, rseqs, ref, [0, 0, 1, 2, 2], [1, 377, 5, 2, L[2] - W])
        finally:
            rc.free()
    finally:
        g.free()


# ---- 5. errors, as return codes ----------------------------------------------------------------------------------------------------------

def test_errors(alp_ref):
    ctx = _lib.Context(0)
    try:
        c = cc.bad_case()
        seqs, ref, W = c["seqs"], c["ref"], c["W"]
        g = ctx.genome_from_host(seqs)
        # before kgma_set_strobe_ref, and after kgma_set_refs
        assert status(lambda: ctx.strobe_window_dists(g, [0], [1]))[0] == _lib.KGMA_E_STATE
        assert status(lambda: ctx.strobe_mutation_dists([b"ACGTACGTAC"], [0.1], 1, 1))[0] == _lib.KGMA_E_STATE
        ctx.set_refs(6, [alp_ref["RV"]], [alp_ref["ws"]], [30.0], [alp_ref["N"]])
        assert status(lambda: ctx.strobe_window_dists(g, [0], [1]))[0] == _lib.KGMA_E_STATE
        assert status(lambda: ctx.strobe_mutation_dists([b"ACGTACGTAC"], [0.1], 1, 1))[0] == _lib.KGMA_E_STATE
        set_ref(ctx, ref)
        L = len(seqs[0])
        for cq, what in (((0, 0), "start 0"), ((0, L - W + 1), "start L - W + 1"), ((0, -3), "negative"), ((2, 1), "shorter than W"),
                         ((4, 1), "no record"), ((-1, 1), "no record")):
            st, msg = status(lambda: ctx.strobe_window_dists(g, [0, cq[0]], [L - W, cq[1]]))
            assert st == _lib.KGMA_E_ARG and "window 1" in msg, what
        L0 = _lib.load()
        import ctypes as C
        one_c, one_s = (C.c_int32 * 1)(0), (C.c_int64 * 1)(1)
        assert L0.kgma_strobe_window_dists(ctx._h, g._h, 1, None, one_s, None, None) == _lib.KGMA_E_ARG
        assert L0.kgma_strobe_window_dists(ctx._h, g._h, 1, one_c, None, None, None) == _lib.KGMA_E_ARG
        assert L0.kgma_strobe_window_dists(ctx._h, None, 1, one_c, one_s, None, None) == _lib.KGMA_E_ARG
        assert L0.kgma_strobe_window_dists(ctx._h, g._h, -1, one_c, one_s, None, None) == _lib.KGMA_E_ARG
        # either output may be NULL
        assert L0.kgma_strobe_window_dists(ctx._h, g._h, 1, one_c, one_s, None, None) == 0
        Dn = (C.c_int64 * 1)(0)
        assert L0.kgma_strobe_window_dists(ctx._h, g._h, 1, one_c, one_s, Dn, None) == 0
        assert Dn[0] == scr.window_D(seqs[0], ref["S"], ref["N"], ref["cfg"], W, 1)
        # a bad residue inside the window (record 1, residue 41): the first window, and a later one that covers it
        for q in (1, 2, 41):
            st, msg = status(lambda: ctx.strobe_window_dists(g, [0, 1], [5, q]))
            assert st == _lib.KGMA_E_BADBASE and "record 1 position 41" in msg
        # ... and inside the permanent item only: the window's own residues q .. q + W - 1 are clean
        for q in (42, 100, len(seqs[1]) - W):
            st, msg = status(lambda: ctx.strobe_window_dists(g, [1, 0], [q, 5]))
            assert st == _lib.KGMA_E_BADBASE and "record 1 position 41" in msg
        assert isinstance(pytest.raises(KeyError, lambda: ctx.strobe_window_dists(g, [1], [100])).value, _lib.BadBaseError)
        # a bad residue outside every requested window (record 3, residue 201) is no error
        clean = bytearray(seqs[3])
        clean[200] = ord("A")
        starts = [60, 154, 202, 254]
        D, _ = ctx.strobe_window_dists(g, [3] * 4 + [0], starts + [7])
        assert D.tolist() == [scr.window_D(bytes(clean), ref["S"], ref["N"], ref["cfg"], W, q) for q in starts] + [
            scr.window_D(seqs[0], ref["S"], ref["N"], ref["cfg"], W, 7)]
        g.free()
    finally:
        ctx.close()


# ---- 6. the mutation form -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", cc.MUT_SETS, ids=lambda v: str(v))
def test_mutation_dists(ctx, cfg):
    c = cc.mutation_case(cfg)
    ref, seqs = c["ref"], c["seqs"]
    S, N = ref["S"], ref["N"]
    scale = set_ref(ctx, ref)
    rates, nt, seed = list(cc.MUT_RATES), cc.MUT_TRIALS, cc.MUT_SEED
    D, dist = ctx.strobe_mutation_dists(seqs, rates, nt, seed)
    assert ctx.kernel_name() == form(cfg[0], "mutation")
    st = ctx.stats()
    assert st["n_launches"] == 1 and st["scan_ms"] > 0
    assert D.shape == dist.shape == (2, 4, 3)
    want = [[[scr.mutation_D(seq, S, N, cfg, rate, seed, (i, r, t)) for t in range(nt)] for r, rate in enumerate(rates)]
            for i, seq in enumerate(seqs)]
    assert D.tolist() == want
    assert np.array_equal(dist, D.astype(np.float64) / scale)
    for i, seq in enumerate(seqs):                                                # rate 0: the unmutated sequence
        assert set(D[i, 0].tolist()) == {scr.D_of_counts(S, N, so.strobe_count(seq, *cfg))}
    # nothing depends on the sequences or trials that follow
    D1, _ = ctx.strobe_mutation_dists(seqs[:1], rates, 1, seed)
    assert np.array_equal(D1[0, :, 0], D[0, :, 0])
    # shorter than k: sum S^2; lengths k and k + 1
    Ds, _ = ctx.strobe_mutation_dists(c["short"], [0.0, 0.5], 2, 7)
    wants = [[[scr.mutation_D(seq, S, N, cfg, rate, 7, (i, r, t)) for t in range(2)] for r, rate in enumerate([0.0, 0.5])]
             for i, seq in enumerate(c["short"])]
    assert Ds.tolist() == wants
    assert set(Ds[0].ravel().tolist()) == {sum(int(x) ** 2 for x in S)}
    Dz, dz = ctx.strobe_mutation_dists([], rates, nt, seed)                       # no sequences
    assert Dz.size == 0 and dz.size == 0 and ctx.stats()["n_launches"] == 0


def test_mutation_errors(ctx):
    c = cc.mutation_case((2, 3, 5, 5))
    set_ref(ctx, c["ref"])
    st, msg = status(lambda: ctx.strobe_mutation_dists([c["seqs"][1], b"ACGTACGNACGT"], [0.1], 1, 1))
    assert st == _lib.KGMA_E_BADBASE and "sequence 1 position 8" in msg
    assert status(lambda: ctx.strobe_mutation_dists(c["seqs"], [0.1, 1.5], 1, 1))[0] == _lib.KGMA_E_ARG
    assert status(lambda: ctx.strobe_mutation_dists(c["seqs"], [0.1], 0, 1))[0] == _lib.KGMA_E_ARG
    assert status(lambda: ctx.strobe_mutation_dists(c["seqs"], [], 1, 1))[0] == _lib.KGMA_E_ARG


# ---- 7. nothing else is disturbed ---------------------------------------------------------------------------------------------------------

def test_scan_results_survive(ctx):
    RV, W, _cons, (S, N) = refprep.gen_ref_ws_cons_strobe(REF, 2, 3, 5, 5, return_int=True)
    seqs = [r.sequence for r in fasta.read_fasta(LOCI)]
    ctx.set_strobe_ref(2, 3, 5, 5, RV, W, 30.0, N)
    g = ctx.genome_from_host(seqs)
    try:
        ctx.strobe_scan(g, 50, _lib.F_RETURN_DISTS, None)
        hits, dips, d, st0 = ctx.hits(), ctx.dips(), ctx.dists(1).copy(), ctx.stats()
        assert len(hits) >= 1
        ctx.strobe_window_dists(g, [0, 1, 3], [1, 100, 5])
        assert ctx.kernel_name() == form(2)
        st1 = ctx.stats()
        ctx.strobe_mutation_dists([random_dna(np.random.default_rng(7), 400)], [0.0, 0.1], 2, 3)
        assert ctx.kernel_name() == form(2, "mutation")
        st2 = ctx.stats()
        assert ctx.hits() == hits and ctx.dips() == dips
        assert np.array_equal(ctx.dists(1), d)
        for st in (st1, st2):
            assert {f for f in st0 if st0[f] != st[f]} <= {"scan_ms", "n_launches"}
            assert st["n_launches"] == 1
        # the reference and the threshold: the same scan gives the same hits
        ctx.strobe_scan(g, 50, 0, None)
        assert ctx.hits() == hits
    finally:
        g.free()


# ---- 8. end to end on the committed fixtures ----------------------------------------------------------------------------------------------

def test_hits_of_findgenes(ctx):
    RV, W, _cons, (S, N) = refprep.gen_ref_ws_cons_strobe(REF, 2, 3, 5, 5, return_int=True)
    for thr in (20.0, 30.0, 40.0):                                               # the thresholds of tests/test_gpu_strobe.py
        api.Strobemer_findGenes(genome_path=LOCI, ref_path=REF, KmerDistThr=thr, do_align=False, verbose=False, ctx=ctx,
                                float_chain=False)
        hits = ctx.hits()
        assert len(hits) >= 1
        contig = [h["contig"] for h in hits]
        start = [h["cmi"] for h in hits]
        D, dist = api.strobe_window_dists(LOCI, RV, W, contig, start, s=2, w_min=3, w_max=5, q=5, n_refs=N, ctx=ctx)
        assert D.tolist() == [h["D"] for h in hits]
        assert dist.tolist() == [h["dist"] for h in hits]


def test_estimated_threshold_is_off_the_lattice(ctx):
    RV, W, _cons, (S, N) = refprep.gen_ref_ws_cons_strobe(REF, 2, 3, 5, 5, return_int=True)
    kw = dict(s=2, w_min=3, w_max=5, q=5, n_refs=N, ctx=ctx)
    seqs = [r.sequence for r in fasta.read_fasta(LOCI)]
    lens = [len(x) for x in seqs]
    scale = 2 * 6 * N * N
    for quantile in (0.001, 0.5):
        thr = api.estimate_strobe_threshold_from_genome(LOCI, RV, W, n_samples=5000, seed=3, quantile=quantile, **kw)
        # the documented rule, from the same windows
        c, s = api.sample_window_starts(lens, W + 1, 5000, 3)
        _D, d = api.strobe_window_dists(LOCI, RV, W, c, s, **kw)
        est = float(np.sort(d)[int(np.ceil(quantile * d.size)) - 1])
        assert thr == api.off_lattice_threshold(est, float(scale))
        assert thr * scale != int(thr * scale) and abs(thr * scale - np.floor(thr * scale) - 0.5) < 1e-6      # not on the lattice
        ctx.set_strobe_ref(2, 3, 5, 5, RV, W, thr, N)
        g = ctx.genome_from_host(seqs)
        try:
            ctx.strobe_scan(g, 50, 0, None)
            assert ctx.stats()["n_at_threshold"] == 0
            if quantile == 0.5:
                assert len(ctx.dips()) > 0
        finally:
            g.free()
    mean = api.estimate_strobe_threshold_from_genome(LOCI, RV, W, n_samples=5000, seed=3, **kw)
    raw = api.estimate_strobe_threshold_from_genome(LOCI, RV, W, n_samples=5000, seed=3, off_lattice=False, buffer=2.5, **kw)
    assert abs(mean - 2.5 - raw) <= 1.0 / scale


def test_strobe_2_mer_dists_of_the_reference(ctx):
    out = api.test_strobe_2_mer_dists(REF, 5, ctx=ctx)
    assert out.shape == (81, 5)
    assert np.all(out[0] == 0.0)                                                  # rate 0: the record's distance to itself
    assert np.all(out[80] > 0.0)                                                  # rate 1: every residue substituted
    rec = fasta.read_fasta(REF)[0].sequence
    RKV = refprep.ungapped_strobe_2_mer_count(rec, 2, 3, 5, 5).astype(np.int64)
    for r, t in ((1, 0), (40, 3), (80, 4)):
        want = scr.mutation_D(rec, RKV, 1, (2, 3, 5, 5), float(np.arange(0, 1 + 1e-9, 0.0125)[r]), 42, (0, r, t))
        assert out[r, t] == want / (2.0 * 6)
