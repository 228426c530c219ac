"""kmat_norm_kernel / kmat_kernel / kmat_select_kernel (kgma_kmat.hip, through kgma_kmer_dist_matrix, kgma_kmer_nearest, their
_ranges forms and the screened assignment) against the model (tests/kmat_ref.py): D exactly, dist bit for bit, the nearest in
(D, index) order, and the screened assignment equal to tests/assign_ref.assign over the model's candidates.

Unless a test says otherwise both sources run: `seqs` uploads A, `ranges` reads it from a resident genome that holds the
sequences back to back in one record.  The case lists are tests/kmat_cases.py's (tests/test_kmat_host.py shows that they are not
vacuous and that the model agrees with the oracle)."""
import os

import numpy as np
import pytest

from kmergma_amd import _lib, api, fasta
from tests import assign_cases
from tests import assign_ref
from tests import kmat_cases as cases
from tests import kmat_ref as model
from tests.conftest import DATA

pytestmark = pytest.mark.gpu

FIELDS = ("ref", "score", "n_eq", "n_x", "n_ins", "n_del", "q_lo", "q_hi")
ALP = os.path.join(DATA, "Alp_V_ref.fasta")
LOCI = os.path.join(DATA, "Loci.fasta")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)          # no references are set on this context: the calls need none
    yield c
    c.close()


def pack(seqs, lead=b"N*", tail=b"?"):
    """One record holding the sequences back to back between bytes outside the alphabet, and their ranges on record 0."""
    rec = lead + b"".join(seqs) + tail
    pos = len(lead) + np.cumsum([0] + [len(s) for s in seqs])
    return rec, ([0] * len(seqs), [int(p) + 1 for p in pos[:-1]], [int(p) for p in pos[1:]])


def check_stats(ctx, k, n_pairs, nearest):
    st = ctx.kmat_stats()
    assert st["form"] == cases.form_of(k) and st["tile"] == cases.TILE[k], (k, st)      # the form the case means to test ran
    assert st["n_pairs"] == n_pairs and st["n_launches"] == (3 if nearest else 2) and st["kmat_ms"] > 0
    assert nearest or st["select_ms"] == 0
    return st


def check_matrix(ctx, k, A, B, want=None, sources=("seqs", "ranges")):
    want = model.D_matrix(A, B, k) if want is None else want
    want_dist = model.dist_matrix(want, k)
    g = None
    try:
        for src in sources:
            if src == "seqs":
                D, dist = ctx.kmer_dist_matrix(A, B, k)
            elif B is None:
                continue                                         # (the symmetric form is the sequence source's)
            else:
                rec, (c, lo, hi) = pack(A)
                g = ctx.genome_from_host([rec])
                D, dist = ctx.kmer_dist_matrix_ranges(g, c, lo, hi, B, k)
            assert D.dtype == np.int32 and D.shape == want.shape and dist.shape == want.shape
            bad = np.argwhere(D != want)
            assert bad.size == 0, (src, k, "D of (a, b)", bad[0].tolist(), int(D[tuple(bad[0])]), int(want[tuple(bad[0])]))
            assert np.array_equal(dist.view(np.uint64), want_dist.view(np.uint64)), (src, k)      # bit for bit
            check_stats(ctx, k, want.size, False)
    finally:
        if g is not None:
            g.free()
    return want


# ---- the matrix ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", cases.KS)
def test_lengths_around_k_and_the_lane_loop(ctx, k):
    _, A, B = cases.length_case(k)
    check_matrix(ctx, k, A, B)


@pytest.mark.parametrize("k", cases.TILE_KS)
def test_tiles_and_chunks(ctx, k):
    """n_b = 1, T - 1, T, T + 1, 2 T + 1 against 70 rows in two chunks; fewer columns of B are the model's leading columns."""
    _, A, B = cases.tile_case(k)
    want = model.D_matrix(A, B, k)
    for nb in cases.tile_widths(k):
        check_matrix(ctx, k, A, B[:nb], want[:, :nb], sources=("seqs",) if nb not in (1, len(B)) else ("seqs", "ranges"))
        assert ctx.kmat_stats()["chunks"] == 2


@pytest.mark.parametrize("n", range(len(cases.long_cases())))
def test_a_sequence_of_32767_residues(ctx, n):
    check_matrix(ctx, *cases.long_cases()[n])


@pytest.mark.parametrize("n", range(len(cases.counter_cases())))
def test_counter_edges(ctx, n):
    k, A, B = cases.counter_cases()[n]
    want = check_matrix(ctx, k, A, B, sources=("seqs",) if n else ("seqs", "ranges"))
    if n == 0:
        assert int(want[0, 1]) == cases.D_MAX


@pytest.mark.parametrize("n", range(len(cases.alphabet_cases())))
def test_lower_case_and_n(ctx, n):
    k, A, B = cases.alphabet_cases()[n]
    want = check_matrix(ctx, k, A, B)
    assert int(want[4, 1]) == 0 and int(want[5, 3]) == 0         # N only against T only


def test_symmetric_mode(ctx):
    """b = None equals the explicit A-against-A matrix, is symmetric and has a zero diagonal."""
    for k in (4, 6, 9):
        _, A, _B = cases.length_case(k)
        D, dist = ctx.kmer_dist_matrix(A, None, k)
        D2, dist2 = ctx.kmer_dist_matrix(A, A, k)
        assert np.array_equal(D, D2) and np.array_equal(dist, dist2) and np.array_equal(D, D.T) and not np.diag(D).any()
        assert np.array_equal(D, model.D_matrix(A, None, k))


# ---- bad residues -------------------------------------------------------------------------------------------------------
def test_bad_residues_name_the_side_the_sequence_and_the_position(ctx):
    for k, A, B, words in cases.bad_cases():
        with pytest.raises(_lib.BadBaseError) as ei:
            ctx.kmer_dist_matrix(A, B, k)
        assert all(w in ei.value.message for w in words), (k, words, ei.value.message)
        assert ctx.kmat_stats()["n_launches"] == 0 and ctx.kmat_stats()["kmat_ms"] == 0
        with pytest.raises(_lib.BadBaseError):
            ctx.kmer_nearest(A, A if B is None else B, k, 1)
    check_matrix(ctx, 6, [b"ACGTACGTAC"], [b"ACGTACGTAA"], sources=("seqs",))


def test_ranges_at_record_edges_and_a_bad_residue_outside_them(ctx):
    recs, ranges, B, bad = cases.record_case()
    c, lo, hi = ([r[i] for r in ranges] for i in range(3))
    g = ctx.genome_from_host(recs)
    try:
        for k in (3, 6, 8):
            want = model.D_matrix(cases.ranges_text(recs, ranges), B, k)
            D, dist = ctx.kmer_dist_matrix_ranges(g, c, lo, hi, B, k)
            assert np.array_equal(D, want) and np.array_equal(dist, model.dist_matrix(want, k))
            idx, Dn = ctx.kmer_nearest_ranges(g, c, lo, hi, B, k, 3)
            widx, wDn = model.nearest(want, 3)
            assert np.array_equal(idx, widx) and np.array_equal(Dn, wDn)
            with pytest.raises(_lib.BadBaseError) as ei:
                ctx.kmer_dist_matrix_ranges(g, c + [bad[0]], lo + [bad[1]], hi + [bad[2]], B, k)
            assert f"range {len(ranges)}" in ei.value.message and "record 2 position 5" in ei.value.message
    finally:
        g.free()
    clean = [r.replace(b"*", b"A") for r in recs]
    g = ctx.genome_from_host(clean)
    try:
        rc = g.revcomp()
        try:
            want = model.D_matrix(cases.ranges_text(clean, ranges, revcomp=True), B, 6)
            assert not np.array_equal(want, model.D_matrix(cases.ranges_text(clean, ranges), B, 6))
            D, _ = ctx.kmer_dist_matrix_ranges(rc, c, lo, hi, B, 6)
            assert np.array_equal(D, want)
        finally:
            rc.free()
    finally:
        g.free()


# ---- nearest ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(len(cases.nearest_cases())))
def test_nearest_equals_the_model(ctx, n):
    k, A, B, n_nears = cases.nearest_cases()[n]
    D = model.D_matrix(A, B, k)
    rec, (c, lo, hi) = pack(A)
    g = ctx.genome_from_host([rec])
    try:
        for nn in n_nears:
            widx, wD = model.nearest(D, nn)
            for src in ("seqs", "ranges"):
                idx, Dn = ctx.kmer_nearest(A, B, k, nn) if src == "seqs" else ctx.kmer_nearest_ranges(g, c, lo, hi, B, k, nn)
                assert idx.dtype == np.int32 and np.array_equal(idx, widx) and np.array_equal(Dn, wD), (src, k, nn)
                check_stats(ctx, k, D.size, True)
    finally:
        g.free()


# ---- the screened assignment ----------------------------------------------------------------------------------------------
def rows(out):
    return [[assign_ref.Want(*(int(a[f]) for f in FIELDS)) for a in row] for row in out]


def test_screened_assignment_equals_the_model_under_every_gap_model(ctx):
    refs, queries = cases.small_screen_case()
    rec, (c, lo, hi) = pack(queries, lead=b"NN", tail=b"n")
    g = ctx.genome_from_host([rec])
    try:
        for go, ge in assign_cases.GAPS:
            for k, nn, top in ((6, 4, 2), (3, 9, 9), (8, 1, 1)):
                want, wcand, wscores = model.screened_assign(refs, queries, go, ge, top, k, nn)
                for src in ("seqs", "ranges"):
                    if src == "seqs":
                        out, cand, scores = ctx.assign_seqs_screened(refs, queries, go, ge, top, k, nn)
                    else:
                        out, cand, scores = ctx.assign_ranges_screened(g, refs, c, lo, hi, go, ge, top, k, nn)
                    assert np.array_equal(cand, wcand) and np.array_equal(scores, wscores), (src, go, ge, k, nn)
                    assert rows(out) == want, (src, go, ge, k, nn)
                    st = ctx.assign_stats()
                    assert st["n_pairs"] == len(queries) * nn and st["n_traced"] == len(queries) * top
                    assert st["n_cells"] == sum(len(q) * len(refs[int(r)]) for q, row in zip(queries, wcand) for r in row)
                    check_stats(ctx, k, len(queries) * len(refs), True)
    finally:
        g.free()


@pytest.mark.parametrize("n_refs", [40, 84])
def test_screened_with_every_reference_is_the_unscreened_call(ctx, n_refs):
    genes = [r.sequence for r in fasta.read_fasta(ALP)]
    _, queries = cases.fixture_queries(genes)
    refs = genes[:n_refs]
    rec, (c, lo, hi) = pack(queries, lead=b"NN", tail=b"n")
    g = ctx.genome_from_host([rec])
    try:
        for top in (1, 3):
            plain, S = ctx.assign_seqs(refs, queries, -69, -1, top)
            out, cand, scores = ctx.assign_seqs_screened(refs, queries, -69, -1, top, 6, n_refs)
            assert np.array_equal(out, plain)
            assert np.array_equal(np.sort(cand, axis=1), np.tile(np.arange(n_refs), (len(queries), 1)))
            assert np.array_equal(scores, np.take_along_axis(S, cand.astype(np.int64), axis=1))
            out_r, _, _ = ctx.assign_ranges_screened(g, refs, c, lo, hi, -69, -1, top, 6, n_refs)
            assert np.array_equal(out_r, ctx.assign_ranges(g, refs, c, lo, hi, -69, -1, top)[0]) and np.array_equal(out_r, plain)
    finally:
        g.free()


def test_prescreen_of_eight_names_the_same_best_reference_on_the_fixture_queries(ctx):
    refs = fasta.read_fasta(ALP)
    _, queries = cases.fixture_queries([r.sequence for r in refs])
    full = api.assignGenes(queries, refs, ctx=ctx)
    fast = api.assignGenes(queries, refs, prescreen=8, ctx=ctx)
    assert [a[0] for a in fast] == [a[0] for a in full]
    assert ctx.kmat_stats()["n_pairs"] == len(queries) * 84 and ctx.assign_stats()["n_pairs"] == len(queries) * 8
    near = api.nearest_refs(queries, refs, k=6, n=8, ctx=ctx)
    assert all(f[0].ref_index in [r[1] for r in row] for f, row in zip(full, near))
    widx, wD = model.nearest(model.D_matrix(queries, [r.sequence for r in refs], 6), 8)
    assert [[r[1] for r in row] for row in near] == widx.tolist()
    assert [[r[2] for r in row] for row in near] == ((1.0 / 12) * wD.astype(np.float64)).tolist()
    assert all(row[0][0] == refs[row[0][1]].description.split()[0] for row in near)
    d = api.kmer_dist_matrix(queries, ALP, 6, ctx=ctx)
    assert np.array_equal(d, model.dist_matrix(model.D_matrix(queries, [r.sequence for r in refs], 6), 6))


@pytest.mark.parametrize("strand,n_hits", [("+", 7), ("both", 10)])
def test_find_then_assign_with_a_prescreen_of_all(strand, n_hits):
    ctx = api.default_context()
    hits = api.findGenes(genome_path=LOCI, ref_path=ALP, k=6, KmerDistThr=30.0, verbose=False, ctx=ctx, strand=strand)[0]
    assert len(hits) == n_hits
    plain = api.assignGenes(hits, ALP, annotate=True, ctx=ctx)
    noted = api.assignGenes(hits, ALP, prescreen=84, annotate=True, ctx=ctx)
    assert [r.description for r in noted] == [r.description for r in plain] and all(" | Ref = " in r.description for r in noted)
    assert [r.sequence for r in noted] == [h.sequence for h in hits]
    if strand == "+":
        g = ctx.genome_from_path(LOCI)
        try:
            ids = [g.header(c).split()[0] for c in range(g.n_contigs)]
            where = [(ids.index(h.description.split(" | ")[0]),) + tuple(int(x) for x in h.description.split("MatchPos = ")[1].split(" | ")[0].split(":"))
                     for h in hits]
            cl = [[w[i] for w in where] for i in range(3)]
            assert api.assign_ranges(g, *cl, ALP, top=2, prescreen=84, ctx=ctx) == api.assign_ranges(g, *cl, ALP, top=2, ctx=ctx)
            d = api.kmer_dist_matrix_ranges(g, *cl, ALP, 6, integer=True, ctx=ctx)
            assert np.array_equal(d, model.D_matrix([h.sequence for h in hits], [r.sequence for r in fasta.read_fasta(ALP)], 6))
        finally:
            g.free()


# ---- errors -------------------------------------------------------------------------------------------------------------
def test_argument_errors_and_limits(ctx):
    L, C = _lib.load(), _lib.C
    A, B = [b"ACGTACGTTT", b"ACG", b""], [b"ACGTACGTAA", b"TTTTTTTTT"]
    rec, (c, lo, hi) = pack(A)
    g = ctx.genome_from_host([rec, b"ACGT" * 8200])
    scan = _lib.Context(0)                      # an earlier scan's hits stay retrievable on a context that serves these calls
    ARG, UNS = _lib.KGMA_E_ARG, _lib.KGMA_E_UNSUPPORTED

    def fine(on=ctx):
        D, _ = on.kmer_dist_matrix(A, B, 6)
        assert np.array_equal(D, model.D_matrix(A, B, 6)) and on.kmat_stats()["n_pairs"] == 6

    def raises(status, needle, fn, *args):
        fine()
        with pytest.raises(_lib.KgmaError) as ei:
            fn(*args)
        assert ei.value.status == status and needle in ei.value.message, (status, needle, ei.value)
        st = ctx.kmat_stats()                    # zeroed by the failed call
        assert st["n_pairs"] == 0 and st["n_launches"] == 0 and st["kmat_ms"] == 0 and st["select_ms"] == 0
        fine()                                   # after every error a valid call on the same context succeeds

    try:
        assert ctx.kmat_stats()["n_pairs"] >= 0
        assert ctx.kmer_dist_matrix([], B, 6)[0].shape == (0, 2) and ctx.kmat_stats()["n_launches"] == 0       # n_a == 0 is no error
        assert ctx.kmer_nearest_ranges(g, [], [], [], B, 6, 2)[0].shape == (0, 2)
        assert ctx.kmer_dist_matrix([], None, 6)[0].shape == (0, 0)
        raises(ARG, "n_b = 0", ctx.kmer_dist_matrix, A, [], 6)
        raises(ARG, "k = 0", ctx.kmer_dist_matrix, A, B, 0)
        raises(UNS, "k = 11", ctx.kmer_dist_matrix, A, B, 11)
        raises(UNS, "k = 11", ctx.kmer_nearest, A, B, 11, 1)
        raises(ARG, "n_near = 0", ctx.kmer_nearest, A, B, 6, 0)
        raises(ARG, "n_near = 3", ctx.kmer_nearest, A, B, 6, 3)
        raises(ARG, "n_near = 129", ctx.kmer_nearest, A, [b"ACGT"] * 200, 6, 129)
        raises(ARG, "n_near = 3", ctx.kmer_nearest_ranges, g, c, lo, hi, B, 6, 3)
        raises(ARG, "no record 2", ctx.kmer_dist_matrix_ranges, g, [0, 2], [1, 1], [4, 4], B, 6)
        raises(ARG, "no record -1", ctx.kmer_dist_matrix_ranges, g, [-1], [1], [4], B, 6)
        raises(ARG, "outside record 0", ctx.kmer_dist_matrix_ranges, g, [0], [0], [4], B, 6)
        raises(ARG, "outside record 0", ctx.kmer_dist_matrix_ranges, g, [0], [3], [len(rec) + 1], B, 6)
        raises(ARG, "outside record 0", ctx.kmer_dist_matrix_ranges, g, [0], [9], [7], B, 6)
        raises(UNS, "A sequence 1 has 32768", ctx.kmer_dist_matrix, [b"ACGT", b"A" * 32768], B, 6)
        raises(UNS, "B sequence 0 has 32768", ctx.kmer_dist_matrix, A, [b"C" * 32768], 6)
        raises(UNS, "range 0 has 32768", ctx.kmer_dist_matrix_ranges, g, [1], [2], [32769], B, 6)
        D, _ = ctx.kmer_dist_matrix_ranges(g, [1], [2], [32768], [b"CGTA" * 8191 + b"CGT"], 6)                    # 32767 residues are served
        assert D.tolist() == [[0]]
        # the screened assignment's own limits
        refs, queries = [b"ACGTACGT", b"ACGAACGT", b"TTTTACGT"], [b"TTACGTACGTAA", b"ACGT"]
        raises(ARG, "n_near = 4", ctx.assign_seqs_screened, refs, queries, -69, -1, 1, 6, 4)
        raises(ARG, "n_near = 0", ctx.assign_seqs_screened, refs, queries, -69, -1, 1, 6, 0)
        raises(ARG, "top = 3 exceeds n_near = 2", ctx.assign_seqs_screened, refs, queries, -69, -1, 3, 6, 2)
        raises(ARG, "top = 3 exceeds n_near = 2", ctx.assign_ranges_screened, g, refs, [0], [3], [9], -69, -1, 3, 6, 2)
        raises(ARG, "screen_k = 0", ctx.assign_seqs_screened, refs, queries, -69, -1, 1, 0, 2)
        raises(UNS, "screen_k = 11", ctx.assign_seqs_screened, refs, queries, -69, -1, 1, 11, 2)
        raises(ARG, "query 1 is empty", ctx.assign_seqs_screened, refs, [b"ACGT", b""], -69, -1, 1, 6, 2)
        raises(UNS, "query 0 has 8192", ctx.assign_ranges_screened, g, refs, [1], [2], [8193], -69, -1, 1, 6, 2)
        with pytest.raises(_lib.BadBaseError) as ei:                                   # the unscreened call counts such a byte as N
            ctx.assign_seqs_screened(refs, [b"ACGT", b"AC-GT"], -69, -1, 1, 6, 2)
        assert "query 1 position 3" in ei.value.message and ctx.assign_seqs(refs, [b"ACGT", b"AC-GT"], -69, -1, 1)[0].shape == (2, 1)
        with pytest.raises(_lib.BadBaseError) as ei:
            ctx.assign_seqs_screened([b"ACGT", b"ACRT"], queries, -69, -1, 1, 6, 2)
        assert "reference 1 position 3" in ei.value.message and ctx.assign_stats()["n_pairs"] == 0
        assert ctx.assign_seqs_screened(refs, [], -69, -1, 1, 6, 2)[0].shape == (0, 1)
        # null pointers and decreasing offsets: only the C ABI can say those
        h = ctx._h
        at, bt = b"".join(A), b"".join(B)
        aoff, boff, dec = (C.c_int64 * 4)(0, 10, 13, 13), (C.c_int64 * 3)(0, 10, 19), (C.c_int64 * 3)(0, 10, 4)
        D = np.zeros(6, dtype=np.int32)
        Dp = _lib._np_ptr(D, C.c_int32)
        assert L.kgma_kmer_dist_matrix(h, 6, None, aoff, 3, bt, boff, 2, Dp, None) == ARG
        assert L.kgma_kmer_dist_matrix(h, 6, at, None, 3, bt, boff, 2, Dp, None) == ARG
        assert L.kgma_kmer_dist_matrix(h, 6, at, aoff, 3, bt, None, 2, Dp, None) == ARG
        assert L.kgma_kmer_dist_matrix(h, 6, at, aoff, -1, bt, boff, 2, Dp, None) == ARG
        assert L.kgma_kmer_dist_matrix(h, 6, at, dec, 2, bt, boff, 2, Dp, None) == ARG and b"a_off[1] > a_off[2]" in L.kgma_last_error(h)
        assert L.kgma_kmer_dist_matrix(h, 6, at, aoff, 3, bt, dec, 2, Dp, None) == ARG and b"b_off[1] > b_off[2]" in L.kgma_last_error(h)
        assert L.kgma_kmer_dist_matrix_ranges(h, None, 6, 0, None, None, None, bt, boff, 2, None, None) == ARG
        assert L.kgma_kmer_dist_matrix_ranges(h, g._h, 6, 1, None, None, None, bt, boff, 2, Dp, None) == ARG
        assert L.kgma_kmer_dist_matrix_ranges(h, g._h, 6, 3, *(_lib._np_ptr(np.asarray(x, dtype=t), ct) for x, t, ct in
                                                              ((c, np.int32, C.c_int32), (lo, np.int64, C.c_int64), (hi, np.int64, C.c_int64))),
                                              None, boff, 2, Dp, None) == ARG
        # more than 2^30 pairs: refused before anything but the offsets is read
        big = np.zeros(32770, dtype=np.int64)
        bp = _lib._np_ptr(big, C.c_int64)
        assert L.kgma_kmer_dist_matrix(h, 6, b"", bp, 32769, b"", bp, 32768, None, None) == UNS and b"2^30 pairs" in L.kgma_last_error(h)
        assert L.kgma_kmer_dist_matrix(h, 6, b"", bp, 32769, None, None, 0, None, None) == UNS
        assert L.kgma_kmer_dist_matrix(h, 6, at, aoff, 3, bt, boff, 2, Dp, None) == 0 and D.tolist() == model.D_matrix(A, B, 6).ravel().tolist()
        assert L.kgma_kmer_dist_matrix(h, 6, at, aoff, 3, bt, boff, 2, None, None) == 0           # both outputs may be NULL
        # an earlier scan's hits survive the calls, failed ones included, and the context needs no references for them
        from kmergma_amd import refprep
        RV, W, _cons, (S, N) = refprep.gen_ref_ws_cons(ALP, 6, return_int=True)
        loci = scan.genome_from_path(LOCI)
        scan.set_refs(6, [RV], [W], [30.0], [N])
        scan.scan(loci, _lib.MODE_SINGLE, 50, 0, 0, None)
        before = scan.hits()
        assert len(before) > 0
        fine(scan)
        with pytest.raises(_lib.KgmaError):
            scan.kmer_dist_matrix(A, B, 11)
        assert scan.assign_seqs_screened(refs, queries, -69, -1, 1, 6, 2)[0].shape == (2, 1)
        assert scan.hits() == before
        loci.free()
    finally:
        g.free()
        scan.close()
