"""assign_score_kernel / assign_trace_kernel (kgma_assign.hip, through kgma_assign_seqs and kgma_assign_ranges) against the
assignment's model (tests/assign_ref.py): the whole score matrix equals align_ref.optimum pair by pair, the chosen references
follow (-score, index), and the counted columns are those of the host aligner's CIGAR, itself checked against the model.

Unless a test says otherwise both sources run: `seqs` uploads the queries, `ranges` reads them from a resident genome that holds
them back to back in one record.  The case lists are tests/assign_cases.py's (tests/test_assign_host.py shows they are not vacuous)."""
import os

import numpy as np
import pytest

from kmergma_amd import _lib, api, fasta
from tests import align_cases as ac
from tests import assign_cases as cases
from tests import assign_ref as model
from tests.conftest import DATA

pytestmark = pytest.mark.gpu

FIELDS = ("ref", "score", "n_eq", "n_x", "n_ins", "n_del", "q_lo", "q_hi")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)          # no references are set on this context: the assignment needs none
    yield c
    c.close()


def rows(out):
    return [[model.Want(*(int(a[f]) for f in FIELDS)) for a in row] for row in out]


def pack(queries, lead=b"NN", tail=b"n"):
    """One record holding the queries back to back, and their ranges on record 0."""
    rec = lead + b"".join(queries) + tail
    pos = len(lead) + np.cumsum([0] + [len(q) for q in queries])
    return rec, [(0, int(pos[k]) + 1, int(pos[k + 1])) for k in range(len(queries))]


def check(ctx, refs, queries, go, ge, tops, sources=("seqs", "ranges"), genome=None, ranges=None):
    """Every entry of the matrix and every assignment of every query, for every `top`, from every source."""
    want_S = model.score_matrix(refs, queries, go, ge)
    own = None
    if "ranges" in sources and genome is None:
        rec, ranges = pack(queries)
        own = genome = ctx.genome_from_host([rec])
    try:
        for top in tops:
            want = model.assign(refs, queries, go, ge, top, want_S)
            for src in sources:
                if src == "seqs":
                    out, S = ctx.assign_seqs(refs, queries, go, ge, top)
                else:
                    out, S = ctx.assign_ranges(genome, refs, [r[0] for r in ranges], [r[1] for r in ranges], [r[2] for r in ranges], go, ge, top)
                assert S.shape == want_S.shape and out.shape == (len(queries), top)
                bad = np.argwhere(S != want_S)
                assert bad.size == 0, (src, go, ge, "score of (query, ref)", bad[0].tolist(), int(S[tuple(bad[0])]), int(want_S[tuple(bad[0])]))
                got = rows(out)
                for k in range(len(queries)):
                    assert got[k] == want[k], (src, go, ge, top, "query", k, len(queries[k]), got[k], want[k])
                st = ctx.assign_stats()
                assert st["n_pairs"] == len(queries) * len(refs) and st["n_traced"] == len(queries) * top
                assert st["n_cells"] == sum(map(len, queries)) * sum(map(len, refs))
    finally:
        if own is not None:
            own.free()


# ---- strip and wave edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", cases.STRIP_M)
def test_strip_and_wave_edges(ctx, m):
    refs, queries = cases.strip_case(m)
    for go, ge in cases.GAPS:
        check(ctx, refs, queries, go, ge, (1, len(refs)))


# ---- ties -----------------------------------------------------------------------------------------------------------
def test_equal_scores_are_ordered_by_reference_index(ctx):
    refs, queries = cases.tie_case()
    for go, ge in ((-69, -1), (0, -1)):
        check(ctx, refs, queries, go, ge, (1, 2, 3))
        out, S = ctx.assign_seqs(refs, queries, go, ge, 3)
        assert (S[:, 1] == S[:, 3]).all() and (S[:, 1] == S[:, 4]).all()
        assert out["ref"][0].tolist() == [1, 3, 4] and out["ref"][1].tolist() == [1, 3, 4]


# ---- alphabet -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", range(len(cases.alphabet_cases())))
def test_alphabet_and_low_complexity(ctx, group):
    """Lower case, N, bytes outside the alphabet, homopolymers; the free-opening models (0, -1) and (0, -2), where nearly every
    cell is a tie, are among LOW_COMPLEXITY_GAPS.  top = all: every pair is traced and its counts equal the host CIGAR's."""
    refs, queries = cases.alphabet_cases()[group]
    assert (0, -1) in ac.LOW_COMPLEXITY_GAPS
    for go, ge in ac.LOW_COMPLEXITY_GAPS:
        check(ctx, refs, queries, go, ge, (len(refs),))


# ---- batch geometry ---------------------------------------------------------------------------------------------------
def test_one_query_one_reference(ctx):
    check(ctx, [b"ACGTTGCA"], [b"TTACGTAGCATT"], -69, -1, (1,))
    check(ctx, [b"A"], [b"C"], -5, -3, (1,))


def test_more_pairs_than_one_score_launch(ctx):
    """260 x 253 = 65780 pairs > KGMA_ASSIGN_PAIRS_PER_LAUNCH = 65536: the score pass takes two launches."""
    refs, queries = cases.chunked_case()
    check(ctx, refs, queries, -5, -3, (1,), sources=("seqs",))
    assert ctx.assign_stats()["n_score_launches"] == 2
    check(ctx, refs[:7], queries, -5, -3, (2,), sources=("ranges",))


def test_one_long_query_among_short_ones(ctx):
    """The 8191-residue query runs in its own length class; the 40 short ones, in two others, must still be right."""
    refs, queries = cases.long_query_case()
    check(ctx, refs, queries, -69, -1, (1, 2))
    assert ctx.assign_stats()["n_score_launches"] == 3 and ctx.assign_stats()["n_trace_launches"] == 3


def test_the_longest_reference(ctx):
    refs, queries = cases.long_ref_case()
    check(ctx, refs, queries, -69, -1, (2,))
    check(ctx, refs, queries, -69, -5, (1,), sources=("seqs",))


def test_two_geometries_on_one_context(ctx):
    """A call with long sequences, then 1 x 1, then the first again: nothing of one call's geometry survives into the next."""
    refs, queries = cases.long_query_case()
    one = ctx.assign_seqs(refs, queries, -69, -1, 2)
    check(ctx, [b"A"], [b"A"], -69, -1, (1,))
    two = ctx.assign_seqs(refs, queries, -69, -1, 2)
    assert (one[0] == two[0]).all() and (one[1] == two[1]).all()


# ---- ranges source ----------------------------------------------------------------------------------------------------
def test_ranges_at_record_edges_and_on_the_reverse_complement(ctx):
    refs, recs, ranges = cases.record_case()
    queries = [recs[c][lo - 1:hi] for c, lo, hi in ranges]
    g = ctx.genome_from_host(recs)
    try:
        for go, ge in ((-69, -1), (-5, -3)):
            check(ctx, refs, queries, go, ge, (1, 3), sources=("ranges",), genome=g, ranges=ranges)
        rc = g.revcomp()
        try:
            rc_queries = [fasta.reverse_complement(recs[c])[lo - 1:hi] for c, lo, hi in ranges]
            assert rc_queries != queries
            check(ctx, refs, rc_queries, -69, -1, (3,), sources=("ranges",), genome=rc, ranges=ranges)
        finally:
            rc.free()
    finally:
        g.free()


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_argument_errors_and_limits(ctx):
    L = _lib.load()
    C = _lib.C
    refs, queries = [b"ACGTACGT", b"ACGAACGT"], [b"TTACGTACGTAA", b"ACGT"]
    rec, ranges = pack(queries)
    g = ctx.genome_from_host([rec, b"ACGT" * 2100])

    def fine():
        check(ctx, refs, queries, -69, -1, (2,), genome=g, ranges=ranges)

    def raises(status, needle, fn, *args, **kw):
        with pytest.raises(_lib.KgmaError) as ei:
            fn(*args, **kw)
        assert ei.value.status == status and needle in ei.value.message, (status, needle, ei.value)
        fine()                                   # after every error a valid call on the same context succeeds

    ARG, UNS = _lib.KGMA_E_ARG, _lib.KGMA_E_UNSUPPORTED
    try:
        fine()
        assert ctx.assign_seqs(refs, [], -69, -1, 1)[0].shape == (0, 1)                  # n_queries == 0 is no error
        assert ctx.assign_ranges(g, refs, [], [], [], -69, -1, 2)[0].shape == (0, 2)
        raises(ARG, "n_refs", ctx.assign_seqs, [], queries, -69, -1, 1)
        raises(ARG, "top = 0", ctx.assign_seqs, refs, queries, -69, -1, 0)
        raises(ARG, "top = 3", ctx.assign_seqs, refs, queries, -69, -1, 3)
        raises(ARG, "top = 3", ctx.assign_ranges, g, refs, [0], [1], [4], -69, -1, 3)
        raises(ARG, "reference 1 is empty", ctx.assign_seqs, [b"ACGT", b""], queries, -69, -1, 1)
        raises(ARG, "query 1 is empty", ctx.assign_seqs, refs, [b"ACGT", b""], -69, -1, 1)
        raises(ARG, "query 0 is empty", ctx.assign_ranges, g, refs, [0], [5], [4], -69, -1, 1)
        raises(ARG, "no record 2", ctx.assign_ranges, g, refs, [0, 2], [1, 1], [4, 4], -69, -1, 1)
        raises(ARG, "no record -1", ctx.assign_ranges, g, refs, [-1], [1], [4], -69, -1, 1)
        raises(ARG, "outside record 0", ctx.assign_ranges, g, refs, [0], [0], [4], -69, -1, 1)
        raises(ARG, "outside record 0", ctx.assign_ranges, g, refs, [0], [3], [len(rec) + 1], -69, -1, 1)
        raises(ARG, "outside record 0", ctx.assign_ranges, g, refs, [0], [9], [4], -69, -1, 1)
        raises(ARG, "not positive", ctx.assign_seqs, refs, queries, 1, -1, 1)
        raises(ARG, "not positive", ctx.assign_seqs, refs, queries, -69, 1, 1)
        # limits: 8192 residues on either side, and gap scores that could reach the sentinel
        raises(UNS, "reference 1 has 8192", ctx.assign_seqs, [b"ACGT", b"A" * 8192], queries, -69, -1, 1)
        raises(UNS, "query 1 has 8192", ctx.assign_seqs, refs, [b"ACGT", b"C" * 8192], -69, -1, 1)
        raises(UNS, "query 0 has 8192", ctx.assign_ranges, g, refs, [1], [2], [8193], -69, -1, 1)
        raises(UNS, "reference 0 has 8192", ctx.assign_ranges, g, [b"G" * 8192, b"A"], [0], [1], [4], -69, -1, 1)
        raises(UNS, "2^27", ctx.assign_seqs, refs, queries, -(1 << 27) - 1, 0, 1)
        raises(UNS, "2^27", ctx.assign_seqs, refs, queries, 0, -(1 << 14) - 1, 1)
        check(ctx, refs, queries, -(1 << 27), 0, (2,), sources=("seqs",))                # the bound itself is served
        check(ctx, refs, queries, 0, -(1 << 14), (2,), sources=("seqs",))
        check(ctx, refs, [rec[1:], (b"ACGT" * 2100)[1:8192]], -69, -1, (1,), sources=("ranges",), genome=g,
              ranges=[(0, 2, len(rec)), (1, 2, 8192)])                                   # 8191 residues are served
        # null pointers and decreasing offsets: only the C ABI can say those
        off2 = (C.c_int64 * 3)(0, 8, 16)
        dec = (C.c_int64 * 3)(0, 8, 4)
        qoff = (C.c_int64 * 3)(0, 12, 16)
        out = np.zeros(4, dtype=_lib.ASSIGNMENT_DTYPE)
        rt, qt = b"".join(refs), b"".join(queries)
        h = ctx._h

        def status(*a):
            return L.kgma_assign_seqs(h, *a)

        assert status(None, off2, 2, qt, qoff, 2, -69, -1, 1, out.ctypes.data, None) == ARG
        assert status(rt, None, 2, qt, qoff, 2, -69, -1, 1, out.ctypes.data, None) == ARG
        assert status(rt, off2, 2, None, qoff, 2, -69, -1, 1, out.ctypes.data, None) == ARG
        assert status(rt, off2, 2, qt, None, 2, -69, -1, 1, out.ctypes.data, None) == ARG
        assert status(rt, off2, 2, qt, qoff, 2, -69, -1, 1, None, None) == ARG
        assert status(rt, dec, 2, qt, qoff, 2, -69, -1, 1, out.ctypes.data, None) == ARG
        assert b"ref_offsets[1] > ref_offsets[2]" in L.kgma_last_error(h)
        assert status(rt, off2, 2, qt, dec, 2, -69, -1, 1, out.ctypes.data, None) == ARG
        assert b"query_offsets[1] > query_offsets[2]" in L.kgma_last_error(h)
        # more than 2^30 pairs in one call: refused before anything is read beyond the reference offsets
        big = np.arange(32769, dtype=np.int64)
        assert status(b"A" * 32768, _lib._np_ptr(big, C.c_int64), 32768, qt, qoff, 32769, -69, -1, 1, out.ctypes.data, None) == UNS
        assert b"2^30 pairs" in L.kgma_last_error(h)
        assert L.kgma_assign_ranges(h, None, rt, off2, 2, 0, None, None, None, -69, -1, 1, None, None) == ARG
        assert L.kgma_assign_ranges(h, g._h, rt, off2, 2, 1, None, None, None, -69, -1, 1, out.ctypes.data, None) == ARG
        assert status(rt, off2, 2, qt, qoff, 2, -69, -1, 1, out.ctypes.data, None) == 0  # scores may be NULL
        assert out["ref"][:2].tolist() == [0, 0] and int(out["score"][0]) == 40
        fine()
    finally:
        g.free()


# ---- end to end -------------------------------------------------------------------------------------------------------
LOCI = os.path.join(DATA, "Loci.fasta")
ALP = os.path.join(DATA, "Alp_V_ref.fasta")


@pytest.mark.parametrize("strand,n_hits", [("+", 7), ("both", 10)])
def test_find_then_assign(tmp_path, strand, n_hits):
    """findGenes on the loci fixture, then assignGenes against the first 24 alpaca IGHV genes: every hit's three best references,
    their scores and column counts equal the model's; annotated records go through write_results and read back as written."""
    ctx = api.default_context()
    hits = api.findGenes(genome_path=LOCI, ref_path=ALP, k=6, KmerDistThr=30.0, verbose=False, ctx=ctx, strand=strand)[0]
    assert len(hits) == n_hits
    refs = fasta.read_fasta(ALP)[:24]
    got = api.assignGenes(hits, refs, top=3, ctx=ctx)
    seqs = [r.sequence for r in refs]
    want = model.assign(seqs, [h.sequence for h in hits], -69, -1, 3)
    assert len(got) == n_hits
    for g3, w3 in zip(got, want):
        assert [(a.ref_index, a.score, a.n_eq, a.n_x, a.n_ins, a.n_del, a.q_lo, a.q_hi) for a in g3] == [tuple(w) for w in w3]
        assert [a.ref_id for a in g3] == [refs[w.ref].description.split()[0] for w in w3]
        assert all(a.identity == a.n_eq / (a.n_eq + a.n_x + a.n_ins + a.n_del) for a in g3)
    assert any(w3[0].ref != 0 for w3 in want)
    noted = api.assignGenes(hits, refs, annotate=True, ctx=ctx)
    for r, h, g3 in zip(noted, hits, got):
        assert r.description == f"{h.description} | Ref = {g3[0].ref_id} | Identity = {g3[0].identity:.3f}" and r.sequence == h.sequence
    if strand == "both":
        assert sum(h.description.endswith("| Strand = -") for h in hits) == 3
        assert all(" | Strand = - | Ref = " in r.description for r in noted[7:])
    path = str(tmp_path / "assigned.fasta")
    api.write_results(noted, path)
    assert [(r.description, r.sequence) for r in fasta.read_fasta(path)] == [(r.description, r.sequence) for r in noted]
    # the same hits as ranges of the resident genome (plus strand: the records' MatchPos ranges)
    if strand == "+":
        g = ctx.genome_from_path(LOCI)
        try:
            ids = [g.header(c).split()[0] for c in range(g.n_contigs)]
            where = [(ids.index(h.description.split(" | ")[0]),) + tuple(int(x) for x in h.description.split("MatchPos = ")[1].split(" | ")[0].split(":"))
                     for h in hits]
            again = api.assign_ranges(g, [w[0] for w in where], [w[1] for w in where], [w[2] for w in where], refs, top=3, ctx=ctx)
            assert again == got
        finally:
            g.free()
