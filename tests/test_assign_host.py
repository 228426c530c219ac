"""Gene assignment without a device: the model (tests/assign_ref.py) on the GPU tests' case lists -- that it is well defined and
that the lists are not vacuous --, and the Python glue of api.assignGenes / api.assign_ranges over a stubbed context."""
import numpy as np
import pytest

from kmergma_amd import _lib, align, api
from kmergma_amd.fasta import Record
from tests import align_ref as ar
from tests import assign_cases as cases
from tests import assign_ref as model


# ---- the model ------------------------------------------------------------------------------------------------------
def test_count_columns_takes_only_the_end_runs_of_d_off():
    assert model.count_columns("3D5=2X1I4=2D6=7D", 29) == (15, 2, 1, 2, 4, 22)
    assert model.count_columns("5=", 5) == (5, 0, 0, 0, 1, 5)
    assert model.count_columns("2I3D", 3) == (0, 0, 2, 0, 1, 0)          # nothing of the query is left: q_hi < q_lo
    assert model.count_columns("4D2I", 4) == (0, 0, 2, 0, 5, 4)
    assert model.count_columns("1X", 1) == (0, 1, 0, 0, 1, 1)


def test_choose_is_stable_on_equal_scores():
    assert model.choose([5, 9, 9, 3, 9], 3) == [1, 2, 4]
    assert model.choose([5, 9, 9, 3, 9], 5) == [1, 2, 4, 0, 3]
    assert model.choose([-7], 1) == [0]


def test_the_model_on_a_small_batch_by_hand():
    refs = [b"ACGT", b"ACGA", b"TTTT"]
    got = model.assign(refs, [b"GGACGTGG"], -69, -1, 3)[0]
    assert got[0] == model.Want(0, 20, 4, 0, 0, 0, 3, 6)
    assert got[1] == model.Want(1, 11, 3, 1, 0, 0, 3, 6)
    assert got[2][:6] == (2, 5 - 3 * 4, 1, 3, 0, 0)                      # one T of TTTT pairs with the query's only T


@pytest.mark.parametrize("go,ge", [(-69, -1), (0, -1)])
def test_every_pair_of_the_tie_and_alphabet_lists_rests_on_a_checked_alignment(go, ge):
    """model.pair asserts rescore(CIGAR) == optimum == the host aligner's score: run it over whole lists (all pairs)."""
    for refs, queries in [cases.tie_case()] + cases.alphabet_cases():
        for row in model.assign(refs, queries, go, ge, len(refs)):
            assert [w.ref for w in row] == model.choose([w.score for w in sorted(row, key=lambda w: w.ref)], len(refs))
            for w in row:
                assert w.n_eq + w.n_x + w.n_ins == len(refs[w.ref])                   # the reference is global
                assert w.n_eq + w.n_x + w.n_del == max(w.q_hi - w.q_lo + 1, 0)         # what the overhangs leave of the query


# ---- non-vacuity of the GPU case lists --------------------------------------------------------------------------------
def test_the_case_lists_are_not_vacuous():
    winner_not_zero = inner_d = uses_i = exact_tie = False
    for refs, queries in [cases.strip_case(65), cases.tie_case()] + cases.alphabet_cases():
        S = model.score_matrix(refs, queries, -69, -1)
        for k, q in enumerate(queries):
            best = model.choose(S[k], 1)[0]
            winner_not_zero |= best != 0
            exact_tie |= len(refs) > 1 and sorted(S[k])[-1] == sorted(S[k])[-2]
    for go, ge in ((-69, -1), (-5, -3)):
        for refs, queries in [cases.strip_case(65), cases.tie_case()]:
            for r in refs:
                for q in queries:
                    cigar, _ = align.semiglobal_cigar(r, q, go, ge)
                    inner_d |= model.uses(cigar, "D")
                    uses_i |= model.uses(cigar, "I")
    assert winner_not_zero and inner_d and uses_i and exact_tie


def test_the_tie_list_ties_where_it_says():
    refs, queries = cases.tie_case()
    assert refs[1] == refs[3] and refs[4] != refs[1] and refs[4].upper() == refs[1]
    for go, ge in cases.GAPS:
        S = model.score_matrix(refs, queries, go, ge)
        assert (S[:, 1] == S[:, 3]).all() and (S[:, 1] == S[:, 4]).all()
        assert model.choose(S[0], 3) == [1, 3, 4] and model.choose(S[1], 3) == [1, 3, 4]


def test_the_chunked_list_needs_two_launches_and_the_limit_lists_sit_on_the_limit():
    refs, queries = cases.chunked_case()
    assert cases.PAIRS_PER_LAUNCH < len(refs) * len(queries) < 2 * cases.PAIRS_PER_LAUNCH
    assert max(map(len, cases.long_query_case()[1])) == cases.MAX_LEN == _lib.ASSIGN_MAX_LEN
    assert len(cases.long_ref_case()[0][0]) == cases.MAX_LEN


# ---- glue over a stubbed context --------------------------------------------------------------------------------------
class StubContext:
    """assign_seqs / assign_ranges that return a fixed matrix of assignments and remember what they were asked."""

    def __init__(self, rows):
        self.rows = rows
        self.calls = []

    def _out(self, nq, top):
        out = np.zeros((nq, top), dtype=_lib.ASSIGNMENT_DTYPE)
        for q in range(nq):
            for t in range(top):
                out[q, t] = self.rows[q][t]
        return out, np.zeros((nq, 1), dtype=np.int32)

    def assign_seqs(self, refs, queries, gap_open, gap_extend, top):
        self.calls.append(("seqs", list(refs), list(queries), gap_open, gap_extend, top))
        return self._out(len(queries), top)

    def assign_ranges(self, genome, refs, contig, lo, hi, gap_open, gap_extend, top):
        self.calls.append(("ranges", genome, list(refs), list(contig), list(lo), list(hi), gap_open, gap_extend, top))
        return self._out(len(contig), top)


ROWS = [[(1, 1400, 280, 10, 3, 7, 51, 347), (0, 1391, 279, 11, 3, 7, 51, 347)],
        [(0, -80, 0, 0, 0, 0, 1, 0), (1, -81, 0, 1, 4, 0, 1, 1)]]
REFS = [Record("IGHV1S1 first gene", b"ACGTACGT"), Record("IGHV2S7", b"acgtnacg")]
HITS = [Record("chr1 | dist = 11.8 | MatchPos = 5:300 | GenomePos = 0 | Len = 296", b"ACGTTACGT"),
        Record("chr2 | dist = 3.0 | MatchPos = 9:20 | GenomePos = 500 | Len = 12 | Strand = -", b"TTTT")]


def test_assignment_tuples_and_identity():
    stub = StubContext(ROWS)
    got = api.assignGenes(HITS, REFS, top=2, gap_open_score=-5, gap_extend_score=-3, ctx=stub)
    assert stub.calls == [("seqs", [b"ACGTACGT", b"acgtnacg"], [b"ACGTTACGT", b"TTTT"], -5, -3, 2)]
    assert got[0][0] == api.Assignment("IGHV2S7", 1, 1400, 280 / 300, 280, 10, 3, 7, 51, 347)
    assert got[0][1] == api.Assignment("IGHV1S1", 0, 1391, 279 / 300, 279, 11, 3, 7, 51, 347)
    assert got[1][0].identity == 0.0 and got[1][0].q_hi < got[1][0].q_lo            # no column at all: 0.0, not a division by zero
    assert got[1][1].identity == 0.0 and got[1][1].ref_id == "IGHV2S7"
    assert api.Assignment._fields == ("ref_id", "ref_index", "score", "identity", "n_eq", "n_x", "n_ins", "n_del", "q_lo", "q_hi")


def test_annotate_appends_after_the_last_field_and_leaves_the_input_alone():
    stub = StubContext(ROWS)
    before = [Record(h.description, h.sequence) for h in HITS]
    out = api.assignGenes(HITS, REFS, annotate=True, ctx=stub)
    assert HITS == before and stub.calls[0][5] == 1
    assert out[0].description == "chr1 | dist = 11.8 | MatchPos = 5:300 | GenomePos = 0 | Len = 296 | Ref = IGHV2S7 | Identity = 0.933"
    assert out[1].description == "chr2 | dist = 3.0 | MatchPos = 9:20 | GenomePos = 500 | Len = 12 | Strand = - | Ref = IGHV1S1 | Identity = 0.000"
    assert [r.sequence for r in out] == [h.sequence for h in HITS]
    assert api.assignGenes(HITS, REFS, ctx=stub)[0][0].ref_id == "IGHV2S7"           # the default returns tuples, not records


def test_bare_sequences_and_empty_input():
    stub = StubContext(ROWS)
    got = api.assignGenes([b"ACGT", "acgt"], [b"AC", "GT"], top=1, ctx=stub)
    assert stub.calls[0][1:3] == ([b"AC", b"GT"], [b"ACGT", b"acgt"]) and got[0][0].ref_id == ""
    assert api.assignGenes([], REFS, ctx=stub) == [] and len(stub.calls) == 1        # no hits: no device call


def test_assign_ranges_passes_an_open_genome_through():
    stub = StubContext(ROWS)
    g = object.__new__(_lib.Genome)              # never dereferenced by the stub
    got = api.assign_ranges(g, [0, 3], [1, 10], [5, 40], REFS, top=2, ctx=stub)
    assert stub.calls == [("ranges", g, [b"ACGTACGT", b"acgtnacg"], [0, 3], [1, 10], [5, 40], -69, -1, 2)]
    assert got[0][0].ref_index == 1 and got[1][1].n_ins == 4
    g._h = None                                  # (its finaliser finds nothing to free)


def test_argument_errors_that_need_no_device():
    stub = StubContext(ROWS)
    with pytest.raises(ValueError, match="top = 0"):
        api.assignGenes(HITS, REFS, top=0, ctx=stub)
    with pytest.raises(ValueError, match="top = 3"):
        api.assignGenes(HITS, REFS, top=3, ctx=stub)
    with pytest.raises(ValueError, match="no reference"):
        api.assignGenes(HITS, [], ctx=stub)
    with pytest.raises(TypeError, match="annotate"):
        api.assignGenes([b"ACGT"], REFS, annotate=True, ctx=stub)
    with pytest.raises(TypeError, match="subject"):
        api.assign_ranges(12, [0], [1], [2], REFS, ctx=stub)
    with pytest.raises(ValueError, match="top = 5"):
        api.assign_ranges("unopened.fasta", [0], [1], [2], REFS, top=5, ctx=stub)
    assert stub.calls == []


def test_the_library_exports_the_entry_points():
    assert {"kgma_assign_seqs", "kgma_assign_ranges", "kgma_get_assign_stats"} <= set(_lib.EXPORTS)
    assert _lib.ASSIGNMENT_DTYPE.itemsize == 32
