"""The k-mer distance matrix without a device: the model (tests/kmat_ref.py) checked against the oracle and a dense computation,
the GPU tests' case lists shown not to be vacuous, the fixture condition the prescreen's end-to-end test rests on, and the Python
glue of api.kmer_dist_matrix / nearest_refs / assignGenes(prescreen=) over a stubbed context."""
import os

import numpy as np
import pytest

from kmergma_amd import _lib, api, fasta, refprep
from kmergma_amd.fasta import Record
from oracle import oracle as orc
from tests import assign_ref
from tests import kmat_cases as cases
from tests import kmat_ref as model
from tests.conftest import DATA

ALP = os.path.join(DATA, "Alp_V_ref.fasta")


# ---- the model is itself checked ------------------------------------------------------------------------------------------
def test_model_dist_equals_the_oracle_bit_for_bit():
    """kmer_dist(seq1, seq2, k) of the CPU oracle, pair by pair, on a sample of the matrix cases at k <= 8."""
    n = 0
    for k, A, B in [cases.length_case(k) for k in (1, 2, 5, 6, 7, 8)] + cases.alphabet_cases():
        B = A if B is None else B
        dist = model.dist_matrix(model.D_matrix(A, B, k), k)
        for i in range(0, len(A), 2):
            for j in range(0, len(B), 3):
                want = orc.kmer_dist_seq(A[i], B[j], k)
                assert dist[i, j] == want, (k, i, j, dist[i, j], want)
                n += 1
    assert n > 100


def test_model_D_equals_a_dense_bincount():
    for k, A, B in [cases.length_case(k) for k in (1, 3, 6)] + [cases.counter_cases()[1], cases.alphabet_cases()[0]]:
        dense = lambda s: np.bincount(refprep.kmer_indices(s, k), minlength=4 ** k).astype(np.int64)
        want = np.array([[int(((dense(a) - dense(b)) ** 2).sum()) for b in B] for a in A])
        assert np.array_equal(model.D_matrix(A, B, k), want)


def test_model_nearest_orders_ties_by_index():
    D = np.array([[5, 2, 9, 2, 2], [7, 7, 7, 7, 7]], dtype=np.int64)
    idx, Dn = model.nearest(D, 4)
    assert idx.tolist() == [[1, 3, 4, 0], [0, 1, 2, 3]] and Dn.tolist() == [[2, 2, 2, 5], [7, 7, 7, 7]]


# ---- no case is vacuous ---------------------------------------------------------------------------------------------------
def test_the_edge_case_reaches_the_largest_D_and_fits_int32():
    k, A, B = cases.counter_cases()[0]
    D = model.D_matrix(A, B, k)
    assert int(D[0, 1]) == cases.D_MAX == 2147352578 < 2 ** 31 and int(D[0, 0]) == int(D[1, 1]) == int(D[2, 2]) == 0
    assert np.array_equal(D, D.T)
    k, A, B = cases.counter_cases()[3]                # homopolymers at k = 7: N and T are the same k-mer
    D = model.D_matrix(A, B, k)
    assert int(D[1, 2]) == 0 and int(D[0, 1]) == (cases.MAX_LEN - 6) ** 2 + (5000 - 6) ** 2
    assert int(D[4, 4]) == 0 and not refprep.kmer_indices(A[4], k).size          # six residues at k = 7: nothing counted


def test_the_tie_cases_have_ties_and_winners_other_than_zero():
    ties = not_zero = all_equal = False
    for k, A, B, _ in cases.nearest_cases():
        D = model.D_matrix(A, B, k)
        for row in D:
            s = np.sort(row)
            ties |= bool(s[0] == s[1])
            all_equal |= bool(s[0] == s[-1]) and row.size >= cases.MAX_NEAR
        not_zero |= bool((model.nearest(D, 1)[0][:, 0] != 0).any())
    assert ties and not_zero and all_equal
    for k in cases.KS:                                # every length case has a row whose nearest column is not the first
        _, A, B = cases.length_case(k)
        assert (model.nearest(model.D_matrix(A, B, k), 1)[0][:, 0] != 0).any(), k


def test_the_shapes_sit_on_the_kernel_edges():
    assert cases.TILE[5] == 16 and cases.TILE[6] == 8 and cases.TILE[7] == 4 and cases.TILE[8] == 1
    assert cases.form_of(7) == cases.FORM_LDS and cases.form_of(8) == cases.FORM_GLOBAL
    for k in cases.KS:
        _, A, B = cases.length_case(k)
        assert len(B) == 2 * cases.TILE[k] + 1
        assert [max(len(a) - k + 1, 0) for a in A] == [0, 0, 1, 2, 63, 64, 65, 128, 129]
    assert cases.tile_widths(6) == [1, 7, 8, 9, 17] and cases.tile_widths(8) == [1, 2, 3]
    assert any(len(s) == cases.MAX_LEN == _lib.KMAT_MAX_LEN for _, A, _ in cases.long_cases() for s in A)
    assert sorted(len(B) for _, _, B, _ in cases.nearest_cases())[-4:] == [64, 65, 130, 200]
    assert _lib.KMAT_MAX_NEAR == cases.MAX_NEAR


def test_every_bad_case_is_bad_where_it_says():
    for k, A, B, words in cases.bad_cases():
        side, idx = words[0].split(" sequence ")
        seq = (A if side == "A" else (A if B is None else B))[int(idx)]
        pos = int(words[1].split()[1])
        assert seq[pos - 1:pos] not in b"ACGTNacgtn" and all(ch in b"ACGTNacgtn" for ch in seq[:pos - 1])
        with pytest.raises(KeyError):
            model.counts(seq, k)
    recs, ranges, B, bad = cases.record_case()
    assert b"*" in recs[2] and all(b"*" not in t for t in cases.ranges_text(recs, ranges)) and b"*" in recs[bad[0]][bad[1] - 1:bad[2]]
    assert any(hi == lo - 1 for _, lo, hi in ranges)


# ---- the fixture condition of the prescreen -------------------------------------------------------------------------------
def test_the_full_winner_is_among_the_eight_nearest_on_the_fixture_queries():
    """A condition on the INPUTS of test_gpu_kmat's end-to-end test: for every fixture query the model's winner of the full
    assignment lies among the model's 8 nearest references at k = 6 (measured: worst rank 1, counted from 0, over all 84 genes)."""
    genes = [r.sequence for r in fasta.read_fasta(ALP)]
    pick, queries = cases.fixture_queries(genes)
    assert len(queries) >= 12 and len(set(pick)) == len(pick)
    near, _ = model.nearest(model.D_matrix(queries, genes, 6), 8)
    S = assign_ref.score_matrix(genes, queries, -69, -1)
    for q in range(len(queries)):
        winner = assign_ref.choose(S[q], 1)[0]
        assert winner in near[q].tolist(), (q, pick[q], winner, near[q].tolist())


# ---- glue over a stubbed context ----------------------------------------------------------------------------------------
class StubContext:
    def __init__(self):
        self.calls = []

    @staticmethod
    def _out(nq, top):
        out = np.zeros((nq, top), dtype=_lib.ASSIGNMENT_DTYPE)
        out["ref"] = 1
        out["n_eq"] = 4
        return out

    def assign_seqs(self, refs, queries, go, ge, top):
        self.calls.append(("seqs", len(refs), len(queries), go, ge, top))
        return self._out(len(queries), top), None

    def assign_ranges(self, genome, refs, contig, lo, hi, go, ge, top):
        self.calls.append(("ranges", len(refs), list(contig), go, ge, top))
        return self._out(len(contig), top), None

    def assign_seqs_screened(self, refs, queries, go, ge, top, screen_k, n_near):
        self.calls.append(("seqs_screened", len(refs), len(queries), go, ge, top, screen_k, n_near))
        return self._out(len(queries), top), None, None

    def assign_ranges_screened(self, genome, refs, contig, lo, hi, go, ge, top, screen_k, n_near):
        self.calls.append(("ranges_screened", len(refs), list(contig), go, ge, top, screen_k, n_near))
        return self._out(len(contig), top), None, None

    def kmer_dist_matrix(self, a, b, k):
        self.calls.append(("matrix", list(a), None if b is None else list(b), k))
        nb = len(a) if b is None else len(b)
        return np.full((len(a), nb), 24, dtype=np.int32), np.full((len(a), nb), 2.0)

    def kmer_dist_matrix_ranges(self, genome, contig, lo, hi, b, k):
        self.calls.append(("matrix_ranges", genome, list(contig), list(lo), list(hi), list(b), k))
        return np.full((len(contig), len(b)), 24, dtype=np.int32), np.full((len(contig), len(b)), 2.0)

    def kmer_nearest(self, a, b, k, n_near):
        self.calls.append(("nearest", list(a), list(b), k, n_near))
        return np.tile(np.arange(n_near, dtype=np.int32)[::-1], (len(a), 1)), np.full((len(a), n_near), 24, dtype=np.int32)


REFS = [Record("IGHV1S1 first gene", b"ACGTACGT"), Record("IGHV2S7", b"acgtnacg"), Record("IGHV3", b"ACGTTTTT")]
HITS = [Record("chr1 | dist = 11.8 | MatchPos = 5:300 | GenomePos = 0 | Len = 296", b"ACGTTACGT"), Record("chr2 | x", b"TTTT")]


def test_prescreen_none_is_the_unscreened_call_and_an_integer_the_screened_one():
    stub = StubContext()
    api.assignGenes(HITS, REFS, top=2, ctx=stub)
    api.assignGenes(HITS, REFS, top=2, prescreen=None, prescreen_k=4, ctx=stub)
    api.assignGenes(HITS, REFS, top=2, prescreen=3, prescreen_k=5, gap_open_score=-5, gap_extend_score=-3, ctx=stub)
    g = object.__new__(_lib.Genome)
    api.assign_ranges(g, [0, 1], [1, 1], [4, 4], REFS, ctx=stub)
    api.assign_ranges(g, [0, 1], [1, 1], [4, 4], REFS, prescreen=2, ctx=stub)
    g._h = None
    assert stub.calls == [("seqs", 3, 2, -69, -1, 2), ("seqs", 3, 2, -69, -1, 2), ("seqs_screened", 3, 2, -5, -3, 2, 5, 3),
                          ("ranges", 3, [0, 1], -69, -1, 1), ("ranges_screened", 3, [0, 1], -69, -1, 1, 6, 2)]
    noted = api.assignGenes(HITS, REFS, prescreen=1, annotate=True, ctx=stub)
    assert noted[1].description == "chr2 | x | Ref = IGHV2S7 | Identity = 1.000"


def test_prescreen_argument_errors():
    stub = StubContext()
    for bad in (0, 1, 4, 129, 2.0, "8", True):
        with pytest.raises(ValueError, match="prescreen"):
            api.assignGenes(HITS, REFS, top=2, prescreen=bad, ctx=stub)
        with pytest.raises(ValueError, match="prescreen"):
            api.assign_ranges("unopened.fasta", [0], [1], [2], REFS, top=2, prescreen=bad, ctx=stub)
    many = [b"ACGT"] * 200
    with pytest.raises(ValueError, match="prescreen = 129"):
        api.assignGenes(HITS, many, prescreen=129, ctx=stub)
    with pytest.raises(ValueError, match="top = 4"):
        api.assignGenes(HITS, REFS, top=4, prescreen=3, ctx=stub)
    assert stub.calls == []
    api.assignGenes(HITS, many, prescreen=128, ctx=stub)
    assert stub.calls[-1][-1] == 128


def test_matrix_and_nearest_glue():
    stub = StubContext()
    d = api.kmer_dist_matrix(REFS, [b"ACGT", "acgt"], 3, ctx=stub)
    assert d.dtype == np.float64 and d.shape == (3, 2)
    D = api.kmer_dist_matrix([b"ACGT", "ac"], k=4, integer=True, ctx=stub)
    assert D.dtype == np.int32 and D.shape == (2, 2)
    assert stub.calls == [("matrix", [b"ACGTACGT", b"acgtnacg", b"ACGTTTTT"], [b"ACGT", b"acgt"], 3), ("matrix", [b"ACGT", b"ac"], None, 4)]
    g = object.__new__(_lib.Genome)
    assert api.kmer_dist_matrix_ranges(g, [0], [1], [9], REFS, 5, integer=True, ctx=stub).shape == (1, 3)
    assert stub.calls[-1] == ("matrix_ranges", g, [0], [1], [9], [b"ACGTACGT", b"acgtnacg", b"ACGTTTTT"], 5)
    g._h = None
    with pytest.raises(TypeError, match="subject"):
        api.kmer_dist_matrix_ranges(12, [0], [1], [2], REFS, ctx=stub)
    with pytest.raises(ValueError, match="no reference"):
        api.kmer_dist_matrix([], ctx=stub)
    near = api.nearest_refs(HITS, REFS, k=4, n=2, ctx=stub)                    # D = 24 at k = 4: dist = 24 / 8
    assert near == [[("IGHV2S7", 1, 3.0), ("IGHV1S1", 0, 3.0)]] * 2 and stub.calls[-1] == ("nearest", [b"ACGTTACGT", b"TTTT"], [r.sequence for r in REFS], 4, 2)
    assert api.nearest_refs([], REFS, ctx=stub) == []
    for n in (0, 4):
        with pytest.raises(ValueError, match=f"n = {n}"):
            api.nearest_refs(HITS, REFS, n=n, ctx=stub)


def test_the_library_exports_the_entry_points():
    assert {"kgma_kmer_dist_matrix", "kgma_kmer_dist_matrix_ranges", "kgma_kmer_nearest", "kgma_kmer_nearest_ranges", "kgma_get_kmat_stats",
            "kgma_assign_seqs_screened", "kgma_assign_ranges_screened"} <= set(_lib.EXPORTS)
    assert _lib.C.sizeof(_lib.KgmaKmatStats) == 40
