"""Host-side alignment helper vs the reference's expectations that go through BioAlignments
(test/test_folder/test-KmerGMA.jl:128-145 and the loci of :179-193), and vs the model stated on its own in tests/align_ref.py:
the score is the model's optimum and the CIGAR is a well-formed alignment with exactly that score.  Runs on the CPU."""
import ctypes as C
import os

import numpy as np
import pytest

from kmergma_amd import _lib, align, fasta, refprep
from tests import align_cases as ac
from tests import align_ref as ar


def test_cigar_to_unitrange_goldens(golden):
    for case in golden["scan"]["alignment"]["cigar_to_UnitRange"]:
        got = align.align_range(case["a"].encode(), case["b"].encode(), case["gap_open"], case["gap_extend"])
        assert list(got) == case["expected"]
    assert align.cigar_to_UnitRange("5D8=5D") == (6, 13)
    assert align.cigar_to_UnitRange("5D4=2D4=5D") == (6, 15)
    # quirks of src/Alignment.jl:13-30: last op dropped, first op taken whatever its type
    assert align.cigar_to_UnitRange("8=") == (1, 0)
    assert align.cigar_to_UnitRange("3=2I3=4D") == (4, 8)


def test_align_unitrange_golden(golden, data_dir):
    g = golden["scan"]["alignment"]["align_unitrange"]
    cons = golden["refprep"]["test_consensus_seq"].encode()
    rec = fasta.read_fasta(os.path.join(data_dir, g["genome"]))[g["record"] - 1]
    lo, hi = g["range"]
    a, b = align.align_range(cons[:g["windowsize"]], rec.sequence[lo - 1:hi], -69, -1)
    assert [max(1, lo + a - 1), min(lo + b - 1, g["seq_len"])] == g["expected"]


def test_fixture_hit_loci_through_aligner(golden, data_dir, loci):
    """Pre-alignment candidates (golden G4) -> aligner -> the loci of test-KmerGMA.jl:189."""
    g = golden["scan"]["single_align"]
    RV, W, cons = refprep.gen_ref_ws_cons(os.path.join(data_dir, "Alp_V_ref.fasta"), 6)
    pre = [(0, 8498, 8886, 0), (0, 20380, 20768, 0), (2, 640, 1028, 221227), (2, 12746, 13134, 221227),
           (3, 6807, 7195, 444023), (3, 23864, 24252, 444023), (3, 33800, 34188, 444023)]
    out = []
    for c, lo, hi, gp in pre:
        a, b = align.align_range(cons[:W], loci[c].sequence[lo - 1:hi], g["gap_open"], g["gap_extend"])
        out.append(max(1, lo + a - 1) + gp)
    assert out == g["hit_loci"]


# ---- against the independent model (tests/align_ref.py) -----------------------------------------------------------------------

TINY_GAPS = [(-69, -1), (-200, -1), (-5, -3), (-3, -1), (0, -2)]
MEDIUM_GAPS = [(-69, -1), (-200, -1), (-5, -3), (-69, -5)]
MEDIUM_M = [1, 2, 63, 64, 65, 127, 128, 129, 289, 300]


def check_unitrange(cigar):
    """cigar_to_UnitRange (src/Alignment.jl:13-30): first - 1 is the first run's length, last the sum of all runs but the last.
    The last run is never read, so a CIGAR of a single run gives (1, 0) ("8=" above)."""
    rr = ar.runs(cigar)
    first, last = align.cigar_to_UnitRange(cigar)
    assert first - 1 == (rr[0][0] if len(rr) > 1 else 0), cigar
    assert last == sum(x for x, _ in rr[:-1]), cigar


def check_host(a, b, go, ge, brute=False):
    """host score == the model's optimum == the score of the host's own CIGAR, which must be a valid alignment of a and b."""
    cigar, score = align.semiglobal_cigar(a, b, go, ge)
    ctx = (a, b, go, ge, cigar)
    if brute:
        assert score == ar.optimum_bruteforce(a, b, go, ge), ctx
    assert score == ar.optimum(a, b, go, ge), ctx
    assert score == ar.rescore(cigar, a, b, go, ge), ctx
    check_unitrange(cigar)
    return cigar


def test_tiny_random_cases_reach_the_models_optimum():
    """1500 cases with m in 1..8, n in 1..10, a third on the tie-rich two-letter alphabet, half of the segments derived from the
    consensus, under five gap models: brute force over every substring == row DP == host score == rescored host CIGAR."""
    rng = np.random.default_rng(2024)
    seen_ops = set()
    for c in range(1500):
        alphabet = b"AC" if c % 3 == 0 else b"ACGTN"
        a = ac.rand_seq(rng, rng.integers(1, 9), alphabet)
        if c % 2:
            b = ac.rand_seq(rng, rng.integers(1, 11), alphabet)
        else:                                               # the consensus with an edit and flanks, cut to 10
            g = bytearray(a)
            p = int(rng.integers(0, len(g) + 1))
            if rng.random() < 0.5:
                g[p:p] = ac.rand_seq(rng, rng.integers(1, 3), alphabet)
            elif len(g) > 1:
                del g[min(p, len(g) - 1)]
            b = (ac.rand_seq(rng, rng.integers(0, 3), alphabet) + bytes(g) + ac.rand_seq(rng, rng.integers(0, 3), alphabet))[:10]
        for go, ge in TINY_GAPS:
            seen_ops.update(o for _, o in ar.runs(check_host(a, b, go, ge, brute=True)))
    assert seen_ops == set("=XDI")


@pytest.mark.parametrize("m", MEDIUM_M)
def test_medium_cases_reach_the_models_optimum(m):
    """Consensus lengths around the 64-row strips of the device kernel; segments are the consensus with substitutions, N, indels
    of 1-29 residues and 0-99 residues of flank, pieces shorter than the consensus, a single residue, and unrelated sequence."""
    rng = np.random.default_rng(1000 + m)
    cons = ac.rand_seq(rng, m)
    segs = [ac.mutated(rng, cons) for _ in range(5)]
    segs += [ac.mutated(rng, cons, flank=0), cons, cons[:1], ac.rand_seq(rng, 1), ac.rand_seq(rng, m + 40)]
    if m > 2:
        lo = int(rng.integers(0, m // 2))
        segs += [cons[lo:lo + m // 2], cons[m // 3:], cons[:m - 1], ac.mutated(rng, cons, flank=0)[:max(1, m // 4)]]
    assert any(len(s) < m for s in segs) or m == 1
    for go, ge in MEDIUM_GAPS:
        for seg in segs:
            check_host(cons, seg, go, ge)


def test_low_complexity_and_alphabet_cases_reach_the_models_optimum():
    for a, b in ac.low_complexity_cases():
        for go, ge in ac.LOW_COMPLEXITY_GAPS:
            check_host(a, b, go, ge, brute=len(a) <= 10 and len(b) <= 10)


def test_bytes_outside_the_alphabet_count_as_n():
    a, b = b"ACGTRAC-GT", b"AC-TRACNGTT"
    tr = bytes.maketrans(b"R-", b"NN")
    for go, ge in TINY_GAPS:
        assert align.semiglobal_cigar(a, b, go, ge) == align.semiglobal_cigar(a.translate(tr), b.translate(tr), go, ge)
        assert align.semiglobal_cigar(a, b, go, ge) == align.semiglobal_cigar(a.lower(), b, go, ge)


def _raw(a, b, cap):
    buf = C.create_string_buffer(max(cap, 1))
    score = C.c_int64(0)
    st = _lib.load().kgma_host_semiglobal_cigar(bytes(a), len(a), bytes(b), len(b), -69, -1, buf, cap, C.byref(score))
    return st, buf.value.decode()


def test_host_aligner_error_paths():
    a = b"ACGTACGT"
    assert _raw(a, a, 3) == (_lib.KGMA_OK, "8=")                       # "8=" and its terminator just fit
    assert _raw(a, a, 2)[0] == _lib.KGMA_E_ARG
    assert _raw(a, a, 1)[0] == _lib.KGMA_E_ARG
    b = b"TT" + a[:3] + b"C" + a[4:] + b"TT"
    assert _raw(a, b, 11) == (_lib.KGMA_OK, "2D3=1X4=2D")            # ten characters and the terminator
    assert _raw(a, b, 10)[0] == _lib.KGMA_E_ARG
    # (m + 1)(n + 1) > 2^31 cells: refused before anything is allocated or read
    big_a, big_b = bytes(65536), bytes(32768)
    assert (len(big_a) + 1) * (len(big_b) + 1) > 1 << 31
    assert _raw(big_a, big_b, 64)[0] == _lib.KGMA_E_UNSUPPORTED


def test_co_optimal_choice_follows_the_stated_order():
    """Among alignments of equal score the traceback, walking back from the end, prefers match, then deletion, then insertion, and
    keeps a gap run going where extending and opening tie (the `>=` of the extend flags).  Worked by hand; the independent model
    cannot tell these apart, and the reference's goldens do not visit them."""
    # one base against two copies: 5 either way; the match is taken at the end of the segment
    assert align.semiglobal_cigar(b"A", b"AA", -69, -1) == ("1D1=", 5)
    # two bases against one: 5 - 70 either way; the match is taken at the end of the consensus
    assert align.semiglobal_cigar(b"AA", b"A", -69, -1) == ("1I1=", -65)
    # free trailing gaps: "1=2D" and "1D1=1D" both score 5; the trailing deletion run, once begun, is extended over the second A
    assert align.semiglobal_cigar(b"A", b"AAC", -69, -1) == ("1=2D", 5)
    # free gap opening: A against a gap then C unaligned (-2) beats the mismatch (-4) in either order; deletion wins at the end
    assert align.semiglobal_cigar(b"A", b"C", 0, -2) == ("1I1D", -2)
    assert align.semiglobal_cigar(b"A", b"CCC", 0, -2) == ("1I3D", -2)
    for a, b, go, ge in ((b"A", b"AA", -69, -1), (b"AA", b"A", -69, -1), (b"A", b"AAC", -69, -1), (b"A", b"C", 0, -2), (b"A", b"CCC", 0, -2)):
        check_host(a, b, go, ge, brute=True)
