"""Host-side checks of the codon-weight-matrix search (no GPU): the oracle against the definition, kgma_codon_fold against the
oracle's fold on both strands and under another genetic code, the minus matrix against the plus search of the reverse-complemented
text, api.translate / prot_pattern / prot_threshold / prot_matrix_from_sequences against values worked out by hand and by brute
force, that every case list hits what it is for, that every argument check is made before a context is touched, the library's
surface and the golden file."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

from kmergma_amd import _lib, api
from tests import codon_cases as cc
from tests import codon_oracle as co
from tests.conftest import DATA, GOLDEN, ROOT

LOCI = os.path.join(DATA, "Loci.fasta")
# NCBI table 2 (vertebrate mitochondrial) in TCAG order: TGA is W, ATA is M, AGA and AGG are stops
TABLE2 = "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSS**VVVVAAAADDEEGGGG"


@pytest.fixture(scope="module")
def loci_records():
    return co.read_fasta_sequences(LOCI)


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def test_scores_by_hand():
    W = np.zeros((2, 65), dtype=np.int64)
    W[0, co.codon_index(b"ATG")], W[0, co.codon_index(b"TGG")], W[0, 64] = 5, 3, -2
    W[1, co.codon_index(b"TGG")], W[1, co.codon_index(b"GGA")], W[1, 64] = 7, 1, -9
    assert (co.codon_index(b"AAA"), co.codon_index(b"AAC"), co.codon_index(b"ACA"), co.codon_index(b"CAA"), co.codon_index(b"TTT")) == (0, 1, 4, 16, 63)
    assert co.codon_index(b"atg") == co.codon_index(b"ATG") == 14 and co.codon_index(b"ANG") == co.codon_index(b"NNN") == 64
    # ATGTGGA: ATG+TGG 5+7, TGT+GGA 0+1; with one residue more the third frame: GTG+GAx 0+0
    assert co.profile(W, b"ATGTGGA").tolist() == [12, 1] and co.profile(W, b"ATGTGGAC").tolist() == [12, 1, 0]
    assert co.profile(W, b"ATGTG").size == 0 and co.profile(W, b"ATGTGG").tolist() == [12]
    assert co.profile(W, b"atgNGG").tolist() == [5 - 9] and co.profile(W, b"NTGTGG").tolist() == [-2 + 7]
    assert co.find(W, b"ATGTGGA", 1) == [(1, 12), (2, 1)] and co.find(W, b"ATGTGGA", 2) == [(1, 12)]
    assert (co.lowest(W), co.highest(W)) == (-11, 12)
    with pytest.raises(ValueError):
        co.find(W, b"ATGTGG", -11)
    with pytest.raises(ValueError):
        co.find(W, b"ATGXGG", 5)
    assert co.match_list([W, W], [b"ATGTGGA", b"TGGGGA"], [12, 1]) == [(0, 0, 1, 12), (1, 0, 1, 12), (1, 0, 2, 1), (1, 1, 1, 4)]


@pytest.mark.parametrize("m", [1, 2, 5, 21, 64])
def test_profile_is_the_definition(m):
    rng = np.random.default_rng(m)
    W = cc.rand_matrix(rng, m, constant=(1,) if m > 2 else ())
    for n in (0, 3 * m - 1, 3 * m, 3 * m + 1, 3 * m + 2, 400):
        t = bytearray(cc.rand_dna(rng, n))
        for i in rng.integers(0, max(n, 1), size=n // 10):
            t[i] = ord("N")
        t = bytes(t[:n // 2]).lower() + bytes(t[n // 2:])
        p = co.profile(W, t)
        assert p.dtype == np.int64 and p.size == max(0, n - 3 * m + 1)
        assert p.tolist() == [co.score_at(W, t, s) for s in range(1, p.size + 1)]


# ---- kgma_codon_fold -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letters", [co.TABLE1, TABLE2], ids=["table1", "table2"])
@pytest.mark.parametrize("m", [1, 2, 7, 64])
def test_fold_is_the_oracles(m, letters):
    rng = np.random.default_rng(300 + m)
    P = rng.integers(-32768, 32768, size=(m, 21))
    x = rng.integers(-32768, 32768, size=m)
    code = co.code_columns(letters)
    assert api.genetic_code(letters).tolist() == code
    for minus in (False, True):
        got = _lib.codon_fold(P, code, x, minus)
        assert got.shape == (m, 65) and got.dtype == np.int64 and np.array_equal(got, co.fold(P, code, x, minus))
        assert np.array_equal(api.prot_fold(P, genetic_code=letters, x_weight=x, minus=minus), got)
    assert np.array_equal(api.prot_fold(P, genetic_code=letters)[:, 64], P.min(axis=1))         # X: the row's minimum by default
    plus = co.fold(P, code, x)
    for aa, codon in (("M", b"ATG"), ("W", b"TGG"), ("*", b"TAA"), ("F", b"TTT"), ("K", b"AAA")):
        assert np.array_equal(plus[:, co.codon_index(codon)], P[:, co.AMINO_ACIDS.index(aa)])
    tga = "W" if letters == TABLE2 else "*"
    assert np.array_equal(plus[:, co.codon_index(b"TGA")], P[:, co.AMINO_ACIDS.index(tga)])


@pytest.mark.parametrize("m", [1, 3, 20])
def test_minus_matrix_is_the_plus_search_of_the_reverse_complement(m):
    """A hit of the minus matrix at the forward start s is a hit of the plus matrix at L - s - 3m + 2 of the reverse-complemented
    record, with the same score: start for start."""
    rng = np.random.default_rng(400 + m)
    P = cc.rand_profile(rng, m)
    plus, minus = _lib.codon_fold(P, co.code_columns(), P.min(axis=1), False), _lib.codon_fold(P, co.code_columns(), P.min(axis=1), True)
    t = bytearray(cc.rand_dna(rng, 2000))
    t[700:720] = b"N" * 20
    cc.plant(t, 100, cc.best_site(plus))
    cc.plant(t, 1000, co.revcomp_text(cc.best_site(plus)))
    t = bytes(t[:1500]) + bytes(t[1500:]).lower()
    L, thr = len(t), co.highest(plus) - (0 if m == 1 else 400)
    on_rc = co.find(plus, co.revcomp_text(t), thr)
    mapped = sorted((L - s - 3 * m + 2, k) for s, k in on_rc)
    assert co.find(minus, t, thr) == mapped and (1001, co.highest(plus)) in mapped and len(mapped) >= 1
    # and the whole profile, not only the hits
    assert co.profile(minus, t).tolist() == co.profile(plus, co.revcomp_text(t)).tolist()[::-1]
    want = [(0, L - s - 3 * m + 2, L - s + 1, "-", -((s - 1) % 3 + 1), k) for s, k in on_rc]
    assert co.api_list(P, [t], thr, "-") == sorted(want, key=lambda h: h[1])
    # the peptide under a minus hit, read by translate in the hit's frame, is the best peptide
    lo, hi, frame = next((lo, hi, f) for _, lo, hi, _, f, k in co.api_list(P, [t], thr, "-") if lo == 1001)
    pep = api.translate(t, frame)
    at = (L - hi - (-frame - 1)) // 3
    assert pep[at:at + m] == "".join(co.AMINO_ACIDS[i] for i in P[:, :20].argmax(axis=1))


def test_fold_argument_errors_through_the_c_abi():
    L = _lib.load()
    aa, x, out = (C.c_int16 * 42)(), (C.c_int16 * 2)(), (C.c_int16 * 130)()
    code = (C.c_uint8 * 64)(*co.code_columns())
    assert L.kgma_codon_fold(aa, 2, code, x, 0, out) == _lib.KGMA_OK
    for args in ((None, 2, code, x, 0, out), (aa, 2, None, x, 0, out), (aa, 2, code, None, 0, out), (aa, 2, code, x, 0, None),
                 (aa, 0, code, x, 0, out), (aa, 65, code, x, 0, out), (aa, -1, code, x, 1, out)):
        assert L.kgma_codon_fold(*args) == _lib.KGMA_E_ARG
    code[17] = 21
    assert L.kgma_codon_fold(aa, 2, code, x, 0, out) == _lib.KGMA_E_ARG
    for bad in (dict(aa_weights=np.zeros((2, 20), int)), dict(x_weight=[0]), dict(code=[0] * 63), dict(aa_weights=np.full((2, 21), 40000))):
        kw = dict(aa_weights=np.zeros((2, 21), int), code=co.code_columns(), x_weight=[0, 0])
        kw.update(bad)
        with pytest.raises(ValueError):
            _lib.codon_fold(**kw)
    with pytest.raises(_lib.KgmaError):
        _lib.codon_fold(np.zeros((2, 21), int), [21] * 64, [0, 0])


# ---- api.translate, api.genetic_code ---------------------------------------------------------------------------------------------
def test_translate_on_pinned_codons():
    for codon, aa in (("ATG", "M"), ("TGG", "W"), ("TAA", "*"), ("TAG", "*"), ("TGA", "*"), ("NTG", "X"), ("ANG", "X"), ("ATN", "X"),
                      ("CTN", "X"), ("CTA", "L"), ("CTC", "L"), ("CTG", "L"), ("CTT", "L"), ("atg", "M"), ("GGG", "G"), ("TTT", "F"), ("AAA", "K")):
        assert api.translate(codon) == aa == co.translate(codon), codon
    assert api.translate("ATGTGGTAATAGTGACTNCTAC") == "MW***XL" and api.translate(b"ATGTGGT", 2) == "CG" and api.translate("ATGTGGTA", 3) == "VV"
    assert api.translate("CCACAT", -1) == "MW" and api.translate("ACCACAT", -1) == "MW" and api.translate("CCACATA", -2) == "MW"
    assert api.translate("A", 1) == api.translate("AT", 1) == api.translate("ATG", 2) == ""
    assert api.translate("TGAATAAGA", genetic_code=TABLE2) == "WM*" and api.translate("TGAATAAGA") == "*IR"
    rng = np.random.default_rng(5)
    t = cc.rand_dna(rng, 301).replace(b"GATT", b"GANT")
    for frame in (1, 2, 3, -1, -2, -3):
        assert api.translate(t, frame) == co.translate(t, frame)
    with pytest.raises(ValueError):
        api.translate("ATG", 0)
    with pytest.raises(ValueError):
        api.translate("ATG", 4)


def test_genetic_code():
    code = api.genetic_code(1)
    assert code.tolist() == co.code_columns() == api.genetic_code(co.TABLE1).tolist() == api.genetic_code(api.genetic_code()).tolist()
    assert sorted(set(code.tolist())) == list(range(21)) and (code == 20).sum() == 3 and api.AMINO_ACIDS == co.AMINO_ACIDS
    assert api.GENETIC_CODES[1] == "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
    for bad, exc in ((2, ValueError), ("FFLL", ValueError), (co.TABLE1[:-1] + "X", ValueError), (1.5, TypeError), (np.zeros(63, int), ValueError),
                     (np.full(64, 21), ValueError)):
        with pytest.raises(exc):
            api.genetic_code(bad)


# ---- api.prot_pattern ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern, m", [
    ("W-[VIFY]-R-Q-[AVPS]-P-G-K", 8), ("[DE]-[TS]-[AG]-[VMIL]-Y-[YFH]-C", 7), ("C-x-W", 3), ("C-x(3)-W", 5), ("C-{PG}-W", 3),
    ("C-{PG*}(2)-*", 4), ("*", 1), ("c-X(2)-[vi](2)-w.", 6), ("CxW", 3), ("C-x(62)-W", 64), ("[*W]-A(3)", 4)])
def test_prot_pattern_syntax(pattern, m):
    M, n = api.prot_pattern(pattern)
    assert n == m and M.shape == (m, 21) and M.dtype == np.int64 and set(np.unique(M).tolist()) <= {0, -1}
    assert np.array_equal(M, co.parse_pattern(pattern.rstrip(".")))


def test_prot_pattern_by_hand():
    col = {a: i for i, a in enumerate(co.AMINO_ACIDS)}
    M, n = api.prot_pattern("W-[VI]-x-{P}-*")
    assert n == 5
    assert [a for a in co.AMINO_ACIDS if M[0, col[a]] == 0] == ["W"] and [a for a in co.AMINO_ACIDS if M[1, col[a]] == 0] == ["I", "V"]
    assert (M[2] == 0).all() and [a for a in co.AMINO_ACIDS if M[3, col[a]] == -1] == ["P"] and M[3, col["*"]] == 0
    assert [a for a in co.AMINO_ACIDS if M[4, col[a]] == 0] == ["*"]


@pytest.mark.parametrize("pattern, text", [
    ("", "empty"), ("-", "empty"), ("C-[]-W", "empty set"), ("C-[VI-W", "not closed"), ("C-{P-W", "not closed"), ("C-B-W", "'B'"),
    ("C-[VX]-W", "x stands alone"), ("C-x(2,4)-W", "repeat count"), ("C-x(0)-W", "repeat count"), ("C-x(-W", "repeat count"),
    ("<C-W", "'<'"), ("C-x(64)-W", "more than 64"), ("C-1-W", "'1'")])
def test_prot_pattern_refuses(pattern, text):
    with pytest.raises(ValueError) as ei:
        api.prot_pattern(pattern)
    assert text in str(ei.value), str(ei.value)


def test_prot_pattern_wants_a_string():
    with pytest.raises(TypeError):
        api.prot_pattern(b"C-W")


# ---- api.prot_threshold ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bg", [None, (.4, .1, .15, .35)], ids=["uniform", "skewed"])
@pytest.mark.parametrize("letters", [co.TABLE1, TABLE2], ids=["table1", "table2"])
def test_prot_threshold_agrees_with_brute_force_over_all_codon_pairs(bg, letters):
    rng = np.random.default_rng(70)
    P = rng.integers(-40, 41, size=(2, 21))
    kw = {} if bg is None else {"background": bg}
    lowest, p = api.prot_score_distribution(P, genetic_code=letters, **kw)
    brute = co.score_distribution_brute(P, bg or (.25,) * 4, co.code_columns(letters))
    assert math.isclose(p.sum(), 1.0, rel_tol=0, abs_tol=1e-12) and (p >= 0).all()
    assert lowest == min(brute) and lowest + p.size - 1 == max(brute)
    for k in range(p.size):
        assert math.isclose(p[k], brute.get(lowest + k, 0.0), rel_tol=1e-12, abs_tol=1e-15)
    tail = {t: math.fsum(q for s, q in brute.items() if s >= t) for t in range(lowest, lowest + p.size + 1)}
    last = lowest
    for pv in (0.9, 0.5, 0.1, 0.01, 1e-3, 1e-4, 1e-9):
        t = api.prot_threshold(P, pv, genetic_code=letters, **kw)
        assert t >= last                                                       # monotone: a smaller pvalue never lowers the threshold
        last = t
        assert tail[t] <= pv * (1 + 1e-12) and (t == lowest or tail[t - 1] > pv * (1 - 1e-12)), (pv, t)
    assert api.prot_threshold(P, 1e-9, genetic_code=letters, **kw) == max(brute) + 1   # rarer than the best pair: one above it


def test_prot_threshold_of_a_pattern():
    M, _ = api.prot_pattern("W-M")                                             # one codon each: P(score = 0) = 1 / 4096
    lowest, p = api.prot_score_distribution(M)
    assert lowest == -2 and p.tolist() == [63 * 63 / 4096, 2 * 63 / 4096, 1 / 4096]
    assert api.prot_threshold(M, 1 / 4096) == 0 and api.prot_threshold(M, 1 / 4097) == 1 and api.prot_threshold(M, 0.04) == -1
    for pv in (0, 1, -1):
        with pytest.raises(ValueError):
            api.prot_threshold(M, pv)


def test_prot_matrix_from_sequences_by_hand():
    # three peptides, pseudocount 1, uniform background 1/20: odds = ((count + 1/20) / 4) * 20 = 5 count + 1/4
    M = api.prot_matrix_from_sequences(["WV", "wI", b"WV"])
    cb = {c: round(100 * math.log2(5 * c + 0.25)) for c in (0, 1, 2, 3)}
    col = {a: i for i, a in enumerate(co.AMINO_ACIDS)}
    assert M.shape == (2, 21) and M.dtype == np.int64
    assert M[0, col["W"]] == cb[3] and M[1, col["V"]] == cb[2] and M[1, col["I"]] == cb[1] and M[0, col["A"]] == cb[0] == -200
    assert M[0, 20] == M[0, :20].min() and M[1, 20] == cb[0]                   # the stop: the row's minimum
    for seqs, kw, text in (([], {}, "at least one"), (["WV", "W"], {}, "differ in length"), (["W*"], {}, "20 amino-acid"),
                           (["WB"], {}, "20 amino-acid"), (["W" * 65], {}, "65 residues"), (["WV"], {"pseudocount": 0}, "row 1"),
                           (["WV"], {"background": (.25,) * 4}, "background")):
        with pytest.raises(ValueError) as ei:
            api.prot_matrix_from_sequences(seqs, **kw)
        assert text in str(ei.value)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def searched():
    return [(c, co.match_list(c.matrices, c.records, c.thresholds)) for c in cc.host_cases()]


def test_every_case_hits_what_it_is_for(searched):
    assert len(searched) >= 25 and len({c.name for c, _ in searched}) == len(searched)
    for c, found in searched:
        at = {(i, r, s) for i, r, s, _ in found}
        assert c.aim, c.name
        missing = [h for h in c.aim.get("hits", []) if h not in at]
        assert not missing, (c.name, missing)
        assert not any(h in at for h in c.aim.get("absent", [])), c.name
        assert (found == []) == bool(c.aim.get("none")), c.name
        assert len(found) > c.aim.get("many", -1), (c.name, len(found))
        for i, r, s in c.aim.get("absent", []):                                # what is absent is a record and a matrix that exist
            assert 0 <= i < len(c.matrices) and 0 <= r < len(c.records) and s >= 1, c.name


def test_length_cases_cover_the_lengths():
    cases = cc.length_cases()
    assert [len(c.matrices[0]) for c in cases] == list(cc.LENGTHS) == [1, 2, 21, 22, 63, 64]
    for c in cases:
        m = len(c.matrices[0])
        assert {len(r) for r in c.records} >= {3 * m - 1, 3 * m, 3 * m + 1, 3 * m + 2}
        assert (0, 0, len(c.records[0]) - 3 * m + 1) in c.aim["hits"]          # the last valid start of the long record
    tiny = cc.tiny_records_case()
    assert len(tiny.records) == 300 and {len(r) for r in tiny.records} == {1, 2, 3, 4, 5}


def test_seam_cases_lie_on_the_seams(searched):
    lane, wave, wg = cc.HOST_GEOMETRY
    bounds = cc.seam_boundaries(lane, wave, wg)
    assert bounds["wave"] == wave and bounds["wg"] == wg and bounds["wg2"] == 2 * wg
    by_name = {c.name: (c, found) for c, found in searched}
    for name, B in bounds.items():
        c, found = by_name[f"{name}_seam"]
        m = len(c.matrices[0])
        starts0 = {s - 1 for _, _, s, k in found if k == co.highest(c.matrices[0])}
        assert starts0 >= set(range(max(0, B - 3 * m), B + 4)), name           # a top site begins at every offset -3m ... +3
        last = [r for r in range(len(c.records)) if len(c.records[r]) == B + 3 * m]
        assert last and all((0, r, B + 1) in {(i, rr, s) for i, rr, s, _ in found} for r in last)
        assert max(len(r) for r in c.records) < B + 100


def test_batch_case_is_both_strands_of_eight_profiles():
    c, profs = cc.batch_case()
    assert len(profs) == 8 and len(c.matrices) == 16
    for i, P in enumerate(profs):
        assert np.array_equal(c.matrices[2 * i], api.prot_fold(P)) and np.array_equal(c.matrices[2 * i + 1], api.prot_fold(P, minus=True))


def test_cross_check_matrix_scores_like_the_position_weight_matrix():
    from tests import pwm_oracle as po
    rng = np.random.default_rng(12)
    W = rng.integers(-300, 300, size=(21, 4))
    t = cc.rand_dna(rng, 500)
    assert co.profile(cc.codon_matrix_of_pwm(W), t).tolist() == po.profile_rows(W, t).tolist()


# ---- api.protMatch: the checks come before any device call -----------------------------------------------------------------------
class NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before the argument checks")


OKP = np.zeros((2, 21), dtype=np.int64)
OKP[0, 18], OKP[1, 10], OKP[:, 20] = 5, 3, -1                                  # W then M; the stop costs 1


@pytest.mark.parametrize("profile, kw, exc, text", [
    (OKP, {}, ValueError, "exactly one"),
    (OKP, {"threshold": 5, "pvalue": 0.1}, ValueError, "exactly one"),
    ("W-M", {"threshold": 0, "max_mismatch": 0}, ValueError, "exactly one"),
    (OKP, {"max_mismatch": 0}, ValueError, "max_mismatch counts"),
    (OKP, {"threshold": -2}, ValueError, "does not exceed the sum of its row minima, -2"),
    (OKP, {"threshold": 2 ** 31}, ValueError, "int32"),
    (OKP, {"pvalue": 0}, ValueError, "pvalue"),
    (OKP, {"threshold": 5, "strand": "x"}, ValueError, ""),
    (OKP, {"threshold": 5, "genetic_code": 99}, ValueError, "not shipped"),
    (OKP, {"threshold": 5, "background": (.25,) * 4}, ValueError, "background"),
    ("W-M", {"max_mismatch": 2}, ValueError, "max_mismatch 2"),
    ("W-x-M", {"max_mismatch": 2}, ValueError, "2 positions other than x"),
    ("W-M", {"max_mismatch": -1}, ValueError, "max_mismatch -1"),
    ("x-x", {}, ValueError, "max_mismatch 0"),
    ("W-B", {}, ValueError, "'B'"),
    (np.zeros((0, 21), dtype=np.int64), {"threshold": 1}, ValueError, "0 rows"),
    (np.ones((65, 21), dtype=np.int64), {"threshold": 1}, ValueError, "65 rows"),
    ([[0, 1, 2, 3]], {"threshold": 1}, ValueError, "rows of 21"),
    (np.full((1, 21), 32768), {"threshold": 1}, ValueError, "row 1: weight 32768"),
    (np.full((1, 21), 0.5), {"threshold": 1}, TypeError, "integers"),
    (b"WM", {"threshold": 1}, TypeError, "Invalid"),
    (None, {"threshold": 1}, TypeError, "Invalid"),
])
def test_argument_checks_come_first(profile, kw, exc, text):
    for subject in (b"ACGTACGT", "no_such_file.fasta"):
        with pytest.raises(exc) as ei:
            api.protMatch(profile, subject, ctx=NoDevice(), **kw)
        assert text in str(ei.value), str(ei.value)
    with pytest.raises(exc):
        api.protMatch_batch([OKP, profile], "no_such_file.fasta", ctx=NoDevice(), **kw)


def test_batch_needs_one_threshold_per_profile_and_a_subject():
    with pytest.raises(ValueError):
        api.protMatch_batch([OKP, OKP], "x.fasta", threshold=[1], ctx=NoDevice())
    with pytest.raises(ValueError):
        api.protMatch_batch(["W-M", "W-M"], "x.fasta", max_mismatch=[0], ctx=NoDevice())
    with pytest.raises(TypeError):
        api.protMatch_batch([OKP], 17, threshold=1, ctx=NoDevice())


# ---- the library's surface -------------------------------------------------------------------------------------------------------
def header_text() -> str:
    with open(os.path.join(ROOT, "include", "kgma.h")) as f:
        return f.read()


def header_fields(name: str) -> list:
    """[(c type, field)] of a struct of include/kgma.h, comments removed, `a, b` declarations split."""
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} " + name + ";", header_text()).group(1), flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            out += [(ctype, n.strip()) for n in names.split(",")]
    return out


@pytest.mark.parametrize("name, mirror, size", [("kgma_codon_hit", _lib.KgmaCodonHit, 24), ("kgma_codon_stats", _lib.KgmaCodonStats, 40)])
def test_struct_mirrors_follow_the_header(name, mirror, size):
    ctypes_of = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    assert [(n, t) for n, t in mirror._fields_] == [(n, ctypes_of[t]) for t, n in header_fields(name)]
    assert C.sizeof(mirror) == size
    off = 0
    for n, t in mirror._fields_:                                               # (natural alignment, no holes)
        assert getattr(mirror, n).offset == off
        off += C.sizeof(t)
    if name == "kgma_codon_hit":
        assert [n for n, _ in mirror._fields_] == ["matrix", "contig", "start", "score", "reserved"]
        assert _lib.CODON_HIT_DTYPE.itemsize == size and list(_lib.CODON_HIT_DTYPE.names) == [n for n, _ in mirror._fields_]
        assert [_lib.CODON_HIT_DTYPE.fields[n][1] for n, _ in mirror._fields_] == [getattr(mirror, n).offset for n, _ in mirror._fields_]


def test_symbols_are_in_the_header_and_exported():
    text = header_text()
    lib = C.CDLL(_lib.LIB_PATH)                                                # (loading needs no device)
    for name in ("kgma_codon_match", "kgma_get_codon_matches", "kgma_get_codon_stats", "kgma_codon_fold"):
        assert re.search(r"\bint " + name + r"\(", text) and name in _lib.EXPORTS and hasattr(lib, name), name
    for macro, value in (("KGMA_CODON_ENTRIES", _lib.CODON_ENTRIES), ("KGMA_CODON_MAX_ROWS", _lib.CODON_MAX_ROWS),
                         ("KGMA_CODON_AA_COLUMNS", _lib.CODON_AA_COLUMNS)):
        assert re.search(r"#define " + macro + r" " + str(value) + r"\b", text), macro
    assert (_lib.CODON_ENTRIES, _lib.CODON_MAX_ROWS, _lib.CODON_AA_COLUMNS, api.PROT_MAX_ROWS) == (65, 64, 21, 64)
    for name in ("protMatch", "protMatch_batch", "prot_pattern", "prot_matrix_from_sequences", "prot_threshold", "prot_score_distribution",
                 "prot_fold", "translate", "genetic_code"):
        assert callable(getattr(api, name))
    for name in ("codon_match", "codon_matches", "codon_stats"):
        assert callable(getattr(_lib.Context, name))
    assert callable(_lib.codon_fold)


# ---- the golden file -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_codon():
    with open(os.path.join(GOLDEN, "codon.json")) as f:
        return json.load(f)


def test_golden_file_holds_the_nine_hits_of_the_fixture(golden_codon, loci_records):
    g = golden_codon
    assert g["made_by"] == co.MADE_BY and g["genetic_code"] == co.TABLE1 == api.GENETIC_CODES[1]
    fr2 = g["patterns"]["fr2"]
    assert fr2["pattern"] == "W-[VIFY]-R-Q-[AVPS]-P-G-K" and fr2["threshold"] == 0
    plus = [(c, lo) for c, lo, hi, st, fr, k in fr2["hits"] if st == "+"]
    minus = [(c, lo) for c, lo, hi, st, fr, k in fr2["hits"] if st == "-"]
    assert plus == [(0, 8648), (0, 20530), (2, 790), (2, 12896), (3, 6957), (3, 24018), (3, 33950)]
    assert minus == [(0, 35652), (2, 28031)]
    assert all(hi - lo == 23 and k == 0 for c, lo, hi, st, fr, k in fr2["hits"])
    fr3 = g["patterns"]["fr3"]
    assert fr3["pattern"] == "[DE]-[TS]-[AG]-[VMIL]-Y-[YFH]-C" and [h[3] for h in fr3["hits"]].count("+") == 7 and len(fr3["hits"]) == 9
    # each fr3 site lies 3 * 54 (in two genes 3 * 53) residues behind its fr2 site on the gene's own strand, in the same frame
    for a, b in zip(fr2["hits"], fr3["hits"]):
        assert a[0] == b[0] and a[3] == b[3] and a[4] == b[4] and (b[1] - a[1] if a[3] == "+" else a[2] - b[2]) in (159, 162)
    # the oracle again, and the peptides under the hits
    assert co.make_golden(loci_records) == g
    for name, pat in (("fr2", co.FR2_PATTERN), ("fr3", co.FR3_PATTERN)):
        M = co.parse_pattern(pat)
        for c, lo, hi, st, fr, k in g["patterns"][name]["hits"]:
            site = loci_records[c][lo - 1:hi]
            pep = api.translate(site if st == "+" else co.revcomp_text(site))
            assert len(pep) == len(M) and all(M[i, co.AMINO_ACIDS.index(a)] == 0 for i, a in enumerate(pep)), (name, c, lo, pep)
            L = len(loci_records[c])
            assert fr == ((lo - 1) % 3 + 1 if st == "+" else -((L - hi) % 3 + 1))
