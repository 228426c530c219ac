"""Host-side checks of the position-weight-matrix search (no GPU): the oracle's two statements against each other, the host
mathematics around a matrix (api.pwm_from_sequences, pwm_threshold, pwm_revcomp, pwm_from_motif) against values worked out by hand
and by brute force, the motif equivalence on the fixture, that every case list hits what it is for, that every argument check is
made before a context is touched, the library's surface and the golden file."""
import ctypes as C
import itertools
import json
import math
import os
import re

import numpy as np
import pytest

from kmergma_amd import _lib, api
from tests import motif_oracle as mo
from tests import pwm_cases as pc
from tests import pwm_oracle as po
from tests.conftest import DATA, GOLDEN, ROOT

LOCI = os.path.join(DATA, "Loci.fasta")


@pytest.fixture(scope="module")
def loci_records():
    return po.read_fasta_sequences(LOCI)


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 5, 31, 39, 64])
def test_the_two_statements_agree(m):
    rng = np.random.default_rng(m)
    W = pc.rand_matrix(rng, m, constant=(1,) if m > 2 else ())
    for n in (0, m - 1, m, m + 1, 700):
        t = bytearray(pc.rand_dna(rng, n))
        for i in rng.integers(0, max(n, 1), size=n // 10):
            t[i] = ord("N")
        t = bytes(t[:n // 2]).lower() + bytes(t[n // 2:])
        a, b = po.profile_rows(W, t), po.profile_gather(W, t)
        assert a.dtype == b.dtype == np.int64 and a.size == max(0, n - m + 1) and np.array_equal(a, b)


def test_scores_by_hand():
    W = [[1, 2, 3, 4], [10, 20, 30, 40], [-5, 0, 5, -7]]
    assert po.profile_rows(W, b"ACGT").tolist() == [1 + 20 + 5, 2 + 30 - 7]
    assert po.profile_rows(W, b"nNn").tolist() == [1 + 10 - 7]                # N: the row minima
    assert po.profile_rows(W, b"tNa").tolist() == [4 + 10 - 5]
    # ACG 1 + 20 + 5, CGT 2 + 30 - 7, GTA 3 + 40 - 5, TAC 4 + 10 + 0, ACG
    assert po.profile_rows(W, b"ACGTACG").tolist() == [26, 25, 38, 14, 26]
    assert po.find(W, b"ACGTACG", 26) == [(1, 26), (3, 38), (5, 26)] and po.find(W, b"ACGTACG", 25) == [(1, 26), (2, 25), (3, 38), (5, 26)]
    assert (po.lowest(W), po.highest(W)) == (4, 49)
    with pytest.raises(ValueError):
        po.find(W, b"ACGT", 4)
    with pytest.raises(ValueError):
        po.find(W, b"ACXT", 5)
    assert po.match_list([W, W], [b"ACGT", b"CGT"], [26, 25]) == [(0, 0, 1, 26), (1, 0, 1, 26), (1, 0, 2, 25), (1, 1, 1, 25)]


# ---- api.pwm_from_sequences ------------------------------------------------------------------------------------------------------
def test_pwm_from_sequences_by_hand():
    # three sites, pseudocount 1, uniform background: frequency (count + 1/4) / 4, odds = 4 * frequency = count + 1/4
    W = api.pwm_from_sequences([b"ACG", "AcT", b"AGT"])
    cb = {0: round(100 * math.log2(0.25)), 1: round(100 * math.log2(1.25)), 2: round(100 * math.log2(2.25)), 3: round(100 * math.log2(3.25))}
    assert cb == {0: -200, 1: 32, 2: 117, 3: 170}
    assert W.dtype == np.int64 and W.tolist() == [[cb[3], cb[0], cb[0], cb[0]], [cb[0], cb[2], cb[1], cb[0]], [cb[0], cb[0], cb[1], cb[2]]]
    assert np.array_equal(W, po.from_sequences([b"ACG", b"ACT", b"AGT"]))
    # a skewed background and another scale: position 1, A: log2(((3 + 0.4) / 4) / 0.4), C: log2(((0 + 0.1) / 4) / 0.1) = -2
    V = api.pwm_from_sequences([b"ACG", b"ACT", b"AGT"], background=(.4, .1, .1, .4), scale=10)
    assert V[0].tolist() == [round(10 * math.log2(3.4 / 1.6)), -20, -20, -20]
    assert np.array_equal(V, po.from_sequences([b"ACG", b"ACT", b"AGT"], 1.0, (.4, .1, .1, .4), 10))


@pytest.mark.parametrize("seqs, kw, text", [
    ([], {}, "at least one"), ([b"ACG", b"AC"], {}, "differ in length"), ([b"ACN"], {}, "A, C, G and T only"),
    ([b"A" * 65], {}, "65 symbols"), ([b"ACG"], {"pseudocount": 0}, "row 1"), ([b"ACG"], {"scale": 1e6}, "row 1"),
    ([b"ACG"], {"background": (.5, .5, .5, .5)}, "background"), ([b"ACG"], {"background": (1, 0, 0, 0)}, "background")])
def test_pwm_from_sequences_refuses(seqs, kw, text):
    with pytest.raises(ValueError) as ei:
        api.pwm_from_sequences(seqs, **kw)
    assert text in str(ei.value)


# ---- api.pwm_threshold -----------------------------------------------------------------------------------------------------------
def brute_force(W, background):
    """[(score, probability)] of all 4^m sequences."""
    W = np.asarray(W)
    return [(sum(int(W[i, b]) for i, b in enumerate(seq)), math.prod(background[b] for b in seq))
            for seq in itertools.product(range(4), repeat=W.shape[0])]


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 6])
def test_pwm_threshold_uniform_background_is_exact(m):
    rng = np.random.default_rng(50 + m)
    W = rng.integers(-40, 41, size=(m, 4))
    if m == 4:
        W[2] = 7                                                               # a constant row
    all_ = brute_force(W, (.25,) * 4)
    lowest, p = api.pwm_score_distribution(W)
    assert lowest == po.lowest(W) and lowest + p.size - 1 == po.highest(W)
    counts = np.zeros(p.size, dtype=np.int64)
    for s, _ in all_:
        counts[s - lowest] += 1
    assert np.array_equal(p, counts / 4.0 ** m)                                # every probability is k / 4^m: exact
    for k in sorted({1, 2, 3, 4 ** m // 7, 4 ** m // 2, 4 ** m - 1}):
        if not 0 < k < 4 ** m:
            continue
        for pv in (k / 4.0 ** m, (k + 0.5) / 4.0 ** m):
            t = api.pwm_threshold(W, pv)
            assert sum(1 for s, _ in all_ if s >= t) <= pv * 4 ** m < sum(1 for s, _ in all_ if s >= t - 1), (k, pv, t)
            assert t == po.threshold(W, pv)


def test_pwm_threshold_skewed_background():
    rng = np.random.default_rng(60)
    W = rng.integers(-30, 31, size=(5, 4))
    bg = (.4, .1, .15, .35)
    all_ = brute_force(W, bg)
    lowest, p = api.pwm_score_distribution(W, bg)
    for k in range(p.size):
        assert math.isclose(p[k], math.fsum(q for s, q in all_ if s == lowest + k), rel_tol=1e-12, abs_tol=1e-300)
    assert math.isclose(p.sum(), 1.0, rel_tol=1e-12)
    scores = sorted({s for s, _ in all_}, reverse=True)
    tails = [math.fsum(q for s, q in all_ if s >= x) for x in scores]
    for i in (0, 1, 5, len(scores) // 2):
        pv = (tails[i] + tails[i + 1]) / 2                                     # between two attainable tails: no tie to break
        assert api.pwm_threshold(W, pv, bg) == scores[i + 1] + 1 == po.threshold(W, pv, bg)
    assert api.pwm_threshold(W, tails[0] / 2, bg) == scores[0] + 1             # rarer than the top score: one above it


def test_pwm_threshold_of_the_fixture_matrix(golden_pwm):
    W = np.array(golden_pwm["matrix"])
    for p, t in golden_pwm["thresholds"].items():
        assert api.pwm_threshold(W, float(p)) == t
    with pytest.raises(ValueError):
        api.pwm_threshold(W, 0)
    with pytest.raises(ValueError):
        api.pwm_threshold(W, 1)


# ---- api.pwm_revcomp -------------------------------------------------------------------------------------------------------------
def test_pwm_revcomp_mirrors_the_profile():
    rng = np.random.default_rng(70)
    for m in (1, 4, 9, 39):
        W = pc.rand_matrix(rng, m)
        R = api.pwm_revcomp(W)
        assert np.array_equal(R, po.revcomp_matrix(W)) and np.array_equal(api.pwm_revcomp(R), W)
        assert R[0].tolist() == W[-1][::-1].tolist()
        t = bytearray(pc.rand_dna(rng, 500))
        t[100:104] = b"NNnn"
        t = bytes(t)
        # the other strand's profile, read backwards, is the mirrored matrix's profile on the forward text
        assert np.array_equal(po.profile_rows(W, po.revcomp_text(t))[::-1], po.profile_rows(R, t))


# ---- the motif equivalence -------------------------------------------------------------------------------------------------------
def test_motif_equivalence_on_the_fixture(loci_records):
    W, informative = api.pwm_from_motif(api.HumanRSSD)
    assert informative == 16 and W.shape == (39, 4) and W[0].tolist() == [0, 1, 0, 0] and W[10].tolist() == [0, 0, 0, 0]
    W2, inf2 = po.from_motif(api.HumanRSSD)
    assert np.array_equal(W, W2) and inf2 == 16
    found = po.match_list([W], loci_records, [informative - 1])
    assert [(c, s, 16 - k) for _, c, s, k in found] == mo.LOCI_RSSD_D1
    assert [(c, s, informative - k) for _, c, s, k in found] == [(c, s, k) for _, c, s, k in mo.match_list([api.HumanRSSD], loci_records, 1)]


@pytest.mark.parametrize("motif, d", [(b"RYNNSW", 1), (b"ACGNNTKM", 2), (b"BDHVN", 0), (b"acgtRY", 3)])
def test_motif_equivalence_on_random_text(motif, d):
    rng = np.random.default_rng(80)
    t = bytearray(pc.rand_dna(rng, 4000))
    t[500:520] = b"N" * 20
    recs = [bytes(t), pc.rand_dna(rng, 300).lower()]
    W, informative = api.pwm_from_motif(motif)
    assert W.tolist() == po.from_motif(motif)[0].tolist()
    got = po.match_list([W], recs, [informative - d])
    want = mo.match_list([motif], recs, d)
    assert len(want) > 3 and [(i, c, s, informative - k) for i, c, s, k in got] == want


# ---- the case lists --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def searched():
    return [(c, po.match_list(c.matrices, c.records, c.thresholds)) for c in pc.host_cases()]


def test_case_names_are_unique(searched):
    names = [c.name for c, _ in searched]
    assert len(set(names)) == len(names) > 30


def test_every_case_hits_what_it_is_for(searched):
    for c, found in searched:
        at = {(i, r, s) for i, r, s, _ in found}
        assert all(h in at for h in c.aim.get("hits", [])), (c.name, [h for h in c.aim["hits"] if h not in at])
        assert not any(h in at for h in c.aim.get("absent", [])), c.name
        assert (found == []) == bool(c.aim.get("none")), (c.name, len(found))
        assert len(found) > c.aim.get("many", -1), (c.name, len(found))
        assert c.aim.get("hits") or c.aim.get("none") or "many" in c.aim, c.name
        assert all(len(W) <= 64 and t > po.lowest(W) for W, t in zip(c.matrices, c.thresholds)), c.name


def test_length_cases_cover_the_lengths():
    cases = pc.length_cases()
    assert [len(c.matrices[0]) for c in cases] == list(pc.LENGTHS)
    for c in cases:
        m = len(c.matrices[0])
        assert {len(r) for r in c.records} >= ({m - 1, m, m + 1} - {0})


def test_seam_cases_lie_on_the_seams(searched):
    lane, wave, wg = pc.HOST_GEOMETRY
    bounds = pc.seam_boundaries(lane, wave, wg)
    assert bounds["wave"] == wave and bounds["wg"] == wg and bounds["wg2"] == 2 * wg
    by_name = {c.name: (c, found) for c, found in searched}
    for name, B in bounds.items():
        c, found = by_name[f"{name}_seam"]
        m = len(c.matrices[0])
        starts0 = {s - 1 for _, _, s, k in found if k == po.highest(c.matrices[0])}
        assert starts0 >= set(range(max(0, B - m), B + 2)), name               # a top site begins at every offset -m ... +1
        last = [r for r in range(len(c.records)) if len(c.records[r]) == B + m]
        assert last and all((0, r, B + 1) in {(i, rr, s) for i, rr, s, _ in found} for r in last)
        assert max(len(r) for r in c.records) < B + 100


# ---- api.pwmMatch: the checks come before any device call ------------------------------------------------------------------------
class NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before the argument checks")


OK = [[0, 5, 0, 1], [3, 0, 0, 0]]


@pytest.mark.parametrize("matrix, kw, exc, text", [
    (OK, {}, ValueError, "exactly one"),
    (OK, {"threshold": 5, "pvalue": 0.1}, ValueError, "exactly one"),
    (OK, {"threshold": 0}, ValueError, "does not exceed the sum of its row minima, 0"),
    (OK, {"threshold": -3}, ValueError, "does not exceed"),
    (OK, {"threshold": 2 ** 31}, ValueError, "int32"),
    (OK, {"pvalue": 0}, ValueError, "pvalue"),
    (OK, {"pvalue": 1.5}, ValueError, "pvalue"),
    (OK, {"threshold": 5, "strand": "x"}, ValueError, ""),
    (np.zeros((0, 4), dtype=np.int64), {"threshold": 1}, ValueError, "0 rows"),
    (np.ones((65, 4), dtype=np.int64), {"threshold": 1}, ValueError, "65 rows"),
    ([[0, 1, 2]], {"threshold": 1}, ValueError, "rows of four"),
    ([0, 1, 2, 3], {"threshold": 1}, ValueError, "rows of four"),
    ([[0, 1, 2, 3], [0, 0, 32768, 0]], {"threshold": 1}, ValueError, "row 2: weight 32768"),
    ([[0, -32769, 2, 3]], {"threshold": 1}, ValueError, "row 1: weight -32769"),
    ([[0.5, 1, 2, 3]], {"threshold": 1}, TypeError, "integers"),
    (b"ACGT", {"threshold": 1}, TypeError, "Invalid"),
    (None, {"threshold": 1}, TypeError, "Invalid"),
])
def test_argument_checks_come_first(matrix, kw, exc, text):
    for subject in (b"ACGTACGT", "no_such_file.fasta"):
        with pytest.raises(exc) as ei:
            api.pwmMatch(matrix, subject, ctx=NoDevice(), **kw)
        assert text in str(ei.value)
    with pytest.raises(exc) as ei:
        api.pwmMatch_batch([OK, matrix], "no_such_file.fasta", ctx=NoDevice(), **kw)
    if text.startswith("row ") or text.endswith(" rows"):
        assert "matrix 1" in str(ei.value)                                     # matrix and row are named


def test_batch_needs_one_threshold_per_matrix_and_a_subject():
    with pytest.raises(ValueError):
        api.pwmMatch_batch([OK, OK], "x.fasta", threshold=[1], ctx=NoDevice())
    with pytest.raises(ValueError):
        api.pwmMatch_batch([OK, OK], "x.fasta", pvalue=[.1, .1, .1], ctx=NoDevice())
    with pytest.raises(TypeError):
        api.pwmMatch_batch([OK], 17, threshold=1, ctx=NoDevice())
    with pytest.raises(ValueError) as ei:
        api.findRSS_pwm("x.fasta", [b"ACGT", b"ACG"], ctx=NoDevice())
    assert "differ in length" in str(ei.value)
    with pytest.raises(ValueError):
        api.findRSS_pwm("x.fasta", OK, pvalue=2, ctx=NoDevice())
    with pytest.raises(ValueError):
        api.findRSS_pwm("x.fasta", OK, strand="?", ctx=NoDevice())


# ---- the library's surface -------------------------------------------------------------------------------------------------------
def header_fields(name: str) -> list:
    """[(c type, field)] of a struct of include/kgma.h, comments removed, `a, b` declarations split."""
    with open(os.path.join(ROOT, "include", "kgma.h")) as f:
        text = f.read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} " + name + ";", text).group(1), flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            out += [(ctype, n.strip()) for n in names.split(",")]
    return out


@pytest.mark.parametrize("name, mirror, size", [("kgma_pwm_hit", _lib.KgmaPwmHit, 24), ("kgma_pwm_stats", _lib.KgmaPwmStats, 40)])
def test_struct_mirrors_follow_the_header(name, mirror, size):
    ctypes_of = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    assert [(n, t) for n, t in mirror._fields_] == [(n, ctypes_of[t]) for t, n in header_fields(name)]
    assert C.sizeof(mirror) == size
    off = 0
    for n, t in mirror._fields_:                                               # (natural alignment, no holes)
        assert getattr(mirror, n).offset == off
        off += C.sizeof(t)
    if name == "kgma_pwm_hit":
        assert _lib.PWM_HIT_DTYPE.itemsize == size and list(_lib.PWM_HIT_DTYPE.names) == [n for n, _ in mirror._fields_]
        assert [_lib.PWM_HIT_DTYPE.fields[n][1] for n, _ in mirror._fields_] == [getattr(mirror, n).offset for n, _ in mirror._fields_]


def test_symbols_are_in_the_header_and_exported():
    with open(os.path.join(ROOT, "include", "kgma.h")) as f:
        text = f.read()
    lib = C.CDLL(_lib.LIB_PATH)                                                # (loading needs no device)
    for name in ("kgma_pwm_match", "kgma_get_pwm_matches", "kgma_get_pwm_stats"):
        assert re.search(r"\bint " + name + r"\(", text) and name in _lib.EXPORTS and hasattr(lib, name), name
    for name in ("pwmMatch", "pwmMatch_batch", "findRSS_pwm", "pwm_from_sequences", "pwm_from_motif", "pwm_revcomp", "pwm_threshold"):
        assert callable(getattr(api, name))
    for name in ("pwm_match", "pwm_matches", "pwm_stats"):
        assert callable(getattr(_lib.Context, name))


# ---- the golden file -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_pwm():
    with open(os.path.join(GOLDEN, "pwm.json")) as f:
        return json.load(f)


def test_golden_file_holds_what_was_recorded(golden_pwm, loci_records):
    g = golden_pwm
    assert g["made_by"] == po.MADE_BY and sorted(g["thresholds"]) == sorted(po.GOLDEN_PVALUES)
    assert g["sites"] == [s.decode() for s in po.loci_sites(loci_records)] and all(s.startswith("CAC") and len(s) == 39 for s in g["sites"])
    assert g["matrix"] == api.pwm_from_sequences(g["sites"]).tolist()
    assert (g["lowest"], g["highest"]) == (-11700, 6907)
    hits = g["hits"]["1e-6"]
    plus = [(c, lo, k) for c, lo, hi, st, k in hits if st == "+"]
    # the seven sites the matrix was made from, 6468 ... 6868; one more on the plus strand, in record 3; three on the minus
    # strand, one in each of the records 0, 2 and 3
    seven = [(c, s) for c, s, _ in mo.LOCI_RSSD_D1]
    assert [(c, lo) for c, lo, k in plus if (c, lo) in seven] == seven
    assert sorted(k for c, lo, k in plus if (c, lo) in seven)[::6] == [6468, 6868]
    assert [c for c, lo, k in plus if (c, lo) not in seven] == [3]
    assert [c for c, lo, hi, st, k in hits if st == "-"] == [0, 2, 3]
    assert all(hi - lo == 38 and k >= g["thresholds"]["1e-6"] for c, lo, hi, st, k in hits)
    assert len(g["hits"]["1e-4"]) > len(hits) >= len(g["hits"]["1e-8"]) >= 7


def test_golden_file_is_rederived_for_record_2(golden_pwm, loci_records):
    again = po.make_golden(loci_records, only_record=2)
    assert again["matrix"] == golden_pwm["matrix"] and again["thresholds"] == golden_pwm["thresholds"]
    for p in po.GOLDEN_PVALUES:
        assert again["hits"][p] == [h for h in golden_pwm["hits"][p] if h[0] == 2]
    assert len(again["hits"]["1e-6"]) == 3
