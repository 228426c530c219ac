"""Codon-weight-matrix search on the device (kgma_codon_match / api.protMatch) against the numpy oracle (tests/codon_oracle.py).

Every comparison is of the COMPLETE sorted list -- (matrix, record, start, score) -- with the oracle's: the lengths and the record
sizes around 3m, the seams of the kernel's lanes, waves and workgroups in all three frames (read from kgma_get_codon_stats), the
alphabet, the ends of the score range, a batch on both strands, a result that outgrows the device buffer, the position-weight-
matrix kernel on the same text, the fixture, state and errors."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from kmergma_amd import _lib, api
from tests import codon_cases as cc
from tests import codon_oracle as co
from tests import twobit_ref as tb
from tests.conftest import DATA, GOLDEN

pytestmark = pytest.mark.gpu
LOCI = os.path.join(DATA, "Loci.fasta")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)          # no references are ever set on this context: the search needs none
    yield c
    c.close()


def one_hot(*codons) -> np.ndarray:
    """A row per codon: 1 for it, 0 for every other entry."""
    W = np.zeros((len(codons), 65), dtype=np.int64)
    for i, c in enumerate(codons):
        W[i, co.codon_index(c)] = 1
    return W


@pytest.fixture(scope="module")
def geometry(ctx):
    """(lane_starts, wave_starts, wg_starts) of the kernel, as the library reports them after a first call."""
    g = ctx.genome_from_host([b"ATGTGGCATGTGG"])
    try:
        ctx.codon_match(g, [one_hot(b"ATG", b"TGG")], [2])
        st = ctx.codon_stats()
    finally:
        g.free()
    assert hits(ctx) == [(0, 0, 1, 2), (0, 0, 8, 2)] and st["n_hits"] == st["n_candidates"] == 2 and st["n_launches"] == 1
    assert st["lane_starts"] >= 1 and st["wave_starts"] % (64 * st["lane_starts"]) == 0 and st["wg_starts"] % st["wave_starts"] == 0
    return st["lane_starts"], st["wave_starts"], st["wg_starts"]


def hits(ctx):
    m = ctx.codon_matches()
    return list(zip(m["matrix"].tolist(), m["contig"].tolist(), m["start"].tolist(), m["score"].tolist()))


def device_list(ctx, records, matrices, thresholds):
    g = ctx.genome_from_host(records)
    try:
        ctx.codon_match(g, matrices, thresholds)
        return hits(ctx)
    finally:
        g.free()


def check(ctx, records, matrices, thresholds):
    got = device_list(ctx, records, matrices, thresholds)
    want = co.match_list(matrices, records, thresholds)
    assert len(got) == len(want) and got == want, (len(got), len(want), [x for x in zip(got, want) if x[0] != x[1]][:3])
    return want


def check_case(ctx, c):
    want = check(ctx, c.records, c.matrices, c.thresholds)
    at = {(i, r, s) for i, r, s, _ in want}
    assert all(h in at for h in c.aim.get("hits", [])) and not any(h in at for h in c.aim.get("absent", [])), c.name
    assert (want == []) == bool(c.aim.get("none")) and len(want) > c.aim.get("many", -1), c.name
    return want


# ---- lengths ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.length_cases() + [cc.tiny_records_case()] + cc.empty_cases(), ids=lambda c: c.name)
def test_lengths_and_records(ctx, case):
    check_case(ctx, case)
    st = ctx.codon_stats()
    assert st["n_launches"] <= 1                               # (none at all when no start can reach the threshold)


# ---- seams -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lane", "row", "wave", "wg", "wg2"])
def test_seams(ctx, geometry, kind):
    (case,) = [c for c in cc.seam_cases(*geometry) if c.name == f"{kind}_seam"]
    B = cc.seam_boundaries(*geometry)[kind]
    want = check_case(ctx, case)
    m, top = len(case.matrices[0]), co.highest(case.matrices[0])
    assert {s - 1 for _, _, s, k in want if k == top} >= set(range(max(0, B - 3 * m), B + 4))      # all three frames, on both sides


# ---- arithmetic, alphabet --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.arithmetic_cases() + cc.alphabet_cases(), ids=lambda c: c.name)
def test_arithmetic_and_alphabet(ctx, case):
    check_case(ctx, case)


def test_soft_masked_2bit_genome(ctx, tmp_path):
    rng = np.random.default_rng(21)
    P = cc.rand_profile(rng, 10)
    W = api.prot_fold(P)
    site = cc.best_site(W)
    recs = []
    for n in (700, 3000):
        t = bytearray(cc.rand_dna(rng, n))
        cc.plant(t, 370, site)
        cc.plant(t, 570, site)
        t[380:390] = bytes(t[380:390]).lower()                # the mask begins inside the first site
        t[500:620] = bytes(t[500:620]).lower()
        t[100:130] = b"N" * 30
        recs.append(bytes(t))
    p = tmp_path / "masked.2bit"
    tb.write_twobit(p, [(f"r{i}", r) for i, r in enumerate(recs)])
    g = ctx.genome_from_2bit(str(p))
    thr = co.highest(W) - 300
    try:
        assert [g.fetch(c, 1, len(r)) for c, r in enumerate(recs)] == recs          # lower case and N as written
        ctx.codon_match(g, [W], [thr])
        got = hits(ctx)
    finally:
        g.free()
    want = co.match_list([W], recs, [thr])
    assert got == want and {(c, s) for _, c, s, k in want if k == co.highest(W)} == {(0, 371), (0, 571), (1, 371), (1, 571)}
    found = api.protMatch(P, str(p), threshold=thr, ctx=ctx)
    assert found == [(c, f"r{c}", s, s + 29, "+", (s - 1) % 3 + 1, k) for _, c, s, k in want]
    assert {fr for c, _, lo, hi, st, fr, k in found if k == co.highest(W)} == {2, 1}


# ---- batch -----------------------------------------------------------------------------------------------------------------------
def test_batch_of_eight_on_both_strands_in_one_launch(ctx):
    c, profs = cc.batch_case()
    g = ctx.genome_from_host(c.records)
    try:
        ctx.codon_match(g, c.matrices, c.thresholds)
        got, st = hits(ctx), ctx.codon_stats()
        singles = []
        for i in range(16):
            ctx.codon_match(g, c.matrices[i:i + 1], c.thresholds[i:i + 1])
            singles += [(i, r, s, k) for _, r, s, k in hits(ctx)]
            assert ctx.codon_stats()["n_launches"] == st["n_launches"] == 1
        want = co.match_list(c.matrices, c.records, c.thresholds)
        assert got == want == singles and st["n_hits"] == st["n_candidates"] == len(want)
        assert all(h in {(i, r, s) for i, r, s, _ in want} for h in c.aim["hits"])
        # the same through the API: eight profiles, both strands, one launch
    finally:
        g.free()
    g = ctx.genome_from_fasta(b"".join(b">rec%d\n%s\n" % (r, t) for r, t in enumerate(c.records)))
    try:
        res = api.protMatch_batch(profs, g, threshold=c.thresholds[::2], strand="both", ctx=ctx)
        assert ctx.codon_stats()["n_launches"] == 1 and ctx.codon_stats()["n_hits"] == len(want)
        for P, t, lst in zip(profs, c.thresholds[::2], res):
            assert [(r, lo, hi, s, fr, k) for r, _, lo, hi, s, fr, k in lst] == co.api_list(P, c.records, t, "both")
            assert all(ident == f"rec{r}" for r, ident, *_ in lst)
    finally:
        g.free()


# ---- volume ----------------------------------------------------------------------------------------------------------------------
def test_result_outgrows_the_buffer():
    c = _lib.Context(0)                                      # a context whose hit buffer has its initial size
    try:
        text = cc.rand_dna(np.random.default_rng(5), 100_000)
        W = np.zeros((1, 65), dtype=np.int64)
        W[0, :48] = 1                                        # every codon that does not begin with T
        g = c.genome_from_host([text])
        c.codon_match(g, [W], [1])
        got, st, st0 = hits(c), c.codon_stats(), c.stats()
        want = co.match_list([W], [text], [1])
        assert 70_000 < len(want) == 99_998 - text[:-2].count(b"T") and len(want) > 65_536 and got == want
        assert st["n_launches"] == 2 and st["n_hits"] == len(want)                                    # counted, regrown, run again
        assert st0["n_launches"] == 2 and st0["bases_scanned"] == 100_000 and st0["scan_ms"] > 0
        c.codon_match(g, [W], [1])
        assert hits(c) == want and c.codon_stats()["n_launches"] == 1                                 # the buffer is kept
        small = one_hot(b"TTT", b"TTT")
        c.codon_match(g, [small], [2])                        # then a small call
        assert hits(c) == co.match_list([small], [text], [2]) and c.codon_stats()["n_launches"] == 1
        g.free()
    finally:
        c.close()


# ---- the family ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 7, 21])
def test_three_rows_of_a_position_weight_matrix_are_one_codon_row(ctx, m):
    """On an N-free text the codon matrix row_i[c] = W[3i][b0] + W[3i + 1][b1] + W[3i + 2][b2] finds kgma_pwm_match's hits of the
    3m-row matrix W, start for start and score for score."""
    rng = np.random.default_rng(500 + m)
    W = rng.integers(-300, 300, size=(3 * m, 4)).astype(np.int64)
    W[np.arange(3 * m), rng.integers(0, 4, size=3 * m)] = 320
    if m > 1:
        W[4] = 17                                            # a constant row inside a codon
    text = [bytearray(cc.rand_dna(rng, 20_000)), bytearray(cc.rand_dna(rng, 3 * m + 1).lower())]
    best = cc.BASES[W.argmax(axis=1)].tobytes()
    cc.plant(text[0], 8190, best)
    cc.plant(text[1], 1, best.lower())
    text = [bytes(t) for t in text]
    thr = int(W.max(axis=1).sum()) - (0 if m == 1 else 500)
    g = ctx.genome_from_host(text)
    try:
        ctx.pwm_match(g, [W], [thr])
        pw = ctx.pwm_matches()
        pw = list(zip(pw["matrix"].tolist(), pw["contig"].tolist(), pw["start"].tolist(), pw["score"].tolist()))
        ctx.codon_match(g, [cc.codon_matrix_of_pwm(W)], [thr])
        got = hits(ctx)
    finally:
        g.free()
    assert got == pw and (0, 0, 8191, int(W.max(axis=1).sum())) in got and (0, 1, 2, int(W.max(axis=1).sum())) in got
    assert got == co.match_list([cc.codon_matrix_of_pwm(W)], text, [thr])


def test_stop_free_stretches(ctx):
    """Rows 0 for every amino acid and -1 for the stop, at threshold 0: every stretch of m codons without a stop, per frame."""
    rng = np.random.default_rng(61)
    t = cc.rand_dna(rng, 3000)
    m = 30
    P = np.zeros((m, 21), dtype=np.int64)
    P[:, 20] = -1
    got = api.protMatch(P, t, threshold=0, strand="both", ctx=ctx)
    assert got == [(lo, hi, st, fr, k) for _, lo, hi, st, fr, k in co.api_list(P, [t], 0, "both")] and len(got) > 20
    for lo, hi, st, fr, k in got:
        pep = api.translate(t[lo - 1:hi], 1 if st == "+" else -1)
        assert len(pep) == m and "*" not in pep and k == 0
    assert {fr for *_, fr, _ in got} == {1, 2, 3, -1, -2, -3}


# ---- strands, patterns -----------------------------------------------------------------------------------------------------------
def test_pattern_on_both_strands(ctx):
    rng = np.random.default_rng(41)
    pat = "W-[VIFY]-x(2)-{P}-*"
    pep_dna = b"TGG" + b"ATT" + b"CCC" + b"GGG" + b"AAA" + b"TAG"          # W I P G K *
    near = b"TGG" + b"CTT" + b"CCC" + b"GGG" + b"AAA" + b"TAG"             # W L ...: one mismatch
    recs = [bytearray(cc.rand_dna(rng, 2000)), bytearray(cc.rand_dna(rng, 901))]
    cc.plant(recs[0], 500, pep_dna)
    cc.plant(recs[0], 1501, co.revcomp_text(pep_dna))
    cc.plant(recs[0], 1000, near)
    cc.plant(recs[1], 300, co.revcomp_text(pep_dna))
    cc.plant(recs[1], 600, pep_dna[:13] + b"N" + pep_dna[14:])             # AAA -> ANA: X scores the minimum of the {P} row, a mismatch
    recs = [bytes(r) for r in recs]
    M = co.parse_pattern(pat)
    g = ctx.genome_from_fasta(b"".join(b">rec%d of two\n%s\n" % (c, r) for c, r in enumerate(recs)))
    try:
        got = {(st, d): api.protMatch_batch([pat], g, max_mismatch=d, strand=st, ctx=ctx)[0] for st in ("+", "-", "both") for d in (0, 1)}
        default = api.protMatch(pat, g, ctx=ctx)
    finally:
        g.free()
    for (st, d), lst in got.items():
        assert [(c, lo, hi, s, fr, k) for c, _, lo, hi, s, fr, k in lst] == co.api_list(M, recs, -d, st), (st, d)
        assert all(ident == f"rec{c}" for c, ident, *_ in lst)
    assert default == got[("+", 0)]
    exact = {(c, lo, s, fr) for c, _, lo, hi, s, fr, k in got[("both", 0)]}
    assert exact >= {(0, 501, "+", 3), (0, 1502, "-", -((2000 - 1519) % 3 + 1)), (1, 301, "-", -((901 - 318) % 3 + 1))}
    one = {(c, lo, s, k) for c, _, lo, hi, s, fr, k in got[("+", 1)]}
    assert (0, 1001, "+", -1) in one and (1, 601, "+", -1) in one and (0, 1001) not in {(c, lo) for c, lo, *_ in exact}
    assert got[("both", 1)] == sorted(got[("+", 1)] + got[("-", 1)], key=lambda t: (t[0], t[2], t[4]))
    short = api.protMatch(pat, recs[1], max_mismatch=1, strand="both", ctx=ctx)
    assert short == [(lo, hi, s, fr, k) for c, lo, hi, s, fr, k in co.api_list(M, recs[1:], -1, "both")]


# ---- the fixture -----------------------------------------------------------------------------------------------------------------
def test_patterns_on_the_fixture_equal_the_golden_file(ctx, loci):
    with open(os.path.join(GOLDEN, "codon.json")) as f:
        gold = json.load(f)
    ids = [r.identifier for r in loci]
    for name in ("fr2", "fr3"):
        p = gold["patterns"][name]
        found = api.protMatch(p["pattern"], LOCI, strand="both", ctx=ctx)
        assert [[c, lo, hi, st, fr, k] for c, _, lo, hi, st, fr, k in found] == p["hits"] and len(found) == 9
        assert all(i == ids[c] for c, i, *_ in found)
        plus = api.protMatch(p["pattern"], LOCI, max_mismatch=0, ctx=ctx)
        assert plus == [h for h in found if h[4] == "+"] and len(plus) == 7
    fr2 = api.protMatch(co.FR2_PATTERN, LOCI, strand="both", threshold=0, ctx=ctx)
    assert [(c, lo) for c, _, lo, hi, st, *_ in fr2 if st == "+"] == [(0, 8648), (0, 20530), (2, 790), (2, 12896), (3, 6957), (3, 24018), (3, 33950)]
    assert [(c, lo) for c, _, lo, hi, st, *_ in fr2 if st == "-"] == [(0, 35652), (2, 28031)]
    # a p-value in place of the mismatch count: the exact pattern is far rarer than 1e-9 per start
    assert api.protMatch(co.FR2_PATTERN, LOCI, strand="both", pvalue=1e-9, ctx=ctx) == fr2
    bg = api.protMatch(api.prot_pattern(co.FR2_PATTERN)[0], LOCI, strand="both", pvalue=1e-9, background="genome", ctx=ctx)
    assert bg == fr2


# ---- state and errors ------------------------------------------------------------------------------------------------------------
def test_scan_and_the_other_searches_survive(alp_ref, loci):
    c = _lib.Context(0)
    try:
        assert hits(c) == []                                 # before any call
        seqs = [r.sequence for r in loci]
        c.set_refs(6, [alp_ref["RV"]], [alp_ref["ws"]], [30.0], [alp_ref["N"]])
        g = c.genome_from_host(seqs)
        c.scan(g, _lib.MODE_SINGLE, 50, 0, _lib.F_RETURN_DISTS, None)
        found, dips, d = c.hits(), c.dips(), c.dists(1)
        c.exact_match(g, [seqs[0][1000:1040], b"AAATT"])
        ex = c.matches().copy()
        c.motif_match(g, [api.HumanRSSD], [1])
        mm = c.motif_matches().copy()
        c.approx_match(g, [api.HumanRSSD], [1], True)
        ap = c.approx_matches().copy()
        W, inf = api.pwm_from_motif(api.HumanRSSD)
        c.pwm_match(g, [W], [inf - 1])
        pw = c.pwm_matches().copy()
        assert len(found) > 0 and ex.size > 0 and mm.size == 7 and ap.size == 7 and pw.size == 7
        c.codon_match(g, [api.prot_fold(api.prot_pattern(co.FR2_PATTERN)[0])], [0])
        assert [(r, s) for _, r, s, k in hits(c)] == [(0, 8648), (0, 20530), (2, 790), (2, 12896), (3, 6957), (3, 24018), (3, 33950)]
        assert c.hits() == found and c.dips() == dips and np.array_equal(c.dists(1), d)
        assert np.array_equal(c.matches(), ex) and np.array_equal(c.motif_matches(), mm) and np.array_equal(c.approx_matches(), ap)
        assert np.array_equal(c.pwm_matches(), pw)
        st = c.stats()
        assert st["bases_scanned"] == sum(len(s) for s in seqs) and st["n_launches"] == 1 and st["scan_ms"] > 0
        g.free()
    finally:
        c.close()


def test_bad_genome_residue(ctx):
    W = one_hot(b"ACG", b"TAC")
    g = ctx.genome_from_host([b"ACGTACGT", b"ACGTXACGT", b"ACGT"])
    try:
        ok = ctx.genome_from_host([b"ACGTACGTAC"])
        ctx.codon_match(ok, [W], [2])
        ok.free()
        assert hits(ctx) == [(0, 0, 1, 2), (0, 0, 5, 2)]
        with pytest.raises(_lib.BadBaseError) as ei:
            ctx.codon_match(g, [W], [2])
        assert ei.value.status == _lib.KGMA_E_BADBASE and "record 1" in ei.value.message and "residue 5" in ei.value.message
        assert hits(ctx) == []                               # a failed call leaves no hits of the call before it
        with pytest.raises(_lib.KgmaError):
            api.protMatch("T-Y", g, ctx=ctx)
    finally:
        g.free()


def test_argument_errors_through_the_c_abi(ctx):
    W = one_hot(b"ACG", b"TAC")
    g = ctx.genome_from_host([b"ACGTACGTACNN"])
    try:
        for mats, thr, text in (([np.zeros((0, 65), dtype=np.int64)], [1], "matrix 0 has 0 rows"), ([np.ones((65, 65), dtype=np.int64)], [70], "65 rows"),
                                ([W, np.zeros((0, 65), dtype=np.int64)], [2, 1], "matrix 1 has 0 rows"), ([W], [0], "threshold 0 does not exceed"),
                                ([W], [-5], "threshold -5"), ([W, W], [2, 0], "matrix 1: threshold 0"),
                                ([np.full((64, 65), -32768)], [64 * -32768], "row minima, -2097152")):
            with pytest.raises(_lib.KgmaError) as ei:
                ctx.codon_match(g, mats, thr)
            assert ei.value.status == _lib.KGMA_E_ARG and text in ei.value.message and "matrix" in ei.value.message, (thr, ei.value.message)
        ctx.codon_match(g, [W], [2])
        assert hits(ctx) == [(0, 0, 1, 2), (0, 0, 5, 2)]
        with pytest.raises(_lib.KgmaError):
            ctx.codon_match(g, [W, W], [2, 0])
        assert hits(ctx) == []                               # a failed call leaves no hits of the call before it
        # null pointers
        L = _lib.load()
        off, thr = (C.c_int64 * 2)(0, 2), (C.c_int32 * 1)(2)
        w = (C.c_int16 * 130)(*np.array(W).ravel().tolist())
        ctx.codon_match(g, [W], [2])
        for args in ((None, off, 1, thr), (w, None, 1, thr), (w, off, 1, None), (w, off, -1, thr)):
            assert L.kgma_codon_match(ctx._h, g._h, *args) == _lib.KGMA_E_ARG
            assert hits(ctx) == []
        assert L.kgma_codon_match(ctx._h, None, w, off, 1, thr) == _lib.KGMA_E_ARG and L.kgma_codon_match(None, g._h, w, off, 1, thr) == _lib.KGMA_E_ARG
        assert L.kgma_get_codon_stats(ctx._h, None) == _lib.KGMA_E_ARG and L.kgma_get_codon_matches(ctx._h, None, 0, None) == _lib.KGMA_E_ARG
        assert L.kgma_get_codon_stats(None, None) == _lib.KGMA_E_ARG and L.kgma_get_codon_matches(None, None, 0, None) == _lib.KGMA_E_ARG
        assert L.kgma_codon_match(ctx._h, g._h, w, off, 1, thr) == 0
        buf, n = (_lib.KgmaCodonHit * 1)(), C.c_int64(0)
        assert L.kgma_get_codon_matches(ctx._h, buf, 1, C.byref(n)) == _lib.KGMA_E_ARG and n.value == 2   # too small a buffer
        # the context is still usable; the ambiguous entry is a weight of its own: ACN and CNN score it, NN has no third residue
        V = np.zeros((1, 65), dtype=np.int64)
        V[0, 64] = 4
        ctx.codon_match(g, [W, V], [2, 4])
        assert hits(ctx) == [(0, 0, 1, 2), (0, 0, 5, 2), (1, 0, 9, 4), (1, 0, 10, 4)]
        ctx.codon_match(g, [], [])                           # no matrices: no hits
        assert hits(ctx) == []
        with pytest.raises(ValueError):
            ctx.codon_match(g, [np.full((1, 65), 40000)], [1])
        with pytest.raises(ValueError):
            ctx.codon_match(g, [np.zeros((1, 64), dtype=np.int64)], [1])
    finally:
        g.free()
