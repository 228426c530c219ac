"""Position-weight-matrix search on the device (kgma_pwm_match / api.pwmMatch / api.findRSS_pwm) against the numpy oracle
(tests/pwm_oracle.py).

Every comparison is of the COMPLETE sorted list -- (matrix, record, start, score) -- with the oracle's: the lengths at which the
host's fold and the pair tables change shape, the seams of the kernel's lanes, waves and workgroups (read from kgma_get_pwm_stats),
the ends of the score range, the alphabet, a batch, a result that outgrows the device buffer, motifMatch, strands, the fixture,
state and errors."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from kmergma_amd import _lib, api
from tests import motif_oracle as mo
from tests import pwm_cases as pc
from tests import pwm_oracle as po
from tests import twobit_ref as tb
from tests.conftest import DATA, GOLDEN

pytestmark = pytest.mark.gpu
LOCI = os.path.join(DATA, "Loci.fasta")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)          # no references are ever set on this context: the search needs none
    yield c
    c.close()


@pytest.fixture(scope="module")
def geometry(ctx):
    """(lane_starts, wave_starts, wg_starts) of the kernel, as the library reports them after a first call."""
    g = ctx.genome_from_host([b"ACGTACGT"])
    try:
        ctx.pwm_match(g, [[[1, 0, 0, 0], [0, 1, 0, 0]]], [2])
        st = ctx.pwm_stats()
    finally:
        g.free()
    assert hits(ctx) == [(0, 0, 1, 2), (0, 0, 5, 2)] and st["n_hits"] == st["n_candidates"] == 2 and st["n_launches"] == 1
    assert st["lane_starts"] >= 1 and st["wave_starts"] % (64 * st["lane_starts"]) == 0 and st["wg_starts"] % st["wave_starts"] == 0
    return st["lane_starts"], st["wave_starts"], st["wg_starts"]


def hits(ctx):
    m = ctx.pwm_matches()
    return list(zip(m["matrix"].tolist(), m["contig"].tolist(), m["start"].tolist(), m["score"].tolist()))


def device_list(ctx, records, matrices, thresholds):
    g = ctx.genome_from_host(records)
    try:
        ctx.pwm_match(g, matrices, thresholds)
        return hits(ctx)
    finally:
        g.free()


def check(ctx, records, matrices, thresholds):
    got = device_list(ctx, records, matrices, thresholds)
    want = po.match_list(matrices, records, thresholds)
    assert len(got) == len(want) and got == want, (len(got), len(want), [x for x in zip(got, want) if x[0] != x[1]][:3])
    return want


def check_case(ctx, c):
    want = check(ctx, c.records, c.matrices, c.thresholds)
    at = {(i, r, s) for i, r, s, _ in want}
    assert all(h in at for h in c.aim.get("hits", [])) and not any(h in at for h in c.aim.get("absent", [])), c.name
    assert (want == []) == bool(c.aim.get("none")) and len(want) > c.aim.get("many", -1), c.name
    return want


# ---- lengths ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.length_cases() + [pc.tiny_records_case()] + pc.empty_cases(), ids=lambda c: c.name)
def test_lengths_and_records(ctx, case):
    check_case(ctx, case)
    st = ctx.pwm_stats()
    assert st["n_launches"] <= 1                               # (none at all when no start can reach the threshold)


# ---- seams -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["word32", "word64", "lane", "wave", "wg", "wg2"])
def test_seams(ctx, geometry, kind):
    (case,) = [c for c in pc.seam_cases(*geometry) if c.name == f"{kind}_seam"]
    B = pc.seam_boundaries(*geometry)[kind]
    want = check_case(ctx, case)
    m, top = len(case.matrices[0]), po.highest(case.matrices[0])
    assert {s - 1 for _, _, s, k in want if k == top} >= set(range(max(0, B - m), B + 2))


# ---- arithmetic, alphabet --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.arithmetic_cases() + pc.alphabet_cases(), ids=lambda c: c.name)
def test_arithmetic_and_alphabet(ctx, case):
    check_case(ctx, case)


def test_soft_masked_2bit_genome(ctx, tmp_path):
    rng = np.random.default_rng(21)
    W = pc.rand_matrix(rng, 30, constant=(10, 11, 12))
    site = pc.best_site(W)
    recs = []
    for n in (700, 3000):
        t = bytearray(pc.rand_dna(rng, n))
        pc.plant(t, 370, site)
        pc.plant(t, 570, site)
        t[380:390] = bytes(t[380:390]).lower()                # the mask begins inside the first site
        t[500:620] = bytes(t[500:620]).lower()
        t[100:130] = b"N" * 30
        recs.append(bytes(t))
    p = tmp_path / "masked.2bit"
    tb.write_twobit(p, [(f"r{i}", r) for i, r in enumerate(recs)])
    g = ctx.genome_from_2bit(str(p))
    thr = po.highest(W) - 300
    try:
        assert [g.fetch(c, 1, len(r)) for c, r in enumerate(recs)] == recs          # lower case and N as written
        ctx.pwm_match(g, [W], [thr])
        got = hits(ctx)
    finally:
        g.free()
    want = po.match_list([W], recs, [thr])
    assert got == want and {(c, s) for _, c, s, k in want if k == po.highest(W)} == {(0, 371), (0, 571), (1, 371), (1, 571)}
    found = api.pwmMatch(W, str(p), threshold=thr, ctx=ctx)
    assert found == [(c, f"r{c}", s, s + 29, "+", k) for _, c, s, k in want]


# ---- batch -----------------------------------------------------------------------------------------------------------------------
def test_batch_of_eight_in_one_launch(ctx):
    c = pc.batch_case()
    g = ctx.genome_from_host(c.records)
    try:
        ctx.pwm_match(g, c.matrices, c.thresholds)
        got, st = hits(ctx), ctx.pwm_stats()
        singles = []
        for i in range(8):
            ctx.pwm_match(g, c.matrices[i:i + 1], c.thresholds[i:i + 1])
            singles += [(i, r, s, k) for _, r, s, k in hits(ctx)]
            assert ctx.pwm_stats()["n_launches"] == st["n_launches"] == 1
    finally:
        g.free()
    want = po.match_list(c.matrices, c.records, c.thresholds)
    assert got == want == singles and st["n_hits"] == st["n_candidates"] == len(want)
    assert all(h in {(i, r, s) for i, r, s, _ in want} for h in c.aim["hits"])


# ---- volume ----------------------------------------------------------------------------------------------------------------------
def test_result_outgrows_the_buffer():
    c = _lib.Context(0)                                      # a context whose hit buffer has its initial size
    try:
        text = pc.rand_dna(np.random.default_rng(5), 100_000)
        W = [[1, 1, 1, 0]]
        g = c.genome_from_host([text])
        c.pwm_match(g, [W], [1])
        got, st, st0 = hits(c), c.pwm_stats(), c.stats()
        want = po.match_list([np.array(W)], [text], [1])
        assert 70_000 < len(want) == 100_000 - text.count(b"T") and got == want
        assert st["n_launches"] == 2 and st["n_hits"] == len(want)                                    # counted, regrown, run again
        assert st0["n_launches"] == 2 and st0["bases_scanned"] == 100_000 and st0["scan_ms"] > 0
        c.pwm_match(g, [W], [1])
        assert hits(c) == want and c.pwm_stats()["n_launches"] == 1                                   # the buffer is kept
        c.pwm_match(g, [[[0, 0, 0, 5]] * 6], [30])            # then a small call
        assert hits(c) == po.match_list([np.array([[0, 0, 0, 5]] * 6)], [text], [30]) and c.pwm_stats()["n_launches"] == 1
        g.free()
    finally:
        c.close()


# ---- the family ------------------------------------------------------------------------------------------------------------------
def test_zero_one_matrices_are_motif_match(ctx):
    rng = np.random.default_rng(31)
    t = bytearray(pc.rand_dna(rng, 20_000))
    t[3000:3040] = b"N" * 40
    text = [bytes(t), pc.rand_dna(rng, 5_000).lower()]
    motifs = [(b"RYNNSW", 1), (b"ACGNNTKM", 2), (b"BDHVACG", 0), (b"GATTRCAGGNCTTAAC", 6), (b"N" * 30 + b"WSWS", 1)]
    g = ctx.genome_from_host(text)
    try:
        ctx.motif_match(g, [m for m, _ in motifs], [d for _, d in motifs])
        mm = [(i, c, s, k) for i, c, s, k, _ in ctx.motif_matches().tolist()]
        mats = [api.pwm_from_motif(m) for m, _ in motifs]
        ctx.pwm_match(g, [W for W, _ in mats], [inf - d for (_, inf), (_, d) in zip(mats, motifs)])
        got = hits(ctx)
        assert len(mm) > 200 and {i for i, *_ in mm} == set(range(5))
        assert [(i, c, s, mats[i][1] - k) for i, c, s, k in got] == mm                   # start for start, score = informative - mismatches
    finally:
        g.free()
    g = ctx.genome_from_fasta(b"".join(b">rec%d\n%s\n" % (c, r) for c, r in enumerate(text)))
    try:
        for (m, d), (W, inf) in zip(motifs[:2], mats):
            a = api.motifMatch(m, g, max_mismatch=d, strand="both", ctx=ctx)
            b = api.pwmMatch(W, g, threshold=inf - d, strand="both", ctx=ctx)
            assert len(a) > 10 and [(c, i, lo, hi, st, inf - k) for c, i, lo, hi, st, k in b] == a
    finally:
        g.free()


def test_human_rssd_on_the_fixture_is_motif_match(ctx):
    W, inf = api.pwm_from_motif(api.HumanRSSD)
    got = api.pwmMatch(W, LOCI, threshold=inf - 1, ctx=ctx)
    assert [(c, lo, 16 - k) for c, _, lo, hi, st, k in got] == mo.LOCI_RSSD_D1
    assert [(c, i, lo, hi, st, 16 - k) for c, i, lo, hi, st, k in got] == api.motifMatch(api.HumanRSSD, LOCI, max_mismatch=1, ctx=ctx)


# ---- strands ---------------------------------------------------------------------------------------------------------------------
def test_strands(ctx):
    rng = np.random.default_rng(41)
    W = pc.rand_matrix(rng, 16, constant=(9,))
    site = pc.best_site(W)
    recs = [bytearray(pc.rand_dna(rng, 2000)), bytearray(pc.rand_dna(rng, 900))]
    pc.plant(recs[0], 500, site)
    pc.plant(recs[0], 1500, po.revcomp_text(site))
    pc.plant(recs[1], 300, po.revcomp_text(site))
    recs = [bytes(r) for r in recs]
    thr = po.highest(W) - 400
    g = ctx.genome_from_fasta(b"".join(b">rec%d of two\n%s\n" % (c, r) for c, r in enumerate(recs)))
    try:
        got = {st: api.pwmMatch_batch([W], g, threshold=thr, strand=st, ctx=ctx)[0] for st in ("+", "-", "both")}
    finally:
        g.free()
    for st in got:
        assert [(c, lo, hi, s, k) for c, _, lo, hi, s, k in got[st]] == po.api_list(W, recs, thr, st)
    # "-" is "+" of the oracle on the reverse-complemented record, mapped back: start s there is L - s - m + 2 here
    mapped = sorted((c, len(recs[c]) - s - 16 + 2, k) for c in range(2) for s, k in po.find(W, po.revcomp_text(recs[c]), thr))
    assert [(c, lo, k) for c, _, lo, hi, s, k in got["-"]] == mapped
    assert got["both"] == sorted(got["+"] + got["-"], key=lambda t: (t[0], t[2], t[4]))
    assert all(ident == f"rec{c}" for c, ident, *_ in got["both"])
    top = po.highest(W)
    assert {(c, lo, s) for c, _, lo, hi, s, k in got["both"] if k == top} >= {(0, 501, "+"), (0, 1501, "-"), (1, 301, "-")}
    assert api.pwmMatch(W, recs[1], threshold=thr, strand="both", ctx=ctx) == [(lo, hi, s, k) for c, lo, hi, s, k in po.api_list(W, recs[1:], thr, "both")]


def test_palindromic_matrix_is_reported_on_both_strands(ctx):
    half = pc.rand_matrix(np.random.default_rng(42), 5)
    W = np.concatenate([half, half[::-1, ::-1]])
    assert np.array_equal(api.pwm_revcomp(W), W)
    t = bytearray(pc.rand_dna(np.random.default_rng(43), 1000))
    pc.plant(t, 200, pc.best_site(W))
    got = api.pwmMatch(W, bytes(t), threshold=po.highest(W), strand="both", ctx=ctx)
    assert got == [(201, 210, "+", po.highest(W)), (201, 210, "-", po.highest(W))]


# ---- the fixture -----------------------------------------------------------------------------------------------------------------
def test_find_rss_pwm_on_the_fixture_equals_the_golden_file(ctx, loci):
    with open(os.path.join(GOLDEN, "pwm.json")) as f:
        gold = json.load(f)
    ids = [r.identifier for r in loci]
    found = api.findRSS_pwm(LOCI, gold["sites"], ctx=ctx)                    # p <= 1e-6, both strands
    assert [[c, lo, hi, st, k] for c, _, lo, hi, st, k in found] == gold["hits"]["1e-6"] and len(found) == 11
    assert all(i == ids[c] for c, i, *_ in found)
    assert api.findRSS_pwm(LOCI, np.array(gold["matrix"]), ctx=ctx) == found
    for p in ("1e-4", "1e-8"):
        got = api.findRSS_pwm(LOCI, gold["matrix"], pvalue=float(p), ctx=ctx)
        assert [[c, lo, hi, st, k] for c, _, lo, hi, st, k in got] == gold["hits"][p]
    # the seven sites the matrix was made from are among the plus-strand hits
    plus = [h for h in found if h[4] == "+"]
    assert [(c, lo) for c, _, lo, *_ in plus if (c, lo) in {(c, s) for c, s, _ in mo.LOCI_RSSD_D1}] == [(c, s) for c, s, _ in mo.LOCI_RSSD_D1]


# ---- state and errors ------------------------------------------------------------------------------------------------------------
def test_scan_and_approx_results_survive(alp_ref, loci):
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
        assert len(found) > 0 and ex.size > 0 and mm.size == 7 and ap.size == 7
        W, inf = api.pwm_from_motif(api.HumanRSSD)
        c.pwm_match(g, [W], [inf - 1])
        assert [(r, s, 16 - k) for _, r, s, k in hits(c)] == mo.LOCI_RSSD_D1
        assert c.hits() == found and c.dips() == dips and np.array_equal(c.dists(1), d)
        assert np.array_equal(c.matches(), ex) and np.array_equal(c.motif_matches(), mm) and np.array_equal(c.approx_matches(), ap)
        st = c.stats()
        assert st["bases_scanned"] == sum(len(s) for s in seqs) and st["n_launches"] == 1 and st["scan_ms"] > 0
        g.free()
    finally:
        c.close()


def test_bad_genome_residue(ctx):
    W = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]
    g = ctx.genome_from_host([b"ACGTACGT", b"ACGTXACGT", b"ACGT"])
    try:
        ok = ctx.genome_from_host([b"ACGTACGT"])
        ctx.pwm_match(ok, [W], [3])
        ok.free()
        assert len(hits(ctx)) == 2
        with pytest.raises(_lib.BadBaseError) as ei:
            ctx.pwm_match(g, [W], [3])
        assert ei.value.status == _lib.KGMA_E_BADBASE and "record 1" in ei.value.message and "residue 5" in ei.value.message
        assert hits(ctx) == []                               # a failed call leaves no hits of the call before it
        with pytest.raises(_lib.KgmaError):
            api.pwmMatch(W, g, threshold=3, ctx=ctx)
    finally:
        g.free()


def test_argument_errors_through_the_c_abi(ctx):
    W = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]
    g = ctx.genome_from_host([b"ACGTACGTNN"])
    try:
        for mats, thr, text in (([np.zeros((0, 4), dtype=np.int64)], [1], "matrix 0 has 0 rows"), ([np.ones((65, 4), dtype=np.int64)], [70], "65 rows"),
                                ([W, np.zeros((0, 4), dtype=np.int64)], [3, 1], "matrix 1 has 0 rows"), ([W], [0], "threshold 0 does not exceed"),
                                ([W], [-5], "threshold -5"), ([W, W], [3, 0], "matrix 1: threshold 0"),
                                ([np.full((64, 4), -32768)], [64 * -32768], "row minima, -2097152")):
            with pytest.raises(_lib.KgmaError) as ei:
                ctx.pwm_match(g, mats, thr)
            assert ei.value.status == _lib.KGMA_E_ARG and text in ei.value.message and "matrix" in ei.value.message, (thr, ei.value.message)
        ctx.pwm_match(g, [W], [3])
        assert hits(ctx) == [(0, 0, 1, 3), (0, 0, 5, 3)]
        with pytest.raises(_lib.KgmaError):
            ctx.pwm_match(g, [W, W], [3, 0])
        assert hits(ctx) == []                               # a failed call leaves no hits of the call before it
        # null pointers
        L = _lib.load()
        off, thr = (C.c_int64 * 2)(0, 3), (C.c_int32 * 1)(3)
        w = (C.c_int16 * 12)(*np.array(W).ravel().tolist())
        ctx.pwm_match(g, [W], [3])
        for args in ((None, off, 1, thr), (w, None, 1, thr), (w, off, 1, None), (w, off, -1, thr)):
            assert L.kgma_pwm_match(ctx._h, g._h, *args) == _lib.KGMA_E_ARG
            assert hits(ctx) == []
        assert L.kgma_pwm_match(ctx._h, None, w, off, 1, thr) == _lib.KGMA_E_ARG and L.kgma_pwm_match(None, g._h, w, off, 1, thr) == _lib.KGMA_E_ARG
        assert L.kgma_get_pwm_stats(ctx._h, None) == _lib.KGMA_E_ARG and L.kgma_get_pwm_matches(ctx._h, None, 0, None) == _lib.KGMA_E_ARG
        assert L.kgma_pwm_match(ctx._h, g._h, w, off, 1, thr) == 0
        buf, n = (_lib.KgmaPwmHit * 1)(), C.c_int64(0)
        assert L.kgma_get_pwm_matches(ctx._h, buf, 1, C.byref(n)) == _lib.KGMA_E_ARG and n.value == 2     # too small a buffer
        ctx.pwm_match(g, [W, [[0, 0, 0, 2], [0, 0, 0, 0], [-1, -1, -1, -1]]], [3, 1])                       # the context is still usable; N scores the minimum
        assert hits(ctx) == [(0, 0, 1, 3), (0, 0, 5, 3), (1, 0, 4, 1), (1, 0, 8, 1)]
        ctx.pwm_match(g, [], [])                             # no matrices: no hits
        assert hits(ctx) == []
        with pytest.raises(ValueError):
            ctx.pwm_match(g, [[[0, 0, 0, 40000]]], [1])
    finally:
        g.free()
