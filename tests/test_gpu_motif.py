"""IUPAC motif search with mismatches on the device (kgma_motif_match / api.motifMatch / api.findRSS) against the numpy oracle
(tests/motif_oracle.py).

Every comparison is of the COMPLETE sorted list -- (motif, record, start, mismatches) -- with the oracle's: record and motif
lengths around the 32-base plane word, plants at bit 0 / bit 31 / across one and two word boundaries / on a record's last base,
the alphabet (every symbol against every residue, genome N, lower case), the counter at every plane count, a mixed batch, a seeded
random genome, equivalence with exactMatch, strands, a result that outgrows the device buffer, independence from the scan and
exactMatch state, re-packing after a poke, the errors, and the recombination signal sequences of tests/data/Loci.fasta."""
import os

import numpy as np
import pytest

from kmergma_amd import _lib, api, fasta
from tests import motif_oracle as mo
from tests.conftest import DATA
from tests.motif_oracle import LOCI_CUM as CUM, LOCI_GENES, LOCI_RSSD_D1 as RSSD_D1, LOCI_RSSV_D1 as RSSV_D1

pytestmark = pytest.mark.gpu
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
LOCI = os.path.join(DATA, "Loci.fasta")
SYMS = "ACGTRYSWKMBDHVN"


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)          # no references are ever set on this context: the search needs none
    yield c
    c.close()


def quads(ctx):
    m = ctx.motif_matches()
    return list(zip(m["motif"].tolist(), m["contig"].tolist(), m["start"].tolist(), m["mismatches"].tolist()))


def device_list(ctx, records, motifs, ds):
    if isinstance(ds, int):
        ds = [ds] * len(motifs)
    g = ctx.genome_from_host(records)
    try:
        ctx.motif_match(g, motifs, ds)
        return quads(ctx)
    finally:
        g.free()


def check(ctx, records, motifs, ds):
    got = device_list(ctx, records, motifs, ds)
    want = mo.match_list(motifs, records, ds)
    assert len(got) == len(want) and got == want, (len(got), len(want))
    return want


def rand_dna(rng, n):
    return BASES[rng.integers(0, 4, size=n)].tobytes()


def mutate(rng, motif, n):
    """`motif` (A/C/G/T) with exactly n positions changed to another base."""
    b = bytearray(motif)
    for i in rng.choice(len(b), size=n, replace=False).tolist():
        b[i] = ord(rng.choice([c for c in "ACGT" if ord(c) != b[i]]))
    return bytes(b)


# ---- boundaries -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 31, 32, 33, 63, 64])
def test_record_and_motif_lengths(ctx, m):
    rng = np.random.default_rng(100 + m)
    motif = rand_dna(rng, m)
    lens = [m - 1, m, m + 1, 31, 32, 33, 63, 64, 65, 95, 96, 97]
    recs = [bytearray(rand_dna(rng, n)) for n in lens]
    for r in recs:                                           # ... each ending on the motif where it fits: a match on the last base
        if len(r) >= m:
            r[len(r) - m:] = motif
    # a long record with the motif at bit 0 and bit 31 of a plane word, across one and across two word boundaries, and on the
    # record's last base; then the motif cut in two over the end of one record and the start of the next
    L = 8 * 1024 + 77
    big = bytearray(rand_dna(rng, L))
    plants = [0, 31 + 32 * 10, 32 * 20, 32 * 30 - m // 2, 32 * 40 - 1, 32 * 50 + 17, L - m]
    for p in plants:
        big[p:p + m] = motif
    half = m // 2
    left, right = bytearray(rand_dna(rng, 200)), bytearray(rand_dna(rng, 200))
    if half:
        left[200 - half:] = motif[:half]
        right[:m - half] = motif[half:]
    recs = [bytes(r) for r in recs] + [bytes(big), bytes(left), bytes(right)]
    want = check(ctx, recs, [motif], 0)
    got = {(c, s) for _, c, s, _ in want}
    nb = len(lens)
    assert {(nb, p + 1) for p in plants} <= got
    assert all((c, n - m + 1) in got for c, n in enumerate(lens) if n >= m) and not any(c == 0 for c, _ in got)
    if m >= 2:
        check(ctx, recs, [motif], 1)
    if m >= 31:                                              # (the two-record plant is no match even with mismatches to spare)
        w3 = check(ctx, recs, [motif], 3)
        assert not any(c == nb + 1 and s > 200 - m + 1 for _, c, s, _ in w3)


def test_spans_one_and_two_word_boundaries(ctx):
    rng = np.random.default_rng(9)
    motif = rand_dna(rng, 64)
    rec = bytearray(rand_dna(rng, 4096))
    for w, bit in ((3, 0), (9, 1), (15, 31), (21, 16)):      # 64 symbols from bit 0: two words; from any other bit: three
        rec[32 * w + bit:32 * w + bit + 64] = motif
    want = check(ctx, [bytes(rec)], [motif, motif[:33], motif[:2]], [2, 1, 0])
    assert {s for q, _, s, _ in want if q == 0} >= {32 * 3 + 1, 32 * 9 + 2, 32 * 15 + 32, 32 * 21 + 17}


# ---- alphabet ---------------------------------------------------------------------------------------------------------------
def test_every_symbol_against_every_residue(ctx):
    recs = [r + b"A" for r in (b"A", b"C", b"G", b"T", b"N", b"a", b"c", b"g", b"t", b"n")]
    motifs = [(s + "A").encode() for s in SYMS] + [(s.lower() + "a").encode() for s in SYMS]
    want = check(ctx, recs, motifs, 0)
    got = {(q, c) for q, c, _, _ in want}
    for qi, s in enumerate(SYMS * 2):
        for ci, r in enumerate("ACGTNACGTN"):
            expect = (s == "N") if r == "N" else bool(mo.IUPAC[s] & mo.IUPAC[r])
            assert ((qi, ci) in got) == expect, (s, r)


def test_genome_n_and_lower_case(ctx):
    recs = [b"ACGTNNNNACGTTTTTacgtnnacgtttac", b"NNNNNNNN", b"TTTTTTTT", b"acgtacgtacgt"]
    motifs = [b"GTTT", b"GTNN", b"GTNNNNAC", b"TTTT", b"NNT", b"ACGT", b"acgt", b"WSNNY"]
    want = check(ctx, recs, motifs, 0)
    got = set(want)
    assert (0, 0, 3, 0) not in got and (0, 0, 11, 0) in got          # GTTT: not on GTNN (the planes say match), but on GTTT
    assert (1, 0, 3, 0) in got and (2, 0, 3, 0) in got               # a genome N under a motif N
    assert not any(q == 3 and c == 1 for q, c, _, _ in want) and (3, 2, 1, 0) in got
    assert (5, 3, 1, 0) in got and (6, 0, 1, 0) in got               # either case, both sides
    w1 = check(ctx, recs, motifs[:3], 1)
    assert (0, 0, 3, 1) not in set(w1)                               # GTNN under GTTT: two mismatches, not one
    check(ctx, recs, [b"GTTT", b"TTTTTT"], [2, 3])


# ---- counting ---------------------------------------------------------------------------------------------------------------
D_CASES = [0, 1, 2, 3, 7, 15]                                # every plane count of the counter (0 ... 4), each at its largest d


def counting_case():
    rng = np.random.default_rng(77)
    rec = bytearray(rand_dna(rng, 6000))
    motifs, plants = [], []
    for i, d in enumerate(D_CASES):
        motif = rand_dna(rng, 17 + 9 * i)                  # 17 ... 62 symbols
        at_d, over = 200 + 900 * i + int(rng.integers(0, 32)), 650 + 900 * i + int(rng.integers(0, 32))
        rec[at_d:at_d + len(motif)] = mutate(rng, motif, d)
        rec[over:over + len(motif)] = mutate(rng, motif, d + 1)
        motifs.append(motif)
        plants.append((at_d + 1, over + 1))
    return [bytes(rec), rand_dna(rng, 500)], motifs, plants


@pytest.mark.parametrize("i", range(len(D_CASES)))
def test_exactly_d_and_d_plus_one_mismatches(ctx, i):
    recs, motifs, plants = counting_case()
    d = D_CASES[i]
    want = check(ctx, recs, [motifs[i]], d)
    assert (0, 0, plants[i][0], d) in set(want) and not any(s == plants[i][1] for _, _, s, _ in want)
    w2 = check(ctx, recs, [motifs[i]], d + 1) if d < 15 else want
    assert d == 15 or (0, 0, plants[i][1], d + 1) in set(w2)


def test_mixed_batch(ctx):
    recs, motifs, plants = counting_case()
    g = ctx.genome_from_host(recs)
    try:
        order = [5, 0, 3, 1, 4, 2]
        ms, ds = [motifs[i] for i in order] + [b"ACNNGT", b"RY"], [D_CASES[i] for i in order] + [1, 0]
        ctx.motif_match(g, ms, ds)
        got = quads(ctx)
        assert got == mo.match_list(ms, recs, ds) and ctx.stats()["n_launches"] == 1
        for qi, i in enumerate(order):
            assert (qi, 0, plants[i][0], D_CASES[i]) in set(got)
        ctx.motif_match(g, ms[:1], ds[:1])                   # one launch whatever the batch size
        assert ctx.stats()["n_launches"] == 1 and ctx.stats()["bases_scanned"] == 6500
    finally:
        g.free()


# ---- randomised -------------------------------------------------------------------------------------------------------------
def random_case():
    """A 200 kb genome in three records, 1 % N, mixed case; 20 random IUPAC motifs of 4 ... 64 symbols, an instance of each planted
    with 0 ... 3 mismatches; per motif the largest max_mismatch (0 ... 15, below the informative positions) that keeps its matches
    at 10 000 or fewer -- and there is at least one for every motif, so none drops out."""
    rng = np.random.default_rng(2024)
    lens = [120_000, 50_001, 29_999]
    recs = []
    for n in lens:
        b = np.frombuffer(rand_dna(rng, n), dtype=np.uint8).copy()
        b[rng.random(n) < 0.01] = ord("N")
        low = rng.random(n) < 0.3
        b[low] |= 0x20
        recs.append(bytearray(b.tobytes()))
    weights = np.array([6.0] * 4 + [1.0] * 10 + [2.0])
    motifs = []
    for i in range(20):
        m = 4 + (i * 60) // 19                             # 4 ... 64
        motif = "".join(rng.choice(list(SYMS), size=m, p=weights / weights.sum()))
        if set(motif) == {"N"}:
            motif = "A" + motif[1:]
        inst = bytearray(rng.choice([b for b in "ACGT" if mo.IUPAC[b] & mo.IUPAC[s]]).encode()[0] for s in motif)
        informative = [j for j, s in enumerate(motif) if s != "N"]
        for j in rng.choice(informative, size=min(i % 4, len(informative) - 1), replace=False).tolist():
            inst[j] = ord(rng.choice([b for b in "ACGT" if not mo.IUPAC[b] & mo.IUPAC[motif[j]]]))
        c = i % 3
        p = int(rng.integers(0, lens[c] - m))
        recs[c][p:p + m] = inst
        motifs.append(motif.encode() if i % 2 else motif.lower().encode())
    recs = [bytes(r) for r in recs]
    ds = []
    for motif in motifs:
        informative = int((mo.motif_sets(motif) != 15).sum())
        hist = np.bincount(np.concatenate([mo.mism_profile(motif, r) for r in recs]), minlength=65).cumsum()
        ok = [d for d in range(min(15, informative - 1) + 1) if 1 <= hist[d] <= 10_000]
        assert ok, motif
        ds.append(ok[-1])
    return recs, motifs, ds


def test_random_genome(ctx):
    recs, motifs, ds = random_case()
    want = check(ctx, recs, motifs, ds)
    per = [sum(1 for q, _, _, _ in want if q == i) for i in range(len(motifs))]
    assert len(motifs) == 20 and all(1 <= n <= 10_000 for n in per), per
    assert sorted({len(m) for m in motifs})[0] == 4 and max(len(m) for m in motifs) == 64
    assert sum(per) > 50_000 and {k for _, _, _, k in want} == set(range(16))
    tight = [max(d - 2, 0) for d in ds]
    check(ctx, recs, motifs, tight)


# ---- equivalence with exactMatch --------------------------------------------------------------------------------------------
def test_acgt_motifs_without_mismatches_are_exact_match(ctx):
    recs, _, _ = random_case()
    up = recs[0].upper()
    qs = []
    for L in (1, 2, 5, 16, 17, 33, 40, 64):
        p = 1000 + 37 * L
        while b"N" in up[p:p + L]:
            p += 1
        qs.append(up[p:p + L])
    g = ctx.genome_from_host(recs)
    try:
        ctx.exact_match(g, qs, True)
        ex = ctx.matches()
        ctx.motif_match(g, qs, [0] * len(qs))
        got = quads(ctx)
        assert [(q, c, s) for q, c, s, _ in got] == list(zip(ex["query"].tolist(), ex["contig"].tolist(), ex["start"].tolist()))
        assert len(got) > 50_000 and all(k == 0 for _, _, _, k in got) and {q for q, _, _, _ in got} == set(range(len(qs)))
    finally:
        g.free()


# ---- strands ----------------------------------------------------------------------------------------------------------------
def test_minus_strand_is_plus_on_the_reverse_complement(ctx):
    recs, motifs, ds = random_case()
    pick = [0, 3, 7, 12, 19]
    ms, dd = [motifs[i] for i in pick] + [b"ACNNGT", b"GAATTC"], [ds[i] for i in pick] + [1, 1]
    g = api._GenomeView(ctx, [fasta.Record(f"rec{c} of the random case", r) for c, r in enumerate(recs)])
    rc = g.reversed()
    try:
        plus = api.motifMatch_batch(ms, g, max_mismatch=dd, strand="+", ctx=ctx)
        minus = api.motifMatch_batch(ms, g, max_mismatch=dd, strand="-", ctx=ctx)
        both = api.motifMatch_batch(ms, g, max_mismatch=dd, strand="both", ctx=ctx)
        assert ctx.stats()["n_launches"] == 1                # both strands: twice the motifs, one pass
        on_rc = api.motifMatch_batch(ms, rc, max_mismatch=dd, strand="+", ctx=ctx)
        for i, m in enumerate(ms):
            assert [t[:1] + t[2:] for t in plus[i]] == mo.api_list(m, recs, dd[i], "+")
            assert [t[:1] + t[2:] for t in minus[i]] == mo.api_list(m, recs, dd[i], "-")
            mapped = sorted((c, ident) + api.strand_range(len(recs[c]), lo, hi) + ("-", k) for c, ident, lo, hi, _, k in on_rc[i])
            assert mapped == minus[i] and all(t[4] == "-" and t[1] == f"rec{t[0]}" for t in minus[i])
            assert both[i] == sorted(plus[i] + minus[i], key=lambda t: (t[0], t[2], t[4]))
        assert len(minus[5]) > 0 and len(minus[0]) + len(minus[1]) > 0
        # a motif equal to its own reverse complement: every place twice, plus first
        pal = both[6]
        assert len(pal) > 0 and len(pal) == 2 * len(plus[6])
        assert pal[0::2] == plus[6] and [t[:4] + ("+",) + t[5:] for t in pal[1::2]] == plus[6]
    finally:
        rc.free()
        g.free()


def test_single_sequence_forms(ctx):
    seq = b"ttGAATTCaaGATTTCccGAATTC"
    assert api.motifMatch(b"GAATTC", seq, ctx=ctx) == [(3, 8, "+", 0), (19, 24, "+", 0)]
    assert api.motifMatch("gaattc", fasta.Record("s", seq), max_mismatch=1, ctx=ctx) == [(3, 8, "+", 0), (11, 16, "+", 1), (19, 24, "+", 0)]
    assert api.motifMatch(b"GAAWTC", seq, strand="-", ctx=ctx) == [(3, 8, "-", 0), (11, 16, "-", 0), (19, 24, "-", 0)]
    assert api.motifMatch(b"GAAATC", seq, strand="both", ctx=ctx) == [(11, 16, "-", 0)]
    assert api.motifMatch(b"CCCCCC", seq, ctx=ctx) == []


# ---- buffer growth ----------------------------------------------------------------------------------------------------------
def test_result_outgrows_the_buffer():
    c = _lib.Context(0)                                      # a context whose hit buffer has its initial size
    try:
        g = c.genome_synthetic([700_000, 300_007], 91)
        text = [g.fetch(0, 1, 700_000), g.fetch(1, 1, 300_007)]
        c.motif_match(g, [b"RNY"], [0])
        got, st = quads(c), c.stats()
        want = mo.match_list([b"RNY"], text, 0)
        assert len(want) > 100_000 and len(got) == len(want) and got == want
        assert st["n_launches"] == 2 and st["bases_scanned"] == 1_000_007 and st["scan_ms"] > 0      # counted, regrown, run again
        c.motif_match(g, [b"RNY"], [0])
        assert quads(c) == want and c.stats()["n_launches"] == 1                                    # the buffer is kept
        g.free()
    finally:
        c.close()


# ---- state ------------------------------------------------------------------------------------------------------------------
def test_scan_and_exact_results_survive_a_motif_search(alp_ref, loci):
    c = _lib.Context(0)
    try:
        seqs = [r.sequence for r in loci]
        c.set_refs(6, [alp_ref["RV"]], [alp_ref["ws"]], [30.0], [alp_ref["N"]])
        g = c.genome_from_host(seqs)
        c.scan(g, _lib.MODE_SINGLE, 50, 0, _lib.F_RETURN_DISTS, None)
        hits, dips, d = c.hits(), c.dips(), c.dists(1)
        c.exact_match(g, [seqs[0][1000:1040], b"AAATT"])
        ex = c.matches().copy()
        assert len(hits) > 0 and ex.size > 0
        c.motif_match(g, [api.HumanRSSD], [1])
        assert [(c_, s, k) for _, c_, s, k in quads(c)] == RSSD_D1
        assert c.hits() == hits and c.dips() == dips and np.array_equal(c.dists(1), d) and np.array_equal(c.matches(), ex)
        c.scan(g, _lib.MODE_SINGLE, 50, 0, _lib.F_RETURN_DISTS, None)
        c.exact_match(g, [b"AAATT"])
        assert c.hits() == hits and [(c_, s, k) for _, c_, s, k in quads(c)] == RSSD_D1            # kept until the next search
        g.free()
    finally:
        c.close()


def test_poked_genome_is_repacked(ctx):
    rng = np.random.default_rng(5)
    recs = [bytearray(rand_dna(rng, 5000)), bytearray(rand_dna(rng, 100))]
    motif = rand_dna(rng, 30)
    g = ctx.genome_from_host([bytes(r) for r in recs])
    try:
        ctx.motif_match(g, [motif], [1])
        assert quads(ctx) == []
        g.poke(0, 3001, motif)                               # no repack: the search sees that the text changed
        g.poke(1, 71, mutate(rng, motif, 1))
        recs[0][3000:3030] = motif
        recs[1][70:100] = motif
        ctx.motif_match(g, [motif], [1])
        assert quads(ctx) == [(0, 0, 3001, 0), (0, 1, 71, 1)]
        g.poke(0, 3010, b"N")
        ctx.motif_match(g, [motif], [0])
        assert quads(ctx) == []
        ctx.motif_match(g, [motif], [1])
        assert quads(ctx) == [(0, 0, 3001, 1), (0, 1, 71, 1)]
    finally:
        g.free()


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_bad_genome_residue(ctx):
    g = ctx.genome_from_host([b"ACGTACGT", b"ACGTRACGT", b"ACGT"])
    try:
        with pytest.raises(_lib.BadBaseError) as ei:
            ctx.motif_match(g, [b"ACG"], [0])
        assert ei.value.status == _lib.KGMA_E_BADBASE and "record 1" in ei.value.message and "residue 5" in ei.value.message
        with pytest.raises(_lib.KgmaError):
            api.motifMatch(b"ACG", g, ctx=ctx)
    finally:
        g.free()


def test_argument_errors_through_the_c_abi(ctx):
    g = ctx.genome_from_host([b"ACGTACGTNN"])
    try:
        for motifs, ds in (([b""], [0]), ([b"A" * 65], [0]), ([b"ACXG"], [0]), ([b"AC-G"], [0]), ([b"ACG", b"AC G"], [0, 0]),
                           ([b"ACGT"], [4]), ([b"ACGT"], [-1]), ([b"A" * 20], [16]), ([b"ANNT"], [2]), ([b"NNNN"], [0]), ([b"N"], [0])):
            with pytest.raises(_lib.KgmaError) as ei:
                ctx.motif_match(g, motifs, ds)
            assert ei.value.status == _lib.KGMA_E_ARG, (motifs, ds)
        ctx.motif_match(g, [b"ACG"], [0])
        assert len(quads(ctx)) == 2
        with pytest.raises(_lib.KgmaError) as ei:
            ctx.motif_match(g, [b"ACG", b"ACGTX"], [0, 0])
        assert "motif 1" in ei.value.message and "symbol 5" in ei.value.message
        assert quads(ctx) == []                              # a failed call leaves no hits of the call before it
        ctx.motif_match(g, [b"ACG", b"TNN"], [0, 0])         # the context is still usable
        assert quads(ctx) == [(0, 0, 1, 0), (0, 0, 5, 0), (1, 0, 4, 0), (1, 0, 8, 0)]
    finally:
        g.free()


# ---- the fixture ------------------------------------------------------------------------------------------------------------
def test_find_rss_on_the_fixture(ctx, loci):
    ids = [r.identifier for r in loci]
    found = api.findRSS(LOCI, ctx=ctx)                       # HumanRSSD, one mismatch, both strands
    assert found == [(c, ids[c], s, s + 38, "+", k) for c, s, k in RSSD_D1]
    assert api.findRSS(LOCI, strand="-", ctx=ctx) == []
    assert len(api.findRSS(LOCI, max_mismatch=2, ctx=ctx)) == 14 and len(api.findRSS(LOCI, max_mismatch=3, ctx=ctx)) == 30
    assert api.findRSS(LOCI, api.HumanRSSV, 0, "+", ctx=ctx) == []
    assert api.findRSS(LOCI, api.HumanRSSV, strand="+", ctx=ctx) == [(c, ids[c], s, s + 27, "+", k) for c, s, k in RSSV_D1]
    assert len(api.findRSS(LOCI, api.HumanRSSV, 2, ctx=ctx)) == 8 and len(api.findRSS(LOCI, api.HumanRSSV, 3, ctx=ctx)) == 23
    seqs = [r.sequence for r in loci]
    for rss in (api.HumanRSSD, api.HumanRSSV):
        for d in (2, 3):
            got = api.motifMatch(rss, LOCI, max_mismatch=d, strand="both", ctx=ctx)
            assert [t[:1] + t[2:] for t in got] == mo.api_list(rss, seqs, d, "both")


def test_an_rss_lies_behind_every_gene_the_scan_finds(ctx):
    out = api.findGenes(genome_path=LOCI, ref_path=os.path.join(DATA, "Alp_V_ref.fasta"), KmerDistThr=30.0, verbose=False,
                        do_return_hit_loci=True, ctx=ctx)
    genes = out[1]
    assert genes == LOCI_GENES
    rss = [CUM[c] + lo for c, _, lo, _, _, _ in api.findRSS(LOCI, ctx=ctx)]
    for locus in genes:
        assert sum(1 for s in rss if 293 <= s - locus <= 299) == 1, locus
