"""Edit-distance search on the device (kgma_approx_match / api.approxMatch / api.findRSS_edits) against the numpy oracle
(tests/approx_oracle.py).

Every comparison is of the COMPLETE sorted list -- (query, record, start, end, edits) -- with the oracle's: the seams of the bit
vector's words, the seams of the kernel's tiles, waves and workgroups (read from kgma_get_approx_stats), records of every awkward
length, the alphabet, a result that outgrows the device buffer, a batch, the searches that exist already, strands, the fixture,
state and errors."""
import json
import os

import numpy as np
import pytest

from kmergma_amd import _lib, api
from tests import approx_cases as ac
from tests import approx_oracle as ao
from tests import motif_oracle as mo
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
    """(tile, wg_bases) of the search kernel, as the library reports them after a first call."""
    g = ctx.genome_from_host([b"ACGTACGT"])
    try:
        ctx.approx_match(g, [b"ACGT"], [0])
        st = ctx.approx_stats()
    finally:
        g.free()
    assert st["tile"] >= 16 and st["wg_bases"] % st["tile"] == 0 and (st["wg_bases"] // st["tile"]) % 64 == 0 and st["n_hits"] == 2
    return st["tile"], st["wg_bases"]


def hits(ctx):
    m = ctx.approx_matches()
    return list(zip(m["query"].tolist(), m["contig"].tolist(), m["start"].tolist(), m["end"].tolist(), m["edits"].tolist()))


def device_list(ctx, records, queries, eds, best_only=True):
    if isinstance(eds, int):
        eds = [eds] * len(queries)
    g = ctx.genome_from_host(records)
    try:
        ctx.approx_match(g, queries, eds, best_only)
        return hits(ctx)
    finally:
        g.free()


def check(ctx, records, queries, eds, best_only=True):
    got = device_list(ctx, records, queries, eds, best_only)
    want = ao.search(queries, records, eds, best_only)
    assert len(got) == len(want) and got == want, (len(got), len(want), [x for x in zip(got, want) if x[0] != x[1]][:3])
    return want


def check_case(ctx, c):
    want = check(ctx, c.records, c.queries, c.max_edits, c.best_only)
    if c.best_only:                                           # the other mode of the same case
        check(ctx, c.records, c.queries, c.max_edits, False)
    return want


# ---- word seams -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ac.word_seam_cases(), ids=lambda c: c.name)
def test_word_seams(ctx, case):
    want = check_case(ctx, case)
    assert want
    assert ctx.approx_stats()["words"] in ((2,) if len(case.queries[0]) > 32 else (1, 2))      # (2 below 33 symbols: only under KGMA_APPROX_WORDS=2)


# ---- tile seams -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["tile", "wave", "wg"])
def test_tile_seams(ctx, geometry, kind):
    cases = [c for c in ac.tile_seam_cases(*geometry) if c.name.endswith(f"_{kind}_seam")]
    assert len(cases) == 3
    B = ac.seams(*geometry)[kind]
    for c in cases:
        want = check_case(ctx, c)
        assert all((r, j, k) in {(r2, j2, k2) for _, r2, _, j2, k2 in want} for r, j, k in c.aim["ends"]), c.name
        assert {j for _, _, _, j, _ in want} & {B - 1, B, B + 1, B + 21, B + 20}


# ---- records, alphabet, batch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ac.record_cases() + ac.alphabet_cases(), ids=lambda c: c.name)
def test_records_and_alphabet(ctx, case):
    want = check_case(ctx, case)
    assert (want == []) == bool(case.aim.get("none"))


def test_soft_masked_2bit_genome(ctx, tmp_path):
    rng = np.random.default_rng(21)
    q = ac.plain_query(rng, 30)
    recs = []
    for n in (700, 3000):
        t = bytearray(ac.rand_dna(rng, n))
        ac.place(t, 400, q)
        ac.place(t, 600, ac.deleted(q, 11))
        t[380:390] = bytes(t[380:390]).lower()                # the mask begins inside the first occurrence
        t[500:620] = bytes(t[500:620]).lower()
        t[100:130] = b"N" * 30
        recs.append(bytes(t))
    p = tmp_path / "masked.2bit"
    tb.write_twobit(p, [(f"r{i}", r) for i, r in enumerate(recs)])
    g = ctx.genome_from_2bit(str(p))
    try:
        assert [g.fetch(c, 1, len(r)) for c, r in enumerate(recs)] == recs          # lower case and N as written
        ctx.approx_match(g, [q, b"NNNNNA"], [1, 0], True)
        got = hits(ctx)
    finally:
        g.free()
    want = ao.search([q, b"NNNNNA"], recs, [1, 0], True)
    assert got == want and {(c, j, k) for i, c, s, j, k in want if i == 0} == {(0, 400, 0), (0, 600, 1), (1, 400, 0), (1, 600, 1)}
    found = api.approxMatch(q, str(p), max_edits=1, ctx=ctx)
    assert found == [(c, f"r{c}", s, j, "+", k) for i, c, s, j, k in want if i == 0]


def test_batch_of_eight_in_one_launch(ctx):
    c = ac.batch_case()
    g = ctx.genome_from_host(c.records)
    try:
        ctx.approx_match(g, c.queries, c.max_edits, True)
        got, st = hits(ctx), ctx.approx_stats()
        ctx.approx_match(g, c.queries[2:3], c.max_edits[2:3], True)
        one, st1 = hits(ctx), ctx.approx_stats()
    finally:
        g.free()
    want = ao.search(c.queries, c.records, c.max_edits, True)
    assert got == want and one == [(0, r, s, j, k) for i, r, s, j, k in want if i == 2]
    assert st["n_launches"] == st1["n_launches"] == 2 and st["words"] == 2 and st1["words"] == 1      # search + starts, whatever the batch
    assert st["n_hits"] == len(want) and st["n_ends"] >= st["n_hits"]
    check(ctx, c.records, c.queries, c.max_edits, False)


# ---- volume ---------------------------------------------------------------------------------------------------------------------
def test_result_outgrows_the_buffer():
    c = _lib.Context(0)                                      # a context whose hit buffer has its initial size
    try:
        text = b"A" * 70_000
        g = c.genome_from_host([text])
        c.approx_match(g, [b"AAAAAAAA"], [1], False)
        got, st, st0 = hits(c), c.approx_stats(), c.stats()
        want = ao.search([b"AAAAAAAA"], [text], [1], False)
        assert len(want) == 69_994 > 65_536 and got == want
        assert want[0] == (0, 0, 1, 7, 1) and want[1] == (0, 0, 1, 8, 0) and want[-1] == (0, 0, 69_993, 70_000, 0)
        assert st["n_launches"] == 3 and st["n_ends"] == st["n_hits"] == 69_994                       # counted, regrown, run again, starts
        assert st0["n_launches"] == 3 and st0["bases_scanned"] == 70_000 and st0["scan_ms"] > 0
        c.approx_match(g, [b"AAAAAAAA"], [1], False)
        assert hits(c) == want and c.approx_stats()["n_launches"] == 2                                # the buffer is kept
        c.approx_match(g, [b"AAAAAAAA"], [1], True)
        assert hits(c) == [(0, 0, 1, 8, 0)] == ao.search([b"AAAAAAAA"], [text], [1], True)            # one run: its best end, the leftmost
        assert c.approx_stats()["n_ends"] == 69_994 and c.approx_stats()["n_hits"] == 1
        g.free()
    finally:
        c.close()


def test_random_genome(ctx):
    c = ac.random_case()
    want = check(ctx, c.records, c.queries, c.max_edits, False)
    assert len(want) > c.aim["many"]
    check(ctx, c.records, c.queries, c.max_edits, True)


# ---- what exists already --------------------------------------------------------------------------------------------------------
def test_no_edits_is_exact_match_and_motif_match(ctx):
    rng = np.random.default_rng(31)
    text = [ac.rand_dna(rng, 20_000), ac.rand_dna(rng, 5_000)]
    qs = [text[0][100:104], text[0][700:709], text[1][50:83], text[0][9000:9064]]
    iu = [b"ACNGT", b"RYRYRYR", b"SWNNKM", b"BDHVACG"]
    g = ctx.genome_from_host(text)
    try:
        ctx.exact_match(g, qs, True)
        ex = ctx.matches()
        ctx.approx_match(g, qs, [0] * len(qs), False)
        got = hits(ctx)
        assert len(got) > 50 and [(i, c, j) for i, c, s, j, k in got] == [(int(i), int(c), int(s) + len(qs[int(i)]) - 1) for i, c, s in ex.tolist()]
        assert all(k == 0 and j - s + 1 == len(qs[i]) for i, c, s, j, k in got)
        ctx.motif_match(g, iu, [0] * len(iu))
        mm = ctx.motif_matches().tolist()
        ctx.approx_match(g, iu, [0] * len(iu), False)
        got = hits(ctx)
        assert len(got) > 50 and [(i, c, s, j, k) for i, c, s, j, k in got] == [(i, c, s, s + len(iu[i]) - 1, 0) for i, c, s, _, _ in mm]
        # every motif hit with at most two mismatches is a matching end with no more edits
        motifs = [text[0][3000:3020], b"ACGNNTGCA", text[1][100:140]]
        planted = bytearray(text[0])
        planted[6000:6020] = ac.substituted(ac.substituted(motifs[0], 4), 15)
        g2 = ctx.genome_from_host([bytes(planted), text[1]])
        try:
            ctx.motif_match(g2, motifs, [2, 2, 2])
            mm = ctx.motif_matches().tolist()
            ctx.approx_match(g2, motifs, [2, 2, 2], False)
            by_end = {(i, c, j): k for i, c, s, j, k in hits(ctx)}
        finally:
            g2.free()
        assert len(mm) > 5 and any(k == 2 for *_, k, _ in mm)
        assert all(by_end.get((i, c, s + len(motifs[i]) - 1), 99) <= k for i, c, s, k, _ in mm)
    finally:
        g.free()


# ---- strands --------------------------------------------------------------------------------------------------------------------
def test_strands(ctx):
    rng = np.random.default_rng(41)
    q = b"GATTRCAGGNCTTAAC"
    plus = b"GATTACAGGACTTAAC"
    recs = [bytearray(ac.rand_dna(rng, 2000)), bytearray(ac.rand_dna(rng, 900))]
    ac.place(recs[0], 500, plus)
    ac.place(recs[0], 1500, ao.revcomp(ac.deleted(plus, 7)))
    ac.place(recs[1], 300, ao.revcomp(plus))
    recs = [bytes(r) for r in recs]
    g = ctx.genome_from_fasta(b"".join(b">rec%d of two\n%s\n" % (c, r) for c, r in enumerate(recs)))
    try:
        for all_ends in (False, True):
            got = {st: api.approxMatch_batch([q], g, max_edits=2, strand=st, all_ends=all_ends, ctx=ctx)[0] for st in ("+", "-", "both")}
            for st in got:
                assert [(c, lo, hi, s, k) for c, _, lo, hi, s, k in got[st]] == ao.api_list(q, recs, 2, st, all_ends)
            minus = ao.search([ao.revcomp(q)], recs, [2], not all_ends)
            assert [(c, lo, hi, k) for c, _, lo, hi, s, k in got["-"]] == sorted((c, s, j, k) for _, c, s, j, k in minus)
            assert got["both"] == sorted(got["+"] + got["-"], key=lambda t: (t[0], t[2], t[4], t[3]))
            assert all(ident == f"rec{c}" for c, ident, *_ in got["both"])
        assert {(c, hi, s, k) for c, _, lo, hi, s, k in got["both"]} >= {(0, 500, "+", 0), (0, 1500, "-", 1), (1, 300, "-", 0)}
    finally:
        g.free()
    assert api.approxMatch(q, recs[1], max_edits=2, strand="both", ctx=ctx) == [(lo, hi, s, k) for c, lo, hi, s, k in ao.api_list(q, recs[1:], 2, "both")]


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
def test_loci_against_the_golden_file(ctx):
    with open(os.path.join(GOLDEN, "approx.json")) as f:
        ent = json.load(f)["entries"]
    g = ctx.genome_from_path(LOCI)
    try:
        names = sorted(ao.GOLDEN_MOTIFS)
        sent = [(n, e, st, q) for n in names for e in ao.GOLDEN_EDITS for st, q in (("+", ao.GOLDEN_MOTIFS[n]), ("-", ao.revcomp(ao.GOLDEN_MOTIFS[n])))]
        for mode, best in (("all", False), ("best", True)):
            ctx.approx_match(g, [q for *_, q in sent], [e for _, e, _, _ in sent], best)
            got = hits(ctx)
            for i, (n, e, st, _) in enumerate(sent):
                assert [[c, s, j, k] for qi, c, s, j, k in got if qi == i] == ent[f"{n}|{e}|{st}"][mode], (n, e, st, mode)
    finally:
        g.free()


def test_find_rss_edits_on_the_fixture(ctx, loci):
    ids = [r.identifier for r in loci]
    found = api.findRSS_edits(LOCI, ctx=ctx)                 # HumanRSSD, one edit, both strands
    assert [(c, i, hi, st, k) for c, i, lo, hi, st, k in found] == [(c, ids[c], s + 38, "+", k) for c, s, k in mo.LOCI_RSSD_D1]
    assert [(c, lo, hi) for c, _, lo, hi, _, _ in found] == [(c, lo, hi) for c, _, lo, hi, _, _ in api.findRSS(LOCI, ctx=ctx)]
    # a spacer one base shorter or longer, which findRSS cannot see
    rec = bytearray(loci[2].sequence[:3000])
    s = mo.LOCI_RSSD_D1[2][1]                                # an RSS without a mismatch at 981
    rss = bytes(rec[s - 1:s + 38])
    short, long_ = rss[:20] + rss[21:], rss[:20] + ac.other_base(rss[20]) + rss[20:]
    rec[1500:1500 + 38], rec[2000:2000 + 40] = short, long_
    got = api.findRSS_edits(bytes(rec), strand="+", ctx=ctx)
    assert got == [(lo, hi, st, k) for c, lo, hi, st, k in ao.api_list(api.HumanRSSD, [bytes(rec)], 1, "+")]
    assert [(hi, k) for lo, hi, st, k in got] == [(s + 38, 0), (1538, 1), (2040, 1)]
    assert [(lo, k) for lo, hi, st, k in api.findRSS(bytes(rec), strand="+", ctx=ctx)] == [(s, 0)]


# ---- state and errors -----------------------------------------------------------------------------------------------------------
def test_scan_exact_and_motif_results_survive(alp_ref, loci):
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
        assert len(found) > 0 and ex.size > 0 and mm.size == 7
        c.approx_match(g, [api.HumanRSSD], [1], True)
        assert [(r, j, k) for _, r, s, j, k in hits(c)] == [(r, s + 38, k) for r, s, k in mo.LOCI_RSSD_D1]
        assert c.hits() == found and c.dips() == dips and np.array_equal(c.dists(1), d)
        assert np.array_equal(c.matches(), ex) and np.array_equal(c.motif_matches(), mm)
        st = c.stats()
        assert st["bases_scanned"] == sum(len(s) for s in seqs) and st["n_launches"] == 2 and st["scan_ms"] > 0
        g.free()
    finally:
        c.close()


def test_bad_genome_residue(ctx):
    g = ctx.genome_from_host([b"ACGTACGT", b"ACGTXACGT", b"ACGT"])
    try:
        ok = ctx.genome_from_host([b"ACGTACGT"])
        ctx.approx_match(ok, [b"ACG"], [0])
        ok.free()
        assert len(hits(ctx)) == 2
        with pytest.raises(_lib.BadBaseError) as ei:
            ctx.approx_match(g, [b"ACG"], [0])
        assert ei.value.status == _lib.KGMA_E_BADBASE and "record 1" in ei.value.message and "residue 5" in ei.value.message
        assert hits(ctx) == []                               # a failed call leaves no hits of the call before it
        with pytest.raises(_lib.KgmaError):
            api.approxMatch(b"ACG", g, ctx=ctx)
    finally:
        g.free()


def test_argument_errors_through_the_c_abi(ctx):
    g = ctx.genome_from_host([b"ACGTACGTNN"])
    try:
        for qs, es, text in (([b""], [0], "0 symbols"), ([b"A" * 65], [0], "65 symbols"), ([b"ACXG"], [0], "symbol 3"), ([b"AC-G"], [0], "symbol 3"),
                             ([b"ACG", b"AC G"], [0, 0], "query 1, symbol 3"), ([b"ACGT"], [4], "max_edits 4"), ([b"ACGT"], [-1], "max_edits -1"),
                             ([b"A" * 20], [16], "max_edits 16"), ([b"ANNT"], [2], "2 informative"), ([b"NNNN"], [0], "0 informative"),
                             ([b"ACGT", b"N"], [0, 0], "query 1")):
            with pytest.raises(_lib.KgmaError) as ei:
                ctx.approx_match(g, qs, es)
            assert ei.value.status == _lib.KGMA_E_ARG and text in ei.value.message and "query" in ei.value.message, (qs, es, ei.value.message)
        ctx.approx_match(g, [b"ACG"], [0])
        assert hits(ctx) == [(0, 0, 1, 3, 0), (0, 0, 5, 7, 0)]
        with pytest.raises(_lib.KgmaError) as ei:
            ctx.approx_match(g, [b"ACG", b"ACGTX"], [0, 0])
        assert "query 1" in ei.value.message and "symbol 5" in ei.value.message
        assert hits(ctx) == []                               # a failed call leaves no hits of the call before it
        ctx.approx_match(g, [b"ACG", b"TNN"], [0, 0])        # the context is still usable
        assert hits(ctx) == [(0, 0, 1, 3, 0), (0, 0, 5, 7, 0), (1, 0, 4, 6, 0), (1, 0, 8, 10, 0)]
        ctx.approx_match(g, [], [])                          # no queries: no hits
        assert hits(ctx) == []
    finally:
        g.free()
