"""Exact sequence search on the device (kgma_exact_match / api.exactMatch) against the CPU oracle (tests/exact_oracle.py).

Every comparison is of the COMPLETE sorted match list -- (query, record, start) triples -- with the oracle's, through the C ABI
and through the api functions: the reference's own known answers (tests/golden/exact.json), seeded random genomes with queries
cut from them at every phase of a packed word, symbol equality (N, IUPAC codes, case), both overlap modes, a result that outgrows
the device buffer, batches, independence from the scan state, both kernels (KGMA_EXACT_ASCII=1 in a fresh child process), and the
chr22-size and GRCh38-size synthetic genomes of tests/test_gpu_fullsize.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from kmergma_amd import _lib, api, fasta, workloads
from tests import exact_oracle as eo
from tests.conftest import DATA, GOLDEN, ROOT, PKG

pytestmark = pytest.mark.gpu
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)          # no references are ever set on this context: the search needs none
    yield c
    c.close()


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLDEN, "exact.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def genes():
    return [r.sequence for r in fasta.read_fasta(os.path.join(DATA, "Alp_V_ref.fasta"))]


def triples(ctx):
    m = ctx.matches()
    return list(zip(m["query"].tolist(), m["contig"].tolist(), m["start"].tolist()))


def device_list(ctx, records, queries, overlap=True):
    g = ctx.genome_from_host(records)
    try:
        ctx.exact_match(g, queries, overlap)
        return triples(ctx)
    finally:
        g.free()


def check(ctx, records, queries):
    for overlap in (True, False):
        got = device_list(ctx, records, queries, overlap)
        want = eo.match_list(queries, records, overlap)
        assert len(got) == len(want) and got == want, (overlap, len(got), len(want))
    return want


# ---- the reference's known answers ------------------------------------------------------------------------------------------
def test_golden_single_sequence(ctx, gold):
    for g in gold["single_seq"]:
        want = None if g["expect"] is None else [tuple(x) for x in g["expect"]]
        assert api.exactMatch(g["query"], g["subject"].encode(), overlap=g["overlap"], ctx=ctx) == want
        assert api.exactMatch(fasta.Record("q", g["query"].encode()), fasta.Record("s", g["subject"].encode()), overlap=g["overlap"], ctx=ctx) == want
        got = device_list(ctx, [g["subject"].encode()], [g["query"].encode()], g["overlap"])
        assert got == [(0, 0, lo) for lo, _ in (want or [])]


def test_golden_reader(ctx, gold):
    for g in gold["reader"]:
        path = os.path.join(DATA, g["fasta"])
        recs = fasta.read_fasta(path)
        if "query" in g:
            q = g["query"]
        else:
            f = g["query_from"]
            q = fasta.Record(recs[f["record"] - 1].description, recs[f["record"] - 1].sequence[f["lo"] - 1:f["hi"]])
        want = g["expect"] if isinstance(g["expect"], str) else {k: [tuple(x) for x in v] for k, v in g["expect"].items()}
        assert api.exactMatch(q, path, ctx=ctx) == want
        dev = ctx.genome_from_fasta(path)
        try:
            assert api.exactMatch(q, dev, ctx=ctx) == want
            assert api.exactMatch_batch([q, q], dev, ctx=ctx) == [want, want]
        finally:
            dev.free()


def test_golden_cumulative_len_from_the_handle(ctx, gold):
    g = gold["cumulative_len"]
    dev = ctx.genome_from_fasta(os.path.join(DATA, g["fasta"]))
    try:
        assert api.fasta_id_to_cumulative_len_dict(dev) == g["expect"]
    finally:
        dev.free()


# ---- seeded random genomes -------------------------------------------------------------------------------------------------
def planted_case(seed=5):
    """Records of assorted lengths (some shorter than 16 and than most queries) and queries cut from them."""
    rng = np.random.default_rng(seed)
    lens = [1000, 37, 5000, 12, 3, 16, 15, 2049, 70000, 1, 32, 33]
    recs = [BASES[rng.integers(0, 4, size=n)].tobytes() for n in lens]
    qs = [recs[0][:20], recs[0][-20:], recs[8][:300], recs[8][-300:], recs[2][:5], recs[2][-5:]]          # record start / end
    for p in range(32):                                      # every phase of a packed word, every byte alignment
        for L in (3, 8, 9, 16, 17, 40):
            qs.append(recs[2][100 + p:100 + p + L])
        qs.append(recs[8][16384 - 20 + p:16384 + 60 + p])  # across the boundary of both kernels' runs and tiles
    qs.append(recs[8][32768 - 7:32768 + 9])
    absent = list(range(len(qs), len(qs) + 4))
    qs += [recs[i][-10:] + recs[i + 1][:10] for i in (0, 1, 7)]        # tail of record i + head of record i + 1: no match
    qs.append(BASES[rng.integers(0, 4, size=80000)].tobytes())         # longer than every record
    qs += [recs[8][1000:1000 + 50], recs[8][5:5 + 38]]                 # longer than the short records
    qs += [recs[i] for i in (1, 3, 4, 5, 6, 9, 10, 11)]                # a whole record
    qs += [b"A", b"C", b"G", b"T"]                                     # one symbol
    qs += [recs[2][7:7 + L] for L in range(2, 20)]
    return recs, qs, absent


def test_planted_random_genome(ctx):
    recs, qs, absent = planted_case()
    want = check(ctx, recs, qs)
    found = {q for q, _, _ in want}
    assert len(want) > 20000 and found == set(range(len(qs))) - set(absent)     # (absent: the straddling and the over-long queries)


def test_symbol_equality(ctx):
    recs = [b"ACGTNNNNACGTRYACGTnnacgtN", b"NNNN", b"TTTT", b"acgtRrYyKMSWBDHV-N-acgt", b"AcGtAcGt", b"RRAR"]
    qs = [b"T", b"N", b"NN", b"AN", b"TN", b"R", b"Y", b"A", b"acgtn", b"GTNNNNAC", b"TTTT", b"NNNN", b"r", b"RY", b"-", b"-N-", b"acgtacgt",
          b"ACGT", b"aCgT", b"V", b"B", b"GTRY", b"GTAY", b"KMSWBDHV-N-ACGT"]
    want = check(ctx, recs, qs)
    got = set(want)
    assert (0, 1, 1) not in got and (1, 2, 1) not in got            # genome N / query T and the reverse
    assert (4, 0, 4) in got and (1, 1, 1) in got                    # TN and N against N
    assert {c for q, c, _ in want if q == 5} == {0, 3, 5} and (7, 5, 3) in got and not any(q == 7 and c == 5 and s != 3 for q, c, s in want)


def test_bad_symbols(ctx):
    g = ctx.genome_from_host([b"ACGTACGT", b"ACGTXACGT", b"ACGT"])
    try:
        with pytest.raises(_lib.BadBaseError) as ei:
            ctx.exact_match(g, [b"ACG"])
        assert ei.value.status == _lib.KGMA_E_BADBASE and "record 1" in ei.value.message and "residue 5" in ei.value.message
    finally:
        g.free()
    g = ctx.genome_from_host([b"ACGTACGT"])
    try:
        for bad in ([b"ACXG"], [b"ACG", b""], [b"AC G"]):
            with pytest.raises(_lib.KgmaError) as ei:
                ctx.exact_match(g, bad)
            assert ei.value.status == _lib.KGMA_E_ARG
        ctx.exact_match(g, [b"ACG"])
        assert triples(ctx) == [(0, 0, 1), (0, 0, 5)]
    finally:
        g.free()


def test_overlap_modes(ctx):
    assert [s for _, _, s in device_list(ctx, [b"A" * 10], [b"AAAA"], True)] == [1, 2, 3, 4, 5, 6, 7]
    assert [s for _, _, s in device_list(ctx, [b"A" * 10], [b"AAAA"], False)] == [1, 5]
    recs = [b"GAGAGAGAGAG", b"CGAGAGAGAAGGCCGAGCTTTT", b"GA" * 300 + b"G", b"N" * 100]
    check(ctx, recs, [b"GAGAG", b"GAG", b"AGA", b"GAGAGAGAGAGAGAGAGAGAG", b"NNN", b"GA" * 20])


def test_result_outgrows_the_buffer(ctx):
    g = ctx.genome_synthetic([4_000_000, 1_000_003], 91)
    try:
        text = [g.fetch(0, 1, 4_000_000), g.fetch(1, 1, 1_000_003)]
        ctx.exact_match(g, [b"A"])
        got, st = triples(ctx), ctx.stats()
        want = eo.match_list([b"A"], text)
        assert len(want) > 1_000_000 and len(got) == len(want) and got == want
        assert st["n_launches"] == 2 and st["bases_scanned"] == 5_000_003 and st["scan_ms"] > 0       # counted, regrown, run again
        ctx.exact_match(g, [b"A"], overlap=False)
        assert triples(ctx) == want and ctx.stats()["n_launches"] == 1                               # the buffer is kept
    finally:
        g.free()


# ---- batches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Loci.fasta", "Alp_V_ref.fasta"])
def test_batch_of_all_fixture_genes(ctx, genes, name):
    path = os.path.join(DATA, name)
    recs = fasta.read_fasta(path)
    dev = ctx.genome_from_fasta(path)
    try:
        for overlap in (False, True):
            batch = api.exactMatch_batch(genes, dev, overlap=overlap, ctx=ctx)
            assert triples(ctx) == eo.match_list(genes, [r.sequence for r in recs], overlap)
            assert batch == [api.exactMatch(q, dev, overlap=overlap, ctx=ctx) for q in genes]
        assert api.exactMatch_batch(genes, path, ctx=ctx) == batch
        if name == "Alp_V_ref.fasta":
            assert all(isinstance(b, dict) and recs[i].identifier in b for i, b in enumerate(batch))
        ctx.exact_match(dev, genes[:1])
        n1 = ctx.stats()["n_launches"]
        ctx.exact_match(dev, genes[:64])
        assert ctx.stats()["n_launches"] == n1 == 1
        ctx.exact_match(dev, genes)
        assert ctx.stats()["n_launches"] == 1
    finally:
        dev.free()


def test_scan_results_survive_a_search(alp_ref):
    c = _lib.Context(0)
    try:
        seqs = [r.sequence for r in fasta.read_fasta(os.path.join(DATA, "Loci.fasta"))]
        c.set_refs(6, [alp_ref["RV"]], [alp_ref["ws"]], [30.0], [alp_ref["N"]])
        g = c.genome_from_host(seqs)
        c.scan(g, _lib.MODE_SINGLE, 50, 0, _lib.F_RETURN_DISTS, None)
        hits, dips, d = c.hits(), c.dips(), c.dists(1)
        assert len(hits) > 0
        c.exact_match(g, [seqs[0][1000:1040], b"AAATT"])
        assert triples(c) == eo.match_list([seqs[0][1000:1040], b"AAATT"], seqs)
        assert c.hits() == hits and c.dips() == dips and np.array_equal(c.dists(1), d)
        c.scan(g, _lib.MODE_SINGLE, 50, 0, _lib.F_RETURN_DISTS, None)
        assert c.hits() == hits and c.dips() == dips and np.array_equal(c.dists(1), d)
        assert triples(c) == eo.match_list([seqs[0][1000:1040], b"AAATT"], seqs)        # kept until the next search
        g.free()
    finally:
        c.close()


# ---- both kernels ----------------------------------------------------------------------------------------------------------
def acgt_lists():
    """The match lists of the all-A/C/G/T cases, and the launches of a batch that mixes an A/C/G/T query with one holding N."""
    c = _lib.Context(0)
    try:
        recs, qs, _ = planted_case()
        out = {"planted": [device_list(c, recs, qs, ov) for ov in (True, False)]}
        out["runs"] = [device_list(c, [b"A" * 10, b"GAGAGAGAGAG", b"GA" * 300 + b"G"], [b"AAAA", b"GAGAG", b"GA" * 20], ov) for ov in (True, False)]
        g = c.genome_synthetic([1_500_000], 17)
        c.exact_match(g, [b"C", b"ACGTAC"])
        out["big"] = triples(c)
        c.exact_match(g, [b"ACGTAC", b"ACNT"])
        out["mixed_launches"] = c.stats()["n_launches"]
        g.free()
        return json.loads(json.dumps(out))
    finally:
        c.close()


def test_both_kernels_give_the_same_lists():
    assert "KGMA_EXACT_ASCII" not in os.environ
    here = acgt_lists()
    env = dict(os.environ, KGMA_EXACT_ASCII="1")
    code = ("import sys, json; sys.path[:0] = [%r, %r]; from tests import test_gpu_exact as t; "
            "print('RESULT ' + json.dumps(t.acgt_lists()))" % (ROOT, PKG))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    there = json.loads(line[len("RESULT "):])
    assert here["mixed_launches"] == 2 and there["mixed_launches"] == 1          # the switch took every query to the text kernel
    for key in ("planted", "runs", "big"):
        assert here[key] == there[key] and len(here[key]) > 0
    recs, qs, _ = planted_case()
    assert [tuple(x) for x in here["planted"][0]] == eo.match_list(qs, recs, True)


# ---- BASELINE sizes --------------------------------------------------------------------------------------------------------
def test_chr22_size(ctx, genes):
    g, _ = workloads.make_chr22_like(ctx, [x.upper() for x in genes], seed=22)
    try:
        L = workloads.CHR22_LEN
        rng = np.random.default_rng(2222)
        qs = [BASES[rng.integers(0, 4, size=int(rng.integers(40, 301)))].tobytes() for _ in range(64)]
        for i, q in enumerate(qs):                       # disjoint slots behind the leading run of N; the first one ends the record
            g.poke(0, 10_600_000 + 600_000 * i + int(rng.integers(0, 500_000)) if i else L - len(q) + 1, q)
        g.poke(0, 10_550_000, qs[5].lower())
        g.repack()
        text = b"".join(g.fetch(0, 1 + o, min(1 << 28, L - o)) for o in range(0, L, 1 << 28))
        edge = text.rindex(b"N" * 100, 0, 10_540_000) + 100              # first residue behind a run of N (0-based)
        qs += [text[edge - 5:edge + 40], text[edge - 1:edge + 63], b"N" * 20 + text[edge:edge + 30], qs[7][:8], qs[9][:16], qs[11][:17]]
        ctx.exact_match(g, qs)
        got = triples(ctx)
        want = eo.match_list(qs, [text])
        assert got == want
        assert {q for q, _, _ in want} >= set(range(64 + 3)) and (0, 0, L - len(qs[0]) + 1) in set(want)
        assert sum(1 for q, _, _ in want if q == 5) >= 2                   # the lower-case copy as well
    finally:
        g.free()


def test_grch38_size(ctx, genes):
    g, _, lens = workloads.make_grch38_like(ctx, [x.upper() for x in genes], seed=38, n_plants=8)
    try:
        rng = np.random.default_rng(3838)
        qs = [BASES[rng.integers(0, 4, size=int(rng.integers(40, 290)))].tobytes() for _ in range(16)]
        for i in (3, 9):                                   # two queries that hold an N: they take the residue-text kernel
            q = bytearray(qs[i]); q[len(q) // 2] = ord("N"); qs[i] = bytes(q)
        plants, slot = set(), 0
        for qi, q in enumerate(qs):                        # recorded positions, in slots that do not overlap
            for c in sorted({int(x) for x in rng.integers(0, len(lens), size=5)} | {qi % 25}):
                slot += 1
                pos = (lens[c] // 2 if slot & 1 else 10_500) + 2_000 * slot + int(rng.integers(0, 1_500)) if lens[c] > 1_000_000 else 2_000 + 300 * qi
                g.poke(c, pos, q)
                plants.add((qi, c, pos))
            g.poke(qi, lens[qi] - len(q) + 1, q)           # ... and one that ends its record
            plants.add((qi, qi, lens[qi] - len(q) + 1))
        g.repack()
        ctx.exact_match(g, qs)
        got, st = triples(ctx), ctx.stats()
        assert st["n_launches"] == 2 and st["bases_scanned"] == sum(lens)
        assert got == sorted(got) and len(set(got)) == len(got)
        assert len(plants) >= 16 * 3 and plants <= set(got)        # every plant is reported
        others = [t for t in got if t not in plants]
        for (qi, c, s), b in zip(others, g.fetch_batch([(c, s, len(qs[qi])) for qi, c, s in others])):
            assert b.upper() == qs[qi]
    finally:
        g.free()
