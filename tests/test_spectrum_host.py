"""K-mer counting on resident genomes without a device: the model (tests/spectrum_ref.py) checked against the oracle and the
goldens, its invariants, the GPU tests' case lists shown to hit what they are for, and the Python layer -- genome_spectrum,
genome_background, composition_track and its helpers, pwmMatch(background=) -- over a context that answers with the model."""
import os
import types

import numpy as np
import pytest

from kmergma_amd import _lib, api, fasta
from kmergma_amd.fasta import Record
from oracle import oracle as orc
from tests import spectrum_cases as cases
from tests import spectrum_ref as model
from tests.conftest import DATA

LOCI = os.path.join(DATA, "Loci.fasta")


# ---- the model is itself checked --------------------------------------------------------------------------------------------
def test_model_equals_the_oracle_on_whole_sequences(loci):
    rng = np.random.default_rng(1)
    seqs = [r.sequence for r in loci] + [cases.rand_dna(rng, n) for n in (0, 1, 5, 8, 9, 300, 4097)]
    seqs.append(cases.rand_dna(rng, 500).lower() + b"NnNN" + cases.rand_dna(rng, 200))
    for k in range(1, 9):
        counts, skipped = model.kmer_count(seqs, k, [(c, 1, len(s)) for c, s in enumerate(seqs)], 0)
        assert not skipped.any()
        for c, s in enumerate(seqs):
            assert np.array_equal(counts[c], orc.kmer_count(s, k).astype(np.int64)), (k, c)


def test_model_equals_the_goldens(golden):
    g = golden["kmers"]
    seq = g["test_seq"].encode()
    for k in (1, 2):
        counts, _ = model.kmer_count([seq], k, [(0, 1, len(seq))], 0)
        assert counts[0].tolist() == [int(x) for x in g[f"kmer_count_k{k}"]]


def test_model_ranges_are_views():
    rng = np.random.default_rng(2)
    seq = cases.rand_dna(rng, 400) + b"NN" + cases.rand_dna(rng, 100)
    for k in (1, 3, 6):
        for lo, hi in ((1, 400), (17, 16), (17, 17 + k - 2), (300, 502), (502, 502)):
            counts, _ = model.kmer_count([seq], k, [(0, lo, hi)], 0)
            assert np.array_equal(counts[0], orc.kmer_count(seq[lo - 1:hi], k).astype(np.int64)), (k, lo, hi)


def test_model_bad_base_rule():
    recs = [b"ACGTRACGT", b"ACGTAC*T"]
    with pytest.raises(model.BadBase) as e:
        model.kmer_count(recs, 2, [(1, 1, 8), (0, 1, 9)], 0)
    assert (e.value.record, e.value.position) == (0, 5)
    assert model.kmer_count(recs, 2, [(0, 1, 4), (0, 6, 9), (1, 1, 6)], 0)[0].sum() == 3 + 3 + 5
    with pytest.raises(model.BadBase):
        model.kmer_count(recs, 3, [(0, 5, 5)], 0)                           # shorter than k: still looked up
    with pytest.raises(model.BadBase):
        model.kmer_count(recs, 2, [(0, 4, 4)], model.BY_START)              # the k - 1 residues behind hi are covered
    counts, skipped = model.kmer_count(recs, 2, [(0, 1, 9), (1, 1, 8)], model.SKIP_N)
    assert skipped.tolist() == [2, 2] and counts.sum(axis=1).tolist() == [6, 5]


# ---- invariants ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", model.ALL_FLAGS)
def test_row_sum_plus_skipped_is_the_number_of_considered_starts(flags):
    for k in (1, 2, 5):
        for form in (cases.FORM_WAVE,):
            c = cases.core_case(k, cases.HOST_SPANS[form], flags | model.SKIP_N)
            counts, skipped = cases.expected(c)
            assert np.array_equal(counts.sum(axis=1) + skipped, model.n_considered(c.records, k, c.ranges, c.flags))
    rng = np.random.default_rng(3)
    rec = cases.masked_record(rng)
    ranges = [(0, 1, len(rec)), (0, 990, 2010), (0, 1495, 1525), (0, 5, 4)]
    counts, skipped = model.kmer_count([rec], 3, ranges, flags)
    assert np.array_equal(counts.sum(axis=1) + skipped, model.n_considered([rec], 3, ranges, flags))
    if flags & (model.SKIP_N | model.SKIP_MASKED):
        assert skipped[0] > 0
    else:
        assert not skipped.any()


@pytest.mark.parametrize("k", (1, 2, 6))
def test_by_start_rows_over_a_tiling_sum_to_the_whole_record(k):
    for width in (1, 7, 1000, cases.HOST_SPANS[cases.FORM_WAVE] + 1):
        c = cases.tiling_case(k, cases.HOST_SPANS[cases.FORM_WAVE], width, model.BY_START | model.SKIP_MASKED)
        counts, skipped = cases.expected(c)
        n = len(c.records)
        whole = counts[-n:]
        rec_of = np.array([r[0] for r in c.ranges[:-n]])
        for r in range(n):
            assert np.array_equal(counts[:-n][rec_of == r].sum(axis=0), whole[r])
            assert skipped[:-n][rec_of == r].sum() == skipped[-n:][r]
        # BY_START on a whole record is the default on a whole record
        plain = model.kmer_count(c.records, k, c.ranges[-n:], c.flags & ~model.BY_START)
        assert np.array_equal(plain[0], whole)


# ---- no case is vacuous -------------------------------------------------------------------------------------------------------
def test_the_core_case_sits_on_the_seams():
    for form, span in cases.HOST_SPANS.items():
        for k in (1, 4, 7, 10):
            if k not in cases.FORM_KS[form]:
                continue
            c = cases.core_case(k, span, 0, mean_at_least=1.25 * cases.HOST_SPANS[cases.FORM_WG] if form == cases.FORM_WG else None)
            n = model.n_considered(c.records, k, c.ranges, 0).tolist()
            assert 3 * span + 1 in n and span in n and len(c.ranges) <= cases.max_ranges(k)
            if k < 9:
                assert span - 1 in n and span + 1 in n
            if k < 8:
                assert {r[1] % 16 for r in c.ranges} == set(range(16))
                assert sum(1 for x in n if x == 0) >= 3 and 1 in n and 2 in n
                assert len(set(c.ranges)) < len(c.ranges) and sorted(c.ranges) != c.ranges and {r[0] for r in c.ranges} == {0, 1}
                if form != cases.FORM_GLOBAL:                                  # (unforced, the case runs in the form it was built for)
                    assert cases.auto_form(k, sum(n), len(n)) == form, (form, k)
            rec = c.records[0]
            assert rec[4 + span - 1:4 + span] == b"N" and rec[4 + 2 * span - 1:4 + 2 * span + 1] == b"NN" and rec[4 + 3 * span:4 + 3 * span + 1].islower()


def test_the_contention_cases_pass_a_16_bit_counter():
    for c in cases.contention_cases():
        counts, skipped = cases.expected(c)
        assert counts[0].max() == 70_000 - 5 > 65_535 and counts[0, 0] == counts[0].sum()
        if c.flags == 0:
            assert counts[1, -1] == 70_000 - 5 and not skipped.any()            # N counts as T
        else:
            assert counts[1].sum() == 0 and skipped[1] == 70_000 - 5
        assert sorted(counts[2][counts[2] > 0].tolist()) == [34_997, 34_998]    # ACACAC / CACACA alternate
        assert counts[3, -1] > 65_535


def test_every_iupac_case_is_bad_where_it_says():
    for c in cases.iupac_cases(3, 1024):
        got = cases.expected(c)
        if c.bad is None:
            assert not isinstance(got, model.BadBase), c.name
        else:
            assert isinstance(got, model.BadBase) and (got.record, got.position) == c.bad, c.name
    skipped = cases.expected(cases.iupac_cases(3, 1024)[2])[1]
    assert skipped.tolist() == [3, 3, 3]


# ---- the Python layer over a context that answers with the model --------------------------------------------------------------
class FakeGenome(_lib.Genome):
    def __init__(self, records):
        self.records = [bytes(r) for r in records]
        self._h = None
        self._ctx = types.SimpleNamespace(_h=None)

    n_contigs = property(lambda self: len(self.records))

    def contig_len(self, c):
        return len(self.records[c])

    def header(self, contig):
        raise _lib.KgmaError(_lib.KGMA_E_STATE, "no headers")

    def free(self):
        pass


class FakeContext:
    def __init__(self):
        self.calls = []
        self.pwm = []

    def genome_from_host(self, seqs):
        return FakeGenome(seqs)

    def genome_kmer_count(self, genome, k, contig, lo, hi, flags=0):
        self.calls.append((k, len(list(contig)), flags))
        return model.kmer_count(genome.records, k, list(zip(contig, lo, hi)), flags)

    def pwm_match(self, genome, matrices, thresholds):
        self.pwm.append([int(t) for t in thresholds])

    def pwm_matches(self):
        return np.zeros(0, dtype=np.int64)


RECS = [Record("one first record", b"ACGTTGCANNacgtACGGGT"), Record("two", b"TTTTACGTAGGCCA"), Record("three", b"G")]


def test_genome_kmer_count_defaults_to_whole_records():
    ctx = FakeContext()
    counts, skipped = api.genome_kmer_count(RECS, 2, ctx=ctx)
    want = model.kmer_count([r.sequence for r in RECS], 2, [(c, 1, len(r.sequence)) for c, r in enumerate(RECS)], 0)
    assert np.array_equal(counts, want[0]) and counts.shape == (3, 16) and not skipped.any()
    counts, skipped = api.genome_kmer_count(RECS, 2, [(1, 2, 9), (0, 1, 20)], skip_n=True, skip_masked=True, by_start=True, ctx=ctx)
    assert ctx.calls == [(2, 3, 0), (2, 2, 7)] and skipped.tolist() == [0, 7]
    for bad in (b"ACGT", RECS[0], None, 12):
        with pytest.raises(TypeError, match="subject"):
            api.genome_kmer_count(bad, 2, ctx=ctx)
    for k in (0, 11):
        with pytest.raises(ValueError, match="k = "):
            api.genome_kmer_count(RECS, k, ctx=ctx)


@pytest.mark.parametrize("k", (1, 2, 3, 5))
def test_the_minus_strand_is_the_reverse_complement_permutation(k, loci):
    ctx = FakeContext()
    rng = np.random.default_rng(k)
    recs = [Record("a", cases.masked_record(rng, 700)), Record("b", cases.rand_dna(rng, 301) + b"N"), Record("c", loci[0].sequence[:2000])]
    rc = [model.reverse_complement(r.sequence) for r in recs]
    for skip_masked in (False, True):
        flags = model.SKIP_N | (model.SKIP_MASKED if skip_masked else 0)
        plus = model.kmer_count([r.sequence for r in recs], k, [(c, 1, len(r.sequence)) for c, r in enumerate(recs)], flags)[0].sum(axis=0)
        minus = model.kmer_count(rc, k, [(c, 1, len(s)) for c, s in enumerate(rc)], flags)[0].sum(axis=0)
        assert np.array_equal(api.genome_spectrum(recs, k, skip_masked=skip_masked, ctx=ctx), plus)
        assert np.array_equal(api.genome_spectrum(recs, k, skip_masked=skip_masked, strand="-", ctx=ctx), minus)
        assert np.array_equal(api.genome_spectrum(recs, k, skip_masked=skip_masked, strand="both", ctx=ctx), plus + minus)
    assert model.reverse_complement(b"AACGtn") == fasta.reverse_complement(b"AACGtn") == b"naCGTT"
    perm = api.revcomp_kmer_permutation(k)
    assert np.array_equal(perm[perm], np.arange(4 ** k)) and perm[0] == 4 ** k - 1
    with pytest.raises(ValueError, match="strand"):
        api.genome_spectrum(recs, k, strand="x", ctx=ctx)


def test_genome_background_normalises_symmetrises_and_raises_on_a_zero():
    ctx = FakeContext()
    recs = [Record("a", b"AAAACCGNNTtt"), Record("b", b"RYAC")]
    plus = api.genome_background(recs, strand="+", ctx=ctx)
    assert plus.tolist() == [5 / 12, 3 / 12, 1 / 12, 3 / 12] and ctx.calls[-1] == (1, 2, model.SKIP_N)
    both = api.genome_background(recs, ctx=ctx)
    assert both.tolist() == [8 / 24, 4 / 24, 4 / 24, 8 / 24] and both[0] == both[3] and both[1] == both[2]
    assert api.genome_background(recs, skip_masked=True, strand="+", ctx=ctx).tolist() == [5 / 10, 3 / 10, 1 / 10, 1 / 10]
    assert np.array_equal(api._background(both), both)                         # usable wherever background= is accepted
    with pytest.raises(ValueError, match="base G does not occur"):
        api.genome_background([Record("a", b"AACCTTNN")], strand="+", ctx=ctx)
    assert api.genome_background([Record("a", b"AACCTTNN")], ctx=ctx).tolist() == [1 / 3, 1 / 6, 1 / 6, 1 / 3]   # ("both": G from C)
    with pytest.raises(ValueError, match="does not occur"):
        api.genome_background([Record("a", b"AATTNN")], ctx=ctx)


def test_composition_track_bins_and_splits(monkeypatch):
    ctx = FakeContext()
    tracks = api.composition_track(RECS, 6, 2, ctx=ctx)
    assert [(t.identifier, t.bin, t.k, t.length, t.counts.shape) for t in tracks] == [("one", 6, 2, 20, (4, 16)), ("two", 6, 2, 14, (3, 16)), ("three", 6, 2, 1, (1, 16))]
    seqs = [r.sequence for r in RECS]
    for c, t in enumerate(tracks):
        ranges = [(c, lo, min(lo + 5, t.length)) for lo in range(1, t.length + 1, 6)]
        want = model.kmer_count(seqs, 2, ranges, model.SKIP_N | model.BY_START)
        assert np.array_equal(t.counts, want[0]) and np.array_equal(t.skipped, want[1])
        whole = model.kmer_count(seqs, 2, [(c, 1, t.length)], model.SKIP_N)
        assert np.array_equal(t.counts.sum(axis=0), whole[0][0]) and t.skipped.sum() == whole[1][0]
    assert ctx.calls == [(2, 8, model.SKIP_N | model.BY_START)]
    monkeypatch.setattr(_lib, "SPECTRUM_MAX_COUNTS", 3 * 16)                    # three ranges per call at k = 2
    split = api.composition_track(RECS, 6, 2, skip_n=False, skip_masked=True, ctx=ctx)
    assert ctx.calls[1:] == [(2, 3, 6), (2, 3, 6), (2, 2, 6)]
    assert [t.counts.shape for t in split] == [t.counts.shape for t in tracks]
    assert split[0].skipped.tolist() == [0, 3, 2, 0]
    with pytest.raises(ValueError, match="bin = 0"):
        api.composition_track(RECS, 0, ctx=ctx)


def _track(counts, k, width=10, length=None, skipped=None):
    counts = np.asarray(counts, dtype=np.int64)
    return api.CompositionTrack("chrT", counts, np.zeros(len(counts), dtype=np.int64) if skipped is None else np.asarray(skipped),
                                width, k, len(counts) * width if length is None else length)


def test_gc_fraction_and_cpg_on_hand_computed_tracks(tmp_path):
    t1 = _track([[1, 2, 3, 4], [0, 0, 0, 0], [5, 0, 0, 5]], 1, length=27)
    gc = api.gc_fraction(t1)
    assert gc[0] == 0.5 and np.isnan(gc[1]) and gc[2] == 0.0
    c2 = np.zeros((3, 16), dtype=np.int64)
    c2[0, [0, 6, 4, 9, 15]] = [4, 3, 1, 2, 10]        # AA 4, CG 3, CA 1, GC 2, TT 10: C* = 4, G* = 2, counted 20
    c2[1, [0, 5]] = [7, 3]                            # no G*: NaN
    c2[2, [6]] = [2]                                  # CG 2: C* = 2, G* = 0: NaN
    t2 = _track(c2, 2)
    assert api.gc_fraction(t2).tolist() == [6 / 20, 3 / 10, 1.0]
    oe = api.cpg_obs_exp(t2)
    assert oe[0] == 3 * 20 / (4 * 2) and np.isnan(oe[1]) and np.isnan(oe[2])
    with pytest.raises(ValueError, match="k = 2"):
        api.cpg_obs_exp(t1)
    path = tmp_path / "gc.bedgraph"
    api.write_composition_bedgraph([t1, t2], [gc, [0.1, 1 / 3, 2.0]], str(path))
    assert path.read_text() == ("chrT\t0\t10\t0.5\nchrT\t10\t20\tnan\nchrT\t20\t27\t0.0\n"
                                "chrT\t0\t10\t0.1\nchrT\t10\t20\t0.3333333333333333\nchrT\t20\t30\t2.0\n")
    with pytest.raises(ValueError, match="values"):
        api.write_composition_bedgraph([t1], [[1.0]], str(path))
    with pytest.raises(ValueError, match="one array"):
        api.write_composition_bedgraph([t1, t2], [gc], str(path))


def test_pwm_background_reaches_pwm_threshold(monkeypatch):
    seen = []
    real = api.pwm_threshold

    def spy(matrix, pvalue, *background):
        seen.append((float(pvalue), None if not background else np.asarray(background[0]).tolist()))
        return real(matrix, pvalue, *background)

    monkeypatch.setattr(api, "pwm_threshold", spy)
    ctx = FakeContext()
    W = api.pwm_from_sequences([b"ACGTAC", b"ACGTTC", b"ACGAAC"])
    subject = b"AAAAAAAATTTTTTTTACGTACCCGG"                       # A 10, C 4, G 3, T 9 -> both strands: 19, 7, 7, 19 of 52
    api.pwmMatch(W, subject, pvalue=1e-3, ctx=ctx)
    api.pwmMatch(W, subject, pvalue=1e-3, background=(0.3, 0.2, 0.2, 0.3), ctx=ctx)
    assert seen == [(1e-3, None), (1e-3, [0.3, 0.2, 0.2, 0.3])]
    del seen[:]
    api.pwmMatch(W, subject, pvalue=1e-3, background="genome", strand="both", ctx=ctx)
    assert seen[-1] == (1e-3, [19 / 52, 7 / 52, 7 / 52, 19 / 52]) and ctx.calls[-1] == (1, 1, model.SKIP_N)
    assert ctx.pwm[0] == [real(W, 1e-3)] and ctx.pwm[1] == [real(W, 1e-3, (0.3, 0.2, 0.2, 0.3))]
    assert ctx.pwm[2] == [real(W, 1e-3, (19 / 52, 7 / 52, 7 / 52, 19 / 52))] * 2
    api.findRSS_pwm(FakeGenome([subject]), W, pvalue=1e-2, background="genome", ctx=ctx)
    assert seen[-1] == (1e-2, [19 / 52, 7 / 52, 7 / 52, 19 / 52])
    n = len(ctx.pwm)
    with pytest.raises(ValueError, match="only together with pvalue"):
        api.pwmMatch(W, subject, threshold=100, background=(0.25, 0.25, 0.25, 0.25), ctx=ctx)
    with pytest.raises(ValueError, match="only together with pvalue"):
        api.pwmMatch_batch([W], FakeGenome([subject]), threshold=100, background="genome", ctx=ctx)
    with pytest.raises(ValueError, match="'genome'"):
        api.pwmMatch(W, subject, pvalue=1e-3, background="uniform", ctx=ctx)
    with pytest.raises(ValueError, match="four positive probabilities"):
        api.pwmMatch(W, subject, pvalue=1e-3, background=(0.5, 0.5, 0.0, 0.0), ctx=ctx)
    with pytest.raises(ValueError, match="does not occur"):
        api.pwmMatch(W, b"AAAATTTT", pvalue=1e-3, background="genome", ctx=ctx)
    assert len(ctx.pwm) == n                                        # no search ran


def test_the_library_exports_the_entry_points():
    assert {"kgma_genome_kmer_count", "kgma_get_spectrum_stats"} <= set(_lib.EXPORTS)
    assert _lib.C.sizeof(_lib.KgmaSpectrumStats) == 40
    assert (_lib.COUNT_SKIP_N, _lib.COUNT_SKIP_MASKED, _lib.COUNT_BY_START) == (model.SKIP_N, model.SKIP_MASKED, model.BY_START)
    assert (_lib.SPECTRUM_FORM_WG, _lib.SPECTRUM_FORM_WAVE, _lib.SPECTRUM_FORM_GLOBAL) == (cases.FORM_WG, cases.FORM_WAVE, cases.FORM_GLOBAL)
