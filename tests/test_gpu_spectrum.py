"""K-mer counting on resident genomes on the device (kgma_genome_kmer_count / api.genome_spectrum / api.composition_track) against
the model (tests/spectrum_ref.py).

Every comparison is of the COMPLETE counts and n_skipped arrays, and every case asserts the form that ran.  The geometry -- the
span of each form -- is read from kgma_get_spectrum_stats; the forms are forced, and the workgroups capped, in fresh child
processes (the library reads its switches when it is loaded)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from kmergma_amd import _lib, api, fasta
from oracle import oracle as orc
from tests import spectrum_cases as cases
from tests import spectrum_ref as model
from tests import twobit_ref as tb
from tests.conftest import DATA, PKG, ROOT

pytestmark = pytest.mark.gpu
LOCI = os.path.join(DATA, "Loci.fasta")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)          # no references are ever set on this context: counting needs none
    yield c
    c.close()


def probe_geometry(ctx):
    """{form: span} as the library reports them: `wg` from a whole long record at k = 6, `wave` from 1000-base bins at k = 1,
    `global` from k = 8 (in a child process with a forced form: whatever that form reports)."""
    g = ctx.genome_from_host([b"ACGT" * 17_500])
    spans = {}
    try:
        for k, ranges in ((6, [(0, 1, 70_000)]), (1, [(0, lo, lo + 999) for lo in range(1, 70_000, 1000)]), (8, [(0, 1, 70_000)])):
            ctx.genome_kmer_count(g, k, [r[0] for r in ranges], [r[1] for r in ranges], [r[2] for r in ranges])
            st = ctx.spectrum_stats()
            assert st["span"] >= 64 and st["span"] % 64 == 0 and st["n_launches"] == 1 and st["n_workgroups"] >= 1
            spans[st["form"]] = st["span"]
    finally:
        g.free()
    return spans


@pytest.fixture(scope="module")
def spans(ctx):
    s = probe_geometry(ctx)
    assert sorted(s) == [cases.FORM_WG, cases.FORM_WAVE, cases.FORM_GLOBAL]          # the unforced choices
    return s


def run(ctx, g, case):
    cols = [[r[i] for r in case.ranges] for i in range(3)]
    return ctx.genome_kmer_count(g, case.k, cols[0], cols[1], cols[2], case.flags)


def check_on(ctx, g, case, form=None, max_wgs=None):
    """The case on the open genome g: the complete arrays, or the error with its record and position; then the form."""
    want = cases.expected(case)
    if isinstance(want, model.BadBase):
        with pytest.raises(_lib.BadBaseError) as e:
            run(ctx, g, case)
        assert e.value.status == _lib.KGMA_E_BADBASE and f"record {want.record} position {want.position}:" in str(e.value), (case.name, str(e.value))
        assert (want.record, want.position) == case.bad
        assert ctx.spectrum_stats()["n_launches"] == 0
        return None
    assert case.bad is None, case.name
    counts, skipped = run(ctx, g, case)
    st = ctx.spectrum_stats()
    diff = np.argwhere(counts != want[0])
    assert diff.size == 0, (case.name, st, diff[:3].tolist(), [(int(counts[tuple(d)]), int(want[0][tuple(d)])) for d in diff[:3]])
    assert np.array_equal(skipped, want[1]), (case.name, st, skipped.tolist()[:10], want[1].tolist()[:10])
    assert st["n_ranges"] == len(case.ranges) and st["n_positions"] == int(model.n_considered(case.records, case.k, case.ranges, case.flags).sum())
    if form is not None:
        assert st["form"] == form and ctx.kernel_name() == f"spectrum_kernel<{cases.FORM_NAMES[form]}>", (case.name, st, ctx.kernel_name())
    if max_wgs is not None:
        assert 1 <= st["n_workgroups"] <= max_wgs, (case.name, st)
    return counts, skipped


def check(ctx, case, form=None, max_wgs=None):
    g = ctx.genome_from_host(case.records)
    try:
        return check_on(ctx, g, case, form, max_wgs)
    finally:
        g.free()


def forms_of(k):
    """The forms the library chooses unforced at k, with the mean range length that makes it choose them."""
    return [cases.FORM_GLOBAL] if k >= 8 else [cases.FORM_WG] if k >= 5 else [cases.FORM_WAVE, cases.FORM_WG]


def core_checks(ctx, spans, k, form, forced=False, max_wgs=None, flag_sets=cases.FLAG_SETS):
    """The flag sets of the core case at one k in one form, on one upload of its records."""
    span = spans[form]
    mean = 1.25 * span if form == cases.FORM_WG and not forced else None
    first = cases.core_case(k, span, 0, mean_at_least=mean)
    g = ctx.genome_from_host(first.records)
    try:
        for flags in flag_sets:
            c = cases.core_case(k, span, flags, mean_at_least=mean)
            assert c.records == first.records
            check_on(ctx, g, c, form, max_wgs)
    finally:
        g.free()


# ---- every k, every range shape, every flag set, in the forms the library chooses ------------------------------------------
@pytest.mark.parametrize("k", range(1, 11))
def test_core_case_in_the_chosen_forms(ctx, spans, k):
    for form in forms_of(k):
        core_checks(ctx, spans, k, form)


@pytest.mark.parametrize("k,width,length", [(1, 1, 3000), (3, 1, 3000), (2, 7, None), (6, 7, 3000), (1, 1000, None), (2, 1000, None),
                                            (6, 1000, None), (8, 1000, None), (4, "span+1", None), (7, "span+1", None)])
def test_by_start_tilings_sum_to_the_whole_record(ctx, spans, k, width, length):
    form_span = spans[cases.FORM_GLOBAL if k >= 8 else cases.FORM_WAVE if k <= 4 else cases.FORM_WG]
    width = form_span + 1 if width == "span+1" else width
    for flags in (model.BY_START, model.BY_START | model.SKIP_N | model.SKIP_MASKED):
        c = cases.tiling_case(k, form_span, width, flags, length)
        counts, skipped = check(ctx, c)
        n = len(c.records)
        rec_of = np.array([r[0] for r in c.ranges[:-n]])
        for r in range(n):
            assert np.array_equal(counts[:-n][rec_of == r].sum(axis=0), counts[-n:][r])
            assert skipped[:-n][rec_of == r].sum() == skipped[-n:][r]
        # at the record's end the starts whose k-mer would pass L are not considered
        assert counts[-n:].sum(axis=1).tolist() == [len(r) - k + 1 - int(s) for r, s in zip(c.records, skipped[-n:])]


# ---- alphabet ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 3, 6, 8))
def test_iupac_codes(ctx, spans, k):
    form = forms_of(k)[0]
    for c in cases.iupac_cases(k, spans[form]):
        check(ctx, c)


def test_a_bad_base_leaves_the_context_usable(ctx, spans):
    c = cases.iupac_cases(2, spans[cases.FORM_WAVE])[0]
    check(ctx, c)
    check(ctx, c._replace(flags=model.SKIP_N, bad=None))


def test_twobit_mask_blocks(ctx, tmp_path):
    rng = np.random.default_rng(21)
    recs = [cases.masked_record(rng, 6000), cases.masked_record(rng, 2111)]
    p = tmp_path / "masked.2bit"
    tb.write_twobit(p, [(f"r{i}", r) for i, r in enumerate(recs)])
    whole = [(c, 1, len(r)) for c, r in enumerate(recs)]
    g, plain = ctx.genome_from_2bit(str(p)), ctx.genome_from_2bit(str(p), mask=False)
    try:
        assert [g.fetch(c, 1, len(r)) for c, r in enumerate(recs)] == recs
        for k in (1, 2, 5):
            for flags in (0, model.SKIP_MASKED, model.SKIP_N | model.SKIP_MASKED):
                masked = check_on(ctx, g, cases.Case("masked", recs, k, whole, flags, None))
                upper = check_on(ctx, plain, cases.Case("unmasked", [r.upper() for r in recs], k, whole, flags, None))
                assert (masked[1] > upper[1]).all() if flags & model.SKIP_MASKED else np.array_equal(masked[0], upper[0])
    finally:
        g.free()
        plain.free()
    tracks = api.composition_track(str(p), 500, 1, skip_masked=True, ctx=ctx)
    assert [t.identifier for t in tracks] == ["r0", "r1"] and [len(t.counts) for t in tracks] == [12, 5]
    assert tracks[0].skipped[2] == 500 and tracks[0].skipped[3] == 499          # residues 1001 ... 1999 are masked
    assert np.array_equal(api.genome_spectrum(str(p), 1, skip_masked=True, ctx=ctx), sum(t.counts.sum(axis=0) for t in tracks))


# ---- contention and counter width ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (2, 6, 8))
def test_contention_and_counter_width(ctx, k):
    for c in cases.contention_cases(k):
        counts, _ = check(ctx, c, cases.FORM_GLOBAL if k >= 8 else cases.FORM_WG)
        assert counts[0, 0] == 70_000 - k + 1 > 65_535


# ---- the forms -----------------------------------------------------------------------------------------------------------------
def test_unforced_choices(ctx):
    rng = np.random.default_rng(5)
    recs = [cases.rand_dna(rng, 40_000), cases.rand_dna(rng, 12_345)]
    g = ctx.genome_from_host(recs)
    try:
        for k in (1, 2):
            tracks = api.composition_track(g, 1000, k, ctx=ctx)
            st = ctx.spectrum_stats()
            assert st["form"] == cases.FORM_WAVE and st["n_ranges"] == 40 + 13 and ctx.kernel_name() == "spectrum_kernel<wave>"
            ranges = [(c, lo, min(lo + 999, len(r))) for c, r in enumerate(recs) for lo in range(1, len(r) + 1, 1000)]
            want = model.kmer_count(recs, k, ranges, model.SKIP_N | model.BY_START)
            assert np.array_equal(np.concatenate([t.counts for t in tracks]), want[0])
        check_on(ctx, g, cases.Case("whole", recs, 6, [(0, 1, 40_000), (1, 1, 12_345)], 0, None), cases.FORM_WG)
        check_on(ctx, g, cases.Case("whole", recs, 8, [(0, 1, 40_000), (1, 1, 12_345)], 0, None), cases.FORM_GLOBAL)
        stats = ctx.stats()
        assert stats["n_launches"] == 1 and stats["scan_ms"] == ctx.spectrum_stats()["count_ms"] > 0
    finally:
        g.free()


FORCED_FLAG_SETS = (0, model.SKIP_N | model.SKIP_MASKED, model.BY_START | model.SKIP_N | model.SKIP_MASKED)


def forced_suite(form: int, max_wgs=None) -> dict:
    """Runs in a child process whose environment forces `form` (and caps the workgroups): the core case at every k the form
    serves, a tiling and the contention cases."""
    c = _lib.Context(0)
    try:
        spans = probe_geometry(c)
        assert form in spans, spans                      # (a forced form is taken where k allows it: `wave` not at k = 6 and 8)
        for k in cases.FORM_KS[form]:
            core_checks(c, spans, k, form, forced=True, max_wgs=max_wgs, flag_sets=FORCED_FLAG_SETS)
        k = max(kk for kk in cases.FORM_KS[form] if kk <= 6)
        for case in cases.contention_cases(k) + [cases.tiling_case(2, spans[form], 1000), cases.tiling_case(k, spans[form], spans[form] + 1)]:
            check(c, case, form, max_wgs)
        return {"form": form, "span": spans[form], "ks": list(cases.FORM_KS[form])}
    finally:
        c.close()


@pytest.mark.parametrize("form", (cases.FORM_WG, cases.FORM_WAVE, cases.FORM_GLOBAL), ids=cases.FORM_NAMES)
@pytest.mark.parametrize("max_wgs", (None, 2), ids=("all_wgs", "two_wgs"))
def test_every_form_forced_at_every_k(form, max_wgs):
    assert "KGMA_SPECTRUM_FORM" not in os.environ and "KGMA_SPECTRUM_WGS" not in os.environ
    env = dict(os.environ, KGMA_SPECTRUM_FORM=cases.FORM_NAMES[form])
    if max_wgs:
        env["KGMA_SPECTRUM_WGS"] = str(max_wgs)
    code = ("import sys, json; sys.path[:0] = [%r, %r]; from tests import test_gpu_spectrum as t; "
            "print('RESULT ' + json.dumps(t.forced_suite(%d, %r)))" % (ROOT, PKG, form, max_wgs))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert got["form"] == form and got["ks"] == list(cases.FORM_KS[form])


# ---- agreement with what exists ------------------------------------------------------------------------------------------------
def test_whole_records_equal_kmer_count_batch_and_the_oracle(ctx, loci):
    seqs = [r.sequence for r in loci]
    g = ctx.genome_from_fasta(LOCI)
    try:
        fetched = g.fetch_batch([(c, 1, len(s)) for c, s in enumerate(seqs)])
        assert fetched == seqs
        for k in range(1, 9):
            counts, skipped = ctx.genome_kmer_count(g, k, list(range(len(seqs))), [1] * len(seqs), [len(s) for s in seqs])
            batch = ctx.kmer_count_batch(fetched, k)
            assert np.array_equal(counts, batch.astype(np.int64)) and np.array_equal(counts.astype(np.float64), batch) and not skipped.any()
            for c, s in enumerate(seqs):
                assert np.array_equal(counts[c], orc.kmer_count(s, k).astype(np.int64)), (k, c)
    finally:
        g.free()


# ---- state and errors ----------------------------------------------------------------------------------------------------------
def test_a_call_leaves_every_earlier_result_untouched(alp_ref, loci):
    seqs = [r.sequence for r in loci]
    c = _lib.Context(0)
    try:
        c.set_refs(6, [alp_ref["RV"]], [alp_ref["ws"]], [30.0], [alp_ref["N"]])
        g = c.genome_from_host(seqs)
        c.scan(g, _lib.MODE_SINGLE, 50, 0, _lib.F_RETURN_DISTS, None)
        c.exact_match(g, [seqs[0][100:130]])
        before = (c.hits(), c.dips(), c.dists(1).copy(), c.matches().copy(), c.stats())
        assert before[0] and len(before[3]) >= 1
        counts, _ = c.genome_kmer_count(g, 6, [0], [1], [len(seqs[0])])
        assert np.array_equal(counts[0], orc.kmer_count(seqs[0], 6).astype(np.int64))
        after = (c.hits(), c.dips(), c.dists(1), c.matches(), c.stats())
        assert after[0] == before[0] and after[1] == before[1] and np.array_equal(after[2], before[2]) and np.array_equal(after[3], before[3])
        changed = {key for key in before[4] if before[4][key] != after[4][key]}
        assert changed <= {"scan_ms", "n_launches"} and after[4]["n_launches"] == 1
        c.scan(g, _lib.MODE_SINGLE, 50, 0, 0, None)                                   # the references are still there
        assert c.hits() == before[0]
        g.free()
    finally:
        c.close()


def test_empty_calls(ctx):
    g = ctx.genome_from_host([b"ACGTNACGT", b"A"])
    try:
        counts, skipped = ctx.genome_kmer_count(g, 3, [], [], [])
        assert counts.shape == (0, 64) and skipped.shape == (0,) and ctx.spectrum_stats()["n_ranges"] == 0
        counts, skipped = ctx.genome_kmer_count(g, 3, [0, 1, 0], [4, 1, 10], [3, 0, 9])      # nothing but empty ranges
        assert counts.shape == (3, 64) and not counts.any() and not skipped.any()
        st = ctx.spectrum_stats()
        assert st["n_ranges"] == 3 and st["n_positions"] == 0 and st["n_launches"] == 0
        counts, skipped = ctx.genome_kmer_count(g, 3, [0], [1], [9], _lib.COUNT_SKIP_N)
        assert counts.sum() == 4 and skipped.tolist() == [3]
    finally:
        g.free()


def test_argument_errors_come_with_their_messages(ctx):
    g = ctx.genome_from_host([b"ACGTACGTAC", b"ACGT"])
    L = _lib.load()
    one = (C.c_int32 * 1)(0), (C.c_int64 * 1)(1), (C.c_int64 * 1)(4), (C.c_int64 * 4)(), (C.c_int64 * 1)()

    def raw(k=1, flags=0, n=1, contig=one[0], lo=one[1], hi=one[2], counts=one[3], skipped=one[4], genome=g._h, handle=ctx._h):
        return L.kgma_genome_kmer_count(handle, genome, k, flags, n, contig, lo, hi, counts, skipped)

    try:
        assert raw() == _lib.KGMA_OK and list(one[3]) == [1, 1, 1, 1]
        assert raw(skipped=None) == _lib.KGMA_OK
        for kw in (dict(handle=None), dict(genome=None), dict(contig=None), dict(lo=None), dict(hi=None), dict(counts=None), dict(n=-1)):
            assert raw(**kw) == _lib.KGMA_E_ARG, kw
        assert L.kgma_get_spectrum_stats(ctx._h, None) == _lib.KGMA_E_ARG and L.kgma_get_spectrum_stats(None, None) == _lib.KGMA_E_ARG
        for args, status, words in (((0, [0], [1], [4], 0), _lib.KGMA_E_ARG, "k = 0"),
                                    ((-1, [0], [1], [4], 0), _lib.KGMA_E_ARG, "k = -1"),
                                    ((11, [0], [1], [4], 0), _lib.KGMA_E_UNSUPPORTED, "k = 11"),
                                    ((2, [0], [1], [4], 8), _lib.KGMA_E_ARG, "unknown flag bits 0x8"),
                                    ((2, [0], [1], [4], 0x80000001), _lib.KGMA_E_ARG, "unknown flag bits"),
                                    ((2, [0, 2], [1, 1], [4, 4], 0), _lib.KGMA_E_ARG, "range 1: no record 2"),
                                    ((2, [0, -1], [1, 1], [4, 4], 0), _lib.KGMA_E_ARG, "range 1: no record -1"),
                                    ((2, [1, 0], [1, 0], [4, 4], 0), _lib.KGMA_E_ARG, "range 1: 0:4 outside record 0 of 10 residues"),
                                    ((2, [1], [1], [5], 0), _lib.KGMA_E_ARG, "range 0: 1:5 outside record 1 of 4 residues"),
                                    ((2, [0, 0, 0], [1, 5, 5], [4, 4, 3], 0), _lib.KGMA_E_ARG, "range 2: 5:3 outside record 0"),
                                    ((10, [0] * 257, [1] * 257, [4] * 257, 0), _lib.KGMA_E_UNSUPPORTED, "more than 2^28 counts")):
            k, contig, lo, hi, flags = args
            with pytest.raises(_lib.KgmaError) as e:
                ctx.genome_kmer_count(g, k, contig, lo, hi, flags)
            assert e.value.status == status and words in str(e.value), (args[0], str(e.value))
            assert ctx.spectrum_stats()["n_ranges"] == 0
        counts, _ = ctx.genome_kmer_count(g, 10, [0] * 256, [1] * 256, [10] * 256)     # exactly 2^28 counts
        assert counts.shape == (256, 4 ** 10) and (counts.sum(axis=1) == 1).all()
    finally:
        g.free()


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
def test_fixture_spectrum_background_and_pwm(ctx, loci):
    seqs = [r.sequence for r in loci]
    n = np.array([sum(s.upper().count(b) for s in seqs) for b in (b"A", b"C", b"G", b"T")], dtype=np.int64)
    assert np.array_equal(api.genome_spectrum(LOCI, 1, ctx=ctx), n)
    both = n + n[::-1]
    assert np.array_equal(api.genome_spectrum(LOCI, 1, strand="both", ctx=ctx), both)
    bg = api.genome_background(LOCI, ctx=ctx)
    assert np.array_equal(bg, both / both.sum()) and np.array_equal(api.genome_background(LOCI, strand="+", ctx=ctx), n / n.sum())
    rc = [fasta.reverse_complement(s) for s in seqs]
    assert np.array_equal(api.genome_spectrum(LOCI, 4, strand="-", ctx=ctx),
                          model.kmer_count(rc, 4, [(c, 1, len(s)) for c, s in enumerate(rc)], model.SKIP_N)[0].sum(axis=0))
    site = seqs[0][1000:1012].upper()
    assert set(site) <= set(b"ACGT")
    W = api.pwm_from_sequences([site, site, site, site[:5] + (b"A" if site[5:6] != b"A" else b"C") + site[6:]])
    g = ctx.genome_from_fasta(LOCI)
    try:
        found = api.pwmMatch(W, g, pvalue=1e-6, background="genome", strand="both", ctx=ctx)
        thr = api.pwm_threshold(W, 1e-6, bg)
        assert found == api.pwmMatch(W, g, threshold=thr, strand="both", ctx=ctx)
        assert any(h[0] == 0 and h[2] == 1001 and h[4] == "+" for h in found)
    finally:
        g.free()
