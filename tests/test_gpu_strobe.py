"""The strobemer engine (kgma_set_strobe_ref / kgma_strobe_scan, api.StrobeGMA / api.Strobemer_findGenes) on the device
against the CPU restatement of the reference in tests/strobe_oracle.py.  No check here has a tolerance a measurement set:
  1. without chain replay, hits (contig, cmi, lo, hi, genome_pos, D) and every record's first-window D equal the EXACT oracle,
     and kgma_get_dists is D / (2 k N^2) bit for bit (what the existing distance tests assert for the integer form);
  2. with chain replay, hits equal the FLOAT oracle and `dist` is bit-equal on KGMA_HIT_CHAIN hits;
  3. wherever the two oracles' hit lists of a record differ, the unreplayed scan reports a flagged dip or an at-threshold
     window in that record (Loci.fasta, default parameters: exactly JQ684647.1).
"""
import functools
import os

import numpy as np
import pytest

from kmergma_amd import _lib, align, api, fasta, headers, refprep
from kmergma_amd.fasta import Record
from tests import strobe_oracle as so
from tests.conftest import DATA
from tests.helpers import make_genome, mutate, random_dna

pytestmark = pytest.mark.gpu

CONFIGS = [(2, 3, 5, 5), (3, 4, 7, 5), (1, 2, 4, 5), (2, 3, 5, 7), (2, 3, 5, 1)]
THRS = [20.0, 30.0, 40.0]
FIXTURES = ["Loci.fasta", "Alp_V_locus.fasta"]
REF = os.path.join(DATA, "Alp_V_ref.fasta")
FLAGGED = _lib.HIT_TIE | _lib.HIT_AT_THRESHOLD


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _ref(cfg):
    RV, W, cons, (S, N) = refprep.gen_ref_ws_cons_strobe(REF, *cfg, return_int=True)
    return dict(RV=RV, W=W, cons=cons, S=S, N=N, cfg=cfg, k=cfg[2] + cfg[0] - 1)


@functools.lru_cache(maxsize=None)
def _records(name):
    return fasta.read_fasta(os.path.join(DATA, name))


@functools.lru_cache(maxsize=None)
def _oracle(name, cfg, thr):
    r = _ref(cfg)
    return so.scan([x.sequence for x in _records(name)], r["RV"], r["S"], r["N"], *cfg, r["W"], thr, 50)


def _key(h):
    return (h["contig"], h["cmi"], h["lo"], h["hi"], h["genome_pos"], h["D"])


def _scan(ctx, seqs, ref, thr, flags=0, consensus=None, buff=50, gate=0, genome=None):
    ctx.set_strobe_ref(*ref["cfg"], ref["RV"], ref["W"], thr, ref["N"])
    g = genome if genome is not None else ctx.genome_from_host(seqs)
    try:
        ctx.strobe_scan(g, buff, flags, consensus, -69, -5, gate)
        out = dict(hits=ctx.hits(), first=ctx.first_window(1), dips=ctx.dips(), att=ctx.att(), stats=ctx.stats(),
                   dists=ctx.dists(1) if flags & _lib.F_RETURN_DISTS else None, name=ctx.kernel_name())
    finally:
        if genome is None:
            g.free()
    return out


class _Scores:
    """Host alignment of candidate ranges (kmergma_amd.align: the library's restatement of the reference's pairalign)."""

    def __init__(self, seqs, cons, W):
        self.seqs, self.cons, self.cache = seqs, cons[:W], {}

    def __call__(self, c, lo, hi):
        key = (c, lo, hi)
        if key not in self.cache:
            cigar, score = align.semiglobal_cigar(self.cons, self.seqs[c][lo - 1:hi], -69, -5)
            self.cache[key] = (score,) + tuple(align.cigar_to_UnitRange(cigar))
        return self.cache[key]

    def aligned(self, hits, gate):
        """process_hit! over the oracle's candidates: the gate, then the aligned range."""
        out = []
        for h in hits:
            score, first, last = self(h["contig"], h["lo"], h["hi"])
            if score < gate:
                continue
            h = dict(h)
            L = len(self.seqs[h["contig"]])
            h["lo"], h["hi"] = max(1, h["lo"] + first - 1), min(h["lo"] + last - 1, L)
            out.append(h)
        return out


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("name", FIXTURES)
def test_exact_parity(ctx, name, cfg):
    ref = _ref(cfg)
    seqs = [x.sequence for x in _records(name)]
    g = ctx.genome_from_host(seqs)
    sc = _Scores(seqs, ref["cons"], ref["W"])
    try:
        for thr in THRS:
            o = _oracle(name, cfg, thr)
            r = _scan(ctx, seqs, ref, thr, genome=g)
            assert r["name"] == f"strobe_kernel<{cfg[0]}>"
            assert r["first"].tolist() == o["first_D"]
            assert [_key(h) for h in r["hits"]] == [_key(h) for h in o["exact"]], thr
            scale = 2.0 * ref["k"] * ref["N"] ** 2
            assert all(h["kfv"] == 0 and h["dist"] == h["D"] / scale for h in r["hits"])
            # do_align = true, the reference's default gate of 0
            ra = _scan(ctx, seqs, ref, thr, consensus=ref["cons"], genome=g)
            assert [_key(h) for h in ra["hits"]] == [_key(h) for h in sc.aligned(o["exact"], 0)], thr
    finally:
        g.free()


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("name", FIXTURES)
def test_chain_parity(ctx, name, cfg):
    ref = _ref(cfg)
    seqs = [x.sequence for x in _records(name)]
    g = ctx.genome_from_host(seqs)
    sc = _Scores(seqs, ref["cons"], ref["W"])
    try:
        for thr in THRS:
            o = _oracle(name, cfg, thr)
            r = _scan(ctx, seqs, ref, thr, flags=_lib.F_CHAIN_REPLAY, genome=g)
            assert [_key(h) for h in r["hits"]] == [_key(h) for h in o["float"]], thr
            scale = 2.0 * ref["k"] * ref["N"] ** 2
            for a, b in zip(r["hits"], o["float"]):
                if a["flags"] & _lib.HIT_CHAIN:
                    assert a["dist"] == b["dist"]                      # the reference's running value, bit for bit
                else:
                    assert a["dist"] == a["D"] / scale
            ra = _scan(ctx, seqs, ref, thr, flags=_lib.F_CHAIN_REPLAY, consensus=ref["cons"], genome=g)
            assert [_key(h) for h in ra["hits"]] == [_key(h) for h in sc.aligned(o["float"], 0)], thr
    finally:
        g.free()


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("name", FIXTURES)
def test_differing_records_are_flagged(ctx, name, cfg):
    ref = _ref(cfg)
    recs = _records(name)
    seqs = [x.sequence for x in recs]
    g = ctx.genome_from_host(seqs)
    try:
        for thr in THRS:
            o = _oracle(name, cfg, thr)
            r = _scan(ctx, seqs, ref, thr, genome=g)
            flagged = {d["contig"] for d in r["dips"] if d["flags"] & FLAGGED} | {int(c) for c in r["att"][:, 0]}
            differ = [c for c, (e, f) in enumerate(o["per_record"]) if [_key(h) for h in e] != [_key(h) for h in f]]
            assert set(differ) <= flagged, (thr, differ, sorted(flagged))
            assert r["stats"]["n_tie_flagged"] == sum(1 for d in r["dips"] if d["flags"] & _lib.HIT_TIE)
            if name == "Loci.fasta" and cfg == (2, 3, 5, 5) and thr in (30.0, 40.0):
                # the fixture exercises the path: exactly one record's lists differ (1 against 3 hits at 30, 10 against 18 at 40)
                assert [recs[c].identifier for c in differ] == ["JQ684647.1"]
                e, f = o["per_record"][differ[0]]
                assert (len(e), len(f)) == ((1, 3) if thr == 30.0 else (10, 18))
    finally:
        g.free()


@pytest.mark.parametrize("cfg", [(2, 3, 5, 5), (3, 4, 7, 5), (1, 2, 4, 5)])
def test_dists_are_exact(ctx, cfg):
    """kgma_get_dists: one value per step i >= 1 in record order, the exact D over 2 k N^2 (bit for bit, as the integer form's
    k-mer tests assert)."""
    ref = _ref(cfg)
    seqs = [x.sequence for x in _records("Loci.fasta")]
    o = so.scan(seqs, ref["RV"], ref["S"], ref["N"], *cfg, ref["W"], 30.0, 50, return_dists=True)
    r = _scan(ctx, seqs, ref, 30.0, flags=_lib.F_RETURN_DISTS)
    assert len(r["dists"]) == sum(len(x) - ref["W"] - 1 for x in seqs if len(x) > ref["W"])
    assert np.array_equal(r["dists"], np.asarray(o["dists_exact"], dtype=np.float64) / (2.0 * ref["k"] * ref["N"] ** 2))


def test_score_gate_through_the_api(ctx):
    """api.Strobemer_findGenes with a gate that rejects some candidates: the hit after a rejected one is still subject to
    goal_ind (the counterfactual in which a rejected candidate frees the next dip gives a different list on this input)."""
    cfg, thr = (2, 3, 5, 5), 30
    ref = _ref(cfg)
    recs = _records("Loci.fasta")
    seqs = [x.sequence for x in recs]
    sc = _Scores(seqs, ref["cons"], ref["W"])
    cand = _oracle("Loci.fasta", cfg, float(thr))["float"]
    scores = sorted(sc(h["contig"], h["lo"], h["hi"])[0] for h in cand)
    gate = scores[len(scores) // 2]
    assert scores[0] < gate <= scores[-1]                                # some, not all, fall below
    accept = lambda c, cmi, lo, hi: sc(c, lo, hi)[0] >= gate
    args = (seqs, ref["RV"], ref["S"], ref["N"], *cfg, ref["W"], float(thr), 50)
    want = sc.aligned(so.scan(*args, accept=accept)["float"], gate)
    other = sc.aligned(so.scan(*args, accept=accept, gate_feeds_back=True)["float"], gate)
    assert 0 < len(want) < len(cand)
    assert [_key(h) for h in want] != [_key(h) for h in other]
    out = api.Strobemer_findGenes(genome_path=os.path.join(DATA, "Loci.fasta"), ref_path=REF, KmerDistThr=thr,
                                  align_score_thr=gate, do_return_hit_loci=True, do_return_align=True, do_return_dists=True,
                                  verbose=False, ctx=ctx)
    hits, loci, aligns, dists = out
    assert [r.description for r in hits] == [
        headers.single_header(recs[h["contig"]].identifier, h["dist"], h["lo"], h["hi"], h["genome_pos"]) for h in want]
    assert [r.sequence for r in hits] == [seqs[h["contig"]][h["lo"] - 1:h["hi"]] for h in want]
    assert loci == [h["lo"] + h["genome_pos"] for h in want]
    assert len(aligns) == len(want) and len(dists) == sum(len(x) - ref["W"] - 1 for x in seqs if len(x) > ref["W"])
    # do_align = false: every candidate, candidate ranges
    out = api.Strobemer_findGenes(genome_path=os.path.join(DATA, "Loci.fasta"), ref_path=REF, KmerDistThr=thr, do_align=False,
                                  verbose=False, ctx=ctx)
    assert [r.description for r in out[0]] == [
        headers.single_header(recs[h["contig"]].identifier, h["dist"], h["lo"], h["hi"], h["genome_pos"]) for h in cand]


def test_synthetic_genome_many_streams(ctx):
    """A few Mb with planted references, cut into many streams by the scan."""
    cfg = (2, 3, 5, 5)
    ref = _ref(cfg)
    rng = np.random.default_rng(20240607)
    genes = [r.sequence.upper() for r in fasta.read_fasta(REF)]
    seqs, _ = make_genome(rng, [2_400_000, 300, 150_000, 288, 289, 900_000], genes, n_plants_per_mb=60.0)
    for thr in (30.0,):
        o = so.scan(seqs, ref["RV"], ref["S"], ref["N"], *cfg, ref["W"], thr, 50)
        r = _scan(ctx, seqs, ref, thr)
        assert r["stats"]["n_tiles"] > 100
        assert len(o["exact"]) > 20
        assert r["first"].tolist() == o["first_D"]
        assert [_key(h) for h in r["hits"]] == [_key(h) for h in o["exact"]]
        rc = _scan(ctx, seqs, ref, thr, flags=_lib.F_CHAIN_REPLAY)
        assert [_key(h) for h in rc["hits"]] == [_key(h) for h in o["float"]]
        flagged = {d["contig"] for d in r["dips"] if d["flags"] & FLAGGED} | {int(c) for c in r["att"][:, 0]}
        differ = {c for c, (e, f) in enumerate(o["per_record"]) if [_key(h) for h in e] != [_key(h) for h in f]}
        assert differ <= flagged


def _small_family(rng, L, cfg, n_refs=7, rate=0.04):
    base = random_dna(rng, L)
    refs = [Record(f"g{i}", mutate(rng, base, rate)) for i in range(n_refs)]
    RV, W, cons, (S, N) = refprep.gen_ref_ws_cons_strobe(refs, *cfg, return_int=True)
    assert W == L
    return base, dict(RV=RV, W=W, cons=cons, S=S, N=N, cfg=cfg, k=cfg[2] + cfg[0] - 1)


@pytest.mark.parametrize("cfg,W", [((2, 3, 5, 5), 289), ((2, 3, 5, 5), 40), ((3, 4, 7, 5), 75), ((1, 2, 4, 5), 20), ((2, 9, 15, 3), 120)])
def test_edge_records(ctx, cfg, W):
    """Records of W - 1, W, W + 1, W + 2 residues, a run of N, lower case, a multi-record genome_pos; windows shorter than
    a 64-window step."""
    rng = np.random.default_rng(W + cfg[0])
    base, ref = _small_family(rng, W, cfg)
    k = ref["k"]
    long = bytearray(random_dna(rng, 30_000))
    for pos, rate in ((500, 0.0), (4000, 0.03), (9000, 0.08), (15000, 0.15)):
        long[pos:pos + W] = mutate(rng, base, rate)
    long[20_000:20_700] = b"N" * 700
    long[22_000:22_050] = bytes(long[22_000:22_050]).lower()
    seqs = [random_dna(rng, W - 1), mutate(rng, base, 0.02), bytes(long), random_dna(rng, W + 1), mutate(rng, base, 0.01) + b"AC",
            random_dna(rng, k), random_dna(rng, 3 * W) + mutate(rng, base, 0.02) + random_dna(rng, 3 * W)]
    thr = float(np.round(0.5 * so.scan_record(random_dna(rng, W), ref["RV"], ref["S"], ref["N"], *cfg, W, 1e9, 50)["D1"]
                         / (2 * k * ref["N"] ** 2), 1))
    o = so.scan(seqs, ref["RV"], ref["S"], ref["N"], *cfg, W, thr, 50, return_dists=True)
    r = _scan(ctx, seqs, ref, thr, flags=_lib.F_RETURN_DISTS)
    assert len(o["exact"]) >= 2
    assert o["first_D"][0] == -1 and o["first_D"][1] >= 0 and o["first_D"][5] == -1
    assert r["first"].tolist() == o["first_D"]
    assert [_key(h) for h in r["hits"]] == [_key(h) for h in o["exact"]]
    assert len({h["genome_pos"] for h in r["hits"]}) >= 2                # skipped records do not advance genome_pos
    assert np.array_equal(r["dists"], np.asarray(o["dists_exact"], dtype=np.float64) / (2.0 * k * ref["N"] ** 2))
    rc = _scan(ctx, seqs, ref, thr, flags=_lib.F_CHAIN_REPLAY)
    assert [_key(h) for h in rc["hits"]] == [_key(h) for h in o["float"]]
    for a, b in zip(rc["hits"], o["float"]):
        if a["flags"] & _lib.HIT_CHAIN:
            assert a["dist"] == b["dist"]


def test_bad_residues(ctx):
    """Residues the reference looks up are positions 1 .. max(W, L - 2) of records with L >= W."""
    cfg = (2, 3, 5, 5)
    ref = _ref(cfg)
    W = ref["W"]
    rng = np.random.default_rng(5)
    L = W + 500
    good = random_dna(rng, L)

    def with_bad(pos):                                                  # 1-based
        a = bytearray(good)
        a[pos - 1] = ord("X")
        return bytes(a)

    for seq in (with_bad(L), with_bad(L - 1)):                           # never looked up: not an error
        o = so.scan([seq], ref["RV"], ref["S"], ref["N"], *cfg, W, 30.0, 50)
        r = _scan(ctx, [seq], ref, 30.0)
        assert r["first"].tolist() == o["first_D"] and [_key(h) for h in r["hits"]] == [_key(h) for h in o["exact"]]
    with pytest.raises(so.BadBase):
        so.scan([with_bad(L - 2)], ref["RV"], ref["S"], ref["N"], *cfg, W, 30.0, 50)
    for seq in (with_bad(L - 2), with_bad(7)):
        with pytest.raises(_lib.BadBaseError):
            _scan(ctx, [seq], ref, 30.0)
    # a record shorter than the window is skipped before any lookup; one of exactly W residues looks all of them up
    _scan(ctx, [b"X" * (W - 1), good], ref, 30.0)
    short = bytearray(random_dna(rng, W)); short[W - 1] = ord("X")
    with pytest.raises(_lib.BadBaseError):
        _scan(ctx, [bytes(short)], ref, 30.0)


def test_arguments_and_state(ctx, alp_ref):
    ref = _ref((2, 3, 5, 5))
    RV, W = ref["RV"], ref["W"]

    def status(fn):
        with pytest.raises(_lib.KgmaError) as e:
            fn()
        return e.value.status

    assert status(lambda: ctx.set_strobe_ref(2, 3, 5, 0, RV, W, 30.0, 84)) == _lib.KGMA_E_ARG
    assert status(lambda: ctx.set_strobe_ref(2, 6, 5, 5, RV, W, 30.0, 84)) == _lib.KGMA_E_ARG
    assert status(lambda: ctx.set_strobe_ref(2, 0, 5, 5, RV, W, 30.0, 84)) == _lib.KGMA_E_ARG
    assert status(lambda: ctx.set_strobe_ref(2, 3, 5, 5, RV, 6, 30.0, 84)) == _lib.KGMA_E_ARG            # k >= W
    assert status(lambda: ctx.set_strobe_ref(4, 3, 5, 5, np.zeros(4 ** 8), W, 30.0, 84)) == _lib.KGMA_E_UNSUPPORTED
    assert status(lambda: ctx.set_strobe_ref(2, 3, 16, 5, RV, W, 30.0, 84)) == _lib.KGMA_E_UNSUPPORTED   # k = 17
    assert status(lambda: ctx.set_strobe_ref(2, 3, 5, 5, RV, 70000, 30.0, 84)) == _lib.KGMA_E_UNSUPPORTED
    assert status(lambda: ctx.set_strobe_ref(2, 3, 5, 5, RV * np.sqrt(2.0), W, 30.0, None)) == _lib.KGMA_E_UNSUPPORTED
    rng = np.random.default_rng(1)
    g = ctx.genome_from_host([random_dna(rng, 5000)])
    try:
        ctx.set_refs(6, [alp_ref["RV"]], [alp_ref["ws"]], [30.0], [alp_ref["N"]])
        assert status(lambda: ctx.strobe_scan(g)) == _lib.KGMA_E_STATE
        ctx.set_strobe_ref(2, 3, 5, 5, RV, W, 30.0, None)                # N inferred
        assert status(lambda: ctx.scan(g, _lib.MODE_SINGLE)) == _lib.KGMA_E_STATE
        assert status(lambda: ctx.scan_device(g, _lib.MODE_OMN)) == _lib.KGMA_E_STATE
        for fn in (lambda: ctx.step_hits(g, _lib.MODE_STROBE), lambda: ctx.step_begin(g, _lib.MODE_STROBE),
                   lambda: g.chain_values(0, 1, [(1, 2)]), lambda: ctx.resolve_ties_local(g),
                   lambda: ctx.scan_aligned(g, _lib.MODE_SINGLE, 50, 0, 0, [b"ACGT"], -69, -1),
                   lambda: ctx.chain_export(g, 0, 1, 5, [(1, 2)])):
            assert status(fn) == _lib.KGMA_E_UNSUPPORTED
        ctx.scan(g, _lib.MODE_STROBE)                                    # kgma_scan routes to the strobemer scan
        a = ctx.hits()
        ctx.scan_device(g, _lib.MODE_STROBE)                             # the device part alone
        assert ctx.first_window(1)[0] >= 0
        ctx.strobe_scan(g)
        assert ctx.hits() == a
        assert ctx.kfv_scale(1) == 2.0 * 6 * 84 * 84
        ctx.set_refs(6, [alp_ref["RV"]], [alp_ref["ws"]], [30.0], [alp_ref["N"]])
        ctx.scan(g, _lib.MODE_SINGLE)                                    # k-mer references again
    finally:
        g.free()
