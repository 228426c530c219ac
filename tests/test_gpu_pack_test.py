"""The step's sums-only pack that makes the prefilter's granule test itself (kgma_filter.hip: pack_sums_kernel<K, false, true>;
switches KGMA_PACK_TEST, KGMA_PACK_RUN, KGMA_PACK_TEST_MIN_UNITS): no block sum is stored and no filter kernel runs, and the step
gives what the step with the filter kernel on the pack's sums (KGMA_PACK_TEST=0) and the step with the plain pack (KGMA_FUSE_SUMS=0)
give, in every field, and what the oracle gives; the candidate granules are tests/filter_ref.py's.

A wave takes runs of KGMA_PACK_RUN units (a unit: 128 plane words, 4096 residues), the runs dealt round-robin over the 16 waves of
KGMA_PACK_WGS=1 (32 of 2), each primed with the chunk in front of it.  The genes are planted where that shows (test_layout asserts
the places): across two units of one run, across a run boundary, in unit 0, on a record's last residues in front of the padding, on
the first residue of a record that starts inside a unit, in two records of one unit, behind a record that ends in low sums."""
import functools

import numpy as np
import pytest

from kmergma_amd import _lib
from oracle import oracle as orc
from tests import filter_cases as fc
from tests import filter_ref, pack_test_ref as ptr, sums_ref
from tests import test_gpu_fused_sums as fu
from tests.helpers import hit_key, mutate, random_dna

gpu = pytest.mark.gpu
BUFF = 50
UNIT = 32 * ptr.UNIT_WORDS                                             # residues of a unit
CELLS = [(5, 100), (6, 284)]                                           # nblk = 8 (even) and 19 (odd)
GRIDS = [(wgs, run) for wgs in (1, 2) for run in (1, 2, 3)]
ENV = ("KGMA_OVERLAP", "KGMA_PACK_WGS", "KGMA_SPARSE_PACK", "KGMA_SPARSE_POISON", "KGMA_FILTER_CAP", "KGMA_PACK_TEST", "KGMA_PACK_RUN")


@pytest.fixture(autouse=True)
def _small_genomes(monkeypatch):
    monkeypatch.setenv("KGMA_FILTER_MIN_WINDOWS", "1")
    monkeypatch.setenv("KGMA_FILTER", "1")
    monkeypatch.setenv("KGMA_FUSE_SUMS", "1")
    monkeypatch.setenv("KGMA_PACK_TEST_MIN_UNITS", "1")                 # (the size gate: by default genomes this small keep the filter kernel)
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


# ---- the layout ------------------------------------------------------------------------------------------------------------------
# record lengths in residues; record 0 starts at word 8 (the lead padding), so unit u of the genome starts at its residue
# UNIT * u - 256
def lengths(W):
    head = [
        40 * UNIT + 1000 - 7,       # 0: units 0 ... 40; ends inside unit 40, its last word and last granule partial
        3 * UNIT + 884,             # 1: starts inside a unit, has fast units
        W + 40,                     # 2, 3: two records of one unit, neither has a fast unit
        W + 100,
    ]
    # 4: a little more than a unit, ends in low sums 32 words in front of record 5, which starts TWO words in front of a unit
    # boundary: the gene on its first residue has its first block in a word-by-word unit and its last in the fast unit behind it,
    # and that unit's entry has a negative gbase
    offs4 = ptr.layout(head + [0])[0][4]
    words4 = 138 + (126 - (offs4 + 138 + ptr.PAD_WORDS)) % ptr.UNIT_WORDS
    return head + [
        32 * words4 - 20,
        58 * UNIT + 77,             # 5: the genome's last record
    ]


def unit_start(offs, c, u):
    """Residue of record c at which unit u starts."""
    return 32 * (u * ptr.UNIT_WORDS - offs[c])


def plants_of(W, offs, lens):
    """{name: (record, 0-based window)}"""
    u1 = ptr.unit_of(offs[1], 0)
    return dict(
        unit0=(0, 100),
        carry=(0, unit_start(offs, 0, 7) - W // 2),                     # units 6 | 7: one run at R = 2, 3
        run_edge=(0, unit_start(offs, 0, 12) - W // 2),                 # units 11 | 12: two runs at R = 1, 2, 3
        tail_cross=(0, unit_start(offs, 0, 40) - W // 2),               # units 39 | 40: first block in a fast unit, last in a word-by-word one
        tail=(0, lens[0] - W),                                          # the record's last window: its granule ends in the padding
        first=(1, 0),                                                   # granule 0 of a record that starts inside a unit
        head_cross=(1, unit_start(offs, 1, u1 + 1) - W // 2),           # record 1's first unit boundary: word-by-word | fast
        inner=(1, unit_start(offs, 1, u1 + 2) - W // 3),
        two_a=(2, 40), two_b=(3, 50),                                   # two records of one unit
        behind_low=(5, 0),
        deep_edge=(5, unit_start(offs, 5, 78) - W // 2),                # units 77 | 78: a run boundary that a wave reaches in a later run
        deep_carry=(5, unit_start(offs, 5, 83) - W // 2),               # units 82 | 83: inside a later run at R = 2, 3
        last=(5, lens[5] - W),
    )


@functools.lru_cache(maxsize=None)
def case(k, nk):
    ref = fc.family(k, 7, nk)
    W = ref["ws"]
    lens = lengths(W)
    offs, total = ptr.layout(lens)
    rng = np.random.default_rng([7200, k, nk])
    arrs = [bytearray(random_dna(rng, L)) for L in lens]
    arrs[4][-400:] = b"A" * 400
    plants = plants_of(W, offs, lens)
    for c, pos in plants.values():
        assert 0 <= pos and pos + W <= lens[c]
        arrs[c][pos:pos + W] = mutate(rng, ref["base"], 0.04)[:W]
    contigs = [bytes(a) for a in arrs]
    D = fc.exact_D(contigs, ref["S"], 7, k, W)
    thr = fc.threshold(D, list(plants.values()), k, 7)
    T, T_hi = filter_ref.threshold_band(thr, k, 7)
    U = filter_ref.bound_U(ref["S"], 7, k, W, T, T_hi)
    want = filter_ref.candidates(contigs, ref["S"], k, W, U)
    ohits, _ = orc.single_scan(contigs, ref["RV"], k, W, thr, BUFF)
    return dict(ref=ref, W=W, contigs=contigs, lens=lens, offs=offs, total=total, plants=plants, thr=thr, U=U, want=want, ohits=ohits)


@pytest.mark.parametrize("k,nk", CELLS)
def test_layout(k, nk):
    """(no GPU work: the places the cases below rely on)"""
    W = nk + k - 1
    lens = lengths(W)
    offs, total = ptr.layout(lens)
    p = plants_of(W, offs, lens)
    n_units = -(-total // ptr.UNIT_WORDS)
    assert sum(lens) < 500_000 and ptr.nblk_of(nk) in (8, 19)
    unit = lambda name, end=False: ptr.unit_of(offs[p[name][0]], p[name][1] + (W - 1 if end else 0))
    fast = lambda c, u: unit_start(offs, c, u) >= 0 and unit_start(offs, c, u) + UNIT + k - 1 <= lens[c]
    assert offs[0] == ptr.LEAD_PAD_WORDS and unit("unit0") == unit("unit0", True) == 0 and not fast(0, 0)
    assert (unit("carry"), unit("carry", True)) == (6, 7) and all(6 // r == 7 // r for r in (2, 3)) and fast(0, 6) and fast(0, 7)
    assert (unit("run_edge"), unit("run_edge", True)) == (11, 12) and all(11 // r != 12 // r for r in (1, 2, 3))
    assert all((11 // r) % 16 != (12 // r) % 16 for r in (1, 2, 3))     # the next run is another wave's
    assert unit("tail", True) == 40 and fast(0, 39) and not fast(0, 40)
    assert (unit("tail_cross"), unit("tail_cross", True)) == (39, 40) and p["tail_cross"][1] + W < p["tail"][1]
    u1 = ptr.unit_of(offs[1], 0)
    assert (unit("head_cross"), unit("head_cross", True)) == (u1, u1 + 1) and not fast(1, u1) and fast(1, u1 + 1) and p["head_cross"][1] > W
    nwin0 = lens[0] - W + 1
    assert nwin0 % 16 != 0 and p["tail"][1] // 16 == (nwin0 + 15) // 16 - 1   # the record's last granule, partial
    assert unit_start(offs, 1, ptr.unit_of(offs[1], 0)) < 0 and fast(1, ptr.unit_of(offs[1], 0) + 1)
    assert ptr.unit_of(offs[2], 0) == ptr.unit_of(offs[3], lens[3] - 1)   # records 2 and 3 in one unit
    u5 = ptr.unit_of(offs[5], 0)
    assert offs[5] - (offs[4] + (lens[4] + 31) // 32) == ptr.PAD_WORDS and lens[4] > UNIT
    # record 5 starts two words in front of unit u5 + 1, which is fast: the gene on its first residue crosses into it, and the
    # entry of that unit's first 64 blocks starts at granule 4 - (nblk - 1) < 0
    assert offs[5] % ptr.UNIT_WORDS == ptr.UNIT_WORDS - 2 and not fast(5, u5) and fast(5, u5 + 1) and W > 64 and 4 - (ptr.nblk_of(nk) - 1) < 0
    assert u5 + 2 < 77 and (unit("deep_edge"), unit("deep_edge", True)) == (77, 78) and (unit("deep_carry"), unit("deep_carry", True)) == (82, 83)
    # at every grid of the cases a wave takes more than one run somewhere, and one of the deep boundaries is a run boundary of a
    # wave's second or later run, the other lies inside a run
    for wgs, run in GRIDS:
        runs = -(-n_units // run)
        assert runs > 16 * wgs
    for r in (1, 2, 3):
        edges = [(a // r != b // r, b // r >= 16) for a, b in ((77, 78), (82, 83))]
        assert any(e and late for e, late in edges) and (r == 1 or any(not e for e, _ in edges)), (r, u5)


# ---- steps ------------------------------------------------------------------------------------------------------------------------

def _step(monkeypatch, c, k, env, flags=_lib.F_CHAIN_REPLAY, pokes=(), sums=False, contigs=None):
    """One fresh context, one step (and one more per poke: (record, 1-based position, bytes)); per step the results, the filter's
    numbers, the pack's new stats and, on request, the block sums of every record."""
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    contigs = c["contigs"] if contigs is None else contigs
    ctx = _lib.Context(0)
    g = None
    try:
        ctx.set_refs(k, [c["ref"]["RV"]], [c["W"]], [c["thr"]], [7])
        g = ctx.genome_from_host(contigs)
        outs = []
        for poke in (None,) + tuple(pokes):
            if poke is not None:
                g.poke(*poke)
            ctx.step_hits(g, _lib.MODE_SINGLE, BUFF, 0, flags)
            out = fu._collect(ctx, g, False, len(contigs))
            out["pt"] = ctx.pack_test_stats()
            if sums:
                out["sums"] = [ctx.get_block_sums(g, r) for r in range(len(contigs))]
            outs.append(out)
        return outs
    finally:
        for name in env:
            monkeypatch.delenv(name, raising=False)
        if g is not None:
            g.free()
        ctx.close()


_BASE = {}


def baselines(monkeypatch, k, nk):
    """The step with the filter kernel on the pack's sums and the step with the plain pack, once per cell."""
    if (k, nk) not in _BASE:
        c = case(k, nk)
        (two,) = _step(monkeypatch, c, k, {"KGMA_PACK_TEST": "0"})
        (plain,) = _step(monkeypatch, c, k, {"KGMA_FUSE_SUMS": "0"})
        _BASE[(k, nk)] = (two, plain)
    return _BASE[(k, nk)]


@gpu
@pytest.mark.parametrize("wgs,run", GRIDS, ids=["wgs%d-run%d" % g for g in GRIDS])
@pytest.mark.parametrize("k,nk", CELLS, ids=["k%d-nk%d" % c for c in CELLS])
def test_tested_step_equals_both_other_routes_and_the_oracle(monkeypatch, k, nk, wgs, run):
    c = case(k, nk)
    two, plain = baselines(monkeypatch, k, nk)
    (on,) = _step(monkeypatch, c, k, {"KGMA_PACK_WGS": str(wgs), "KGMA_PACK_RUN": str(run)})
    n_units = -(-c["total"] // ptr.UNIT_WORDS)
    assert on["pt"]["tested"] == 1 and on["pt"]["run"] == run and on["pt"]["units"] == n_units
    fast = lambda r, u: unit_start(c["offs"], r, u) >= 0 and unit_start(c["offs"], r, u) + UNIT + k - 1 <= c["lens"][r]
    n_fast = sum(1 for u in range(n_units) for r in range(len(c["lens"])) if fast(r, u))
    assert on["pt"]["primed_chunks"] == -(-n_units // run) - 1 and on["pt"]["slow_units"] == n_units - n_fast > 8
    assert two["pt"]["tested"] == 0 and plain["pt"]["tested"] == 0
    want_form = fc.form_of(k, int(c["ref"]["S"].max()))
    assert on["fs"]["form"] == want_form | fu.PRESUMMED == two["fs"]["form"] and plain["fs"]["form"] == want_form
    assert (on["fs"]["ran"], on["fs"]["fell_back"], on["fs"]["filter_ms"]) == (1, 0, 0.0)
    assert on["fs"]["bound"] == c["U"]
    assert np.array_equal(on["cand"], c["want"]) and on["fs"]["granules"] == len(c["want"])
    fu._same(on, two)
    fu._same(on, plain)
    assert [hit_key(h) for h in on["hits"]] == [hit_key(h) for h in c["ohits"]]
    have = set(map(tuple, on["cand"].tolist()))
    assert all((r, s // 16) in have for r, s in c["plants"].values())
    assert len(c["ohits"]) >= 4
    # the record in front of the gene on a first residue ends in low sums: its last granule is none
    assert (4, (c["lens"][4] - c["W"] + 1 + 15) // 16 - 1) not in have


@gpu
def test_below_the_gate_and_switched_off(monkeypatch):
    c = case(5, 100)
    two, _ = baselines(monkeypatch, 5, 100)
    (small,) = _step(monkeypatch, c, 5, {"KGMA_PACK_TEST_MIN_UNITS": "1000000"})
    assert small["pt"]["tested"] == 0 and small["fs"]["form"] & fu.PRESUMMED and small["fs"]["filter_ms"] > 0
    fu._same(small, two)
    monkeypatch.delenv("KGMA_PACK_TEST_MIN_UNITS", raising=False)       # the default gate: a genome of 100 units keeps the filter kernel
    (dflt,) = _step(monkeypatch, c, 5, {})
    assert dflt["pt"]["tested"] == 0
    fu._same(dflt, two)


@gpu
def test_list_overflow_falls_back_and_is_remembered(monkeypatch):
    c = case(6, 284)
    _, plain = baselines(monkeypatch, 6, 284)
    first, second = _step(monkeypatch, c, 6, {"KGMA_FILTER_CAP": "2", "KGMA_PACK_WGS": "1", "KGMA_PACK_RUN": "2"}, pokes=((0, 1, c["contigs"][0][:1]),))
    for s in (first, second):
        assert s["hits"] == plain["hits"] and s["dips"] == plain["dips"] and np.array_equal(s["D1"], plain["D1"])
    assert first["pt"]["tested"] == 1
    assert (first["fs"]["ran"], first["fs"]["fell_back"], first["fs"]["reason"]) == (1, 1, _lib.FILTER_OVERFLOW)
    assert (second["fs"]["ran"], second["fs"]["fell_back"], second["fs"]["reason"]) == (0, 1, _lib.FILTER_REMEMBERED)
    assert second["pt"]["tested"] == 0


@gpu
@pytest.mark.parametrize("where", ["second_unit_of_a_run", "primed_chunk"])
def test_bad_residue(monkeypatch, where):
    """An X in the first chunk of a run's second unit (only the run's wave encodes it) and in the chunk that primes the next run
    (the unit's second chunk: two waves encode it)."""
    c = case(6, 284)
    run = 2
    u = 9
    assert u % run == 1
    pos = unit_start(c["offs"], 0, u) + 777 + (0 if where == "second_unit_of_a_run" else UNIT // 2)
    contigs = list(c["contigs"])
    a = bytearray(contigs[0]); a[pos] = ord("X"); contigs[0] = bytes(a)

    def status(env):
        try:
            _step(monkeypatch, c, 6, env, flags=0, contigs=contigs)
        except _lib.KgmaError as e:
            return e.status, e.message
        return 0, ""

    on = status({"KGMA_PACK_WGS": "1", "KGMA_PACK_RUN": str(run)})
    off = status({"KGMA_FUSE_SUMS": "0"})
    assert on == off
    assert on[0] == _lib.KGMA_E_BADBASE and "record 0 position %d" % (pos + 1) in on[1], on


@gpu
def test_block_sums_after_a_tested_step_and_pokes(monkeypatch):
    """The sums are written when somebody asks, for the text the step packed: a poke has them written first.  The step behind the
    poke sees the new text."""
    c = case(6, 284)
    k, W, ref = 6, c["W"], c["ref"]
    want = [sums_ref.block_sums(x, ref["S"], k) for x in c["contigs"]]
    env = {"KGMA_PACK_WGS": "2", "KGMA_PACK_RUN": "3"}
    (on,) = _step(monkeypatch, c, k, env, sums=True)
    assert on["pt"]["tested"] == 1
    fu._check_sums(on["sums"], want)
    # poke, then read: the sums of the text before the poke; then a step: the new text's results and sums
    gene = mutate(np.random.default_rng(7201), ref["base"], 0.03)[:W]
    at = unit_start(c["offs"], 5, ptr.unit_of(c["offs"][5], 0) + 20) - W // 2
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    ctx = _lib.Context(0)
    g = None
    try:
        ctx.set_refs(k, [ref["RV"]], [W], [c["thr"]], [7])
        g = ctx.genome_from_host(c["contigs"])
        ctx.step_hits(g, _lib.MODE_SINGLE, BUFF, 0, _lib.F_CHAIN_REPLAY)
        assert ctx.pack_test_stats()["tested"] == 1
        g.poke(5, at + 1, gene)
        fu._check_sums([ctx.get_block_sums(g, r) for r in range(len(want))], want)
        ctx.step_hits(g, _lib.MODE_SINGLE, BUFF, 0, _lib.F_CHAIN_REPLAY)
        assert ctx.pack_test_stats()["tested"] == 1
        hits = ctx.hits()
        cand = ctx.filter_candidates()
        sums2 = [ctx.get_block_sums(g, r) for r in range(len(want))]
    finally:
        if g is not None:
            g.free()
        ctx.close()
    poked = bytearray(c["contigs"][5]); poked[at:at + W] = gene
    contigs2 = list(c["contigs"][:5]) + [bytes(poked)]
    ohits, _ = orc.single_scan(contigs2, ref["RV"], k, W, c["thr"], BUFF)
    assert [hit_key(h) for h in hits] == [hit_key(h) for h in ohits]
    assert np.array_equal(cand, filter_ref.candidates(contigs2, ref["S"], k, W, c["U"]))
    # (the new text's, not the old one's: the planted gene's granule is a candidate now and was none)
    assert [5, at // 16] in cand.tolist() and [5, at // 16] not in c["want"].tolist()
    fu._check_sums(sums2, [sums_ref.block_sums(x, ref["S"], k) for x in contigs2])


@gpu
def test_poisoned_copy(monkeypatch):
    """KGMA_SPARSE_POISON=1: every word of the 2-bit copy that the step does not pack is garbage, and the step's results stand."""
    c = case(5, 100)
    _, plain = baselines(monkeypatch, 5, 100)
    (on,) = _step(monkeypatch, c, 5, {"KGMA_SPARSE_POISON": "1", "KGMA_PACK_WGS": "1", "KGMA_PACK_RUN": "3"})
    assert on["pt"]["tested"] == 1
    fu._same(on, plain)


@gpu
def test_stats_are_the_last_steps(monkeypatch):
    """A step whose pack is not left to the scan (here: the sums switched off) reports that it did not test, not the step before."""
    c = case(5, 100)
    monkeypatch.setenv("KGMA_PACK_WGS", "1")
    monkeypatch.setenv("KGMA_PACK_RUN", "2")
    ctx = _lib.Context(0)
    g = None
    try:
        ctx.set_refs(5, [c["ref"]["RV"]], [c["W"]], [c["thr"]], [7])
        g = ctx.genome_from_host(c["contigs"])
        ctx.step_hits(g, _lib.MODE_SINGLE, BUFF, 0, 0)
        assert ctx.pack_test_stats()["tested"] == 1
        monkeypatch.setenv("KGMA_FUSE_SUMS", "0")
        ctx.step_hits(g, _lib.MODE_SINGLE, BUFF, 0, 0)
        assert ctx.pack_test_stats() == dict(tested=0, run=0, units=0, slow_units=0, primed_chunks=0)
    finally:
        if g is not None:
            g.free()
        ctx.close()
