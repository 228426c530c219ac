"""stream8_kernel's fast carry against the oracles, on scans that do NOT ask for per-window distances.

A scan that returns distances takes the exact counts in every step; these scans take the fast path, and only steps with a
prefix near a threshold (or a run open) go through the correction rounds.  Each case compares hits, D values and first-window D
with the integer oracle, the run records (dips) with the same scan done the exact way (distances requested), and the chain-mode
hit list with the Float64 oracle.  The cases aimed at the cold path assert that it ran (KGMA_GEOM_DEBUG's cold-step count).
"""
import re

import numpy as np
import pytest

from kmergma_amd import _lib, refprep
from kmergma_amd.fasta import Record
from oracle import oracle as orc
from tests.helpers import hit_key, mutate, random_dna

pytestmark = pytest.mark.gpu

_COLD = re.compile(r"scan cold steps: (\d+)")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture
def cold(monkeypatch, capfd):
    """cold() -> the cold-step count of the last scan since the previous call."""
    monkeypatch.setenv("KGMA_GEOM_DEBUG", "1")
    capfd.readouterr()

    def read():
        counts = _COLD.findall(capfd.readouterr().err)
        return int(counts[-1]) if counts else None
    return read


def _family(rng, L, k, n_refs=6, rate=0.03):
    base = random_dna(rng, L)
    refs = [Record(f"g{i}", mutate(rng, base, rate)) for i in range(n_refs)]
    RV, ws, _, (S, N) = refprep.gen_ref_ws_cons(refs, k, return_int=True)
    assert ws == L
    return base, dict(RV=RV, ws=ws, S=S, N=N, k=k)


def _dip_key(d):
    return tuple(sorted((k, v) for k, v in d.items() if not isinstance(v, float)))


def _check(ctx, cold, contigs, refs, thrs, mode, buff=50, gpos=0):
    """Fast-path scan against the oracles and against the exact-count scan; returns the fast scan's cold-step count."""
    k = refs[0]["k"]
    ctx.set_refs(k, [r["RV"] for r in refs], [r["ws"] for r in refs], thrs, [r["N"] for r in refs])
    T = [orc.int_threshold(t, k, r["N"]) for t, r in zip(thrs, refs)]
    gen = ctx.genome_from_host(contigs)
    try:
        cold()
        ctx.scan(gen, mode, buff, gpos, _lib.F_NO_TIE_RESOLVE, None)
        n_cold = cold()
        assert n_cold is not None, "no cold-step line: the scan did not print its count"
        name = ctx.kernel_name()
        hits, dips = ctx.hits(), ctx.dips()
        D1 = [ctx.first_window(j + 1) for j in range(len(refs))]
        # the same scan with distances: every step on the exact counts
        ctx.scan(gen, mode, buff, gpos, _lib.F_NO_TIE_RESOLVE | _lib.F_RETURN_DISTS, None)
        assert [_dip_key(d) for d in ctx.dips()] == [_dip_key(d) for d in dips], "run records differ from the exact path"
        assert [hit_key(h) for h in ctx.hits()] == [hit_key(h) for h in hits]
        for j in range(len(refs)):
            assert np.array_equal(ctx.first_window(j + 1), D1[j])
        ctx.scan(gen, mode, buff, gpos, _lib.F_CHAIN_REPLAY, None)
        chain_hits = ctx.hits()
        assert ctx.stats()["n_tie_flagged"] == 0
    finally:
        gen.free()
    assert name.startswith("stream8_kernel"), name
    if mode == _lib.MODE_SINGLE:
        r = refs[0]
        ohi, _, oD1 = orc.single_scan_int(contigs, r["S"], r["N"], k, r["ws"], T[0], buff, return_D=True)
        assert np.array_equal(D1[0], oD1)
        fo, _ = orc.single_scan(contigs, r["RV"], k, r["ws"], thrs[0], buff)
    else:
        ohi, _ = orc.omn_scan_int(contigs, [r["S"] for r in refs], [r["N"] for r in refs], k, [r["ws"] for r in refs], T, buff, gpos,
                                  return_D=True)
        fo, _ = orc.omn_scan(contigs, [r["RV"] for r in refs], k, [r["ws"] for r in refs], thrs, buff, gpos)
    assert [hit_key(h) for h in hits] == [hit_key(h) for h in ohi]
    assert [h["D"] for h in hits] == [h["D"] for h in ohi]
    assert [hit_key(h) for h in chain_hits] == [hit_key(h) for h in fo]
    return n_cold, len(ohi)


def test_threshold_just_above_the_minimum(ctx, cold):
    """Random records; thr just above the smallest distance of any window: the cold path runs where that window is."""
    rng = np.random.default_rng(501)
    base, ref = _family(rng, 289, 6)
    contigs = [random_dna(rng, 60_000), random_dna(rng, 25_000) + mutate(rng, base, 0.25) + random_dna(rng, 20_000), random_dna(rng, 9_000)]
    _, d = orc.single_scan(contigs, ref["RV"], 6, 289, 1.0, 50, return_dists=True)
    dmin = float(np.min(d))
    for eps in (0.02, 0.3):
        n_cold, n_hits = _check(ctx, cold, contigs, [ref], [dmin + eps], _lib.MODE_SINGLE)
        assert n_cold > 0 and n_hits > 0


@pytest.mark.parametrize("period", range(1, 9))
def test_tandem_repeats_next_to_a_dip(ctx, cold, period):
    """A repeat of period 1 ... 8 right before and right after a planted gene (the repeat's steps collide in every lane)."""
    rng = np.random.default_rng(600 + period)
    base, ref = _family(rng, 289, 6)
    unit = random_dna(rng, period)
    rep = (unit * (800 // period + 1))[:700]
    contigs = [random_dna(rng, 3000) + rep + mutate(rng, base, 0.05) + rep + random_dna(rng, 4000),
               random_dna(rng, 1000) + mutate(rng, base, 0.08) + rep[:300] + random_dna(rng, 2000)]
    n_cold, n_hits = _check(ctx, cold, contigs, [ref], [20.0], _lib.MODE_SINGLE)
    assert n_cold > 0 and n_hits > 0


def test_heavy_kmer_runs(ctx, cold):
    """Homopolymer and dinucleotide runs with more than 128 copies of one k-mer (heavy mode) next to dips."""
    from tests.test_gpu_parity import _low_complexity_genome
    rng = np.random.default_rng(701)
    base, ref = _family(rng, 289, 6)
    g = bytearray(_low_complexity_genome(rng, 200_000, 289))
    for pos in range(5000, 195_000, 20_000):
        g[pos:pos + 289] = mutate(rng, base, 0.05)
    contigs = [bytes(g), b"A" * 600 + mutate(rng, base, 0.04) + b"AC" * 300 + random_dna(rng, 800)]
    n_cold, n_hits = _check(ctx, cold, contigs, [ref], [25.0], _lib.MODE_SINGLE)
    assert n_cold > 0 and n_hits > 0


def test_c16_window(ctx, cold):
    """A window of 420 residues at k = 6: the 16-bit counter form (64-bit carry)."""
    rng = np.random.default_rng(801)
    base, ref = _family(rng, 420, 6)
    contigs = [random_dna(rng, 30_000) + mutate(rng, base, 0.06) + random_dna(rng, 30_000) + mutate(rng, base, 0.12) + random_dna(rng, 5000),
               random_dna(rng, 12_000)]
    n_cold, n_hits = _check(ctx, cold, contigs, [ref], [25.0], _lib.MODE_SINGLE)
    assert n_cold > 0 and n_hits > 0


def test_three_kfvs_one_size(ctx, cold):
    """Cluster engine, three KFVs of one window size: one launch of the three-KFV variant."""
    rng = np.random.default_rng(901)
    fams = [_family(rng, 289, 6, n_refs=3 + i) for i in range(3)]
    parts = []
    for i in range(9):
        parts += [random_dna(rng, int(rng.integers(3000, 9000))), mutate(rng, fams[i % 3][0], 0.04 + 0.02 * (i % 4))]
    contigs = [b"".join(parts), random_dna(rng, 20_000)]
    n_cold, n_hits = _check(ctx, cold, contigs, [f[1] for f in fams], [24.0, 26.0, 22.0], _lib.MODE_OMN, buff=60, gpos=17)
    assert n_cold > 0 and n_hits > 0


def test_sharded_scan(ctx, cold):
    """Intra-record sharding (parallel.local_scan / merge_payloads / replay_dips) over the fast path equals the whole scan."""
    from kmergma_amd import parallel
    rng = np.random.default_rng(1001)
    base, ref = _family(rng, 289, 6)
    a = bytearray(random_dna(rng, 150_000))
    for pos in range(3000, 148_000, 7_000):
        a[pos:pos + 289] = mutate(rng, base, 0.05)
    contigs = [bytes(a), random_dna(rng, 40_000)]
    ctx.set_refs(6, [ref["RV"]], [289], [25.0], [ref["N"]])
    gen = ctx.genome_from_host(contigs)
    cold()
    ctx.scan(gen, _lib.MODE_SINGLE, 50, 0, _lib.F_NO_TIE_RESOLVE, None)
    assert cold() > 0
    whole = ctx.hits()
    gen.free()
    T = orc.int_threshold(25.0, 6, ref["N"])
    ohi, _, _ = orc.single_scan_int(contigs, ref["S"], ref["N"], 6, 289, T, 50, return_D=True)
    assert [hit_key(h) for h in whole] == [hit_key(h) for h in ohi] and len(ohi) > 3
    for world in (2, 3):
        plan = parallel.plan_slices([len(x) for x in contigs], world, True, [289], 6, 4096)
        payloads = [parallel.local_scan(ctx, contigs, plan[r], _lib.MODE_SINGLE, _lib.F_NO_TIE_RESOLVE) for r in range(world)]
        dips, last_min, first_D = parallel.merge_payloads(payloads, len(contigs), 1)
        ctx.replay_dips(_lib.MODE_SINGLE, 50, 0, _lib.F_NO_TIE_RESOLVE, [len(x) for x in contigs], first_D, dips, last_min, None)
        hits = ctx.hits()
        assert [hit_key(h) for h in hits] == [hit_key(h) for h in whole]
        assert [h["D"] for h in hits] == [h["D"] for h in whole]
