"""The scan's distance-bound prefilter (kgma_filter.hip; include/kgma.h: kgma_get_filter_stats) on the device: a scan with the
filter gives what the scan without it gives -- hits (every field), dips, first-window D, guard-band windows, counters -- and what
the oracles give; the device's candidate granules are the numpy restatement's; every fallback keeps the results and names its
reason.  The size gate is lowered for these genomes (KGMA_FILTER_MIN_WINDOWS)."""
import os

import numpy as np
import pytest

from kmergma_amd import _lib
from oracle import oracle as orc
from tests import filter_ref
from tests.helpers import hit_key, make_genome, mutate, random_dna

pytestmark = pytest.mark.gpu

K, W, BUFF = 6, 289, 50


@pytest.fixture(scope="module")
def genes(data_dir):
    from kmergma_amd import fasta
    return [r.sequence.upper() for r in fasta.read_fasta(os.path.join(data_dir, "Alp_V_ref.fasta"))]


@pytest.fixture(autouse=True)
def _small_genomes(monkeypatch):
    monkeypatch.setenv("KGMA_FILTER_MIN_WINDOWS", "1")


def _scan(monkeypatch, contigs, ref, thr, flags, filter_on=True, env=None, repeat=1):
    """One fresh context, `repeat` scans of the same genome; returns the last scan's results and every scan's filter stats."""
    monkeypatch.setenv("KGMA_FILTER", "1" if filter_on else "0")
    for name, val in (env or {}).items():
        monkeypatch.setenv(name, val)
    ctx = _lib.Context(0)
    try:
        ctx.set_refs(K, [ref["RV"]], [ref["ws"]], [thr], [ref["N"]])
        g = ctx.genome_from_host(contigs)
        fstats = []
        for _ in range(repeat):
            ctx.scan(g, _lib.MODE_SINGLE, BUFF, 0, flags, None)
            fstats.append(ctx.filter_stats())
        st = ctx.stats()
        out = dict(hits=ctx.hits(), dips=ctx.dips(), D1=ctx.first_window(1), att=ctx.att(),
                   counts=(st["n_dips"], st["n_tie_flagged"], st["n_at_threshold"]), windows=st["windows_scanned"],
                   fstats=fstats, cand=ctx.filter_candidates(), kernel=ctx.kernel_name())
        g.free()
        return out
    finally:
        ctx.close()
        for name in (env or {}):
            monkeypatch.delenv(name)


def _same(a, b):
    assert a["hits"] == b["hits"]
    assert a["dips"] == b["dips"]
    assert np.array_equal(a["D1"], b["D1"])
    assert np.array_equal(a["att"], b["att"])
    assert a["counts"] == b["counts"]
    assert a["windows"] == b["windows"]


def _on_off_oracle(monkeypatch, contigs, ref, thr, expect_ran=True):
    """Filter on against filter off, without and with the chain replay, and against the oracles; returns the filtered exact scan."""
    T = orc.int_threshold(thr, K, ref["N"])
    _, _, oD1 = orc.single_scan_int(contigs, ref["S"], ref["N"], K, W, T, BUFF)
    ohits, _ = orc.single_scan(contigs, ref["RV"], K, W, thr, BUFF)
    first = None
    for flags in (0, _lib.F_CHAIN_REPLAY):
        on = _scan(monkeypatch, contigs, ref, thr, flags, True)
        off = _scan(monkeypatch, contigs, ref, thr, flags, False)
        assert on["kernel"].startswith("stream8_kernel")
        _same(on, off)
        fs = on["fstats"][0]
        assert off["fstats"][0]["ran"] == 0 and off["fstats"][0]["fell_back"] == 0
        if expect_ran:
            assert fs["ran"] == 1 and fs["fell_back"] == 0 and fs["reason"] == _lib.FILTER_OK, fs
            assert 0 < fs["windows"] <= fs["total_windows"] and fs["streams"] >= fs["regions"] >= len(contigs) - 1
        has = np.asarray([len(c) >= W for c in contigs])
        assert np.array_equal(on["D1"][has], oD1[has])
        if flags & _lib.F_CHAIN_REPLAY:
            assert [hit_key(h) for h in on["hits"]] == [hit_key(h) for h in ohits]
        first = first or on
    return first, ohits


def test_filter_on_off_and_candidates(monkeypatch, alp_ref, genes):
    """Records of 3 Mb, 500, 289, 288 and 70 kb with planted genes and N runs: same results; the candidate list is the numpy set."""
    rng = np.random.default_rng(6101)
    contigs, _ = make_genome(rng, [3_000_000, 500, 289, 288, 70_000], genes, n_plants_per_mb=30.0)
    on, ohits = _on_off_oracle(monkeypatch, contigs, alp_ref, 30.0)
    assert len(ohits) > 20
    T, T_hi = filter_ref.threshold_band(30.0, K, alp_ref["N"])
    U = filter_ref.bound_U(alp_ref["S"], alp_ref["N"], K, W, T, T_hi)
    fs = on["fstats"][0]
    assert fs["bound"] == U
    want = filter_ref.candidates(contigs, alp_ref["S"], K, W, U)
    assert np.array_equal(on["cand"], want)
    assert fs["granules"] == len(want) > 0
    assert fs["windows"] < fs["total_windows"] // 4                  # (the filter is selective on iid sequence)


def _placements(rng, genes):
    """name -> (records, what must hold).  Window s (0-based) starts at base s; regions start on multiples of 64 windows."""
    g = lambda i, rate: mutate(rng, genes[i], rate)
    out = {}
    out["first_windows"] = [g(2, 0.02) + random_dna(rng, 9_000)]                      # the first window is never tested
    long_gene = next(i for i, x in enumerate(genes) if len(x) >= W)
    out["last_window"] = [random_dna(rng, 9_000) + g(long_gene, 0.02)[:W]]            # a dip open at the record's end is dropped
    out["across_64"] = [random_dna(rng, 64 * 70 - 3) + g(9, 0.03) + random_dna(rng, 5_000),
                        random_dna(rng, 64 * 33 - 150) + g(4, 0.05) + random_dna(rng, 3_000)]
    a = bytearray(b"N" * 3_000 + random_dna(rng, 24_000))
    x, y = g(13, 0.02), g(17, 0.04)
    a[1_000:1_000 + len(x)] = x                                                       # inside the leading N run
    a[3_000:3_000 + len(y)] = y                                                       # just behind it
    out["n_run"] = [bytes(a)]
    out["tandem"] = [random_dna(rng, 12_000) + genes[11] * 24 + random_dna(rng, 12_000)]   # one region, several streams, one dip across the cuts
    return out


@pytest.mark.parametrize("case", ["first_windows", "last_window", "across_64", "n_run", "tandem"])
def test_placements(monkeypatch, alp_ref, genes, case):
    contigs = _placements(np.random.default_rng(6102), genes)[case]
    on, ohits = _on_off_oracle(monkeypatch, contigs, alp_ref, 30.0)
    assert len(on["dips"]) > 0
    fs = on["fstats"][0]
    if case == "tandem":
        assert fs["streams"] > fs["regions"]                        # the long region was cut
        assert max(d["end"] - d["start"] for d in on["dips"]) > 2048   # ... and a dip runs across the cut
    if case == "last_window":
        nwin = len(contigs[0]) - W + 1
        assert any(d["end"] == nwin and d["exit_pos"] == 0 for d in on["dips"])
    T, T_hi = filter_ref.threshold_band(30.0, K, alp_ref["N"])
    U = filter_ref.bound_U(alp_ref["S"], alp_ref["N"], K, W, T, T_hi)
    assert np.array_equal(on["cand"], filter_ref.candidates(contigs, alp_ref["S"], K, W, U))


def test_threshold_on_a_windows_distance(monkeypatch, alp_ref, genes):
    """thr exactly on a window's distance: guard-band windows are found and U honours T_hi."""
    rng = np.random.default_rng(6103)
    contigs = [random_dna(rng, 5_000) + mutate(rng, genes[20], 0.04) + random_dna(rng, 5_000)]
    N = alp_ref["N"]
    _, D, D1 = orc.single_scan_int(contigs, alp_ref["S"], N, K, W, 1, BUFF, return_D=True)
    D = np.concatenate([[D1[0]], D])
    scale = 2.0 * K * N * N
    s = int(np.argmin(np.abs(D / scale - 26.0)))
    thr = float(D[s]) / scale
    T, T_hi = filter_ref.threshold_band(thr, K, N)
    assert T == D[s] <= T_hi
    on, _ = _on_off_oracle(monkeypatch, contigs, alp_ref, thr)
    assert on["counts"][2] > 0 and [s + 1] in on["att"][:, 2:].tolist()
    assert on["fstats"][0]["bound"] == filter_ref.bound_U(alp_ref["S"], N, K, W, T, T_hi)


def test_fallbacks(monkeypatch, alp_ref, genes):
    rng = np.random.default_rng(6104)
    contigs, _ = make_genome(rng, [200_000, 30_000], genes, n_plants_per_mb=60.0)
    off = _scan(monkeypatch, contigs, alp_ref, 30.0, 0, False)
    assert len(off["hits"]) > 3
    # the list overflows
    ovf = _scan(monkeypatch, contigs, alp_ref, 30.0, 0, True, env={"KGMA_FILTER_CAP": "2"}, repeat=2)
    _same(ovf, off)
    assert (ovf["fstats"][0]["ran"], ovf["fstats"][0]["fell_back"], ovf["fstats"][0]["reason"]) == (1, 1, _lib.FILTER_OVERFLOW)
    # ... and the next scan of the same genome, references and thresholds skips the filter
    assert (ovf["fstats"][1]["ran"], ovf["fstats"][1]["fell_back"], ovf["fstats"][1]["reason"]) == (0, 1, _lib.FILTER_REMEMBERED)
    # a threshold at which most windows are candidates
    hi_off = _scan(monkeypatch, contigs, alp_ref, 38.0, 0, False)
    hi_on = _scan(monkeypatch, contigs, alp_ref, 38.0, 0, True)
    _same(hi_on, hi_off)
    fs = hi_on["fstats"][0]
    assert (fs["ran"], fs["fell_back"], fs["reason"]) == (1, 1, _lib.FILTER_FRACTION), fs


def test_other_launch_shapes_do_not_filter(monkeypatch, alp_ref, alp_clusters, genes):
    rng = np.random.default_rng(6105)
    contigs, _ = make_genome(rng, [60_000], genes, n_plants_per_mb=100.0)
    monkeypatch.setenv("KGMA_FILTER", "1")
    ctx = _lib.Context(0)
    try:
        ctx.set_refs(K, [alp_ref["RV"]], [W], [30.0], [alp_ref["N"]])
        g = ctx.genome_from_host(contigs)
        ctx.scan(g, _lib.MODE_SINGLE, BUFF, 0, 0, None)
        assert ctx.filter_stats()["ran"] == 1
        ctx.scan(g, _lib.MODE_SINGLE, BUFF, 0, _lib.F_RETURN_DISTS, None)
        assert ctx.filter_stats()["ran"] == 0 and ctx.filter_stats()["fell_back"] == 0 and len(ctx.filter_candidates()) == 0
        c = alp_clusters
        ctx.set_refs(K, c["KFVs"], c["ws"], [25.0] * len(c["ws"]), c["N"])
        ctx.scan(g, _lib.MODE_OMN, BUFF, 0, 0, None)
        assert ctx.filter_stats()["ran"] == 0
        g.free()
    finally:
        ctx.close()
