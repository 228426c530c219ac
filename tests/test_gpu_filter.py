"""The scan's distance-bound prefilter (kgma_filter.hip; include/kgma.h: kgma_get_filter_stats) on the device: a scan with the
filter gives what the scan without it gives -- hits (every field), dips, first-window D, guard-band windows, counters -- and what
the oracles give; the device's candidate granules are the numpy restatement's; every fallback keeps the results and names its
reason.  The size gate is lowered for these genomes (KGMA_FILTER_MIN_WINDOWS)."""
import os

import numpy as np
import pytest

from kmergma_amd import _lib
from oracle import oracle as orc
from tests import filter_cases as fc
from tests import filter_ref
from tests.helpers import hit_key, kmer_values, make_genome, mutate, random_dna

pytestmark = pytest.mark.gpu

K, W, BUFF = 6, 289, 50


@pytest.fixture(scope="module")
def genes(data_dir):
    from kmergma_amd import fasta
    return [r.sequence.upper() for r in fasta.read_fasta(os.path.join(data_dir, "Alp_V_ref.fasta"))]


@pytest.fixture(autouse=True)
def _small_genomes(monkeypatch):
    monkeypatch.setenv("KGMA_FILTER_MIN_WINDOWS", "1")


def _scan(monkeypatch, contigs, ref, thr, flags, filter_on=True, env=None, repeat=1, k=K):
    """One fresh context, `repeat` scans of the same genome; returns the last scan's results and every scan's filter stats."""
    monkeypatch.setenv("KGMA_FILTER", "1" if filter_on else "0")
    for name, val in (env or {}).items():
        monkeypatch.setenv(name, val)
    ctx = _lib.Context(0)
    try:
        ctx.set_refs(k, [ref["RV"]], [ref["ws"]], [thr], [ref["N"]])
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


def _on_off_oracle(monkeypatch, contigs, ref, thr, expect_ran=True, k=K, W=W, all_flags=(0, _lib.F_CHAIN_REPLAY)):
    """Filter on against filter off, without and with the chain replay, and against the oracles; returns the filtered exact scan."""
    T = orc.int_threshold(thr, k, ref["N"])
    _, _, oD1 = orc.single_scan_int(contigs, ref["S"], ref["N"], k, W, T, BUFF)
    ohits, _ = orc.single_scan(contigs, ref["RV"], k, W, thr, BUFF)
    first = None
    for flags in all_flags:
        on = _scan(monkeypatch, contigs, ref, thr, flags, True, k=k)
        off = _scan(monkeypatch, contigs, ref, thr, flags, False, k=k)
        assert on["kernel"].startswith("stream8_kernel")
        _same(on, off)
        fs = on["fstats"][0]
        assert off["fstats"][0]["ran"] == 0 and off["fstats"][0]["fell_back"] == 0
        if expect_ran:
            assert fs["ran"] == 1 and fs["fell_back"] == 0 and fs["reason"] == _lib.FILTER_OK, fs
            assert 0 < fs["windows"] <= fs["total_windows"] and fs["streams"] >= fs["regions"] >= len(contigs) - 1
        else:
            assert fs["ran"] == 0 and fs["fell_back"] == 0 and fs["form"] == 0, fs
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


# ---- the shape matrix (tests/filter_cases.py): every kernel form, nblk = 2 ... 25, the switch points -----------------------------

def _check_cell(monkeypatch, k, contigs, ref, thr, chain):
    """What test_matrix asserts of one (references, genome, threshold): on == off == oracles, the device's candidates are numpy's,
    the bound and the kernel form are the expected ones, the filter ran and did not fall back."""
    N, W = ref["N"], ref["ws"]
    on, ohits = _on_off_oracle(monkeypatch, contigs, ref, thr, k=k, W=W, all_flags=(0, _lib.F_CHAIN_REPLAY) if chain else (0,))
    T, T_hi = filter_ref.threshold_band(thr, k, N)
    U = filter_ref.bound_U(ref["S"], N, k, W, T, T_hi)
    want = filter_ref.candidates(contigs, ref["S"], k, W, U)
    fs = on["fstats"][0]
    print("k %d N %d nk %d thr %.2f U %d Smax %d: form %#x granules %d regions %d streams %d windows %d of %d, %d hits" % (
        k, N, W - k + 1, thr, U, int(np.max(ref["S"])), fs["form"], fs["granules"], fs["regions"], fs["streams"], fs["windows"],
        fs["total_windows"], len(on["hits"])))
    assert fs["bound"] == U > 0
    assert fs["form"] == fc.form_of(k, int(np.max(ref["S"])))
    assert np.array_equal(on["cand"], want)
    assert fs["granules"] == len(want) > 0
    return on, ohits


@pytest.mark.parametrize("cell", fc.MATRIX, ids=fc.cell_id)
def test_matrix(monkeypatch, cell):
    """k = 5, 6 x one- and two-byte S entries x nblk = 2, 2, 2, 3, 4, 8, 19, 25: the long record with its plants and its tandem
    run (>= 128 candidate granules in a row: lo_cur and lo_prev) and the short records whose last granule is a candidate (lim)."""
    k, N, nk = cell
    c = fc.cell(k, N, nk)
    assert (int(c["ref"]["S"].max()) < 256) == (N == 7) and fc.longest_run(c["want"]) >= 128
    # (the chain replay at every nk up to CHAIN_NK: below a step's 64 k-mers the filtered scan is held to the Float64 oracle's hits too)
    on, ohits = _check_cell(monkeypatch, k, c["contigs"], c["ref"], c["thr"], chain=nk <= fc.CHAIN_NK)
    assert np.array_equal(on["cand"], c["want"]) and on["fstats"][0]["bound"] == c["U"]
    assert on["fstats"][0]["form"] == {(5, 7): 0x2001, (5, 300): 0x2002, (6, 7): 0x2001, (6, 300): 0x0102}[(k, N)]
    assert len(on["hits"]) > 0 and len(on["dips"]) >= 10                # (the plants of the long record at least)


def _edge_ref(k, value):
    """The k = 5 / 6, nk = 100, N = 300 family with the S entry of a k-mer of the base that every plant holds overwritten (255 and 256: the others
    clipped to 255), the matrix genome, and a threshold: the largest planted distance under the new S plus the matrix cell's margin (a
    quarter of the largest planted distance under the family's own S, + 0.05).  The margin is kept absolute because one entry of
    65535 puts (65535 - N c)^2 into every planted window's distance: a quarter of that would put Dmax above sumS2 + N^2 n, U <= 0."""
    c = fc.cell(k, 300, 100)
    base, W = c["ref"]["base"], c["W"]
    km = kmer_values(base, k)
    planted = [set(kmer_values(c["contigs"][r][s:s + W], k).tolist()) for r, s in c["plants"]]
    x = next(int(v) for v in km if np.count_nonzero(km == v) == 1 and all(int(v) in p for p in planted))   # in every plant, once in the base
    S = c["ref"]["S"].copy()
    if value in (255, 256):
        S = np.minimum(S, 255)
    S[x] = value
    ref = fc.ref_from_S(S, 300, k, W, base)
    D = fc.exact_D(c["contigs"], S, 300, k, W)
    thr = round(fc.planted_max(D, c["plants"], k, 300) + 0.25 * fc.planted_max(c["D"], c["plants"], k, 300) + 0.05, 2)
    return c, ref, thr


@pytest.mark.parametrize("k", [5, 6])
@pytest.mark.parametrize("value", [255, 256, 65535, 65536])
def test_entry_width_edges(monkeypatch, k, value):
    """Smax 255 | 256 selects the entry width, 65535 is the last value the two-byte table holds (read without sign extension: the
    plants hold that k-mer), 65536 keeps the filter off."""
    c, ref, thr = _edge_ref(k, value)
    assert int(ref["S"].max()) == value
    if value == 65536:
        on, ohits = _on_off_oracle(monkeypatch, c["contigs"], ref, thr, expect_ran=False, k=k, W=c["W"])
        assert len(ohits) >= 10 and len(on["cand"]) == 0
        return
    on, ohits = _check_cell(monkeypatch, k, c["contigs"], ref, thr, chain=True)
    assert on["fstats"][0]["form"] & 0xFF == (1 if value == 255 else 2)
    assert len(ohits) >= 10
    have = set(map(tuple, on["cand"].tolist()))
    assert all((r, s // 16) in have for r, s in c["plants"])            # found through the overwritten entry


@pytest.mark.parametrize("nk,N", [(17, 7), (17, 300), (383, 7), (383, 300)])
def test_threshold_on_a_windows_distance_k5(monkeypatch, nk, N):
    """test_threshold_on_a_windows_distance at k = 5 with nblk = 2 and 25."""
    k, W = 5, nk + 4
    ref = fc.family(k, N, nk)
    rng = np.random.default_rng([6203, nk, N])
    contigs = [random_dna(rng, 5_000) + mutate(rng, ref["base"], 0.04) + random_dna(rng, 5_000) + ref["base"] + random_dna(rng, 3_000)]
    D = fc.exact_D(contigs, ref["S"], N, k, W)[0]
    scale = 2.0 * k * N * N
    above = np.nonzero(D > D[10_000 + W])[0]
    s = int(above[np.argmin(np.abs(D[above] - 1.15 * D[10_000 + W]))])   # the window nearest above the exact copy's distance
    thr = float(D[s]) / scale
    T, T_hi = filter_ref.threshold_band(thr, k, N)
    assert T == D[s] <= T_hi and D[10_000 + W] < T
    on, _ = _on_off_oracle(monkeypatch, contigs, ref, thr, k=k, W=W)
    assert on["counts"][2] > 0 and [s + 1] in on["att"][:, 2:].tolist()
    fs = on["fstats"][0]
    assert fs["bound"] == filter_ref.bound_U(ref["S"], N, k, W, T, T_hi) and fs["form"] == fc.form_of(k, int(ref["S"].max()))
    assert np.array_equal(on["cand"], filter_ref.candidates(contigs, ref["S"], k, W, fs["bound"]))
    assert len(on["dips"]) > 0


@pytest.mark.parametrize("k,N,nk", [(5, 300, 16), (6, 7, 284), (6, 300, 100)])   # (cells whose numpy set is empty)
def test_no_candidates(monkeypatch, k, N, nk):
    """Plants mutated at 4 % and a threshold no window meets: the filter runs, names nothing, and the scan walks one region per
    record with a window (its first windows) and finds nothing."""
    ref = fc.family(k, N, nk)
    W = ref["ws"]
    contigs, _ = fc.genome(k, nk, ref["base"], plant_rate=0.04)
    contigs[0] = contigs[0][:fc.TANDEM_AT] + contigs[0][:fc.PLANT_EVERY][-10_000:] + contigs[0][fc.TANDEM_AT + 10_000:]   # no exact copy
    assert len(contigs[0]) == fc.LONG
    T, T_hi = filter_ref.threshold_band(0.01, k, N)
    U = filter_ref.bound_U(ref["S"], N, k, W, T, T_hi)
    assert U > 0 and len(filter_ref.candidates(contigs, ref["S"], k, W, U)) == 0
    on, ohits = _on_off_oracle(monkeypatch, contigs, ref, 0.01, k=k, W=W, all_flags=(0,))
    fs = on["fstats"][0]
    assert fs["bound"] == U and fs["form"] == fc.form_of(k, int(ref["S"].max()))
    assert len(on["cand"]) == 0 and fs["granules"] == 0
    assert fs["regions"] == sum(len(c) >= W for c in contigs) == len(contigs) - 1
    assert len(on["hits"]) == 0 and len(ohits) == 0 and len(on["dips"]) == 0


@pytest.mark.parametrize("k,N", [(5, 300), (6, 7)])
def test_bound_not_positive(monkeypatch, k, N):
    """A threshold above every window's distance: U <= 0, every window would be a candidate and the filter is skipped (no
    fallback, the bound stays 0); every record with a window is one long dip."""
    c = fc.cell(k, N, 34)
    ref, W, contigs = c["ref"], c["W"], c["contigs"]
    thr = float(np.ceil(max(int(d.max()) for d in c["D"] if d.size) / (2.0 * k * N * N))) + 1.0
    T, T_hi = filter_ref.threshold_band(thr, k, N)
    assert filter_ref.bound_U(ref["S"], N, k, W, T, T_hi) <= 0
    on, _ = _on_off_oracle(monkeypatch, contigs, ref, thr, expect_ran=False, k=k, W=W, all_flags=(0,))
    assert on["fstats"][0]["bound"] == 0 and len(on["cand"]) == 0
    # (a record's first window is never tested: records of one window have no dip; the dip is open at the record's end)
    assert sorted(d["contig"] for d in on["dips"]) == [r for r, seq in enumerate(contigs) if len(seq) > W]
    assert all(d["end"] == len(contigs[d["contig"]]) - W + 1 for d in on["dips"])


def test_fallback_reports_the_device_set(monkeypatch):
    """A threshold at which more than half of the granules are candidates: the scan falls back (FILTER_FRACTION), the results
    are the unfiltered scan's and kgma_get_filter_candidates still serves the kernel's set -- the numpy set."""
    k, N, nk = 5, 7, 34
    c = fc.cell(k, N, nk)
    ref, W, contigs = c["ref"], c["W"], c["contigs"]
    n_gran = sum((len(seq) - W + 16) // 16 for seq in contigs if len(seq) >= W)
    Dall = np.sort(np.concatenate(c["D"]))
    thr = round(float(Dall[int(0.4 * Dall.size)]) / (2.0 * k * N * N), 2)       # four windows in ten are below it
    T, T_hi = filter_ref.threshold_band(thr, k, N)
    U = filter_ref.bound_U(ref["S"], N, k, W, T, T_hi)
    want = filter_ref.candidates(contigs, ref["S"], k, W, U)
    assert U > 0 and len(want) > 0.6 * n_gran                            # (candidate windows alone pass FILTER_MAX_FRACTION = 0.5)
    on = _scan(monkeypatch, contigs, ref, thr, 0, True, k=k)
    off = _scan(monkeypatch, contigs, ref, thr, 0, False, k=k)
    _same(on, off)
    fs = on["fstats"][0]
    assert (fs["ran"], fs["fell_back"], fs["reason"]) == (1, 1, _lib.FILTER_FRACTION), fs
    assert fs["bound"] == U and fs["form"] == fc.form_of(k, int(ref["S"].max()))
    assert np.array_equal(on["cand"], want) and fs["granules"] == len(want)
