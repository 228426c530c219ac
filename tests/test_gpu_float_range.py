"""The Float64 form of the generic kernel (gen_kernel<f64, ...>) and the generic chain kernel over the range of KFVs kgma_set_refs
accepts: tests/float_cases.py builds signed, wide-range, near-count, absorbing and limit tables for every place the kernel keeps
its counts (cmode 0 ... 5), tests/float_exact.py gives every window's distance as a rational and an a-priori rounding bound, and
tests/test_float_cases.py shows on the CPU that the reference itself stays inside that bound and that the bound notices a wrong
table entry.  Here every case runs on the device:

  * default mode: every distance within bound[q] of exact[q] (an absolute comparison of rationals -- no relative tolerance: at a
    near-count table's exact copy the distance is below its own rounding noise), no distance negative, hits by the rule of
    _assert_float_single, D = round(dist x scale) on hits and dips, a window in the guard band when thr is its distance;
  * kgma_chain_values: the oracle's running value bit for bit at every window, also with 1024-window chain streams;
  * chain mode: the oracle's hits, nothing flagged, chain-decided distances bit for bit;
  * the cluster engine, the dense / sparse entry points, the landscape reductions on near-count distances, the magnitude limit.

Every input is legal and nothing here is repeated on failure."""
import re
from fractions import Fraction

import numpy as np
import pytest

from kmergma_amd import _lib
from oracle import oracle as orc
from tests import float_cases as fc
from tests import float_exact as fx
from tests import landscape_ref as lr
from tests.helpers import hit_key
from tests.test_gpu_parity import _assert_omn_chain_parity

pytestmark = pytest.mark.gpu

_GEOM = re.compile(r"generic (scan|chain) geometry: k (\d+), cmode (\d+),")
AMB = _lib.HIT_TIE | _lib.HIT_AT_THRESHOLD
BUFF = 50


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture
def geom(monkeypatch, capfd):
    """geom() -> {(kind, k, cmode)} of the library's KGMA_GEOM_DEBUG lines since the last call."""
    monkeypatch.setenv("KGMA_GEOM_DEBUG", "1")
    capfd.readouterr()

    def read():
        return {(m[0], int(m[1]), int(m[2])) for m in _GEOM.findall(capfd.readouterr().err)}
    return read


def _setenv(monkeypatch, c):
    monkeypatch.setenv("KGMA_KERNEL", "generic")
    monkeypatch.setenv("KGMA_CHAIN_GENERIC", "1")
    for key, v in c["env"].items():
        monkeypatch.setenv(key, v)


def _set_refs(ctx, c, thr, kfv=None, W=None):
    kfv = c["kfv"] if kfv is None else kfv
    if isinstance(kfv, tuple):
        ctx.set_refs_sparse(c["k"], [kfv[0]], [kfv[1]], [W or c["W"]], [thr], None)
    else:
        ctx.set_refs(c["k"], [kfv], [W or c["W"]], [thr], None)
    assert ctx.kfv_is_float(1)


def _worst_ratio(d, offset, refs, first=1):
    """max |d - exact| / bound over the values of a distance vector (value i of a record: window first + i, 0-based), as rationals;
    fails on the first value outside its bound."""
    worst = Fraction(0)
    for rec, r in enumerate(refs):
        v = d[offset[rec]:offset[rec + 1]].tolist()
        assert len(v) == max(len(r.exact) - first, 0), rec
        for i, x in enumerate(v):
            q = first + i
            err = abs(Fraction(x) - r.exact[q])
            assert err <= r.bound[q], f"record {rec} window {q}: {x!r} is {float(err / r.bound[q]):.3g} x its bound from the exact {float(r.exact[q])!r}"
            worst = max(worst, err / r.bound[q])
    return worst


def _assert_lattice(ctx, d, offset):
    """kgma_hit.D and kgma_dip.D_min are round(dist x scale) of the distance they stand for.  (The first window of a record
    is never tested, GenomeMiner.jl:82, so every dip starts at window 2 or later and lies inside the distance vector.)"""
    scale = ctx.kfv_scale(1)
    for h in ctx.hits():
        assert h["D"] == fx.lattice(h["dist"], scale), h
    for x in ctx.dips():
        assert x["start"] >= 2, x
        lo = offset[x["contig"]] - 2
        assert x["D_min"] == fx.lattice(float(d[lo + x["start"]:lo + x["end"] + 1].min()), scale), x


def _assert_first_windows(ctx, refs):
    """kgma_get_first_window: the lattice point of a value within bound[0] of exact[0], and never negative (-1 says "skipped")."""
    scale = Fraction(ctx.kfv_scale(1))
    fw = ctx.first_window(1).tolist()
    assert len(fw) == len(refs)
    for D, r in zip(fw, refs):
        assert D >= 0, fw
        assert abs(Fraction(D) / scale - r.exact[0]) <= r.bound[0] + 1 / (2 * scale), (D, float(r.exact[0]))


def _assert_default_hits(ctx, c, thr):
    hits, dips, stats = ctx.hits(), ctx.dips(), ctx.stats()
    if [hit_key(h) for h in hits] != [hit_key(h) for h in fc.oracle_hits(c, thr, BUFF)]:
        unresolved = sum(1 for x in dips if x["flags"] & AMB)
        assert unresolved > 0 or stats["n_at_threshold"] > 0, "hits differ from the Float64 oracle although nothing is flagged"
    return stats


@pytest.mark.parametrize("name", fc.SCAN_NAMES)
def test_scan_within_the_bound(ctx, geom, monkeypatch, name):
    """Default mode, every case: the Float64 kernel in the case's count mode, every distance within its a-priori bound of the exact
    rational distance (the worst ratio is printed: DESIGN.md has the table), none negative, hits by _assert_float_single's rule,
    D = round(dist x scale); then the same scan with thr on the device's own distance of one window."""
    c = fc.case(name)
    _setenv(monkeypatch, c)
    refs = fc.reference(c)
    thr = fc.thr_mid(c)
    _set_refs(ctx, c, thr)
    if c["kind"] == "limit":
        assert ctx.kfv_scale(1) == 2.0 * c["k"]
    g = ctx.genome_from_host(c["records"])
    try:
        geom()
        ctx.scan(g, _lib.MODE_SINGLE, BUFF, 0, _lib.F_RETURN_DISTS, None)
        assert ctx.kernel_name().startswith("gen_kernel<f64"), ctx.kernel_name()
        assert {x[1:] for x in geom() if x[0] == "scan"} == {(c["k"], c["cmode"])}
        d, offset = ctx.dists(1), ctx.dist_layout()
        assert np.array_equal(offset, lr.layout([len(s) for s in c["records"]], c["W"]))
        worst = _worst_ratio(d, offset, refs)
        print(f"{name}: device worst err/bound {float(worst):.3g}, min distance {d.min()!r}")
        assert d.min() >= 0.0, f"a negative distance: {d.min()!r} at value {int(d.argmin())}"
        _assert_default_hits(ctx, c, thr)
        _assert_lattice(ctx, d, offset)
        _assert_first_windows(ctx, refs)
        # thr on a window's own device distance: that window sits in the guard band
        rec, q = fc.THR_AT_WINDOW
        thr_at = float(d[offset[rec] + q - 1])
        ctx.set_thresholds([thr_at])
        ctx.scan(g, _lib.MODE_SINGLE, BUFF, 0, _lib.F_RETURN_DISTS, None)
        assert ctx.dists(1).tobytes() == d.tobytes()
        assert _assert_default_hits(ctx, c, thr_at)["n_at_threshold"] >= 1
        _assert_lattice(ctx, d, offset)
    finally:
        g.free()


@pytest.mark.parametrize("name", [n for n in fc.SCAN_NAMES if n.startswith(("signed-", "wide-")) and fc.case(n)["k"] <= 10
                                  and fc.case(n)["cell"] in ("k3-w50", "k6-w305", "k8-w300")])
def test_dense_and_sparse_entry_give_the_same_bits(ctx, monkeypatch, name):
    """kgma_set_refs_sparse with the non-zero entries of a dense table (the -0.0 entries are zeros and stay out): every distance
    bit-identical to kgma_set_refs on the table."""
    c = fc.case(name)
    _setenv(monkeypatch, c)
    thr = fc.thr_mid(c)
    g = ctx.genome_from_host(c["records"])
    try:
        _set_refs(ctx, c, thr)
        ctx.scan(g, _lib.MODE_SINGLE, BUFF, 0, _lib.F_RETURN_DISTS, None)
        dense, dense_first = ctx.dists(1).tobytes(), ctx.first_window(1).tolist()
        keys = np.flatnonzero(c["kfv"] != 0.0)
        assert keys.size < c["kfv"].size or c["kind"] == "signed"
        _set_refs(ctx, c, thr, kfv=(keys.astype(np.uint32), c["kfv"][keys]))
        ctx.scan(g, _lib.MODE_SINGLE, BUFF, 0, _lib.F_RETURN_DISTS, None)
        assert ctx.kernel_name().startswith("gen_kernel<f64")
        assert ctx.dists(1).tobytes() == dense and ctx.first_window(1).tolist() == dense_first
    finally:
        g.free()


def _assert_chain_values(ctx, c, geom):
    _set_refs(ctx, c, fc.thr_mid(c))
    want = fc.oracle_chain(c)
    g = ctx.genome_from_host(c["records"])
    try:
        geom()
        for rec, seq in enumerate(c["records"]):
            nwin = len(seq) - c["W"] + 1
            if c["kind"] in fc.NOISE and rec == 4:
                # the record begins with the exact copy: its first distance is noise, and the device chain, which checks itself
                # against that distance RELATIVELY at every stream start, may decline (kgma.h: KGMA_E_UNSUPPORTED, no fallback in
                # this call; a scan falls back to the host chain: test_chain_mode_scan) -- but it never returns other bits
                try:
                    got = g.chain_values(rec, 1, [(1, nwin)])
                except _lib.KgmaError as e:
                    assert e.status == _lib.KGMA_E_UNSUPPORTED and "drift check" in str(e), str(e)
                    continue
            else:
                got = g.chain_values(rec, 1, [(1, nwin)])
            assert ctx.stats()["chain_device_pairs"] == 1, rec
            assert np.array_equal(got, want[rec]), f"record {rec}: first mismatch at window {int(np.argmax(got != want[rec])) + 1}"
        assert {x[1:] for x in geom() if x[0] == "chain"} == {(c["k"], c["cmode"])}
    finally:
        g.free()


@pytest.mark.parametrize("name", fc.SCAN_NAMES)
def test_chain_values_every_window(ctx, geom, monkeypatch, name):
    """gen_chain_kernel: the reference's running value at every window of every record, bit for bit -- through values that are
    rounding noise of either sign, increments far above and far below the value's ulp, and a binade change every few steps."""
    c = fc.case(name)
    _setenv(monkeypatch, c)
    _assert_chain_values(ctx, c, geom)


@pytest.mark.parametrize("name", fc.STREAM_1024_NAMES)
def test_chain_values_short_chain_streams(ctx, geom, monkeypatch, name):
    c = fc.case(name)
    _setenv(monkeypatch, c)
    monkeypatch.setenv("KGMA_CHAIN_STREAM", "1024")
    _assert_chain_values(ctx, c, geom)


@pytest.mark.parametrize("name", fc.SCAN_NAMES)
def test_chain_mode_scan(ctx, monkeypatch, name):
    """KGMA_F_CHAIN_REPLAY: the oracle's hits, nothing flagged; a chain-decided hit carries the oracle's distance bit for bit, any
    other lies within 2 x bound of it.  The scan is not repeated with a wider band where the oracle's own drift from the exact
    distance (tests/float_cases.py: oracle_drift, CPU arithmetic) is below 2^-32; elsewhere the drift it reports is below half
    the band it ended with."""
    c = fc.case(name)
    _setenv(monkeypatch, c)
    refs = fc.reference(c)
    thr = fc.thr_mid(c)
    ohits = fc.oracle_hits(c, thr, BUFF)
    _set_refs(ctx, c, thr)
    g = ctx.genome_from_host(c["records"])
    try:
        ctx.scan(g, _lib.MODE_SINGLE, BUFF, 0, _lib.F_CHAIN_REPLAY, None)
        hits, dips, st = ctx.hits(), ctx.dips(), ctx.stats()
    finally:
        g.free()
    assert [hit_key(h) for h in hits] == [hit_key(h) for h in ohits]
    assert st["n_tie_flagged"] == 0 and not any(x["flags"] & AMB for x in dips)
    for a, b in zip(hits, ohits):
        if a["flags"] & _lib.HIT_CHAIN:
            assert a["dist"] == b["dist"], (a, b)
        else:
            r = refs[a["contig"]]
            q = min(max(a["cmi"] - c["k"], 0), len(r.bound) - 1)
            assert abs(Fraction(a["dist"]) - Fraction(b["dist"])) <= 2 * r.bound[q], (a, b)
    if fc.oracle_drift(c, thr) < Fraction(1, 2 ** 32):
        assert st["chain_rescans"] == 0, st
    else:
        assert st["chain_max_drift"] < 2.0 ** -(st["chain_band_log2"] + 1), st


def _first_windows_of(r, n):
    """The first n windows of a float_exact.Record."""
    out = fx.Record()
    out.exact, out.bound = r.exact[:n], r.bound[:n]
    return out


def test_cluster_engine(ctx, monkeypatch):
    """One MODE_OMN scan at k = 6 with a signed (W = 40), a near-count (W = 305) and an absorbing (W = 120) table: every distance
    of every KFV within its bound, chain mode identical to the Float64 oracle."""
    k = 6
    base = fc.case("nearcount-k6-w305")
    records = base["records"]
    kfvs = [fc.case("signed-k6-w40")["kfv"], base["kfv"], fc.case("absorb-k6-w305")["kfv"]]
    ws = [40, 305, 120]
    monkeypatch.setenv("KGMA_KERNEL", "generic")
    monkeypatch.setenv("KGMA_CHAIN_GENERIC", "1")
    refs = [fc.reference(base) if W == 305 else tuple(fx.scan(s, kfv, k, W) for s in records) for kfv, W in zip(kfvs, ws)]
    thr = []
    for r in refs:
        every = sorted(x for rr in r for x in rr.exact)
        thr.append(float((min(r[0].exact[fc.MUT_AT - 20:fc.MUT_AT + 21]) + every[len(every) // 2]) / 2))
    # the cluster engine walks every KFV over the windows of the longest one: L - max(ws) - k + 2 values per record
    n_val = [max(len(s) - max(ws) - k + 2, 0) for s in records]
    offset = np.concatenate([[0], np.cumsum(n_val)])
    ctx.set_refs(k, kfvs, ws, thr, None)
    gen = ctx.genome_from_host(records)
    try:
        ctx.scan(gen, _lib.MODE_OMN, 100, 55, _lib.F_RETURN_DISTS, None)
        assert ctx.kernel_name().startswith("gen_kernel<f64")
        for j, r in enumerate(refs):
            d = ctx.dists(j + 1)
            assert d.size == offset[-1], j
            worst = _worst_ratio(d, offset, [_first_windows_of(rr, n + 1 if n else 0) for rr, n in zip(r, n_val)])
            print(f"cluster KFV {j + 1} (W = {ws[j]}): device worst err/bound {float(worst):.3g}, min distance {d.min()!r}")
            assert d.min() >= 0.0
        fo, _ = orc.omn_scan(records, kfvs, k, ws, thr, 100, 55)
        ctx.scan(gen, _lib.MODE_OMN, 100, 55, _lib.F_CHAIN_REPLAY, None)
        _assert_omn_chain_parity(ctx.hits(), ctx.dips(), ctx.stats(), fo)
    finally:
        gen.free()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", fc.NEARCOUNT_NAMES)
def test_landscape_of_noise_level_distances(ctx, monkeypatch, name):
    """A table that is a window's count vector up to noise: the distance there is rounding noise, and the first-window identity
    d0 = SF/2 ((sum ref^2 - 2 sum ref[K_p]) + (n + 2 pairs)) cancels to a value of either sign.  Every scan writes non-negative
    doubles all the same (kgma.h; the bin minima are ordered by their bit patterns): none is negative, and kgma_dist_bins /
    kgma_dist_sweep equal the NumPy model on the returned vector taken as signed doubles."""
    c = fc.case(name)
    _setenv(monkeypatch, c)
    thr = fc.thr_mid(c)
    _set_refs(ctx, c, thr)
    g = ctx.genome_from_host(c["records"])
    try:
        ctx.scan(g, _lib.MODE_SINGLE, BUFF, 0, _lib.F_RETURN_DISTS, None)
    finally:
        g.free()
    d, offset = ctx.dists(1), ctx.dist_layout()
    plant = float(d[offset[0] + c["exact_at"] - 1])
    print(f"{name}: distance at the exact copy {plant!r} (exact {float(fc.reference(c)[0].exact[c['exact_at']]):.3g}), negative values: {int(np.count_nonzero(d < 0))}")
    assert d.min() >= 0.0, f"a negative distance: {d.min()!r} at value {int(d.argmin())}"
    for width in (1, 64, 1000):
        bmin, barg, boff = ctx.dist_bins(1, width)
        m, a, o = lr.bins(d, offset, width)
        assert np.array_equal(boff, o), width
        assert np.array_equal(_bits(bmin), _bits(m)), (width, int(np.argmax(_bits(bmin) != _bits(m))))
        assert np.array_equal(barg, a), (width, int(np.argmax(barg != a)))
    step = max(abs(plant), 1e-17)
    sweep = np.array([plant - step, plant, plant + step, thr])
    below, dips = ctx.dist_sweep(sweep, 1)
    want = lr.sweep_brute(d, offset, sweep)
    assert np.array_equal(below, want[0]) and np.array_equal(dips, want[1]), (below, dips, want)
    assert below[2] >= 1


@pytest.mark.parametrize("name", fc.OVER_NAMES)
def test_magnitude_beyond_the_limit_is_refused(ctx, monkeypatch, name):
    """sum ref^2 + n^2 + 2 n max|ref| + 1 half a percent above 2^61: KGMA_E_UNSUPPORTED with the magnitude in the message, from both
    entry points, and the context serves a normal KFV afterwards."""
    c = fc.case(name)
    _setenv(monkeypatch, c)
    keys = np.flatnonzero(c["kfv"] != 0.0)
    for kfv in (c["kfv"], (keys.astype(np.uint32), c["kfv"][keys])):
        with pytest.raises(_lib.KgmaError) as e:
            if isinstance(kfv, tuple):
                ctx.set_refs_sparse(c["k"], [kfv[0]], [kfv[1]], [c["W"]], [1.0], None)
            else:
                ctx.set_refs(c["k"], [kfv], [c["W"]], [1.0], None)
        assert e.value.status == _lib.KGMA_E_UNSUPPORTED
        assert "magnitude" in str(e.value) and f"{np.abs(c['kfv']).max():.3g}" in str(e.value), str(e.value)
    ok = fc.case(name.replace("over-", "signed-"))
    thr = fc.thr_mid(ok)
    _set_refs(ctx, ok, thr)
    g = ctx.genome_from_host(ok["records"])
    try:
        ctx.scan(g, _lib.MODE_SINGLE, BUFF, 0, _lib.F_RETURN_DISTS, None)
        _worst_ratio(ctx.dists(1), ctx.dist_layout(), fc.reference(ok))
    finally:
        g.free()
