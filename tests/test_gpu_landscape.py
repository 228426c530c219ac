"""The distance landscape on the device (kgma_dist_layout / kgma_dist_bins / kgma_dist_sweep and the api functions above them)
against the NumPy model of tests/landscape_ref.py, on ctx.dists(kfv) of the same scan: bin minima bit for bit, window starts and
counts exactly.  (The existing suites hold those distances to the oracles.)  The cases and what each is there for:
tests/landscape_cases.py; every property is asserted again here on the device's own distances."""
import numpy as np
import pytest

from kmergma_amd import _lib, api
from kmergma_amd.fasta import Record, reverse_complement
from tests import filter_cases as fc
from tests import landscape_cases as lc
from tests import landscape_ref as lr
from tests import range_cases as rc

pytestmark = pytest.mark.gpu

FEW_BINS = (1, 64, 65, 129, lc.BINS_WG + 1, 10 ** 7)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _check_bins(ctx, kfv, d, offset, widths):
    for width in widths:
        bmin, barg, boff = ctx.dist_bins(kfv, width)
        m, a, o = lr.bins(d, offset, width)
        assert np.array_equal(boff, o), width
        assert np.array_equal(_bits(bmin), _bits(m)), (width, int(np.argmax(_bits(bmin) != _bits(m))))
        assert np.array_equal(barg, a), (width, int(np.argmax(barg != a)))
        st = ctx.landscape_stats()
        assert st["n_values"] == d.size and st["n_bins"] == m.size and st["n_launches"] == (2 if m.size else 0)


def _check_sweep(ctx, kfv, d, offset, thr, brute=False):
    below, dips = ctx.dist_sweep(thr, kfv)
    want = lr.sweep_brute(d, offset, thr) if brute else lr.sweep(d, offset, thr)
    assert np.array_equal(below, want[0]), int(np.argmax(below != want[0]))
    assert np.array_equal(dips, want[1]), int(np.argmax(dips != want[1]))
    st = ctx.landscape_stats()
    assert st["sweep_slots"] == (64 if len(thr) <= 64 else 512 if len(thr) <= 512 else 4096) and st["n_values"] == d.size
    return below, dips


def _check_all(ctx, kfv, d, offset, widths):
    _check_bins(ctx, kfv, d, offset, widths)
    for key, thr in lc.sweep_cases(d, offset).items():
        _check_sweep(ctx, kfv, d, offset, thr, brute=thr.size <= 2)


def _scan(ctx, ref, contigs, thr=3.0, mode=_lib.MODE_SINGLE):
    ctx.set_refs(ref["k"], [ref["RV"]], [ref["ws"]], [thr], [ref["N"]])
    g = ctx.genome_from_host(contigs)
    try:
        ctx.scan(g, mode, 50, 0, _lib.F_RETURN_DISTS, None)
    finally:
        g.free()
    return ctx.dists(1), ctx.dist_layout()


@pytest.mark.parametrize("name", lc.GENOMES)
def test_bins_and_sweeps_of_the_cases(ctx, name):
    contigs = lc.genome(name)
    d, offset = _scan(ctx, lc.ref(), contigs)
    ed, eo = lc.exact(name)
    assert np.array_equal(offset, eo) and np.array_equal(offset, lr.layout([len(c) for c in contigs], lc.W))
    assert np.array_equal(_bits(d), _bits(ed))
    lc.check_genome(name, d, offset)
    _check_all(ctx, 1, d, offset, lc.BINS)
    n_rec = int(np.count_nonzero(np.diff(offset)))
    below, dips = _check_sweep(ctx, 1, d, offset, lc.sweep_cases(d, offset)["1-over"], brute=True)
    assert below[0] == d.size and dips[0] == n_rec            # records below in a row: one dip each
    if name == "long":
        thr, at = lc.boundary_thresholds(d, offset)
        _check_sweep(ctx, 1, d, offset, thr, brute=True)
        bmin, barg, _ = ctx.dist_bins(1, 10 ** 7)
        assert barg.tolist() == [lc.EQUAL_AT[0] + 2] and bmin[0] == d.min()
    if name == "homo":
        bmin, barg, boff = ctx.dist_bins(1, 64)
        b = np.arange(boff[1], boff[2])
        assert np.array_equal(barg[b], 64 * (b - boff[1]) + 2)


def _dips_of_scan(ctx, ref, contigs, est):
    thr = api.off_lattice_threshold(est, ctx.kfv_scale(1))
    d, offset = _scan(ctx, ref, contigs, thr)
    n_dips = len(ctx.dips())
    below, dips = _check_sweep(ctx, 1, d, offset, np.array([thr]), brute=True)
    return n_dips, int(dips[0]), int(below[0])


def test_dips_below_is_the_scans_dip_count(ctx, alp_ref, loci):
    """kgma_get_dips of a scan at an off-lattice threshold lists as many dips as the sweep counts at that threshold."""
    ref = dict(k=6, RV=alp_ref["RV"], ws=alp_ref["ws"], N=alp_ref["N"])
    ctx.set_refs(6, [ref["RV"]], [ref["ws"]], [30.0], [ref["N"]])
    seen = []
    for est in (10.0, 30.0, 40.0):
        n_dips, swept, below = _dips_of_scan(ctx, ref, [r.sequence for r in loci], est)
        assert n_dips == swept, (est, n_dips, swept)
        seen.append(n_dips)
    assert seen[0] >= 3 and seen[2] > seen[0]
    ctx.set_refs(lc.K, [lc.ref()["RV"]], [lc.W], [3.0], [lc.ref()["N"]])
    for est in (0.5, 3.0, 6.0):
        n_dips, swept, below = _dips_of_scan(ctx, lc.ref(), lc.genome("long"), est)
        assert n_dips == swept >= 5, (est, n_dips, swept)


def test_cluster_engine_every_kfv(ctx):
    """3 KFVs of 2 window sizes in lock-step: every KFV's vector has the layout of kgma_dist_layout and its own landscape."""
    refs = [fc.family(6, 5, 60, seed=lc.SEED + 1), fc.family(6, 4, 60, seed=lc.SEED + 2), fc.family(6, 5, 90, seed=lc.SEED + 3)]
    assert sorted({r["ws"] for r in refs}) == [65, 95]
    rng = np.random.default_rng(lc.SEED + 4)
    a = bytearray(lc.genome("long")[0][:6000])
    for i, r in enumerate(refs):
        a[700 + 1500 * i:700 + 1500 * i + r["ws"]] = r["base"]
    contigs = lc.genome("edges")[2:] + [bytes(a), rng.permutation(np.frombuffer(bytes(a[:300]), dtype=np.uint8)).tobytes()]
    ctx.set_refs(6, [r["RV"] for r in refs], [r["ws"] for r in refs], [3.0] * 3, [r["N"] for r in refs])
    g = ctx.genome_from_host(contigs)
    try:
        ctx.scan(g, _lib.MODE_OMN, 50, 0, _lib.F_RETURN_DISTS, None)
    finally:
        g.free()
    offset = ctx.dist_layout()
    assert offset.size == len(contigs) + 1
    vectors = [ctx.dists(j + 1) for j in range(3)]
    assert all(v.size == offset[-1] for v in vectors) and not np.array_equal(vectors[0], vectors[1])
    for j, d in enumerate(vectors):
        _check_all(ctx, j + 1, d, offset, FEW_BINS)
    with pytest.raises(_lib.KgmaError) as e:
        ctx.dist_bins(4, 64)
    assert e.value.status == _lib.KGMA_E_ARG


def test_float64_kfv(ctx):
    ref = dict(lc.ref())
    rng = np.random.default_rng(lc.SEED + 5)
    ref["RV"] = ref["RV"] + 0.37 * rng.random(ref["RV"].size)
    ctx.set_refs(ref["k"], [ref["RV"]], [ref["ws"]], [3.0], None)
    assert ctx.kfv_is_float(1)
    g = ctx.genome_from_host(lc.genome("long") + lc.genome("edges"))
    try:
        ctx.scan(g, _lib.MODE_SINGLE, 50, 0, _lib.F_RETURN_DISTS, None)
    finally:
        g.free()
    d, offset = ctx.dists(1), ctx.dist_layout()
    assert np.unique(d).size > 2000
    _check_all(ctx, 1, d, offset, lc.BINS)


def test_distances_beyond_2_53(ctx):
    """A cell of tests/range_cases.py whose D passes 2^53: the landscape is defined on the doubles the scan wrote."""
    x = rc.cell("d61", 6, 100, "copies", "-")
    ref = x["ref"]
    assert x["dmax"] > 2 ** 53
    d, offset = _scan(ctx, dict(k=x["k"], RV=ref["RV"], ws=x["W"], N=ref["N"]), x["contigs"], x["thr"][0])
    assert d.max() * ctx.kfv_scale(1) > 2.0 ** 53
    _check_all(ctx, 1, d, offset, FEW_BINS)


def _status(f):
    with pytest.raises(_lib.KgmaError) as e:
        f()
    return e.value.status, e.value.message


def test_errors(ctx):
    ref, contigs = lc.ref(), lc.genome("edges")
    ctx.set_refs(ref["k"], [ref["RV"]], [ref["ws"]], [3.0], [ref["N"]])
    assert _status(ctx.dist_layout)[0] == _lib.KGMA_E_STATE                     # no scan yet
    g = ctx.genome_from_host(contigs)
    try:
        ctx.scan(g, _lib.MODE_SINGLE, 50, 0, 0, None)                            # distances not kept
        want = _status(lambda: ctx.dists(1))
        assert want[0] == _lib.KGMA_E_STATE
        assert _status(lambda: ctx.dist_bins(1, 64)) == want
        assert _status(lambda: ctx.dist_sweep([1.0], 1)) == want
        assert np.array_equal(ctx.dist_layout(), lr.layout([len(c) for c in contigs], lc.W))    # the layout needs none
        ctx.scan(g, _lib.MODE_SINGLE, 50, 0, _lib.F_RETURN_DISTS, None)
    finally:
        g.free()
    arg = _lib.KGMA_E_ARG
    assert _status(lambda: ctx.dist_bins(2, 64))[0] == arg and _status(lambda: ctx.dist_bins(0, 64))[0] == arg
    assert _status(lambda: ctx.dist_bins(1, 0))[0] == arg and _status(lambda: ctx.dist_bins(1, -5))[0] == arg
    assert _status(lambda: ctx.dist_sweep([1.0], 2))[0] == arg
    for bad in ([], [1.0, 1.0], [2.0, 1.0], [1.0, np.inf], [np.nan], [-np.inf, 1.0], np.arange(4097.0)):
        assert _status(lambda: ctx.dist_sweep(bad, 1))[0] == arg, bad
    below, dips = ctx.dist_sweep(np.arange(4096.0), 1)                            # 4096 are served
    assert below[-1] == ctx.dists(1).size
    # strobemer references: another window convention
    from kmergma_amd import refprep
    RV, W, _cons, (_S, N) = refprep.gen_ref_ws_cons_strobe([Record("b", ref["base"] * 3)], 2, 3, 5, 5, return_int=True)
    ctx.set_strobe_ref(2, 3, 5, 5, RV, W, 30.0, N)
    g = ctx.genome_from_host([lc.genome("long")[0][:3000]])
    try:
        ctx.strobe_scan(g, 50, _lib.F_RETURN_DISTS)
        assert ctx.dists(1).size > 0
        uns = _lib.KGMA_E_UNSUPPORTED
        assert _status(lambda: ctx.dist_bins(1, 64))[0] == uns and _status(lambda: ctx.dist_sweep([1.0], 1))[0] == uns
        assert _status(ctx.dist_layout)[0] == uns
    finally:
        g.free()


def test_api_landscape_both_strands_best_loci_and_sweep(ctx, tmp_path):
    ref = lc.ref()
    contigs = lc.genome("edges") + [lc.genome("long")[0][:5000]]
    records = [Record("rec%d some text" % i, s) for i, s in enumerate(contigs)]
    width = 50
    track = api.dist_landscape(records, ref["RV"], lc.W, lc.K, bin=width, n_refs=ref["N"], strand="both", ctx=ctx)
    assert len(track) == 2 * len(contigs) and [t.strand for t in track] == ["+"] * len(contigs) + ["-"] * len(contigs)
    for strand, seqs in (("+", contigs), ("-", [reverse_complement(s) for s in contigs])):
        d, offset = _scan(ctx, ref, seqs)
        m, a, o = lr.bins(d, offset, width)
        for c, s in enumerate(seqs):
            t = track[c + (len(contigs) if strand == "-" else 0)]
            want = a[o[c]:o[c + 1]]
            if strand == "-":
                want = len(s) - want - lc.W + 2                                    # forward start of the same window
                for b, fwd in enumerate(want):                                     # ... which holds the reversed window's residues
                    i = int(a[o[c] + b])
                    assert reverse_complement(contigs[c][fwd - 1:fwd - 1 + lc.W]) == s[i - 1:i - 1 + lc.W]
            assert t.identifier == "rec%d" % c and t.length == len(s) and t.bin == width and t.windowsize == lc.W
            assert np.array_equal(_bits(t.bin_min), _bits(m[o[c]:o[c + 1]])) and np.array_equal(t.bin_argmin, want)
    default = api.dist_landscape(records, ref["RV"], lc.W, lc.K, n_refs=ref["N"], ctx=ctx)
    assert [t.bin for t in default] == [lc.W] * len(contigs)
    for n, sep in ((5, None), (40, 10), (10 ** 6, 1)):
        assert api.best_loci(track, n, sep) == lr.best_loci(track, n, lc.W if sep is None else sep)
    api.write_bedgraph(track, str(tmp_path / "t.bedgraph"))
    assert len(open(tmp_path / "t.bedgraph").read().splitlines()) == sum(t.bin_min.size for t in track)
    # the sweep: explicit thresholds on both strands, then the default list
    thr = np.array([0.5, 2.0, 5.0, 9.0])
    sw = api.threshold_sweep(records, ref["RV"], lc.W, lc.K, thr, n_refs=ref["N"], strand="both", ctx=ctx)
    want = np.zeros((2, thr.size), dtype=np.int64)
    for seqs in (contigs, [reverse_complement(s) for s in contigs]):
        d, offset = _scan(ctx, ref, seqs)
        want += np.array(lr.sweep_brute(d, offset, thr))
    assert np.array_equal(sw.windows_below, want[0]) and np.array_equal(sw.dips_below, want[1]) and np.array_equal(sw.thresholds, thr)
    sw = api.threshold_sweep(records, ref["RV"], lc.W, lc.K, n_refs=ref["N"], ctx=ctx)
    d, offset = _scan(ctx, ref, contigs)
    scale = ctx.kfv_scale(1)
    assert 100 < sw.thresholds.size <= 4096 and np.all(np.diff(sw.thresholds) > 0)
    assert np.allclose(sw.thresholds * scale % 1.0, 0.5)                           # halfway between lattice points
    got = lr.sweep(d, offset, sw.thresholds)
    assert np.array_equal(sw.windows_below, got[0]) and np.array_equal(sw.dips_below, got[1])
    t = api.threshold_for_dips(sw, 3)
    assert t is not None and sw.dips_below[np.searchsorted(sw.thresholds, t)] <= 3
