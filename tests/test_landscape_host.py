"""The distance landscape without a GPU: the model (tests/landscape_ref.py) on the CPU oracle's distances, the case lists
(tests/landscape_cases.py) held to what they are there for, api.best_loci / write_bedgraph (host functions), and the new symbols
of libkgma.so.

The oracle reports hits and distances, no dip list: "the dips the oracle's scan has" at a threshold are counted here from its own
distance vector by a loop written for this test (a dip opens where a tested window is below the threshold and the one before it,
in the same record, is not), and every hit the oracle emits at that threshold is held to lie in one of them."""
import ctypes
import os

import numpy as np
import pytest

from kmergma_amd import _lib, api, headers
from oracle import oracle as orc
from tests import landscape_cases as lc
from tests import landscape_ref as lr

NEW_SYMBOLS = ("kgma_dist_layout", "kgma_dist_bins", "kgma_dist_sweep", "kgma_get_landscape_stats")


def test_library_exports_the_landscape_calls():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), f"libkgma.so does not export {s}"
        assert s in _lib.EXPORTS
    assert ctypes.sizeof(_lib.KgmaLandscapeStats) == 48
    for name in ("dist_layout", "dist_bins", "dist_sweep", "landscape_stats"):
        assert callable(getattr(_lib.Context, name))


def _count_dips(d, offset, thr):
    n = 0
    for c in range(len(offset) - 1):
        inside = False
        for x in d[offset[c]:offset[c + 1]]:
            below = x < thr
            n += below and not inside
            inside = below
    return n


@pytest.fixture(scope="module")
def loci_scan(alp_ref, loci, golden):
    """The oracle's scan of Loci.fasta at the golden threshold (30): hits, distances, layout."""
    g = golden["scan"]["single_no_align"]
    seqs = [r.sequence for r in loci]
    hits, d = orc.single_scan(seqs, alp_ref["RV"], 6, alp_ref["ws"], float(g["thr"]), g["buff"], return_dists=True)
    assert len(hits) == g["n_hits"] == 7
    for i, want in g["headers"].items():
        h = hits[int(i) - 1]
        assert headers.single_header(loci[h["contig"]].identifier, h["dist"], h["lo"], h["hi"], h["genome_pos"]) == want
    offset = lr.layout([len(s) for s in seqs], alp_ref["ws"])
    assert offset[-1] == d.size == 484127
    return dict(hits=hits, d=d, offset=offset, seqs=seqs)


def test_golden_hits_lie_in_bins_at_or_below_their_distance(loci_scan, alp_ref):
    d, offset, k = loci_scan["d"], loci_scan["offset"], alp_ref["k"]
    for width in (1, 289, 1000, 10 ** 7):
        bmin, barg, boff = lr.bins(d, offset, width)
        assert boff[-1] == bmin.size == barg.size
        for h in loci_scan["hits"]:
            i = h["cmi"] - k - 1                                   # CMI = i_left + 1 at the minimum; value i was pushed at i_left = k + i
            assert 0 <= i < offset[h["contig"] + 1] - offset[h["contig"]]
            b = boff[h["contig"]] + i // width
            assert bmin[b] <= h["dist"]
            assert d[offset[h["contig"]] + barg[b] - 2] == bmin[b]
    # bin = 1 is the vector itself
    bmin, barg, _ = lr.bins(d, offset, 1)
    assert np.array_equal(bmin, d)
    assert np.array_equal(barg, np.concatenate([np.arange(n) + 2 for n in np.diff(offset)]))


def test_dips_below_equals_the_oracles_dips(loci_scan, alp_ref):
    d, offset = loci_scan["d"], loci_scan["offset"]
    scale = 2.0 * alp_ref["k"] * alp_ref["N"] ** 2
    for est in (10.0, 30.0, 40.0):
        thr = api.off_lattice_threshold(est, scale)
        hits, d2 = orc.single_scan(loci_scan["seqs"], alp_ref["RV"], 6, alp_ref["ws"], thr, 50, return_dists=True)
        assert np.array_equal(d, d2)
        below, dips = lr.sweep(d, offset, [thr])
        n_dips = _count_dips(d, offset, thr)
        assert dips[0] == n_dips and below[0] == np.count_nonzero(d < thr)
        assert 1 <= len(hits) <= n_dips
        for h in hits:
            assert h["dist"] < thr
    thr = np.array([api.off_lattice_threshold(e, scale) for e in np.linspace(5, 45, 41)])
    got, want = lr.sweep(d, offset, thr), lr.sweep_brute(d, offset, thr)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("name", lc.GENOMES)
def test_cases_are_not_vacuous_and_the_model_agrees_with_itself(name):
    d, offset = lc.exact(name)
    lc.check_genome(name, d, offset)
    for width in lc.BINS:
        bmin, barg, boff = lr.bins(d, offset, width)
        n = np.diff(offset)
        assert np.array_equal(np.diff(boff), -(-n // width))
        rec = np.repeat(np.arange(n.size), np.diff(boff))
        assert np.array_equal(d[offset[rec] + barg - 2], bmin)
    cases = lc.sweep_cases(d, offset)
    for key, thr in cases.items():
        below, dips = lr.sweep(d, offset, thr)
        if thr.size <= 64 or name != "long":
            b2, d2 = lr.sweep_brute(d, offset, thr)
            assert np.array_equal(below, b2) and np.array_equal(dips, d2), key
    n_rec = int(np.count_nonzero(np.diff(offset)))
    assert lr.sweep(d, offset, cases["1-under"])[0][0] == 0 == lr.sweep(d, offset, cases["1-at-min"])[0][0]
    below, dips = lr.sweep(d, offset, cases["1-over"])
    assert below[0] == d.size and dips[0] == n_rec                # every record its own dip: two records below in a row are two
    assert lr.sweep(d, offset, cases["1-at-max"])[0][0] == d.size - np.count_nonzero(d == d.max())
    if name == "tiny":
        assert n_rec == 301
    if name == "long":
        assert cases["4096-even"].size == 4096 == cases["4096-with-values"].size
        assert np.count_nonzero(np.isin(cases["4096-with-values"], d)) >= 100
        thr, at = lc.boundary_thresholds(d, offset)
        below, dips = lr.sweep(d, offset, thr)
        b2, d2 = lr.sweep_brute(d, offset, thr)
        assert np.array_equal(below, b2) and np.array_equal(dips, d2)
        for B in at:                                              # a run begins exactly at B under its threshold
            t = d[B - 1]
            assert d[B] < t and not d[B - 1] < t
        # the equal minima: a bin over the whole record names the first of them, bins of 64 each their own
        bmin, barg, _ = lr.bins(d, offset, 10 ** 7)
        assert barg.tolist() == [lc.EQUAL_AT[0] + 2]
        bmin, barg, _ = lr.bins(d, offset, 128)
        assert np.count_nonzero(bmin == d.min()) == 4 and barg[lc.EQUAL_AT[0] // 128] == lc.EQUAL_AT[0] + 2
    if name == "homo":
        bmin, barg, boff = lr.bins(d, offset, 64)
        b = np.arange(boff[1], boff[2])
        assert np.array_equal(barg[b], 64 * (b - boff[1]) + 2)


def _track(name, width):
    d, offset = lc.exact(name)
    bmin, barg, boff = lr.bins(d, offset, width)
    return [api.LandscapeTrack("rec%d" % c, bmin[boff[c]:boff[c + 1]], barg[boff[c]:boff[c + 1]], "+", width, lc.W, len(s))
            for c, s in enumerate(lc.genome(name))]


@pytest.mark.parametrize("name,width,n,sep", [("long", 64, 12, None), ("long", 1, 40, 10), ("edges", 2, 25, 3), ("homo", 64, 30, 64),
                                              ("tiny", 1, 1000, 1), ("long", 10 ** 7, 3, None)])
def test_best_loci_against_the_naive_restatement(name, width, n, sep):
    track = _track(name, width)
    got = api.best_loci(track, n, sep)
    want = lr.best_loci(track, n, lc.W if sep is None else sep)
    assert got == want and len(got) <= n
    if name == "long" and width == 64:
        assert [a - 2 for _, a, _ in got[:5]] == list(lc.EQUAL_AT)          # equal minima: in order of position
        assert len(got) == n
    assert api.best_loci(track, 0) == [] and api.best_loci([], 5) == []


def test_threshold_for_dips():
    sweep = api.ThresholdSweep(np.array([1.0, 2.0, 3.0, 4.0]), np.array([0, 5, 9, 30]), np.array([0, 3, 2, 7]))
    assert api.threshold_for_dips(sweep, 2) == 3.0 and api.threshold_for_dips(sweep, 0) == 1.0
    assert api.threshold_for_dips(sweep, 7) == 4.0
    assert api.threshold_for_dips((sweep[0], sweep[1], sweep[2] + 1), 0) is None


def test_write_bedgraph(tmp_path):
    plus = api.LandscapeTrack("chrA", np.array([3.5, 1.25, 9.0]), np.array([2, 7, 10]), "+", 4, 5, 14)      # 10 windows, 9 values
    minus = api.LandscapeTrack("chrA", np.array([3.5, 1.25, 9.0]), np.array([9, 4, 1]), "-", 4, 5, 14)
    path = os.path.join(tmp_path, "t.bedgraph")
    api.write_bedgraph([plus, minus], path)
    rows = [line.split("\t") for line in open(path).read().splitlines()]
    assert rows[:3] == [["chrA", "1", "5", "3.5"], ["chrA", "5", "9", "1.25"], ["chrA", "9", "10", "9.0"]]
    # reversed starts 2..5, 6..9, 10 are forward starts 9..6, 5..2, 1
    assert rows[3:] == [["chrA", "0", "1", "9.0"], ["chrA", "1", "5", "1.25"], ["chrA", "5", "9", "3.5"]]
    for t in (plus, minus):                                              # every argmin lies in its bin's line
        lines = rows[:3] if t.strand == "+" else rows[3:][::-1]
        for a, (_, lo, hi, _) in zip(t.bin_argmin, lines):
            assert int(lo) < a <= int(hi)

