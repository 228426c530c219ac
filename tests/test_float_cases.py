"""tests/float_cases.py and tests/float_exact.py on the host: the exact reference agrees with an independent one, the C oracle's
running value -- the reference the device is modelled on -- stays inside the a-priori bound at every window of every case, the
bound is tight enough that a wrong table entry, a float32 table or a wrong residue code shows, and every case holds what it is
there for (tests/test_gpu_float_range.py runs them on the device).  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

from tests import calib_ref as cr
from tests import float_cases as fc
from tests import float_exact as fx

TWO61 = Fraction(2) ** 61


class _Table:
    """A KFV of either form as calib_ref.float_dist reads it: ref[x]."""
    def __init__(self, c):
        self.v = fc.dense_of(c)

    def __getitem__(self, x):
        return self.v.get(x, 0.0)


def _max_ratio(c, values):
    """max |value - exact| / bound over every window (values: per record)."""
    worst = Fraction(0)
    for r, v in zip(fc.reference(c), values):
        assert len(v) == len(r.exact)
        for e, b, x in zip(r.exact, r.bound, np.asarray(v).tolist()):
            worst = max(worst, abs(Fraction(x) - e) / b)
    return worst


@pytest.mark.parametrize("name", fc.SCAN_NAMES)
def test_exact_reference_against_an_independent_one(name):
    """20 windows per case: the incremental exact distance equals calib_ref.float_dist (from the window's counts alone, another
    author's code) and float_exact.window, as rationals."""
    c = fc.case(name)
    k, W = c["k"], c["W"]
    rng = np.random.default_rng([fc.SEED + 2, fc.NAMES.index(name)])
    tab = _Table(c)
    sum_r2 = cr.sum_ref2(tab.v.values())
    ref = fc.reference(c)
    R = fx.entries(c["kfv"])
    picks = [(0, 0), (0, c["exact_at"]), (0, len(ref[0].exact) - 1), (1, 400), (1, 1450), (3, 0)]
    while len(picks) < 20:
        rec = int(rng.integers(0, 3))
        picks.append((rec, int(rng.integers(0, len(ref[rec].exact)))))
    for rec, q in picks:
        seq = c["records"][rec]
        assert ref[rec].exact[q] == cr.float_dist(seq[q:q + W], tab, k, sum_r2), (rec, q)
        assert ref[rec].exact[q] == fx.window(seq, c["kfv"], k, W, q, R=R, sum_r2=sum_r2), (rec, q)


@pytest.mark.parametrize("name", fc.SCAN_NAMES)
def test_oracle_within_the_bound(name):
    """The reference's left-to-right first window and serial chain, at every window: |value - exact| <= bound."""
    c = fc.case(name)
    worst = _max_ratio(c, fc.oracle_chain(c))
    drift = fc.oracle_drift(c, fc.thr_mid(c))         # (what decides, in the GPU module, whether a chain-mode scan may be repeated)
    print(f"{name}: oracle worst err/bound {float(worst):.3g}, drift {float(drift):.3g} ({'below' if drift < Fraction(1, 2 ** 32) else 'above'} 2^-32)")
    assert worst <= 1


def _swapped(c):
    """The KFV with the largest and the smallest value among the k-mers of record 0 exchanged."""
    tab = fc.dense_of(c)
    occ = sorted(set(fx.kmers(c["records"][0], c["k"])))
    hi = max(occ, key=lambda x: tab.get(x, 0.0))
    lo = min(occ, key=lambda x: tab.get(x, 0.0))
    assert tab.get(hi, 0.0) != tab.get(lo, 0.0)
    tab[hi], tab[lo] = tab.get(lo, 0.0), tab.get(hi, 0.0)
    keys = sorted(tab)
    return keys, [tab[x] for x in keys]


# A near-count table is integers plus noise and its float32 form is those integers (the noise survives only on zero counts), so
# rounding it to float32 moves a distance by about (1 / k) sum |counts - window| x noise, while the bound grows with the table's
# size.  At noise 1e-9 that still exceeds 100 x bound up to k = 6 and at k = 11 (a sparse table); it cannot with 4^7 or 4^8 entries
# in the bound's first term, nor at noise 1e-12.  Those cells are listed, and held to falling short: a cell leaves the list only
# by reaching 100.
FLOAT32_OUT_OF_REACH = {"nearcount-k7-w120", "nearcount-k8-w300", "nearcount-k8-w300-global", "nearcount12-k3-w50", "nearcount12-k6-w305"}


def _max_move(c, rec, other):
    """max |exact - other's exact| / bound over the windows of record `rec`."""
    r = fc.reference(c)[rec]
    return max(abs(a - b) / bd for a, b, bd in zip(r.exact, other.exact, r.bound))


@pytest.mark.parametrize("name", fc.SCAN_NAMES)
def test_bound_notices_wrong_inputs(name):
    """The exact distance of some window moves by more than 100 x bound when the table is rounded to float32, when two k-mers of
    the record exchange their entries, and when N reads as A instead of T: an implementation that did any of it is outside the
    bound by two orders.  (The float32 table at the cells of FLOAT32_OUT_OF_REACH: asserted to stay below 100.)"""
    c = fc.case(name)
    k, W = c["k"], c["W"]
    tab = fc.dense_of(c)
    keys = sorted(tab)
    f32 = [float(np.float32(tab[x])) for x in keys]
    moved = _max_move(c, 0, fx.scan(c["records"][0], (keys, f32), k, W))
    print(f"{name}: float32 table moves a distance by {float(moved):.3g} x bound")
    if name in FLOAT32_OUT_OF_REACH:
        assert c["kind"] in fc.NOISE and 0 < moved < 100, float(moved)
    else:
        assert moved > 100, float(moved)
    assert _max_move(c, 0, fx.scan(c["records"][0], _swapped(c), k, W)) > 100, "two entries exchanged"
    assert b"N" in c["records"][1]
    assert _max_move(c, 1, fx.scan(c["records"][1], c["kfv"], k, W, n_as=0)) > 100, "N read as A"


@pytest.mark.parametrize("name", fc.SCAN_NAMES)
def test_case_properties(name):
    c = fc.case(name)
    ref = fc.reference(c)
    nk = c["nk"]
    assert [len(r.exact) for r in ref] == [max(len(s) - c["W"] + 1, 0) for s in c["records"]]
    assert len(ref[0].exact) >= 2050 and len(ref[3].exact) == 1
    # the poly-A plateau: pairs = n (n - 1) / 2 and no increment
    assert any(i == 0 for i in ref[1].inc[450:500])
    sum_r2 = sum((r * r for r in fx.entries(c["kfv"]).values()), Fraction(0))
    a_tab = fx.entries(c["kfv"]).get(0, Fraction(0))
    assert ref[1].A[450] == sum_r2 + 2 * nk * abs(a_tab) + nk + nk * (nk - 1)
    # the planted copies: the mutated one is the record's second-best dip where the table knows the base
    if c["kind"] in fc.NOISE:
        q = c["exact_at"]
        assert ref[0].exact[q] < ref[0].bound[q], "the sign of the computed value must be undetermined at the exact copy"
        assert ref[0].exact[q] == min(ref[0].exact)
        assert min(ref[0].exact[c["mut_at"] - 5:c["mut_at"] + 6]) < sorted(ref[0].exact)[len(ref[0].exact) // 20]
    if c["kind"] in ("absorb", "limit"):
        small = big = 0
        for r in ref:
            for e, i in zip(r.exact, r.inc):
                if i != 0:
                    if abs(i) < fx.ulp(e) / 2:
                        small += 1
                    else:
                        big += 1
        assert small > 1000 and big >= 6, (small, big)
    if c["kind"] == "signed":
        # increments of both signs above 1 % of the distance: the chain's value changes binade every few dozen steps.  A table
        # with entries in [-3, 3] on all 4^k k-mers keeps every distance near sum ref^2 / 2k = 3 x 4^k / 2k while an increment
        # stays below (8 + counts) / k, so from k = 6 on no window can have one (asserted, so that the reason stays true); the
        # k = 1, 3 and 11 tables (4, 64 and ~500 entries) do, and so do the nearcount cases at every k around their copies.
        up = sum(1 for r in ref for e, i in zip(r.exact, r.inc) if i > e / 100)
        down = sum(1 for r in ref for e, i in zip(r.exact, r.inc) if -i > e / 100)
        if c["k"] in (1, 3, 11):
            assert up >= 10 and down >= 10, (up, down)
        else:
            assert sum_r2 > 3200
    if c["kind"] == "nearcount":
        q = c["exact_at"]
        assert ref[0].inc[q] < -10 * ref[0].exact[q] and ref[0].inc[q + 1] > 10 * ref[0].exact[q]   # increments far above the distance
    if c["kind"] == "wide":
        v = c["kfv"]
        assert np.count_nonzero(np.signbit(v) & (v == 0.0)) == 3 and np.count_nonzero(v == 0.0) == 7
        assert np.count_nonzero((v != 0.0) & (np.abs(v) < 2.3e-308)) == 2
        assert np.abs(v).max() > 1e3 and np.abs(v[v != 0.0]).min() < 1e-300
    if c["kind"] in fc.NOISE:
        assert ref[4].exact[0] < ref[4].bound[0]          # (record 4 begins with the exact copy)
    # thr_mid lies between the mutated copy's minimum and the median window (a near-count table: the copy below the bulk)
    near = min(ref[0].exact[c["mut_at"] - c["W"] // 2:c["mut_at"] + c["W"] // 2 + 1])
    every = sorted(x for r in ref for x in r.exact)
    median = every[len(every) // 2]
    t = Fraction(fc.thr_mid(c))
    lo, hi = min(near, median), max(near, median)
    assert abs(t - (lo + hi) / 2) <= fx.ulp(hi) / 2       # (the Float64 nearest their midpoint)
    if hi - lo > 4 * fx.ulp(hi):                          # (absorb / limit at k = 6: the two lie within an ulp of each other)
        assert lo < t < hi
    if c["kind"] in fc.NOISE:
        assert near < t < median


@pytest.mark.parametrize("name", [n for n in fc.NAMES if n.startswith(("limit-", "over-"))])
def test_limit_arithmetic(name):
    """The magnitude kgma_set_refs tests, in exact arithmetic: within 1 % of 2^61 on the case's side; the accepted case's lattice is
    2k (no power of four keeps the largest D below 2^61)."""
    c = fc.case(name)
    s = fc.limit_sum(c["kfv"], c["nk"])
    if c["kind"] == "limit":
        assert TWO61 * 99 / 100 < s < TWO61
        assert s * 4 >= TWO61
    else:
        assert TWO61 < s < TWO61 * 101 / 100
        assert c["refused"]
    big = fc.large_keys(c["k"], c["W"])
    occ = set(x for seq in c["records"] for x in fx.kmers(seq, c["k"]))
    assert len(set(big)) == 3 and set(big) <= occ


def test_names_and_cells():
    assert [c["name"] for c in fc.cases()] == fc.NAMES and len(set(fc.NAMES)) == len(fc.NAMES)
    for tag in ("k3-w50", "k6-w305"):
        assert {c["kind"] for c in fc.cases() if c["cell"] == tag} == set(fc.ALL_KINDS)
    assert {c["cmode"] for c in fc.cases()} == {0, 1, 2, 3, 4, 5}
    assert any(c["nk"] < 64 and c["k"] == 6 for c in fc.cases())
