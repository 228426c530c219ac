"""tests/range_cases.py builds what it says (no GPU): every cell of test_gpu_range.py lies on the intended side of its predicate, the
integer oracle equals a recomputation in Python integers at the magnitudes the cells reach, and the conditions that keep a cell from
being vacuous hold on oracle values -- they are asserted where the cell is built, so building it is part of the check.

Attained shares of the bounds (printed by test_attained_shares, copied into DESIGN.md):
  max D - min D over dmax            1.0000 in every cell but near_copies (>= 0.9969: the base itself is not at D = 0 there);
  E = dmax / 2N over 2^29            fits32 edge- cells: >= 0.99992 (1.000000 to six places at 20 k-mers per window);
  |D[q + 64] - D[q]| / 2N over 2^30  big_ok edge cells: 0.87 - 0.89 at 284 k-mers per window, 0.97 at 1000, copies and run_heavy alike.
"""
import numpy as np
import pytest

from tests import range_cases as rc

ALL_CELLS = sorted(set(rc.SINGLE_CELLS + rc.CHAIN_CELLS + [rc.FORCED_CELL]), key=str)


def test_matrix_covers_what_the_device_tests_promise():
    cells = set(rc.SINGLE_CELLS)
    for side in "-+":
        for k in (5, 6, 7):
            assert {("fits32", k, 289 - k + 1, "near_copies", side), ("fits32", k, 20, "copies", side)} <= cells
            assert {("big_ok", k, nk, fam, side) for nk in (284, 1000) for fam in ("copies", "run_heavy")} <= cells
        for k in (3, 4, 8, 10):
            assert ("fits32", k, 289 - k + 1, "copies", side) in cells
        for k in (5, 6):
            assert ("n22", k, 10, "copies", side) in cells
    assert any(c[0] == "d61" and c[4] == "-" for c in cells) and all(c[4] == "+" for c in rc.REFUSED_CELLS)
    assert {("fits32", 6, 284, "near_copies", "x3"), ("big_ok", 6, 284, "copies", "x3"), ("big_ok", 5, 1000, "run_heavy", "x3")} <= cells
    assert rc.FORCED_CELL in cells and set(rc.CHAIN_CELLS) <= cells
    assert {(c[0], c[1], c[4]) for c in rc.CHAIN_CELLS} == {("fits32", 6, "+"), ("fits32", 7, "+"), ("big_ok", 6, "-"), ("big_ok", 7, "-")}


def test_predicates_on_hand_made_tables():
    """The restated predicates at values worked out by hand (one entry S = N nk: dmax = 2 N^2 nk^2, dmax / 2N = N nk^2)."""
    S = lambda v: np.array([0, v, 0, 0], dtype=np.int64)
    assert rc.dmax(S(6), 3, 2) == 36 + 36
    assert rc.fits32(S(2 ** 27), 2 ** 27, 1) and not rc.fits32(S(2 ** 29), 2 ** 29, 1)          # N nk^2 = 2^27, 2^29
    assert rc.fits32(S(2 * (2 ** 27 - 1)), 2 ** 27 - 1, 2) and not rc.fits32(S(2 ** 28), 2 ** 27, 2)    # 4 N = 2^29 - 4, 2^29
    assert rc.big_ok(S(2 ** 23), 2 ** 21, 4) and not rc.big_ok(S(2 ** 23 + 1), 2 ** 21, 4)       # 64 (2^23 + 2^23) = 2^30
    assert rc.big_ok(S(1), 2 ** 22 - 1, 1) and not rc.big_ok(S(1), 2 ** 22, 1)
    assert rc.d61(S(2 ** 30), 2 ** 30 - 1, 1) and not rc.d61(S(2 ** 30), 2 ** 30, 1)


def test_edges_are_edges():
    for pred, k, nk, family, side in ALL_CELLS + rc.REFUSED_CELLS:
        W = nk + k - 1
        lo, hi = rc.edge_N(pred, k, W, family)
        p = rc.PREDICATES[pred]
        assert hi == lo + 1 and p(rc.table(family, k, W, lo), lo, nk) and not p(rc.table(family, k, W, hi), hi, nk)
    assert rc.edge_N("n22", 6, 15, "copies") == (2 ** 22 - 1, 2 ** 22)
    for k in (5, 6, 7):                                                 # the short window's edge is above a million references
        assert rc.edge_N("fits32", k, 20 + k - 1, "copies")[0] > 10 ** 6


@pytest.mark.parametrize("c", ALL_CELLS, ids=rc.cell_id)
def test_cell(c):
    pred, k, nk, family, side = c
    x = rc.cell(*c)                                                     # (asserts the span of D and, big_ok, the step-local prefix)
    ref, N, W, S, D, contigs = x["ref"], x["N"], x["W"], x["ref"]["S"], x["D"], x["contigs"]
    # the intended side of the cell's own predicate, and of the others where the cell is meant to move ONE thing
    assert rc.PREDICATES[pred](S, N, nk) == (side == "-")
    if pred == "n22":
        assert rc.fits32(S, N, nk)                                      # only stream8_applies changes between the two sides
    if pred == "big_ok":
        assert not rc.fits32(S, N, nk) and nk >= 100
    if pred == "fits32":
        assert N < 2 ** 22
    assert rc.d61(S, N, nk)
    # the table: S / N with n_refs = N, no entry on the genome's homopolymers, the family's width
    assert all(S[v] == 0 for v in rc.absent_kmers(k)) and S.min() >= 0 and np.array_equal(np.rint(ref["RV"] * N).astype(np.int64), S)
    if family == "near_copies":
        assert np.count_nonzero(S % N) >= 4
    if family == "run_heavy":
        assert int(S.max()) == N * (nk - 10) and S[0] == S.max()
    # the genome
    assert sum(len(s) for s in contigs) <= 40_000
    assert x["names"][:3] == ["A", "B", "C"] and [len(contigs[i]) for i, n in enumerate(x["names"]) if n == "D"] == [W - 1, W, W + 1]
    t = rc.touched(ref["base"])
    assert contigs[0].startswith(ref["base"] + b"C" * (W + 200) + t) and contigs[1] == b"C" * (W + 200) + t + b"G" * (W + 200) + t
    assert t != ref["base"] and t[1:] == ref["base"][1:] and not set(rc.kmer_values(t, k).tolist()) & set(rc.absent_kmers(k))
    if family == "copies":
        assert D[0][2 * W + 200] == D[1][W + 200] == D[1][-1] == 2 * N * N
    assert ("E" in x["names"]) == (family == "run_heavy")
    # magnitudes: every D below 2^61, distances comparable bit for bit
    Dall = np.concatenate(D)
    assert 0 <= int(Dall.min()) and int(Dall.max()) == x["dmax"] < 2 ** 61
    assert 2 * k * N * N < 2 ** 53
    assert D[1][0] == x["dmax"]                                         # record B starts inside the absent homopolymer
    if family != "near_copies":
        assert D[0][0] == 0
    # the oracle against Python integers at a dozen windows, the extreme ones among them
    rng = np.random.default_rng(nk + k)
    picks = [(0, 0), (1, 0), (0, int(np.argmax(D[0]))), (1, int(np.argmin(D[1]))), (2, x["plants"][0][1])]
    picks += [(len(contigs) - 1, 0)] if family == "run_heavy" else []
    picks += [(r, int(rng.integers(0, D[r].size))) for r in (0, 0, 0, 1, 1, 1, 2, 2)]
    for r, s in picks:
        assert int(D[r][s]) == rc.bigint_D(contigs[r][s:s + W], S, N, k), (r, s)
    # thresholds
    mid, above, low = x["thr"]
    scale = 2 * k * N * N
    assert all(D[r][s] < mid * scale for r, s, _ in x["plants"]) and D[0][-1] > mid * scale and above * scale > x["dmax"]
    # record F: from dmax down to its fragment's share and back, never under `low` (from 100 k-mers per window on)
    F = D[x["names"].index("F")]
    assert F[0] == F[-1] == x["dmax"] and x["names"].count("F") == 1
    if nk >= 100:
        assert rc.LOW_SHARE * x["dmax"] * 1.1 < F.min() < x["dmax"] / 3 * 0.96 and abs(low * scale / x["dmax"] - rc.LOW_SHARE) < 1e-9


@pytest.mark.parametrize("name", sorted(rc.CLUSTER_CELLS))
def test_cluster_cell(name):
    x = rc.cluster_cell(name)                                           # (asserts the span of every KFV's D)
    k, W, nk = x["k"], x["W"], x["W"] - x["k"] + 1
    sides = [(rc.fits32(S, N, nk), rc.big_ok(S, N, nk), int(S.max()) > 32767) for S, N in zip(x["S"], x["N"])]
    if name == "k6-84-fits32lo-fits32hi":
        assert x["N"][0] == 84 and [s[0] for s in sides] == [True, True, False]        # (each at the edge of its OWN base's table)
        assert not rc.fits32(rc.table("copies", k, W, x["N"][1] + 1, 2), x["N"][1] + 1, nk)
        assert rc.fits32(rc.table("copies", k, W, x["N"][2] - 1, 3), x["N"][2] - 1, nk)
    elif name == "k6-84-beyond-big_ok":
        assert x["N"][0] == 84 and sides[0][:2] == (True, True) and sides[1][:2] == (False, False)
        assert rc.big_ok(rc.table("copies", k, W, x["N"][1] - 1, 2), x["N"][1] - 1, nk)
    else:
        assert k == 7 and sides == [(True, True, True)] * 2
        assert all(not rc.fits32(rc.table("copies", k, W, N + 1, j + 1), N + 1, nk) for j, N in enumerate(x["N"]))
    assert sum(len(s) for s in x["contigs"]) <= 40_000
    assert all(2 * k * N * N < 2 ** 53 for N in x["N"])


def test_which_clauses_can_decide_alone():
    """fits32's second clause, N nk < 2^30, and big_ok's second, N < 2^22, next to the clause beside them: at the smallest N that
    fails the clause, for every window of 1 ... 65535 k-mers, does the other clause still hold for SOME table?  dmax and Smax grow
    with the table, so the most favourable table is the smallest: a single entry of 1.
      fits32: never.  N nk >= 2^30 gives dmax / 2N >= N nk^2 / 2 >= 2^29 nk: the clause is implied at every nk.
      big_ok: at nk = 1, 2, 3 only (2^22 nk + Smax <= 2^24 leaves room up to nk = 3), where N may reach 2^24 / nk: the clause is NOT
      implied there.  (Every user of big_ok also asks stream8_c16_applies, which repeats N < 2^22.)"""
    S = np.array([1], dtype=np.int64)
    alone32, alone_big = [], []
    for nk in range(1, 65536):
        N = -(-2 ** 30 // nk)
        assert N * nk >= 2 ** 30 > (N - 1) * nk
        if rc.dmax(S, N, nk) // (2 * N) < 2 ** 29:
            alone32.append(nk)
        N = 2 ** 22
        if 64 * (1 + N * nk) <= 2 ** 30:
            alone_big.append(nk)
    assert alone32 == [] and alone_big == [1, 2, 3]


def test_attained_shares():
    """The figures of the module docstring (printed: pytest -s)."""
    rows = []
    for c in ALL_CELLS:
        x = rc.cell(*c)
        rows.append((rc.cell_id(c), x["N"], x["span"] / x["dmax"], x["dmax"] // (2 * x["N"]) / 2 ** 29, x["step"] / 2 ** 30, x["kernel"]))
    for r in rows:
        print("%-40s N %9d  span/dmax %.6f  E/2^29 %.6f  step/2^30 %.4f  %s" % r)
    for (name, N, span, e, step, kern), c in zip(rows, ALL_CELLS):
        assert span >= rc.SPAN_SHARE
        if c[0] == "fits32" and c[4] == "-":
            assert 0.999 <= e < 1.0                                      # the prefix bound is attained, not merely approached
        if c[0] == "big_ok":
            assert 0.5 <= step <= (1.0 if c[4] != "x3" else 3.0)
