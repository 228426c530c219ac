"""The fixtures of tests/strobe_cases.py, without a GPU and without the library: what keeps each case of test_gpu_strobe_edges.py from
being vacuous is asserted here, on oracle values alone."""
import time

import numpy as np
import pytest

from kmergma_amd import refprep
from tests import range_cases as rc
from tests import strobe_cases as sc
from tests import strobe_oracle as so


# ---- 1. the discriminating table --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", [1, 2, 3])
def test_discriminating_table(s):
    S = sc.disc_table(s)
    x = np.arange(4 ** (2 * s))
    assert S.size == 4 ** (2 * s) and int(S.min()) >= 1 and int(S.max()) <= 997
    assert np.all(S != S[x ^ 1])                                          # the two counters of a dword
    assert np.all((S != S[x >> (2 * s)]) | (x == x >> (2 * s)))           # the bin of the first strobe alone
    ref = sc.ref_of(S, sc.DISC_N, (s, 1, 1, 1), 10)
    assert ref["N"] == 7 and sc.takes_integer_form(ref)
    assert np.array_equal(np.rint(ref["RV"] * 7.0).astype(np.int64), S)


def test_offsets_of_the_oracle():
    """strobe_bins_offsets against the per-position definition."""
    rng = np.random.default_rng(5)
    seq = bytes(rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=300, p=[.24, .24, .24, .24, .04]))
    for cfg in ((2, 3, 5, 5), (3, 1, 14, 33), (1, 1, 16, 2)):
        s, w_min, w_max, q = cfg
        k = sc.k_of(cfg)
        bins, off = so.strobe_bins_offsets(seq, *cfg)
        assert np.array_equal(bins, so.strobe_bins(seq, *cfg))
        val = lambda a: refprep.as_UInt(seq[a:a + s])
        for i in range(len(seq) - k + 1):
            ind = w_min
            for o in range(w_min, w_max + 1):                             # Strobemers.jl:52-60 with min_score 0 and `<=`
                if (val(i) + val(i + o - 1)) % q <= 0:
                    ind = o
            assert off[i] == ind and bins[i] == val(i) * 4 ** s + val(i + ind - 1)


# ---- 2. randstrobe selection ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg,sums,seed", sc.SELECT_SETS, ids=lambda v: str(v))
def test_selection_sets_are_not_vacuous(cfg, sums, seed):
    s, w_min, w_max, q = cfg
    assert seed == sc.first_select_seed(cfg, sums)                        # the recorded seed is the first that serves
    c = sc.select_cell(cfg)
    seqs = c["seqs"]
    assert 6500 <= sum(len(x) for x in seqs) <= 7500 and len(seqs) == 4
    text = b"".join(seqs)
    assert b"N" * 60 in text and any(ch in text for ch in b"acgt") and all(bytes([r]) * (sc.k_of(cfg) + 1) in text for r in b"ACGT")
    facts = sc.select_facts(cfg, seqs)
    if w_min < w_max:
        assert len(facts["offsets"]) >= 3 and {w_min, w_max} <= facts["offsets"], facts["offsets"]
    else:
        assert facts["offsets"] == {w_min}
    assert set(sums) <= facts["sums"], (sums, sorted(facts["sums"]))
    if s == 3:
        assert {x >> 5 for x in sums} <= {x >> 5 for x in facts["sums"]}  # the `zero` words the set is listed for
    if cfg == (3, 1, 14, 33):
        assert 1 in facts["offsets"] and {x >> 5 for x in facts["sums"]} == {0, 1, 2, 3}
    if cfg == (3, 4, 7, 97):
        assert facts["sums"] == {0, 97}
    if cfg in ((3, 4, 7, 2 ** 40), (2, 3, 5, 31)):
        assert facts["sums"] == {0}
    # the three restatements of the bin agree
    for seq in seqs:
        a = so.strobe_bins(seq, *cfg)
        assert a.tolist() == refprep.strobe_indices(seq, *cfg).tolist()
    seq, k = seqs[0][650:800] + seqs[0][1690:1740], sc.k_of(cfg)
    per = [refprep.as_UInt(refprep.get_strobe_2_mer(seq[i:i + k], *cfg, withGap=False)) for i in range(len(seq) - k + 1)]
    assert so.strobe_bins(seq, *cfg).tolist() == per
    # the scan's fixture: the discriminating table, no hit at threshold 0, every record scanned
    assert sc.takes_integer_form(c["ref"]) and c["n_hits"] == 0 and min(c["first_D"]) > 0
    assert c["D"].size == sum(len(x) - c["ref"]["W"] - 1 for x in seqs) and int(c["D"].min()) > 0


# ---- 3. short windows -------------------------------------------------------------------------------------------------------------------

def test_short_cells_cover_the_issue():
    cells = sc.short_cells()
    assert len(cells) == len(set(cells)) == 3 * 15 + 4
    assert {nk for _, nk in cells} == {1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65, 66, 127, 128, 129}


@pytest.mark.parametrize("cfg,nk", sc.short_cells(), ids=lambda v: str(v))
def test_short_cell_is_not_vacuous(cfg, nk):
    c = sc.short_cell(cfg, nk)
    k, W, seqs = sc.k_of(cfg), c["W"], c["seqs"]
    assert W == nk + k and sc.takes_integer_form(c["ref"])
    assert {len(x) for x in seqs} >= {W - 1, W, W + 1, W + 2, k} and sum(len(x) for x in seqs) < 8000
    for name in ("sparse", "dense"):
        o = c["oracle"][name]
        assert len(o["exact"]) >= 2, name
        assert sum(1 for d in o["first_D"] if d == -1) >= 1
        assert sc.band_free(np.concatenate(c["per"]), c["thr"][name], c["ref"])
    assert c["in_step"] and sc.enters_and_leaves_in_step(so.strobe_bins(seqs[c["long"]], *cfg), nk)
    # D = 0 is reached: in the long record, whose permanent item is the base's (elsewhere only where a record's happens to be the same bin)
    assert int(c["per"][c["long"]].min()) == 0 and c["oracle"]["sparse"]["first_D"][c["long"]] > 0
    # the dense threshold is AT a window's distance: not below it in exact arithmetic
    T = sc.int_T(c["thr"]["dense"], c["ref"])
    assert T == c["dense_D"] and c["at_threshold"] >= 1 and not any(h["D"] >= T for h in c["oracle"]["dense"]["exact"])


def test_every_bin_touched_twice_in_a_step_is_seen():
    """strobe_kernel's correction rounds start from the lanes whose atomic returned another count than the one read at the start of
    the step, and then correct EVERY lane of that lane's bin.  Emulated here on the steps of the short cells (all entering atomics of a
    step, then all leaving ones, each in any serial order): a bin that two or more lanes touch always has such a lane -- only one
    adder can see the start count, and a leaving lane sees it only behind as many leavers as there were adders, so the first leaver
    does not when there is an adder and the second does not when there is none.  So the `nk < 64` clause that sends every acting
    lane into the rounds changes no result: replacing it by `false` is an equivalent mutant (no GPU test can fail on it)."""
    rng = np.random.default_rng(64)
    steps = touched_twice = 0
    for cfg, nk in (((1, 2, 4, 5), 1), ((1, 2, 4, 5), 3), ((2, 3, 5, 5), 2), ((2, 3, 5, 5), 17), ((3, 4, 7, 5), 33), ((1, 1, 16, 2), 63), ((1, 2, 4, 5), 65)):
        c = sc.short_cell(cfg, nk)
        bins = so.strobe_bins(c["seqs"][c["long"]], *cfg).tolist()
        count = {}
        for b0 in range(0, len(bins) - 63, 64):
            adds = [(p, bins[p]) for p in range(b0, b0 + 64) if p < nk or bins[p] != bins[p - nk]]
            subs = [(p, bins[p - nk]) for p in range(b0, b0 + 64) if p >= nk and bins[p] != bins[p - nk]]
            start, live, pending = dict(count), dict(count), set()
            for i in rng.permutation(len(adds)):
                p, x = adds[i]
                if live.get(x, 0) != start.get(x, 0):
                    pending.add(x)
                live[x] = live.get(x, 0) + 1
            for i in rng.permutation(len(subs)):
                p, x = subs[i]
                if live.get(x, 0) != start.get(x, 0):
                    pending.add(x)
                live[x] = live.get(x, 0) - 1
            ops = [x for _, x in adds] + [x for _, x in subs]
            twice = {x for x in ops if ops.count(x) >= 2}
            assert twice <= pending, (cfg, nk, b0)
            assert min(live.values()) >= 0
            count, steps, touched_twice = live, steps + 1, touched_twice + len(twice)
    assert steps > 200 and touched_twice > 200


# ---- 4. streams that are not a record's first -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nk", sc.STREAMS_NKS)
def test_streams_cell_straddles_every_boundary(nk):
    c = sc.streams_cell(nk)
    P, D, T = c["P"], c["per"][0], c["T"]
    assert D.size + 1 >= 6300 and (D.size + 1 + P - 1) // P >= 3 + 1      # windows; streams of P
    for t in (1, 2, 3):
        d = c["straddle"][t]
        assert d["start"] <= t * P < t * P + 1 <= d["end"]
        assert all(int(D[w - 2]) < T for w in range(d["start"], d["end"] + 1))
        assert int(D[d["start"] - 3]) >= T and int(D[d["end"] - 1]) >= T   # the run's neighbours
    tie = c["straddle"][2]
    assert int(D[2 * P - 2]) == int(D[2 * P + 1 - 2]) == tie["D_min"] == int(D[tie["start"] - 2:tie["end"] - 1].min())
    assert (tie["argmin"], tie["last_min"], tie["nmin"]) == (2 * P, 2 * P + 1, 2) and tie["tie"]
    assert len(c["oracle"]["exact"]) >= 3 and c["band_free"]
    assert {h["cmi"] for h in c["oracle"]["exact"]} >= {2 * P}             # the hit of the tie: the first of the tied windows


# ---- 5. the top of the 16-bit counters --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", sc.TOP_CFGS, ids=lambda v: str(v))
def test_top_cell_fills_the_low_half_word(cfg):
    t0 = time.perf_counter()
    c = sc.top_cell(cfg)
    S, N, n = c["ref"]["S"], c["N"], sc.TOP_N_ITEMS
    assert c["W"] - sc.k_of(cfg) + 1 == n == 65_535
    assert S[0] == 0 and S[1] == 3 * N and sc.takes_integer_form(c["ref"])
    dmax = sum(int(x) ** 2 for x in S) + N * N * n * n
    assert c["first_D"] == [dmax] and c["dmax"] == dmax
    assert c["bin0_at_bin1"] >= n - 64
    assert 0 <= int(c["D"].min()) and int(c["D"].max()) == dmax
    assert len(c["oracle"]["exact"]) >= 1 and any(abs(h["cmi"] - (c["at"] + 1)) <= 16 for h in c["oracle"]["exact"])
    assert c["band_free"]
    t1 = time.perf_counter()
    sc.oracle(c["seqs"], c["ref"], c["thr"])
    assert time.perf_counter() - t1 < 1.0 and time.perf_counter() - t0 < 30.0


# ---- 6. the ends of the integer range ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", sc.TOP_CFGS, ids=lambda v: str(v))
def test_largest_N(cfg):
    lo, hi = sc.top_edge_N(cfg)
    assert hi == lo + 1 and 20_000 < lo < 25_000
    assert sc.top_dmax(cfg, lo) < 2 ** 61 <= sc.top_dmax(cfg, hi)
    assert sc.top_dmax(cfg, lo) > 0.999 * 2 ** 61
    c = sc.top_cell(cfg, lo)
    S = c["ref"]["S"]
    assert sc.takes_integer_form(c["ref"]) and int(S.max()) < 2 ** 31
    assert c["dmax"] == sc.top_dmax(cfg, lo) == sum(int(x) ** 2 for x in S) + lo * lo * 65_535 ** 2
    assert c["first_D"] == [c["dmax"]]
    assert 0 <= int(c["D"].min()) and int(c["D"].max()) == c["dmax"]        # D never leaves [0, dmax]
    assert len(c["oracle"]["exact"]) >= 1 and c["band_free"]
    assert sc.takes_integer_form(sc.ref_of(sc._top_genome(cfg)["shape"] * np.int64(hi), hi, cfg, c["W"]))   # edge+ is refused for its range alone


def test_largest_entry():
    c = sc.entry_cell()
    lo, hi = c["S_lo"], c["S_hi"]
    assert hi == lo + 1 and lo * lo + 4 < 2 ** 61 <= hi * hi + 4 and lo < 2 ** 31 and 1.5e9 < lo < 1.52e9
    assert rc.d61(c["ref"]["S"], 1, 2) and sc.takes_integer_form(c["ref"]) and c["W"] - sc.k_of(c["cfg"]) + 1 == 2
    assert 0 <= int(c["D"].min()) and int(c["D"].max()) <= c["dmax"] and max(c["first_D"]) <= c["dmax"]
    assert {c["one"], c["two"]} <= set(c["D"].tolist()) and int(c["D"].max()) >= lo * lo + 2
    T = sc.int_T(c["thr"], c["ref"])
    assert c["two"] < T <= c["one"] and len(c["oracle"]["exact"]) >= 1
    assert all(h["D"] == c["two"] for h in c["oracle"]["exact"])
