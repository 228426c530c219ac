"""Host side of the strobemer calibration calls (no GPU): the plain-Python model of tests/strobe_calib_ref.py on every case the
device tests use -- the kernel's position identity against sum (S - N c)^2, the single-sweep form against the per-start form and
against the scan oracle -- and that each case is not vacuous; the header declares the two entry points and the built library
exports them."""
import ctypes
import os
import re

import numpy as np
import pytest

from kmergma_amd import _lib, api
from tests import strobe_calib_cases as cc
from tests import strobe_calib_ref as scr
from tests import strobe_cases as sc
from tests import strobe_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sampled(L, W):
    v = list(scr.valid_starts(L, W))
    return sorted(set(v[:3] + v[-2:] + v[::97]))


def _naive_D(seq, ref, start):
    """The window's own W - k + 1 randstrobes, WITHOUT the permanent item: what the reference's count vector is not."""
    W, cfg = ref["W"], ref["cfg"]
    return scr.D_of_counts(ref["S"], ref["N"], so.strobe_count(seq[start - 1:start - 1 + W], *cfg))


@pytest.mark.parametrize("cfg,W", cc.parity_sets(), ids=lambda v: str(v))
def test_parity_cases(cfg, W):
    c = cc.parity_case(cfg, W)
    ref = c["ref"]
    S, N = ref["S"], ref["N"]
    differs = 0
    for seq in c["seqs"]:
        sweep = scr.all_window_D(seq, S, N, cfg, W)
        assert len(sweep) == len(scr.valid_starts(len(seq), W))
        for q in _sampled(len(seq), W):
            d = scr.window_D(seq, S, N, cfg, W, q)
            assert sweep[q - 1] == d
            assert scr.window_position_D(seq, S, N, cfg, W, q) == d            # the kernel's identity
            differs += q >= 2 and _naive_D(seq, ref, q) != d
    assert differs >= 3                                                           # the permanent item shows in D
    # the scan oracle's first window and step distances are the same numbers
    o = sc.oracle(c["seqs"], ref, 0.0)
    per = sc.split_dists(c["seqs"], W, o["dists_exact"])
    for r, seq in enumerate(c["seqs"]):
        sweep = scr.all_window_D(seq, S, N, cfg, W)
        assert sweep[0] == o["first_D"][r] and sweep[1:] == per[r].tolist()
    assert [len(p) for p in per] == [1300 - W - 1, 0, 0]


def test_sweep_equals_window_D_at_every_start():
    """The single sweep against window_counts_direct at EVERY start of one parity case (the others: sampled starts, above)."""
    cfg, W = cc.DEFAULT_SETS[1]
    c = cc.parity_case(cfg, W)
    S, N = c["ref"]["S"], c["ref"]["N"]
    for seq in c["seqs"]:
        assert scr.all_window_D(seq, S, N, cfg, W) == [scr.window_D(seq, S, N, cfg, W, q) for q in scr.valid_starts(len(seq), W)]


@pytest.mark.parametrize("n_items", cc.STRIDE_ITEMS)
def test_stride_cases(n_items):
    c = cc.stride_case(n_items)
    ref, W, cfg = c["ref"], c["W"], c["cfg"]
    assert W - sc.k_of(cfg) + 1 == n_items
    L = len(c["seqs"][0])
    assert c["start"][:3] == [1, 2, L - W] and list(scr.valid_starts(W + 1, W)) == [1]
    for ci, q in zip(c["contig"], c["start"]):
        seq = c["seqs"][ci]
        d = scr.window_D(seq, ref["S"], ref["N"], cfg, W, q)
        assert scr.window_position_D(seq, ref["S"], ref["N"], cfg, W, q) == d
        assert len(scr.item_positions(len(seq), cfg, W, q)) == n_items
        if q >= 2:
            assert _naive_D(seq, ref, q) != d


def test_onebin_case():
    c = cc.onebin_case()
    ref, W, cfg = c["ref"], c["W"], c["cfg"]
    seq = c["seqs"][0]
    bins = so.strobe_bins(seq, *cfg)
    n = cc.ONEBIN_ITEMS
    for q in c["start"]:
        pos = scr.item_positions(len(seq), cfg, W, q)
        assert len(pos) == n and {int(bins[p]) for p in pos} == {0}              # every item in one bin
        d = scr.window_position_D(seq, ref["S"], ref["N"], cfg, W, q)
        assert d == sum(int(x) ** 2 for x in ref["S"]) - 31 * 31 + (31 - ref["N"] * n) ** 2
    assert 2 ** 31 < n * n < 2 ** 32 and sc.rc.d61(ref["S"], ref["N"], n)
    assert scr.window_D(seq, ref["S"], ref["N"], cfg, W, 2) == d


def test_range_cases_are_what_the_device_test_reads():
    """strobe_cases.top_cell at the largest N and entry_cell: the oracle's D per window start, as test_gpu_strobe_calib indexes it."""
    cfg = cc.STRIDE_CFG
    c = sc.top_cell(cfg, sc.top_edge_N(cfg)[0])
    seq = c["seqs"][0]
    L, W = len(seq), c["W"]
    assert c["D"].size == L - W - 1 and c["first_D"][0] == c["dmax"] > 0.999 * 2 ** 61
    for q in (2, c["at"] + 1, L - W):
        assert scr.window_position_D(seq, c["ref"]["S"], c["ref"]["N"], cfg, W, q) == int(c["D"][q - 2])
    e = sc.entry_cell()
    for r, seq in enumerate(e["seqs"]):
        if len(seq) >= e["W"]:
            sweep = scr.all_window_D(seq, e["ref"]["S"], 1, e["cfg"], e["W"])
            assert sweep[0] == e["first_D"][r]
    assert e["dmax"] in (scr.all_window_D(e["seqs"][0], e["ref"]["S"], 1, e["cfg"], e["W"]) + [e["dmax"]])


def test_list_case():
    c = cc.list_case()
    ref, W, cfg = c["ref"], c["W"], c["cfg"]
    for seq in c["seqs"]:
        sweep = scr.all_window_D(seq, ref["S"], ref["N"], cfg, W)
        for q in _sampled(len(seq), W):
            assert sweep[q - 1] == scr.window_D(seq, ref["S"], ref["N"], cfg, W, q) == scr.window_position_D(seq, ref["S"], ref["N"], cfg, W, q)
    # the permanent item is the window's own record's: another record's gives another D
    a, b = c["seqs"][1], c["seqs"][2]
    q = 100
    swapped = b[:W] + a[W:]
    assert so.strobe_bins(a, *cfg)[W - 6] != so.strobe_bins(swapped, *cfg)[W - 6]
    assert scr.window_D(a, ref["S"], ref["N"], cfg, W, q) != scr.window_D(swapped, ref["S"], ref["N"], cfg, W, q)


def test_bad_case():
    c = cc.bad_case()
    W, cfg = c["W"], c["cfg"]
    k = sc.k_of(cfg)
    assert W - k == cc.BAD_POS and c["seqs"][1][cc.BAD_POS:cc.BAD_POS + 1] == b"X"
    L = len(c["seqs"][1])
    for q in (42, 100, L - W):
        assert not (q - 1 <= cc.BAD_POS <= q + W - 2)                              # outside residues q .. q + W - 1 ...
        assert cc.BAD_POS in scr.residues_read(L, cfg, W, q)                       # ... and read by the permanent item
    for q in (1, 2, 41):
        assert cc.BAD_POS in scr.residues_read(L, cfg, W, q) and q - 1 <= cc.BAD_POS <= q + W - 2
    for q in (60, 154, 202, 254):                                                 # record 3: the X at residue 200 is never read
        assert 200 not in scr.residues_read(300, cfg, W, q)
    assert len(c["seqs"][2]) < W
    with pytest.raises(so.BadBase):
        scr.window_D(c["seqs"][1], c["ref"]["S"], c["ref"]["N"], cfg, W, 1)


@pytest.mark.parametrize("cfg", cc.MUT_SETS, ids=lambda v: str(v))
def test_mutation_cases(cfg):
    c = cc.mutation_case(cfg)
    ref = c["ref"]
    k = sc.k_of(cfg)
    S, N = ref["S"], ref["N"]
    seen = set()
    for i, seq in enumerate(c["seqs"]):
        for r, rate in enumerate(cc.MUT_RATES):
            for t in range(cc.MUT_TRIALS):
                d = scr.mutation_D(seq, S, N, cfg, rate, cc.MUT_SEED, (i, r, t))
                m = api.mutate_seq(seq, rate, seed=cc.MUT_SEED, stream=(i, r, t))
                assert scr.position_D(so.strobe_bins(m, *cfg), S, N) == d
                seen.add((i, r, d))
                if rate == 0.0:
                    assert d == scr.D_of_counts(S, N, so.strobe_count(seq, *cfg))
    assert len(seen) >= 2 * (1 + 2 + 3 + 3) - 2                                      # the trials differ (rate 0 excepted)
    sumS2 = sum(int(x) ** 2 for x in S)
    assert [len(x) - k + 1 for x in c["short"]] == [0, 1, 2]
    assert scr.mutation_D(c["short"][0], S, N, cfg, 0.5, 1, (0, 0, 0)) == sumS2
    assert scr.mutation_D(c["short"][1], S, N, cfg, 0.5, 1, (0, 0, 0)) != sumS2


def test_window_sampling_for_the_strobemer_scan():
    """sample_window_starts(lens, W + 1, ...): exactly the scan's tested starts 1 .. L - W of records longer than W."""
    W = 50
    lens = [49, 50, 51, 60]
    c, s = api.sample_window_starts(lens, W + 1, 1000, 1)
    assert list(zip(c.tolist(), s.tolist())) == [(2, 1)] + [(3, q) for q in range(1, 11)]
    for ci, q in zip(c.tolist(), s.tolist()):
        assert q in scr.valid_starts(lens[ci], W)


def test_symbols_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "kgma.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("kgma_strobe_window_dists", "kgma_strobe_mutation_dists"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    for name in ("strobe_window_dists", "estimate_strobe_threshold_from_genome", "strobe_mutation_dists", "test_strobe_2_mer_dists"):
        assert callable(getattr(api, name))
    assert callable(_lib.Context.strobe_window_dists) and callable(_lib.Context.strobe_mutation_dists)
