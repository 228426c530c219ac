"""tests/short_cases.py builds what it says (no GPU): every case of test_gpu_short_windows.py exists, its plants sit on the lanes the
module docstring names, and the conditions that keep a case from being vacuous hold on oracle values -- they are asserted where the
case is built, so building it is the check."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import short_cases as sc

SINGLE = sorted({(k, N, nk) for _, k, N, nk in sc.single_cells()}, key=str)
STEP = [(k, N, nk) for k in sc.STEP_KS for N in sc.STEP_NS for nk in sc.STEP_NKS]
CHAIN = [(k, 7, nk) for k in sc.CHAIN_KS for nk in sc.CHAIN_NKS]


def test_matrix_covers_what_the_device_tests_promise():
    cells = sc.single_cells()
    assert set(sc.NKS_MANDATORY) <= set(sc.NKS) and max(sc.NKS_MANDATORY) == 65 and min(sc.NKS) == 2
    for form, ks in (("stream8", sc.STREAM8_KS), ("stream", sc.STREAM_KS), ("bitslice", sc.BITSLICE_KS), ("scan", sc.SCAN_DEFAULT_KS),
                     ("generic", sc.GENERIC_FORCED_KS), ("gen", sc.GENERIC_DEFAULT_KS)):
        for k in ks:
            have = {nk for f, kk, N, nk in cells if f == form and kk == k}
            assert set(sc.NKS_MANDATORY) <= have, (form, k)
    for form in ("stream8", "stream", "bitslice", "generic"):
        assert {nk for f, k, N, nk in cells if f == form and k == 6 and N == 7} == set(sc.NKS), form
    assert {(k, N) for f, k, N, nk in cells if f == "stream8"} == {(5, 7), (5, 300), (5, "int32"), (6, 7), (6, 300), (6, "int32"), (7, 7), (7, 300)}


@pytest.mark.parametrize("k,N,nk", sorted(set(SINGLE + STEP + CHAIN), key=str), ids=lambda v: str(v))
def test_single_cell(k, N, nk):
    c = sc.cell(k, N, nk)                                               # (asserts hit counts and the share below the dense threshold)
    ref, W, contigs, plants = c["ref"], c["W"], c["contigs"], c["plants"]
    assert W == nk + k - 1 and len(ref["base"]) == W and sc.LONG == len(contigs[0]) and 30_000 <= sc.LONG <= 40_000
    Smax = int(ref["S"].max())
    assert (Smax < 256) if N == 7 else (256 <= Smax <= 32767) if N == 300 else Smax > 32767
    # the long record's copies: two per phase, on that lane, the first exact
    ph = sc.phases(nk)
    assert set(ph) == {p for p in (0, 1, 63 - nk, 62, 63, 65) if p >= 0}
    long_plants = [s for r, s in plants if r == 0]
    assert [s % 64 for s in long_plants] == [p % 64 for p in ph for _ in (0, 1)]
    assert long_plants == sorted(long_plants) and min(np.diff(long_plants)) > W + 64
    for i, s in enumerate(long_plants):
        seq = contigs[0][s:s + W].upper()
        n_sub = sum(a != b for a, b in zip(seq, ref["base"]))
        assert n_sub == 0 if (i % 2 == 0 or nk < 15) else (1 <= n_sub if nk < 34 else True) and n_sub <= max(4, W // 5)
    assert contigs[0][long_plants[2]:long_plants[2] + W].islower()
    # the tandem run, the low-complexity runs
    n_rep = -(-(sc.TANDEM_WINDOWS + W) // W)
    assert contigs[0][sc.TANDEM_AT:sc.TANDEM_AT + n_rep * W] == ref["base"] * n_rep and (n_rep - 1) * W + 1 >= sc.TANDEM_WINDOWS
    D0 = c["D"][0]
    assert len(set(D0[sc.TANDEM_AT:sc.TANDEM_AT + sc.TANDEM_WINDOWS:W].tolist())) == 1     # every W-th window of the run is the base again
    assert D0[sc.TANDEM_AT] == D0[long_plants[0]]
    assert contigs[0][sc.A_AT:sc.A_AT + 300] == b"A" * 300 and contigs[0][sc.AC_AT:sc.AC_AT + 300] == b"AC" * 150
    assert contigs[0][sc.N_AT:sc.N_AT + 200] == b"N" * 100 + b"n" * 100
    # the short records
    assert [len(x) for x in contigs[1:9]] == [W - 1, W, W + 1, W + 62, W + 63, W + 64, W + 65, 2 * W]
    assert [(r, s) for r, s in plants if 0 < r < 9] == [(r, len(contigs[r]) - W) for r in range(2, 9)]
    assert len(contigs) == 9 + sc.MEDIUM and all(len(x) >= 100 + 2 * W for x in contigs[9:])
    # thresholds: the dense one between two values of D, the share it leaves below
    T = orc.int_threshold(c["thr"]["dense"], k, ref["N"])
    Dall = np.concatenate(c["D"])
    assert sc.DENSE_BAND[0] <= np.count_nonzero(Dall < T) / Dall.size <= sc.DENSE_BAND[1]
    assert c["n_hits"]["sparse"] >= sc.MIN_SPARSE_HITS and c["n_hits"]["dense"] >= sc.MIN_DENSE_HITS
    Ts = orc.int_threshold(c["thr"]["sparse"], k, ref["N"])
    assert all(c["D"][r][s] < Ts for r, s in plants)                    # every copy is below the sparse threshold


@pytest.mark.parametrize("nk", sc.NKS_MANDATORY)
def test_float_cell(nk):
    c = sc.float_cell(6, nk)
    assert not np.allclose(c["RV"] * 7, np.round(c["RV"] * 7))          # no S / N form
    assert c["n_hits"]["sparse"] >= sc.MIN_SPARSE_HITS and c["n_hits"]["dense"] >= sc.MIN_DENSE_HITS


@pytest.mark.parametrize("k,ws", sorted(set(sc.cluster_shapes())), ids=lambda v: str(v).replace(" ", ""))
def test_cluster_cell(k, ws):
    c = sc.cluster_cell(k, ws)                                          # (asserts >= 30 integer hits of two KFVs or more)
    maxws = max(ws)
    assert [len(x) for x in c["contigs"][1:5]] == [maxws + k - 2, maxws + k - 1, maxws + k, maxws + 64]
    assert 20_000 <= len(c["contigs"][0]) <= 40_000
    ph = sc.phases(min(ws) - k + 1)
    assert [s % 64 for r, s, _ in c["plants"] if r == 0] == [ph[i % len(ph)] % 64 for i in range(2 * len(ws))]
    assert all(sc.DENSE_BAND[0] <= s <= sc.DENSE_BAND[1] for s in c["shares"])
    assert len(c["ohi"]) >= sc.MIN_DENSE_HITS and len(c["ohits"]) >= sc.MIN_DENSE_HITS // 2
