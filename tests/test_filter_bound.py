"""The distance bound behind the scan's prefilter (kgma_filter.hip), on the CPU: a numpy restatement of the filter (granule sums,
U) against the exact D of the integer oracle.  Every window at or below the threshold band must lie in a candidate granule."""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import filter_ref
from tests.helpers import kmer_values, mutate, random_dna

K, W = 6, 289


@pytest.fixture(scope="module")
def genes(data_dir):
    from kmergma_amd import fasta
    return [r.sequence.upper() for r in fasta.read_fasta(os.path.join(data_dir, "Alp_V_ref.fasta"))]


@pytest.fixture(scope="module")
def records(genes):
    """iid sequence with planted mutated fixture genes; an N run with a gene behind it; a tandem repeat of a gene."""
    rng = np.random.default_rng(6021)
    a = bytearray(random_dna(rng, 40_000))
    for i, pos in enumerate(range(1_500, 38_000, 3_100)):
        g = mutate(rng, genes[(7 * i) % len(genes)], 0.012 * i)
        a[pos:pos + len(g)] = g
    b = bytearray(random_dna(rng, 9_000))
    b[0:2_500] = b"N" * 2_500
    g = mutate(rng, genes[3], 0.03)
    b[2_600:2_600 + len(g)] = g
    c = random_dna(rng, 700) + genes[11] * 6 + random_dna(rng, 700)
    return [bytes(a), bytes(b), c, random_dna(rng, W), random_dna(rng, W - 1)]


@pytest.fixture(scope="module")
def exact_D(records, alp_ref):
    """Exact D of every window of every record (the integer oracle: the first window's D apart, then one value per later window)."""
    _, D, D1 = orc.single_scan_int(records, alp_ref["S"], alp_ref["N"], K, W, 1, 50, return_D=True)
    out, at = [], 0
    for c, seq in enumerate(records):
        nwin = len(seq) - W + 1
        if nwin <= 0:
            out.append(np.zeros(0, dtype=np.int64))
            continue
        out.append(np.concatenate([[D1[c]], D[at:at + nwin - 1]]))
        at += nwin - 1
    assert at == D.size
    return out


def _check_cover(records, exact_D, S, N, T, T_hi):
    U = filter_ref.bound_U(S, N, K, W, T, T_hi)
    Dmax = max(T - 1, T_hi)
    n_low = 0
    for seq, D in zip(records, exact_D):
        sums = filter_ref.granule_sums(seq, S, K, W)
        low = np.nonzero(D <= Dmax)[0]
        n_low += low.size
        assert np.all(sums[low // 16] >= U), "a window at or below the threshold band lies outside the candidate granules"
    return U, n_low


@pytest.mark.parametrize("thr", [20.0, 30.0])
def test_every_low_window_is_a_candidate(records, exact_D, alp_ref, thr):
    S, N = alp_ref["S"], alp_ref["N"]
    T, T_hi = filter_ref.threshold_band(thr, K, N)
    assert T == orc.int_threshold(thr, K, N)
    U, n_low = _check_cover(records, exact_D, S, N, T, T_hi)
    assert n_low > 50 and U > 0
    # the filter is selective: on the iid record only granules near the plants pass
    sums = filter_ref.granule_sums(records[0], S, K, W)
    assert np.count_nonzero(sums >= U) < sums.size // 4


def test_threshold_on_a_windows_distance(records, exact_D, alp_ref):
    """thr exactly on a window's distance: T == D of that window, the window is inside the guard band (T <= D <= T_hi) and U
    honours T_hi."""
    S, N = alp_ref["S"], alp_ref["N"]
    D = exact_D[0]
    scale = 2.0 * K * N * N
    s = int(np.argmin(np.abs(D / scale - 24.0)))
    thr = float(D[s]) / scale
    T, T_hi = filter_ref.threshold_band(thr, K, N)
    assert T == D[s] and T_hi >= D[s]
    U, n_low = _check_cover(records, exact_D, S, N, T, T_hi)
    assert n_low > 0
    assert filter_ref.granule_sums(records[0], S, K, W)[s // 16] >= U
    assert filter_ref.bound_U(S, N, K, W, T, T - 1) >= U               # (a band can only lower U)


def test_sum_identity_and_bound(records, exact_D, alp_ref):
    """sum_x S[x] c[x] = sum_p S[K_p], and D >= sumS2 - 2N sumS + N^2 n with equality iff no k-mer repeats."""
    S, N = np.asarray(alp_ref["S"], dtype=np.int64), alp_ref["N"]
    n = W - K + 1
    sumS2 = int(np.sum(S * S))
    for seq, D in zip(records[:3], exact_D[:3]):
        km = kmer_values(seq, K)
        for s in list(range(0, D.size, 997)) + [D.size - 1]:
            c = np.bincount(km[s:s + n], minlength=S.size)
            sumS = int(np.sum(S[km[s:s + n]]))
            assert int(np.sum(S * c)) == sumS
            assert int(np.sum((S - N * c) ** 2)) == D[s]
            lower = sumS2 - 2 * N * sumS + N * N * n
            assert D[s] >= lower and (D[s] == lower) == bool(np.all(c <= 1))
