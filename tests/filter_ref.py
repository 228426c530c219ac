"""numpy restatement of the distance-bound prefilter (kmergma.jl_amd/csrc/kgma_filter.hip), shared by test_filter_bound.py and
test_gpu_filter.py.

D_s = sum_x (S[x] - N c[x])^2 >= sumS2 - 2N sumS(s) + N^2 n with sumS(s) the sum of S over the window's n k-mer positions, so
D_s <= Dmax needs sumS(s) >= U = ceil((sumS2 + N^2 n - Dmax) / 2N).  The device tests granules of 16 window starts on the sum over
every position one of the granule's windows uses: floor((n + 14) / 16) + 1 blocks of 16 positions, positions behind the record's
last k-mer counting as 0."""
import math

import numpy as np

from tests.helpers import kmer_values


def threshold_band(thr: float, k: int, N: int, band_log2: int = 30):
    """(T, T_hi) of kgma_api.cpp's threshold_band: below thr <=> D < T; T <= D <= T_hi: at threshold."""
    fr, e = math.frexp(thr)
    mant = int(math.ldexp(fr, 53))
    e -= 53
    prod = mant * 2 * k * N * N
    lo, hi = prod - (prod >> band_log2), prod + (prod >> band_log2)
    if e >= 0:
        return lo << e, hi << e
    return -((-lo) >> -e), hi >> -e          # ceil, floor


def bound_U(S, N: int, k: int, W: int, T: int, T_hi: int) -> int:
    """U: a window can have D <= Dmax = max(T - 1, T_hi) only if its sum of S reaches U (exact, Python integers)."""
    n = W - k + 1
    Dmax = max(T - 1, T_hi)
    num = sum(int(x) * int(x) for x in np.asarray(S).tolist()) + N * N * n - Dmax
    return -((-num) // (2 * N))


def granule_sums(seq: bytes, S, k: int, W: int) -> np.ndarray:
    """Per granule g (windows 16g ... 16g + 15, 0-based) of one record: the sum of S over the k-mer positions its windows use."""
    nwin = len(seq) - W + 1
    if nwin <= 0:
        return np.zeros(0, dtype=np.int64)
    n = W - k + 1
    nblk = (n + 14) // 16 + 1
    ng = (nwin + 15) // 16
    v = np.zeros(16 * (ng + nblk), dtype=np.int64)
    sv = np.asarray(S, dtype=np.int64)[kmer_values(seq, k)]          # one value per k-mer position 0 ... L - k
    v[:sv.size] = sv
    P = np.concatenate([[0], np.cumsum(v.reshape(-1, 16).sum(axis=1))])
    return P[nblk:nblk + ng] - P[:ng]


def candidates(contigs, S, k: int, W: int, U: int) -> np.ndarray:
    """(n, 2) int64 array (record, granule) of the granules whose sum reaches U, sorted."""
    out = []
    for c, seq in enumerate(contigs):
        g = np.nonzero(granule_sums(seq, S, k, W) >= U)[0]
        out.append(np.stack([np.full(g.size, c, dtype=np.int64), g.astype(np.int64)], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int64)
