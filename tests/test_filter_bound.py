"""The distance bound behind the scan's prefilter (kgma_filter.hip), on the CPU: a numpy restatement of the filter (granule sums,
U) against the exact D of the integer oracle.  Every window at or below the threshold band must lie in a candidate granule."""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import filter_cases as fc
from tests import filter_ref
from tests.helpers import BASES, kmer_values, mutate, random_dna

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


def _check_cover(records, exact_D, S, N, T, T_hi, k=K, W=W):
    U = filter_ref.bound_U(S, N, k, W, T, T_hi)
    Dmax = max(T - 1, T_hi)
    n_low = 0
    for seq, D in zip(records, exact_D):
        sums = filter_ref.granule_sums(seq, S, k, W)
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


# ---- the shape matrix (tests/filter_cases.py): every kernel form and nblk = 2 ... 25 ---------------------------------------------

@pytest.mark.parametrize("cell", fc.MATRIX, ids=fc.cell_id)
def test_matrix_cover(cell):
    """Every window with D <= max(T - 1, T_hi) lies in a granule whose sum reaches U, at every cell of the matrix; and the cell is
    what the GPU test needs: S on the right side of 256, U > 0, every plant below the threshold, a run of >= 128 candidate granules."""
    k, N, nk = cell
    c = fc.cell(k, N, nk)
    S, W = c["ref"]["S"], c["W"]
    assert W == nk + k - 1 and int(S.sum()) == N * nk
    assert (int(S.max()) < 256) == (N == 7)
    assert c["T"] == orc.int_threshold(c["thr"], k, N)
    U, n_low = _check_cover(c["contigs"], c["D"], S, N, c["T"], c["T_hi"], k, W)
    assert U == c["U"] > 0
    assert all(c["D"][r][s] < c["T"] for r, s in c["plants"]) and n_low >= len(c["plants"])
    want = c["want"]
    assert fc.longest_run(want) >= 128                                  # the tandem run: a candidate granule's last block on every lane
    last = {r: (len(seq) - W) // 16 for r, seq in enumerate(c["contigs"]) if r > 0 and len(seq) >= W}
    have = set(map(tuple, want.tolist()))
    assert len(last) == 8 and all((r, g) in have for r, g in last.items())   # every short record's last granule is a candidate
    short = [r for r, seq in enumerate(c["contigs"]) if len(seq) < W]
    assert short == [4] and not np.isin(want[:, 0], short).any()        # the record without a window sits between the others
    n_gran = sum((len(seq) - W + 16) // 16 for seq in c["contigs"] if len(seq) >= W)
    assert len(want) < n_gran // 4                                      # (the filter is selective)


def _naive_granule_sums(seq, S, k, W):
    """Per granule, by Python loops: (sum of S over the union of the k-mer positions of windows 16g ... 16g + 15 that exist in the
    record, sum of S over that union rounded up to whole blocks of 16 positions from 16g on -- what a full granule's windows use,
    n + 15 positions, in blocks -- and clipped to the record's k-mers)."""
    n, nwin = W - k + 1, len(seq) - W + 1
    km = kmer_values(seq, k).tolist()
    nblk = -(-(n + 15) // 16)                                           # the fewest blocks that hold n + 15 positions
    union, blocks = [], []
    for g in range((max(nwin, 0) + 15) // 16):
        pos = set()
        for s in range(16 * g, min(16 * g + 16, nwin)):
            pos.update(range(s, s + n))
        blk = set(p for p in range(16 * g, 16 * (g + nblk)) if p < len(km))
        assert pos <= blk and max(pos) <= len(seq) - k                  # a superset: the sum bounds every window's from above (S >= 0)
        if n % 16 == 1 and 16 * g + 16 <= nwin:
            assert pos == blk                                           # (n + 15 fills its blocks and all 16 windows exist)
        union.append(sum(int(S[km[p]]) for p in pos))
        blocks.append(sum(int(S[km[p]]) for p in blk))
    return union, blocks


@pytest.mark.parametrize("k,nk", [(5, 2), (6, 2), (5, 16), (5, 17), (6, 17), (6, 18), (6, 34), (5, 100), (6, 284)])
def test_granule_sums_against_a_naive_loop(k, nk):
    """filter_ref.granule_sums is what the GPU comparison trusts.  It equals the direct sum of S over the positions the granule's
    windows use, in whole blocks of 16 as the kernel takes them and record ends included; that is never less than the sum over
    the exact union of the existing windows' positions, and the same wherever that union fills its blocks (nk = 17, full granule)."""
    W = nk + k - 1
    assert fc.nblk_of(nk) == -(-(nk + 15) // 16)
    rng = np.random.default_rng([6201, k, nk])
    tables = [fc.family(k, 300, nk)["S"], rng.integers(0, 70_000, size=4 ** k)]
    lengths = [W - 1, W, W + 1, W + 14, W + 15, W + 16, W + 17, W + 31, W + 32, W + 33, min(W + 63, 400), min(W + 64, 400), 400]
    n_equal = 0
    for L in lengths:
        seq = random_dna(rng, L)
        for S in tables:
            got = filter_ref.granule_sums(seq, S, k, W)
            union, blocks = _naive_granule_sums(seq, S, k, W)
            assert got.tolist() == blocks, (L,)
            assert all(b >= u for b, u in zip(blocks, union))
            assert got.size == (max(L - W + 1, 0) + 15) // 16
            if nk == 17:
                full = (L - W + 1) // 16                                # granules with all 16 windows
                assert got.tolist()[:full] == union[:full]
                n_equal += full
    assert nk != 17 or n_equal > 20


def _norepeat_like(rng, base, k, rate):
    """A sequence of len(base) residues without a repeated k-mer that follows `base` except at a fraction `rate` of the positions
    (and where following it would repeat a k-mer)."""
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    while True:
        out, seen, v, ok = [], set(), 0, True
        for i in range(len(base)):
            order = rng.permutation(4).tolist()
            if rng.random() >= rate:
                order = [code[base[i]]] + order
            for b in order:
                x = ((v << 2) | b) & (4 ** k - 1)
                if i < k - 1 or x not in seen:
                    break
            else:
                ok = False
                break
            v = x
            if i >= k - 1:
                seen.add(x)
            out.append(b)
        if ok:
            return BASES[np.asarray(out)].tobytes()


@pytest.mark.parametrize("k", [5, 6])
@pytest.mark.parametrize("nk", [2, 17, 383])
def test_bound_U_against_brute_force(k, nk):
    """For a window without a repeated k-mer D equals the bound, so sumS >= U <=> D <= Dmax exactly: both directions, with the
    threshold on one window's own distance (T == D <= T_hi) and just above and below it."""
    W, N = nk + k - 1, 7
    rng = np.random.default_rng([6202, k, nk])
    base = _norepeat_like(rng, random_dna(rng, W), k, 0.0)
    S = np.zeros(4 ** k, dtype=np.int64)
    for _ in range(N):
        S += np.bincount(kmer_values(mutate(rng, base, 0.03), k), minlength=4 ** k)
    wins = [base] + [_norepeat_like(rng, base, k, r) for r in np.linspace(0.0, 0.5, 60)] + [_norepeat_like(rng, random_dna(rng, W), k, 0.0)]
    D, sumS = [], []
    for w in wins:
        c = np.bincount(kmer_values(w, k), minlength=4 ** k)
        assert c.max() == 1 and c.sum() == nk
        D.append(int(np.sum((S - N * c) ** 2)))                          # brute force: the definition
        sumS.append(int(np.sum(S * c)))
    D, sumS = np.asarray(D), np.asarray(sumS)
    scale = 2.0 * k * N * N
    mid = float(np.sort(D)[len(D) // 2])
    n_in = n_out = 0
    for thr in (mid / scale, (mid + 0.5) / scale, max(mid - 0.5, 0.0) / scale, float(D.min()) / scale, 0.01):
        T, T_hi = filter_ref.threshold_band(thr, k, N)
        U = filter_ref.bound_U(S, N, k, W, T, T_hi)
        Dmax = max(T - 1, T_hi)
        assert np.array_equal(sumS >= U, D <= Dmax), thr
        n_in += int(np.count_nonzero(D <= Dmax))
        n_out += int(np.count_nonzero(D > Dmax))
    assert n_in > 0 and n_out > 0
