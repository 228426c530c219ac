"""Windows of fewer k-mers than a 64-window step (nk = W - k + 1 < 64) and the first sizes beyond it: the references, genomes and
thresholds shared by test_short_cases.py (CPU) and test_gpu_short_windows.py.  Nothing here calls the library under test: every
distance comes from the oracles.

Every scan kernel walks a stream in steps of 64 windows, one lane per window.  With nk < 64 the k-mer that leaves lane p's window
is the one that entered lane p - nk's window in the SAME step, so the genomes put their planted windows at chosen lanes:
PHASES (window index mod 64) 0, 1, 63 - nk (the last lane whose leaving k-mer still precedes the step; where >= 0), 62, 63 and 65
(lane 1 of the step after).

Single mode -- genome(k, nk, base): one record of LONG residues of random sequence with
  * two copies of base per phase (one exact, one mutated at 4 % from 15 k-mers per window on: _copy),
    the first at window 64 * Q0 + phase, one every 64 * DQ windows; a lower-cased stretch over the third copy;
  * one exact tandem run of base over at least 200 windows, an A run of 300, an AC repeat of 300, an N / n run of 200;
  * NOISY residues of back-to-back copies of base, each mutated at 7 % (not plants: they put windows BETWEEN an exact copy and
    random sequence, without which the distance lattice of a window of two or three k-mers has one value for nearly every window);
short records of W - 1, W, W + 1, W + 62 ... W + 65 and 2 W residues, each ending in a copy where it has a window, and MEDIUM
records of 100 + 2 W residues and a few more with a copy in the middle.  (The reference keeps ONE running minimum per record and
resets it only at a hit: a dip that ends inside the previous hit's range leaves it at that dip's minimum, and once that is the
distance of an exact copy the record gives no further hit.  On the coarse lattices of short windows and small k that happens within
a few dips, so the hits the conditions below ask for need records that start afresh.)
Cluster mode -- cluster_genome: the same elements for several bases, short records of maxws + k - 2, maxws + k - 1, maxws + k and
maxws + 64 residues.

Thresholds, from the oracle's exact D only:
  sparse  filter_cases.threshold: 1.25 x the largest planted distance + 0.05;
  dense   half-way between two neighbouring values of the long record's D, the pair that puts the share of windows below the
          threshold nearest to 5 % (on a lattice "the value under which 5 % fall" has a side to choose; of the shares inside
          DENSE_BAND the nearest to 5 % is taken).
What keeps a case from being vacuous is asserted where the case is built: >= MIN_SPARSE_HITS hits of the integer oracle at sparse;
at dense a share of ALL windows inside DENSE_BAND and >= MIN_DENSE_HITS hits.  A seed that misses them is changed, not the numbers.
"""
import functools

import numpy as np

from oracle import oracle as orc
from tests import filter_cases as fc
from tests.helpers import kmer_values, mutate, random_dna

NKS = (2, 3, 15, 16, 17, 31, 32, 33, 47, 62, 63, 64, 65, 66)
NKS_MANDATORY = (2, 3, 17, 33, 63, 64, 65)
SEED, SEEDS = 7300, 40
BUFF = 50                                # single mode
LONG, Q0, DQ, MEDIUM = 36_000, 8, 12, 40
TANDEM_AT, TANDEM_WINDOWS, A_AT, AC_AT, N_AT, NOISY_AT, NOISY = 12_000, 200, 14_000, 15_000, 16_000, 18_000, 8_000
NOISY_RATE = 0.07
DENSE_TARGET, DENSE_BAND = 0.05, (0.02, 0.50)
MIN_SPARSE_HITS, MIN_DENSE_HITS = 10, 30
OMN_BUFF, OMN_GENOME_POS = 20, 55        # cluster mode


def phases(nk):
    """Window index mod 64 of the long record's copies, in the order they are placed (65: lane 1 of the following step)."""
    return tuple(p for p in (0, 1, 63 - nk, 62, 63, 65) if p >= 0)


def _copy(rng, base, nk, exact):
    """The base, or a mutated copy of it: filter_cases.plant_of (4 % from 34 k-mers on); from 15 k-mers on a copy at 4 % with one
    substitution at the least, so that a window that is NOT the base sits on the chosen lane there too.  Below 15 k-mers one
    substitution leaves less than half of the window's k-mers at k >= 6: every copy is exact."""
    if exact or nk < 15:
        return base
    if nk >= 34:
        return fc.plant_of(rng, base, nk)
    out = bytearray(mutate(rng, base, 0.04))
    if bytes(out) == base.upper():
        p = int(rng.integers(0, len(out)))
        out[p] = b"ACGT"[(b"ACGT".index(out[p]) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(out)


def _noisy(rng, base, n):
    out = bytearray()
    while len(out) < n:
        out += mutate(rng, base, NOISY_RATE)
    return bytes(out[:n])


def genome(k, nk, base, seed=SEED):
    """(contigs, plants) of the module docstring; plants: (record, 0-based window), the long record's in phases(nk) order, two each."""
    W = nk + k - 1
    assert len(base) == W
    rng = np.random.default_rng([seed + 1, k, nk])
    a = bytearray(random_dna(rng, LONG))
    plants = []
    q = Q0
    for ph in phases(nk):
        for exact in (True, False):
            pos = 64 * q + ph
            a[pos:pos + W] = _copy(rng, base, nk, exact)
            plants.append((0, pos))
            q += DQ
    assert 64 * q + 65 + W < TANDEM_AT
    lo = plants[2][1]
    a[lo - 5:lo + W + 5] = bytes(a[lo - 5:lo + W + 5]).lower()
    run = base * (-(-(TANDEM_WINDOWS + W) // W))
    assert len(run) - W + 1 >= TANDEM_WINDOWS and TANDEM_AT + len(run) < A_AT
    a[TANDEM_AT:TANDEM_AT + len(run)] = run
    a[A_AT:A_AT + 300] = b"A" * 300
    a[AC_AT:AC_AT + 300] = b"AC" * 150
    a[N_AT:N_AT + 200] = b"N" * 100 + b"n" * 100
    a[NOISY_AT:NOISY_AT + NOISY] = _noisy(rng, base, NOISY)
    assert len(a) == LONG
    contigs = [bytes(a)]
    for L in (W - 1, W, W + 1, W + 62, W + 63, W + 64, W + 65, 2 * W):
        if L < W:
            contigs.append(random_dna(rng, L))
            continue
        contigs.append(random_dna(rng, L - W) + _copy(rng, base, nk, L % 2 == 0))
        plants.append((len(contigs) - 1, L - W))
    for i in range(MEDIUM):
        left = 50 + i % 7
        contigs.append(random_dna(rng, left) + _copy(rng, base, nk, i % 2 == 0) + random_dna(rng, 50 + W))
        plants.append((len(contigs) - 1, left))
    return contigs, plants


# ---- references -------------------------------------------------------------------------------------------------------------------

def _own_D(ref):
    """Exact D of the base itself under its family's S."""
    c = np.bincount(kmer_values(ref["base"], ref["k"]), minlength=4 ** ref["k"]).astype(np.int64)
    return int(np.sum((ref["S"] - ref["N"] * c) ** 2))


def family(k, N, nk, seed=SEED):
    """filter_cases.family with the first seed from `seed` on that gives (N = 300: the two-byte S case) an entry of 256 or more and
    a base that is not at distance 0 from its own family: the few sequences of a short window are often all the base itself, and a
    distance of exactly 0 has no relative error to hold the Float64 oracle's value to."""
    for sd in range(seed, seed + 50):
        ref = fc.family(k, N, nk, seed=sd)
        if (N < 256 or int(ref["S"].max()) >= 256) and _own_D(ref) > 0:
            return ref
    raise AssertionError("no seed gives a usable family at k %d N %d nk %d" % (k, N, nk))


def int32_family(k, nk):
    """S beyond int16 the way test_stream8_int32_s_tables makes it -- many copies of a base with a homopolymer, N just large enough
    for N x (copies of the all-A k-mer) > 32767 -- with one copy in twenty mutated at 10 %, which keeps the base's own distance off 0."""
    W = nk + k - 1
    rng = np.random.default_rng([SEED + 2, k, nk])
    base = bytearray(random_dna(rng, W))
    n_a = max(1, (3 * nk) // 4)                                         # all-A k-mers wanted
    off = min(2, W - (n_a + k - 1))
    base[off:off + n_a + k - 1] = b"A" * (n_a + k - 1)
    base = bytes(base)
    c = np.bincount(kmer_values(base, k), minlength=4 ** k).astype(np.int64)
    N = int(32768 / (0.93 * int(c.max()))) + 2
    n_mut = -(-N // 20)
    S = c * (N - n_mut)
    for _ in range(n_mut):
        S += np.bincount(kmer_values(mutate(rng, base, 0.10), k), minlength=4 ** k)
    ref = fc.ref_from_S(S, N, k, W, base)
    assert int(ref["S"].max()) > 32767 and N < 1 << 22 and _own_D(ref) > 0
    return ref


def float_ref(ref):
    """A general Float64 KFV of the same family: every entry moved by 0.123456789 (no S / N form)."""
    return np.asarray(ref["RV"], dtype=np.float64) + 0.123456789


# ---- thresholds -------------------------------------------------------------------------------------------------------------------

class NoDenseCut(Exception):
    """No value of D puts a share of the windows inside DENSE_BAND below it: a property of the genome, so of the seed."""


def dense_cut(D_long, D_all):
    """(lo, hi, share): neighbouring values of D_long; D <= lo is `share` of D_all, the share inside DENSE_BAND nearest to 5 %."""
    vals, counts = np.unique(D_long, return_counts=True)
    share_long = np.cumsum(counts)[:-1] / D_long.size                   # cut above vals[i]
    all_sorted = np.sort(D_all)
    share_all = np.searchsorted(all_sorted, vals[:-1], side="right") / all_sorted.size
    ok = np.nonzero((share_all >= DENSE_BAND[0]) & (share_all <= DENSE_BAND[1]))[0]
    if not ok.size:
        raise NoDenseCut("no value of D puts between 2 % and 50 % of the windows below it")
    i = int(ok[np.argmin(np.abs(share_long[ok] - DENSE_TARGET))])
    return vals[i], vals[i + 1], float(share_all[i])


def _thresholds_int(contigs, plants, ref):
    k, N, W, S = ref["k"], ref["N"], ref["ws"], ref["S"]
    D = fc.exact_D(contigs, S, N, k, W)
    scale = 2.0 * k * N * N
    Dall = np.concatenate(D)
    lo, hi, share = dense_cut(D[0], Dall)
    thr = dict(sparse=fc.threshold(D, plants, k, N), dense=0.5 * (float(lo) + float(hi)) / scale)
    n_hits = {}
    for name, t in thr.items():
        T = orc.int_threshold(t, k, N)
        n_hits[name] = len(orc.single_scan_int(contigs, S, N, k, W, T, BUFF)[0])
    T = orc.int_threshold(thr["dense"], k, N)
    assert lo < T <= hi and np.count_nonzero(Dall < T) / Dall.size == share
    return D, thr, n_hits, share


def _not_vacuous(n_hits, share):
    return n_hits["sparse"] >= MIN_SPARSE_HITS and n_hits["dense"] >= MIN_DENSE_HITS and DENSE_BAND[0] <= share <= DENSE_BAND[1]


@functools.lru_cache(maxsize=None)
def cell(k, N, nk):
    """What the tests of one (k, N, nk) share, computed once and never modified.  N: a filter_cases family of N sequences; "int32":
    int32_family."""
    ref = int32_family(k, nk) if N == "int32" else family(k, N, nk)
    for seed in range(SEED, SEED + SEEDS):
        contigs, plants = genome(k, nk, ref["base"], seed)
        try:
            D, thr, n_hits, share = _thresholds_int(contigs, plants, ref)
        except NoDenseCut as e:
            last = str(e)
            continue
        if _not_vacuous(n_hits, share):
            break
        last = "%s, share %.3f" % (n_hits, share)
    else:
        raise AssertionError("k %s N %s nk %s: no seed meets the conditions (last: %s)" % (k, N, nk, last))
    return dict(seed=seed, ref=ref, W=ref["ws"], contigs=contigs, plants=plants, D=D, thr=thr, n_hits=n_hits, share=share)


@functools.lru_cache(maxsize=None)
def float_cell(k, nk):
    """cell(k, 7, nk)'s genome under float_ref: thresholds from the Float64 oracle's distances."""
    c = cell(k, 7, nk)
    RV, W, contigs = float_ref(c["ref"]), c["W"], c["contigs"]
    _, od = orc.single_scan(contigs, RV, k, W, 0.0, BUFF, return_dists=True)      # windows 2 ... of every record, in record order
    per, at = [], 0
    for seq in contigs:
        nwin = len(seq) - W + 1
        if nwin <= 0:
            per.append(np.zeros(0))
            continue
        per.append(np.concatenate([[orc.kmer_dist_kfv(seq[:W], RV, k)], od[at:at + nwin - 1]]))
        at += nwin - 1
    assert at == od.size
    dall = np.concatenate(per)
    lo, hi, share = dense_cut(per[0], dall)
    # (sparse: the shift moves every distance by nearly the same amount -- 4^k x 0.123456789^2 / 2k, the cross term sums to zero over
    #  a window -- so the margin above the largest planted distance is the integer family's, kept absolute)
    margin = 0.25 * fc.planted_max(c["D"], c["plants"], k, 7) + 0.05
    thr = dict(sparse=round(max(float(per[r][s]) for r, s in c["plants"]) + margin, 2), dense=0.5 * (float(lo) + float(hi)))
    n_hits = {name: len(orc.single_scan(contigs, RV, k, W, t, BUFF)[0]) for name, t in thr.items()}
    assert n_hits["sparse"] >= MIN_SPARSE_HITS and n_hits["dense"] >= MIN_DENSE_HITS, n_hits
    assert DENSE_BAND[0] <= share <= DENSE_BAND[1]
    return dict(RV=RV, W=W, contigs=contigs, plants=c["plants"], thr=thr, n_hits=n_hits, share=share)


# ---- cluster mode -----------------------------------------------------------------------------------------------------------------

def cluster_genome(k, ws, bases, seed=SEED):
    """(contigs, plants): one long record with two copies of every base mutated at 5 % (windows 64 q + a phase of the shortest
    window's phases(), in turn), the low-complexity runs, up to NOISY / 2 residues of 7 % copies per base and one exact tandem run of the
    first base; then the short records.  plants: (record, 0-based start, KFV)."""
    m, maxws = len(ws), max(ws)
    rng = np.random.default_rng([seed + 3, k, sum(ws), m])
    ph = phases(min(ws) - k + 1)
    per = min(NOISY // 2, 24_000 // m)                                  # residues of 7 % copies per base
    L = 14_000 + per * m
    a = bytearray(random_dna(rng, L))
    plants = []
    q = Q0
    for j, base in enumerate(bases):
        for u in range(2):
            pos = 64 * q + ph[(2 * j + u) % len(ph)]
            a[pos:pos + len(base)] = mutate(rng, base, 0.05)
            plants.append((0, pos, j))
            q += 8
    assert 64 * q < 9_000
    a[9_000:9_300] = b"A" * 300
    a[10_000:10_300] = b"AC" * 150
    a[11_000:11_200] = b"N" * 100 + b"n" * 100
    run = bases[0] * (-(-(TANDEM_WINDOWS + len(bases[0])) // len(bases[0])))
    assert len(run) < 1_500
    a[12_000:12_000 + len(run)] = run
    for j, base in enumerate(bases):
        a[14_000 + per * j:14_000 + per * (j + 1)] = _noisy(rng, base, per)
    contigs = [bytes(a)]
    for Lr in (maxws + k - 2, maxws + k - 1, maxws + k, maxws + 64):
        contigs.append(random_dna(rng, Lr))
    contigs.append(bases[-1] + random_dna(rng, 200))
    for i in range(MEDIUM):
        j, left = i % m, 50 + i % 7
        contigs.append(random_dna(rng, left) + mutate(rng, bases[j], 0.05) + random_dna(rng, 50 + maxws))
        plants.append((len(contigs) - 1, left, j))
    return contigs, plants


@functools.lru_cache(maxsize=None)
def cluster_cell(k, ws):
    """ws: a tuple of window sizes, one KFV each (a filter_cases family of 4 + j sequences).  Thresholds: per KFV, dense_cut of its
    exact D over the whole genome.  The integer oracle must find MIN_DENSE_HITS hits, of two KFVs or more."""
    m = len(ws)
    fams = [family(k, 4 + j, w - k + 1, seed=SEED + 100 * (j + 1)) for j, w in enumerate(ws)]
    S, N, KFVs = [f["S"] for f in fams], [f["N"] for f in fams], [f["RV"] for f in fams]
    assert max(int(s.max()) for s in S) < 256
    for seed in range(SEED, SEED + SEEDS):
        contigs, plants = cluster_genome(k, ws, [f["base"] for f in fams], seed)
        _, oD = orc.omn_scan_int(contigs, S, N, k, list(ws), [1] * m, OMN_BUFF, OMN_GENOME_POS, return_D=True)
        thr, shares = [], []
        for j in range(m):
            lo, hi, share = dense_cut(oD[j], oD[j])
            thr.append(0.5 * (float(lo) + float(hi)) / (2.0 * k * N[j] * N[j]))
            shares.append(share)
        T = [orc.int_threshold(t, k, n) for t, n in zip(thr, N)]
        ohi, oD = orc.omn_scan_int(contigs, S, N, k, list(ws), T, OMN_BUFF, OMN_GENOME_POS, return_D=True)
        if len(ohi) >= MIN_DENSE_HITS and len({h["kfv"] for h in ohi}) >= min(m, 2):
            break
    else:
        raise AssertionError("k %d ws %s: no seed meets the conditions (last: %d hits of KFVs %s)" % (k, ws, len(ohi), {h["kfv"] for h in ohi}))
    ohits, _ = orc.omn_scan(contigs, KFVs, k, list(ws), thr, OMN_BUFF, OMN_GENOME_POS)
    return dict(seed=seed, k=k, ws=list(ws), S=S, N=N, KFVs=KFVs, contigs=contigs, plants=plants, thr=thr, T=T, shares=shares, ohi=ohi, oD=oD,
                ohits=ohits)


# ---- what runs where (test_gpu_short_windows.py; test_short_cases.py builds every one of them) -----------------------------------

STREAM8_KS, STREAM_KS, BITSLICE_KS, SCAN_DEFAULT_KS = (5, 6, 7), (5, 6), (5, 6, 7), (2, 3, 4, 8, 9, 10)
GENERIC_FORCED_KS, GENERIC_DEFAULT_KS = (3, 6), (1, 11)
CHAIN_NKS, CHAIN_KS = (2, 17, 63, 64, 65), (6, 7)
STEP_NKS, STEP_KS, STEP_NS = (2, 16, 17, 18, 34, 63, 64, 65), (5, 6), (7, 300)


def nks_for(form, k, N=7):
    """Every nk for the kernels of k = 5, 6, 7 and the forced generic kernel, the mandatory subset elsewhere."""
    return NKS if (form in ("stream8", "stream", "bitslice", "generic") and N != "int32") else NKS_MANDATORY


def single_cells():
    """(form, k, N, nk) of every single-mode case of the device tests."""
    out = []
    for k in STREAM8_KS:
        for N in (7, 300):
            out += [("stream8", k, N, nk) for nk in nks_for("stream8", k, N)]
    out += [("stream8", k, "int32", nk) for k in (5, 6) for nk in NKS_MANDATORY]
    out += [("stream", k, 7, nk) for k in STREAM_KS for nk in nks_for("stream", k)]
    out += [("bitslice", k, 7, nk) for k in BITSLICE_KS for nk in nks_for("bitslice", k)]
    out += [("scan", k, 7, nk) for k in SCAN_DEFAULT_KS for nk in NKS_MANDATORY]
    out += [("generic", k, 7, nk) for k in GENERIC_FORCED_KS for nk in nks_for("generic", k)]
    out += [("gen", k, 7, nk) for k in GENERIC_DEFAULT_KS for nk in NKS_MANDATORY]
    return out


CLUSTER_ONE_SIZE = [(6, (20, 20)), (6, (68, 68, 68)), (5, (67, 67, 67, 67)), (6, (8, 8, 8, 8))]
CLUSTER_DERIVED = [(6, (67, 68)), (6, (68, 69)), (6, (69, 70, 70)), (7, (69, 70, 70, 69)), (6, (7, 8)), (5, (20, 21, 21))]
# (launches with KGMA_STREAM8_WIDE on: the five- / six- / eight-KFV variants take windows of n, n + 1, n + 2 k-mers with at most
#  two KFVs at n + 2 -- kgma_stream.hip: stream8_fn_wide -- so (5, 66 67 68 68 68) stays {66, 67} + {68 x 3})
CLUSTER_WIDE = [(6, (67, 67, 68, 68, 69), 1), (6, (66, 67, 67, 67, 68), 1), (5, (66, 67, 68, 68, 68), 2), (6, (20, 20, 21, 21, 22), 1),
                (7, (69, 69, 69, 69, 70, 70, 70, 71), 1), (6, (67, 67, 67, 68, 68, 69), 1)]
CLUSTER_TWO_KERNEL = [(k, ws) for k in (5, 6, 7) for ws in ((20, 20, 21), (67, 68, 68, 69, 69))]
CLUSTER_BITSLICE_MIXED = [(3, (10, 40, 66, 67)), (8, (30, 71, 72))]


def cluster_shapes():
    return (CLUSTER_ONE_SIZE + CLUSTER_DERIVED + [(k, ws) for k, ws, _ in CLUSTER_WIDE] + CLUSTER_TWO_KERNEL + CLUSTER_BITSLICE_MIXED)
