"""The ends of the integer scan paths' range: references, genomes and thresholds shared by test_range_cases.py (CPU) and
test_gpu_range.py.  Nothing here calls the library under test: every distance comes from the oracles.

Every integer scan kernel keeps part of its arithmetic in 32 bits, and the host decides from magnitude predicates on the number of
references N, the k-mers per window nk and the table S which kernel a KFV may take (kgma_set_refs).  They are restated here in
Python integers from their description, D = sum_x (S[x] - N c[x])^2 over a window's k-mer counts c:
  dmax      sum S^2 + N^2 nk^2: D of a window that shares no k-mer with the table, the largest D there is;
  fits32    dmax / 2N < 2^29 and N nk < 2^30: the prefix E = (D - D0) / 2N fits the int32 kernels;
  big_ok    64 (Smax + N nk) <= 2^30 and N < 2^22: a 64-window step's LOCAL prefix fits int32 (16-bit counter form of stream8);
  n22       N < 2^22: the 24-bit multiplier of the count-table kernels;
  d61       dmax < 2^61: the device path's int64 range -- beyond it the KFV is refused.
edge_N finds, by bisection, the largest N for which a predicate holds (edge-) and that N + 1 (edge+).  A third side, x3, is three
times edge-: one step beyond a bound says nothing about a kernel that has a bit to spare (int32 holds twice what fits32 and big_ok
promise), so a predicate that is two bits too generous is caught there, where the prefix is three times the promised one.

Reference families.  A table S with a given N is built directly in numpy and KFV = S / N is passed with n_refs = N -- no N-fold
reference lists:
  copies       S = N count(base): N identical references;
  near_copies  S = N count(base) + delta, delta = floor(u N) with u in [0, 1) on a third of the non-zero entries and on a few
               zero ones (the generic S / N case: entries that are no integers);
  run_heavy    base is one homopolymer but for five residues at either end: Smax = N (nk - 10), so that the Smax term of big_ok
               and the width of the S table move with N.
The base (and every entry of S) avoids the k-mers C..C and G..G, the two homopolymers of the genome.

The range genome (range_genome) for a window of W residues, a few kilobases:
  A  base + C x (W + 200) + base' + random: D = 0 (copies) at the first window, D = dmax exactly inside the run, so E is driven
     from 0 to dmax / 2N (base': the base with its first residue substituted, see touched());
  B  C x (W + 200) first, then base', G x (W + 200), base': the record STARTS at dmax, E is driven to -dmax / 2N (+ one k-mer);
  C  random sequence with three copies of base mutated at 2, 5 and 10 % (under 34 k-mers per window: one substitution each, in the
     first, second and third residue): hits that come from ordinary dips;
  D  records of W - 1, W and W + 1 residues;
  E  (run_heavy) the reference's own homopolymer running into C..C: S[leaving] and N c[leaving] both maximal;
  F  C x (W + 200) + the first h residues of base + C x (W + 200), h chosen so that the windows that hold the whole fragment are
     at FRAGMENT_SHARE of dmax: a dip from dmax that turns back far above zero.
Three thresholds per cell: `mid`, half-way between the largest distance of a mutated copy and the distance of random sequence (the
last window of record A); `all`, above dmax / 2kN^2, under which EVERY window lies; `low`, at LOW_SHARE of dmax.  Records B and F
start at D0 = dmax, so the kernels' threshold relative to the start, TE = (T - D0) / 2N, is -0.8 dmax / 2N at `low`: where a KFV
whose dmax / 2N is beyond 2^30 reached an int32 kernel, the clamp of TE at -(2^30 - 1) would bite, and record F's dip, which stays
above `low`, would count as under it and give a hit (from 100 k-mers per window on, where h can be chosen finely enough).

What keeps a cell from being vacuous is asserted where it is built, on oracle values only: max D - min D >= 0.95 dmax over the
genome, and for the big_ok cells the largest |D[q + 64] - D[q]| / 2N of a record >= 2^29, half of what the form is promised.
"""
import functools

import numpy as np

from oracle import oracle as orc
from tests import filter_cases as fc
from tests.helpers import kmer_values, mutate, random_dna

SEED = 8100
BUFF = 50
RUN_EXTRA = 200                          # the absent homopolymers are W + RUN_EXTRA residues long
MUT_RATES = (0.02, 0.05, 0.10)
SPAN_SHARE = 0.95                        # of dmax, between the smallest and the largest D of the genome
STEP_BOUND = 1 << 29                     # |D[q + 64] - D[q]| / 2N to reach in the big_ok cells
FRAGMENT_SHARE, FRAGMENT_BAND = 0.27, (0.22, 0.32)   # record F's lowest D over dmax: above LOW_SHARE, below the 1/3 of the x3 cells' clamp
LOW_SHARE = 0.2
OMN_BUFF, OMN_GENOME_POS = 50, 77


# ---- the predicates, in Python integers ---------------------------------------------------------------------------------------------

def _ints(S):
    return [int(x) for x in np.asarray(S)[np.flatnonzero(S)]]


def dmax(S, N, nk):
    return sum(x * x for x in _ints(S)) + N * N * nk * nk


def fits32(S, N, nk):
    return dmax(S, N, nk) // (2 * N) < 2 ** 29 and N * nk < 2 ** 30


def big_ok(S, N, nk):
    return 64 * (max(_ints(S)) + N * nk) <= 2 ** 30 and N < 2 ** 22


def n22(S, N, nk):
    return N < 2 ** 22


def d61(S, N, nk):
    return dmax(S, N, nk) < 2 ** 61


PREDICATES = dict(fits32=fits32, big_ok=big_ok, n22=n22, d61=d61)


# ---- reference families ---------------------------------------------------------------------------------------------------------------

def absent_kmers(k):
    """Natural values of C..C and G..G (first base most significant, A C G T = 0 1 2 3)."""
    ones = (4 ** k - 1) // 3
    return ones, 2 * ones


@functools.lru_cache(maxsize=None)
def base_of(family, k, W, variant=0):
    """The family's base sequence: independent of N, without a run of k C or k G.  variant > 0 (the cluster cells' further bases):
    another draw, with a run of k + 2 A, so that three k-mers coincide and S = 3 N leaves int16 at the fits32 edge of k = 7."""
    rng = np.random.default_rng([SEED, k, W, len(family), variant])
    if family == "run_heavy":
        a = bytearray(random_dna(rng, 5) + b"A" * (W - 10) + random_dna(rng, 5))
        a[4:5], a[W - 5:W - 4] = b"T", b"T"                               # exactly nk - 10 all-A k-mers
    else:
        a = bytearray(random_dna(rng, W))
    if variant:
        a[10 + variant:10 + variant + k + 2] = b"A" * (k + 2)
    for c in b"CG":
        run = 0
        for i in range(W):
            run = run + 1 if a[i] == c else 0
            if run == k:
                a[i], run = ord("T"), 0
    base = bytes(a)
    assert not set(kmer_values(base, k).tolist()) & set(absent_kmers(k))
    return base


@functools.lru_cache(maxsize=None)
def _shape(family, k, W, variant=0):
    """(counts of the base, positions that get a delta, their fractions u)."""
    c = np.bincount(kmer_values(base_of(family, k, W, variant), k), minlength=4 ** k).astype(np.int64)
    if family != "near_copies":
        return c, None, None
    rng = np.random.default_rng([SEED + 1, k, W, variant])
    nz = np.flatnonzero(c)
    at = rng.choice(nz, size=max(1, nz.size // 3), replace=False)
    zeros = np.setdiff1d(rng.integers(0, 4 ** k, size=12), np.concatenate([nz, absent_kmers(k)]))
    assert zeros.size >= 3
    at = np.concatenate([at, zeros])
    return c, at, rng.random(at.size)


def table(family, k, W, N, variant=0):
    """S of the family at N references, int64."""
    c, at, u = _shape(family, k, W, variant)
    S = c * np.int64(N)
    if at is not None:
        S[at] += np.floor(u * N).astype(np.int64)
    return S


def ref_of(family, k, W, N, variant=0):
    S = table(family, k, W, N, variant)
    return dict(S=S, N=N, RV=S / float(N), ws=W, k=k, base=base_of(family, k, W, variant), family=family)


def edge_N(pred, k, W, family, variant=0):
    """(edge-, edge+): the largest N for which PREDICATES[pred] holds for the family's table, and that N + 1."""
    p, nk = PREDICATES[pred], W - k + 1
    return bisect_edge(lambda N: p(table(family, k, W, N, variant), N, nk))


def bisect_edge(ok):
    """(edge-, edge+) of a predicate on the positive integers that holds at 1 and fails from some value on."""
    lo, hi = 1, 2
    assert ok(lo)
    while ok(hi):
        lo, hi = hi, 2 * hi
        assert hi < 2 ** 40
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo, hi


# ---- the genome -----------------------------------------------------------------------------------------------------------------------

def _mutated(rng, base, rate, i, nk):
    """A copy of base mutated at `rate`; under 34 k-mers per window, where that leaves either the base itself or next to none of its
    k-mers, one substitution at residue i instead (i + 1 k-mers lost)."""
    if nk >= 34:
        return mutate(rng, base, rate)
    a = bytearray(base)
    a[i] = b"ACGT"[(b"ACGT".index(a[i]) + 1) % 4]
    return bytes(a)


def touched(base):
    """base with its first residue substituted: one k-mer lost, D = 2 N^2 under `copies`.  Every occurrence of the base after a
    record's first window is this one: the Float64 oracle reaches it by rolling updates, and a rolled value has no relative error to
    be held to where the exact distance is 0."""
    return (b"A" if base[:1] == b"T" else b"T") + base[1:]


@functools.lru_cache(maxsize=None)
def fragment_len(k, W, base):
    """h of record F.  The window's D over dmax depends on the counts alone, not on N: taken at N = 1, S = count(base).  (About
    (1 - h / W)^2: long windows are searched around h = W / 2 only.)"""
    S = np.bincount(kmer_values(base, k), minlength=4 ** k).astype(np.int64)
    dm = dmax(S, 1, W - k + 1)
    share = lambda h: bigint_D(b"C" * ((W - h) // 2) + base[:h] + b"C" * (W - h - (W - h) // 2), S, 1, k) / dm
    cand = range(1, W) if W < 100 else range(int(0.4 * W), int(0.56 * W))
    return min(cand, key=lambda h: abs(share(h) - FRAGMENT_SHARE))


def range_genome(k, W, bases, run_heavy=False, seed=SEED):
    """(contigs, plants, names): the records of the module docstring, A, B and F once per base; plants: (record, 0-based window,
    base index) of the mutated copies of record C; names: the record's letter."""
    rng = np.random.default_rng([seed + 2, k, W, len(bases)])
    run = W + RUN_EXTRA
    contigs, names, plants = [], [], []
    for base in bases:
        contigs.append(base + b"C" * run + touched(base) + random_dna(rng, 1500))
        contigs.append(b"C" * run + touched(base) + b"G" * run + touched(base))
        names += ["A", "B"]
    c = bytearray(random_dna(rng, 700))
    for j, base in enumerate(bases):
        for i, rate in enumerate(MUT_RATES):
            plants.append((len(contigs), len(c), j))
            c += _mutated(rng, base, rate, i, W - k + 1) + random_dna(rng, 600)
    contigs.append(bytes(c))
    names.append("C")
    for L in (W - 1, W, W + 1):
        contigs.append(random_dna(rng, L))
        names.append("D")
    if run_heavy:
        contigs.append(b"A" * (W + 100) + b"C" * run)
        names.append("E")
    for base in bases:
        contigs.append(b"C" * run + base[:fragment_len(k, W, base)] + b"C" * run)
        names.append("F")
    assert sum(len(x) for x in contigs) <= 40_000
    return contigs, plants, names


def bigint_D(seq, S, N, k):
    """D of the window `seq` in Python integers, from the window's own counts."""
    u, c = np.unique(kmer_values(seq, k), return_counts=True)
    D = sum(x * x for x in _ints(S))
    for x, cx in zip(u.tolist(), c.tolist()):
        Sx = int(S[x])
        D += (Sx - N * cx) ** 2 - Sx * Sx
    return D


def thresholds(planted_D, random_D, k, N, S, nk):
    """(mid, all, low) of the module docstring, in the scans' Float64 units."""
    scale = 2.0 * k * N * N
    planted, typical = max(planted_D) / scale, random_D / scale
    assert planted < 0.8 * typical, (planted, typical)
    return 0.5 * (planted + typical), 1.01 * dmax(S, N, nk) / scale, LOW_SHARE * dmax(S, N, nk) / scale


def step_share(D, N):
    """The largest |D[q + 64] - D[q]| / 2N over the records (Python integers)."""
    best = 0
    for d in D:
        if d.size > 64:
            best = max(best, int(np.max(np.abs(d[64:] - d[:-64]))) // (2 * N))      # (|differences| < 2^62: no wrap in int64)
    return best


# ---- cells ----------------------------------------------------------------------------------------------------------------------------

def _cells():
    out = []
    for side in ("-", "+"):
        out += [("fits32", k, 289 - k + 1, "near_copies", side) for k in (5, 6, 7)]
        out += [("fits32", k, 20, "copies", side) for k in (5, 6, 7)]
        out += [("fits32", k, 289 - k + 1, "copies", side) for k in (3, 4, 8, 10)]
        out += [("big_ok", k, nk, fam, side) for k in (5, 6, 7) for nk in (284, 1000) for fam in ("copies", "run_heavy")]
        out += [("n22", k, 10, "copies", side) for k in (5, 6)]
    out += [("d61", 6, 100, "copies", "-"), ("d61", 8, 64, "near_copies", "-")]
    out += [("fits32", k, 289 - k + 1, "near_copies", "x3") for k in (5, 6, 7)] + [("fits32", k, 289 - k + 1, "copies", "x3") for k in (4, 8)]
    out += [("big_ok", k, nk, fam, "x3") for k in (5, 6) for nk in (284, 1000) for fam in ("copies", "run_heavy")]
    return out


SINGLE_CELLS = _cells()
REFUSED_CELLS = [("d61", 6, 100, "copies", "+"), ("d61", 8, 64, "near_copies", "+")]
FORCED_CELL = ("fits32", 6, 284, "near_copies", "-")
CHAIN_CELLS = [("fits32", k, 289 - k + 1, "near_copies", "+") for k in (6, 7)] + [("big_ok", k, 284, "copies", "-") for k in (6, 7)]


def cell_id(c):
    return "%s%s-k%d-nk%d-%s" % (c[0], {"-": "lo", "+": "hi"}.get(c[4], c[4]), c[1], c[2], c[3])


def N_of(pred, k, nk, family, side):
    lo, hi = edge_N(pred, k, nk + k - 1, family)
    return {"-": lo, "+": hi, "x3": 3 * lo}[side]


def expected_kernel(k, S, N, nk):
    """The kernel a single integer KFV is observed to take, by regime ("The ends of the integer range")."""
    f32, big, q = fits32(S, N, nk), big_ok(S, N, nk), N < 2 ** 22
    s16 = int(S.max()) <= 32767
    table_k = k in (5, 6) or (k == 7 and s16)                             # the count-table kernels' k
    if f32 and table_k and q and nk <= 383:
        return "stream8_kernel"                                           # 8-bit counters
    if table_k and big and (not f32 or nk > 383):
        return "stream8_kernel"                                           # 16-bit counters, 64-bit carries
    if not f32:
        return "gen_kernel"
    return "stream_kernel" if k in (5, 6) else "scan_kernel"


@functools.lru_cache(maxsize=None)
def cell(pred, k, nk, family, side):
    """What the tests of one cell share, computed once and never modified."""
    W = nk + k - 1
    N = N_of(pred, k, nk, family, side)
    ref = ref_of(family, k, W, N)
    S = ref["S"]
    contigs, plants, names = range_genome(k, W, [ref["base"]], run_heavy=family == "run_heavy")
    D = fc.exact_D(contigs, S, N, k, W)
    Dall = np.concatenate(D)
    dm = dmax(S, N, nk)
    span = int(Dall.max()) - int(Dall.min())
    assert int(Dall.max()) == dm and span >= SPAN_SHARE * dm, (cell_id((pred, k, nk, family, side)), span / dm)
    step = step_share(D, N)
    if pred == "big_ok":
        assert step >= STEP_BOUND, (cell_id((pred, k, nk, family, side)), step / 2 ** 30)
    thr = thresholds([int(D[r][s]) for r, s, _ in plants], int(D[0][-1]), k, N, S, nk)
    frag = int(D[names.index("F")].min()) / dm
    if nk >= 100:
        assert FRAGMENT_BAND[0] <= frag <= FRAGMENT_BAND[1], (cell_id((pred, k, nk, family, side)), frag)
    return dict(pred=pred, side=side, k=k, nk=nk, W=W, N=N, ref=ref, contigs=contigs, plants=plants, names=names, D=D, dmax=dm, span=span,
                step=step, frag=frag, thr=thr, kernel=expected_kernel(k, S, N, nk))


# ---- cluster engine -------------------------------------------------------------------------------------------------------------------

def _cluster_N(spec, k, W, family, variant):
    if isinstance(spec, int):
        return spec
    pred, side = spec
    return edge_N(pred, k, W, family, variant)[0 if side == "-" else 1]


CLUSTER_CELLS = {
    "k6-84-fits32lo-fits32hi": (6, 289, "copies", (84, ("fits32", "-"), ("fits32", "+")), "stream8_kernel"),
    "k6-84-beyond-big_ok": (6, 289, "copies", (84, ("big_ok", "+")), "gen_kernel"),
    "k7-fits32lo-x2-int32-S": (7, 289, "copies", (("fits32", "-"), ("fits32", "-")), "scan_kernel"),
}


@functools.lru_cache(maxsize=None)
def cluster_cell(name):
    """KFVs of ONE window size, each with a base of its own (base_of's variants 1, 2, ...), and the range genome of all of them."""
    k, W, family, specs, kernel = CLUSTER_CELLS[name]
    nk = W - k + 1
    refs = []
    for j, spec in enumerate(specs):
        refs.append(ref_of(family, k, W, _cluster_N(spec, k, W, family, j + 1), j + 1))
    contigs, plants, names = range_genome(k, W, [r["base"] for r in refs])
    m = len(refs)
    S, Ns, KFVs, ws = [r["S"] for r in refs], [r["N"] for r in refs], [r["RV"] for r in refs], [W] * m
    _, oD = orc.omn_scan_int(contigs, S, Ns, k, ws, [1] * m, OMN_BUFF, OMN_GENOME_POS, return_D=True)
    thr_mid, thr_all, thr_low = [], [], []
    for j in range(m):
        dm = dmax(S[j], Ns[j], nk)
        assert int(oD[j].max()) == dm and int(oD[j].max()) - int(oD[j].min()) >= SPAN_SHARE * dm
        own = [bigint_D(contigs[r][s:s + W], S[j], Ns[j], k) for r, s, b in plants if b == j]
        mid, above, low = thresholds(own, bigint_D(contigs[0][-W:], S[j], Ns[j], k), k, Ns[j], S[j], nk)
        thr_mid.append(mid)
        thr_all.append(above)
        thr_low.append(low)
    return dict(k=k, W=W, ws=ws, S=S, N=Ns, KFVs=KFVs, contigs=contigs, plants=plants, thr=dict(mid=thr_mid, all=thr_all, low=thr_low),
                kernel=kernel)
