"""The strobemer kernel at the edges of its parameters, window sizes, counters and integer range: the references, genomes and
thresholds shared by test_strobe_cases.py (CPU) and test_gpu_strobe_edges.py.  Nothing here calls the library under test: every
expected value comes from tests/strobe_oracle.py, in Python integers.

A window of the strobemer scan holds n = W - k + 1 items: the nk = W - k randstrobes that slide and one permanent copy of the
record's randstrobe at 0-based position nk (tests/test_strobe_host.py).  Window w (1-based; 1 is the first window, never tested)
is the one after the reference's step i = w - 1 and holds the items at 0-based positions w - 1 .. w - 2 + nk.  strobe_kernel walks a
stream of windows 64 per step, lane = position mod 64 (streams start on multiples of 64).

Tables.  A family table is S = N count(base window): a window whose items are the base's has D = 0.  The DISCRIMINATING table
(disc_table) has N = 7 and a fixed pseudo-random S[x] in 1 .. 997 that differs between the two bins of a count dword (x, x ^ 1) and
between x and x >> 2s (the bin's own first strobe): under it a randstrobe counted in the wrong bin changes the distance, which
under a family table -- most bins 0 -- it need not.  Tables are passed as KFV = S / N with n_refs = N; takes_integer_form restates
the library's test for "is S / N".

Thresholds come from the oracle's exact D.  thr_between(lo, hi) lies half-way between two neighbouring values; thr_at(D) is the
largest Float64 whose exact product with 2 k N^2 is <= D, so that windows of exactly D are AT the threshold: not below it in exact
arithmetic, inside the library's 2^-30 guard band, and decided by rounding in the reference's Float64 loop.  band_free asserts that
no window lies in the lower half of the band, where the library (not below) and exact arithmetic (below) part by design.
"""
import functools
from fractions import Fraction

import numpy as np

from tests import range_cases as rc
from tests import strobe_oracle as so
from tests.helpers import mutate, random_dna

SEED = 9200
BUFF = 50
DISC_N = 7
FAMILY_N = 7
STREAM_WINDOWS = 2048                    # the library's stream length for a few thousand windows (its KGMA_GEOM_DEBUG line says)


def k_of(cfg):
    return cfg[2] + cfg[0] - 1


def hit_key(h):
    return (h["contig"], h["cmi"], h["lo"], h["hi"], h["genome_pos"], h["D"])


def _rng(*key):
    return np.random.default_rng([int(x) % (1 << 32) for x in key])


# ---- tables ---------------------------------------------------------------------------------------------------------------------------

def ref_of(S, N, cfg, W):
    S = np.asarray(S, dtype=np.int64)
    return dict(RV=S / float(N), W=W, S=S, N=N, cfg=tuple(cfg), k=k_of(cfg))


def takes_integer_form(ref):
    """The library's "is S / N": every entry times N within a relative 1e-14 of a non-negative integer, and that integer is S."""
    v = ref["RV"] * float(ref["N"])
    r = np.rint(v)
    return bool(np.all(np.abs(v - r) <= 1e-14 * np.maximum(1.0, np.abs(v))) and np.array_equal(r.astype(np.int64), ref["S"])
                and int(ref["S"].min()) >= 0 and int(ref["S"].max()) <= 2_000_000_000)


@functools.lru_cache(maxsize=None)
def disc_table(s):
    NB = 4 ** (2 * s)
    rng = _rng(SEED, 1, s)
    S = rng.integers(1, 998, size=NB)
    x = np.arange(NB)
    for _ in range(200):
        bad = (S == S[x ^ 1]) | ((S == S[x >> (2 * s)]) & (x != x >> (2 * s)))
        if not bad.any():
            break
        S[bad] = rng.integers(1, 998, size=int(bad.sum()))
    else:
        raise AssertionError("no discriminating table at s = %d" % s)
    S = S.astype(np.int64)
    S.setflags(write=False)
    return S


def family_table(base, cfg, N):
    return np.int64(N) * np.bincount(so.strobe_bins(base, *cfg), minlength=4 ** (2 * cfg[0])).astype(np.int64)


# ---- thresholds -----------------------------------------------------------------------------------------------------------------------

def scale_of(ref):
    return 2 * ref["k"] * ref["N"] ** 2


def int_T(thr, ref):
    """D < thr 2 k N^2  <=>  D < int_T (the oracle's own form)."""
    T = Fraction(thr) * scale_of(ref)
    return T.numerator // T.denominator + (1 if T.numerator % T.denominator else 0)


def thr_between(lo, hi, ref):
    assert lo < hi
    return (int(lo) + int(hi)) / 2.0 / scale_of(ref)


def thr_at(D, ref):
    thr = float(int(D)) / scale_of(ref)
    while Fraction(thr) * scale_of(ref) > D:
        thr = float(np.nextafter(thr, 0.0))
    assert int_T(thr, ref) == D
    return thr


def band_free(D, thr, ref):
    """No D in [floor(thr 2kN^2 (1 - 2^-30)), thr 2kN^2): the lower half of the library's guard band."""
    Tf = Fraction(thr) * scale_of(ref)
    lo = Tf * (1 - Fraction(1, 2 ** 30))
    lo = lo.numerator // lo.denominator
    D = np.asarray(D, dtype=np.int64)
    return not bool(np.any((D >= lo) & (D < int_T(thr, ref))))


# ---- the oracle, per record -------------------------------------------------------------------------------------------------------------

def oracle(seqs, ref, thr, dists=True):
    return so.scan(seqs, ref["RV"], ref["S"], ref["N"], *ref["cfg"], ref["W"], thr, BUFF, return_dists=dists)


def split_dists(seqs, W, flat):
    """The oracle's distances (one per step i >= 1, records in order) per record, int64."""
    out, at = [], 0
    for seq in seqs:
        n = max(len(seq) - W - 1, 0) if len(seq) >= W else 0
        out.append(np.asarray(flat[at:at + n], dtype=np.int64))
        at += n
    assert at == len(flat)
    return out


def expected_dips(D1, Dsteps, T, W, N):
    """The dips of one record from its exact distances: maximal runs of windows w >= 2 with D < T, as dict(start, end, argmin, last_min,
    nmin, D_min, exit_pos, D_exit, tie).  tie: the minimum is attained more than once (N is no power of two here: a plateau counts), or
    equals the running minimum an earlier dip left behind (the reference's state machine, StrobeGenomeMiner.jl:73-90)."""
    assert N & (N - 1)
    D = [int(x) for x in Dsteps]
    nwin = len(D) + 1
    dips, w = [], 2
    while w <= nwin:
        if D[w - 2] >= T:
            w += 1
            continue
        e = w
        while e + 1 <= nwin and D[e - 1] < T:
            e += 1
        run = D[w - 2:e - 1]
        m = min(run)
        at = [w + j for j, x in enumerate(run) if x == m]
        dips.append(dict(start=w, end=e, argmin=at[0], last_min=at[-1], nmin=len(at), D_min=m, exit_pos=e + 1 if e + 1 <= nwin else 0,
                         D_exit=D[e - 1] if e + 1 <= nwin else 0))
        w = e + 1
    currmin, stop, cmi, goal = int(D1), True, 2, 0
    for d in dips:
        d["tie"] = d["nmin"] > 1
        if d["D_min"] < currmin:
            currmin, cmi, stop = d["D_min"], d["argmin"] - 1, False
        elif d["D_min"] == currmin:
            d["tie"] = True
        if d["exit_pos"] and not stop:
            stop = True
            cmi += 1
            if cmi > goal:
                goal, currmin = cmi + W - 1, d["D_exit"]
    return dips


# ---- 2. randstrobe selection at the edges of its parameters -----------------------------------------------------------------------------
# (s, w_min, w_max, q), the sums at which a CHOSEN second strobe must score 0 (one per `zero` word the set is listed for), and the
# first seed from SELECT_SEED0 on whose genome meets select_conditions (test_strobe_cases.py checks that it is the first).
SELECT_SEED0 = 0
SELECT_SETS = [
    ((3, 1, 14, 33), (0, 33, 66, 99), 0),
    ((3, 4, 7, 97), (0, 97), 0),
    ((3, 12, 14, 126), (126,), 0),
    ((3, 14, 14, 5), (), 0),
    ((3, 4, 7, 2 ** 40), (0,), 0),
    ((2, 3, 5, 30), (30,), 0),
    ((2, 3, 5, 31), (0,), 0),
    ((2, 1, 15, 2), (), 0),
    ((2, 2, 2, 1), (), 0),
    ((1, 1, 16, 2), (), 0),
    ((1, 1, 1, 1), (), 0),
]
SELECT_NK = 40
HOMOPOLYMER = 25                         # longer than any k <= 16


def select_genome(seed):
    """About 7 kb in four records: a run of N behind "GA" (a first strobe of even value followed by odd ones only: offset 1 wins at
    q = 2), a lower-case stretch, a homopolymer of each residue."""
    rng = _rng(SEED, 2, seed)
    a = bytearray(random_dna(rng, 2500))
    a[698:700] = b"GA"
    a[700:760] = b"N" * 60
    a[1200:1300] = bytes(a[1200:1300]).lower()
    a[1700:1700 + HOMOPOLYMER] = b"A" * HOMOPOLYMER
    b = bytearray(random_dna(rng, 1800))
    b[300:300 + HOMOPOLYMER] = b"C" * HOMOPOLYMER
    b[900:900 + HOMOPOLYMER] = b"G" * HOMOPOLYMER
    c = bytearray(random_dna(rng, 1700))
    c[500:500 + HOMOPOLYMER] = b"T" * HOMOPOLYMER
    c[1000:1040] = b"n" * 40
    return [bytes(a), bytes(b), bytes(c), random_dna(rng, 1000)]


def select_facts(cfg, seqs):
    """What the parameter set does on the genome: the offsets chosen, the sums at which a chosen second strobe scored 0."""
    s, q = cfg[0], cfg[3]
    offsets, sums = set(), set()
    for seq in seqs:
        bins, off = so.strobe_bins_offsets(seq, *cfg)
        tot = (bins >> (2 * s)) + (bins & (4 ** s - 1))
        offsets |= set(np.unique(off).tolist())
        sums |= set(np.unique(tot[tot % q == 0]).tolist())
    return dict(offsets=offsets, sums=sums)


def select_conditions(cfg, sums, facts):
    s, w_min, w_max, q = cfg
    ok = set(sums) <= facts["sums"]
    if w_min < w_max:
        ok = ok and len(facts["offsets"]) >= 3 and {w_min, w_max} <= facts["offsets"]
    if cfg == (3, 1, 14, 33):
        ok = ok and 1 in facts["offsets"]
    return ok


def first_select_seed(cfg, sums, limit=400):
    for seed in range(SELECT_SEED0, SELECT_SEED0 + limit):
        if select_conditions(cfg, sums, select_facts(cfg, select_genome(seed))):
            return seed
    raise AssertionError("no seed meets the conditions of %s" % (cfg,))


@functools.lru_cache(maxsize=None)
def select_cell(cfg):
    sums, seed = next((u, sd) for c, u, sd in SELECT_SETS if c == cfg)
    seqs = select_genome(seed)
    ref = ref_of(disc_table(cfg[0]), DISC_N, cfg, k_of(cfg) + SELECT_NK)
    o = oracle(seqs, ref, 0.0)
    return dict(cfg=cfg, sums=sums, seed=seed, seqs=seqs, ref=ref, first_D=o["first_D"], D=np.asarray(o["dists_exact"], dtype=np.int64),
                n_hits=len(o["exact"]))


# ---- 3. short windows -------------------------------------------------------------------------------------------------------------------
SHORT_NKS = (1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65, 66, 127, 128, 129)
SHORT_CFGS = ((1, 2, 4, 5), (2, 3, 5, 5), (3, 4, 7, 5))
SHORT_EXTRA = ((1, 1, 16, 2), (1, 63, 64, 65))
SHORT_SEEDS = 60
TANDEM_UNIT = 7
DENSE_TARGET = 0.05


def short_cells():
    return [(cfg, nk) for cfg in SHORT_CFGS for nk in SHORT_NKS] + [(SHORT_EXTRA[0], nk) for nk in SHORT_EXTRA[1]]


def _copy(rng, base, rate):
    """base mutated at `rate`, with one substitution at the least."""
    if rate == 0.0:
        return base
    out = bytearray(mutate(rng, base, rate))
    if bytes(out) == base:
        p = int(rng.integers(0, len(out)))
        out[p] = b"ACGT"[(b"ACGT".index(out[p]) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(out)


def short_genome(cfg, nk, seed):
    """(seqs, base, long, plants).  Record `long` has the base window's last k residues at position nk, behind nk random ones: its
    permanent item is the base's last randstrobe, so its exact copies reach D = 0 (elsewhere a copy bottoms out at 2 N^2: the
    permanent item is another record's), while its first window -- the running minimum's start -- does not; it holds copies
    at 0 % (two), 3 % and 8 %, a tandem stretch of period TANDEM_UNIT (a bin that enters a window leaves one again a few lanes on in the same
    64-window step), a run of N and a lower-case stretch.  Around it: records of W - 1, W, W + 1, W + 2 and k residues and four
    records with a copy in the middle.  plants: (record, 0-based start, rate)."""
    k = k_of(cfg)
    W = nk + k
    rng = _rng(SEED, 3, seed, cfg[0], cfg[1], cfg[2], nk)
    base = random_dna(rng, W)
    a, plants, long = bytearray(random_dna(rng, nk) + base[nk:]), [], 1
    for rate in (0.0, 0.03, 0.0, 0.08):
        a += random_dna(rng, 300 + W)
        plants.append((long, len(a), rate))
        a += _copy(rng, base, rate)
    a += random_dna(rng, 300)
    a += random_dna(rng, TANDEM_UNIT) * ((nk + 260) // TANDEM_UNIT)
    a += random_dna(rng, 300) + b"N" * 25 + b"n" * 15 + random_dna(rng, 100)
    lc = len(a)
    a += random_dna(rng, 250)
    a[lc:lc + 50] = bytes(a[lc:lc + 50]).lower()
    seqs = [random_dna(rng, W - 1), bytes(a), random_dna(rng, W), random_dna(rng, W + 1), random_dna(rng, W + 2), random_dna(rng, k)]
    for j, rate in enumerate((0.0, 0.03, 0.0, 0.08)):
        left = 60 + j
        seqs.append(random_dna(rng, left) + _copy(rng, base, rate) + random_dna(rng, 60 + W))
        plants.append((len(seqs) - 1, left, rate))
    return seqs, base, long, plants


def enters_and_leaves_in_step(bins, nk):
    """Is there a 64-position step of the record's stream in which a bin is entered by one lane and left by a higher one?  (An item
    enters at its position p and leaves at p + nk; nothing happens where the entering and the leaving bin are the same.)"""
    bins = [int(x) for x in bins]
    for b0 in range(0, len(bins), 64):
        entered = {}
        for p in range(b0, min(b0 + 64, len(bins))):
            if p >= nk and bins[p] == bins[p - nk]:
                continue
            if p >= nk and bins[p - nk] in entered and entered[bins[p - nk]] < p:
                return True
            entered.setdefault(bins[p], p)
    return False


def _share_below(Dsorted, v):
    return np.searchsorted(Dsorted, v, side="left") / Dsorted.size


@functools.lru_cache(maxsize=None)
def short_cell(cfg, nk):
    """What the tests of one cell share.  Two thresholds: `sparse`, half-way above the smallest distance of the 3 % copy of the long
    record (stepped down while more than half of the windows would lie below); `dense`, AT the value of D that puts the share of
    windows below it nearest to 5 % (above 0, at most 50 %).  The first seed whose exact oracle gives two hits at both is taken."""
    k = k_of(cfg)
    W = nk + k
    last = None
    for seed in range(SHORT_SEEDS):
        seqs, base, long, plants = short_genome(cfg, nk, seed)
        ref = ref_of(family_table(base, cfg, FAMILY_N), FAMILY_N, cfg, W)
        o0 = oracle(seqs, ref, 0.0)
        per = split_dists(seqs, W, o0["dists_exact"])
        Dall = np.sort(np.concatenate(per))
        vals = np.unique(Dall)
        if vals.size < 2:
            last = "one distance only"
            continue
        at = next(p for r, p, rate in plants if r == long and rate == 0.03)
        j = int(np.searchsorted(vals, per[long][max(at - 3, 0):at + 3].min()))
        j = min(j, vals.size - 2)
        while j > 0 and _share_below(Dall, vals[j + 1]) > 0.5:
            j -= 1
        cand = [v for v in vals[1:] if _share_below(Dall, v) <= 0.5]
        if not cand:
            last = "no dense cut"
            continue
        dense = int(min(cand, key=lambda v: abs(_share_below(Dall, v) - DENSE_TARGET)))
        thr = dict(sparse=thr_between(vals[j], vals[j + 1], ref), dense=thr_at(dense, ref))
        orc = {name: oracle(seqs, ref, t) for name, t in thr.items()}
        n_hits = {name: len(x["exact"]) for name, x in orc.items()}
        bins = so.strobe_bins(seqs[long], *cfg)
        facts = dict(n_hits=n_hits, skipped=sum(1 for d in o0["first_D"] if d == -1), zero=int(Dall[0]) == 0,
                     in_step=enters_and_leaves_in_step(bins, nk), at_threshold=int(np.count_nonzero(Dall == dense)),
                     band_free=all(band_free(Dall, t, ref) for t in thr.values()))
        if min(n_hits.values()) >= 2 and facts["skipped"] >= 1 and facts["in_step"] and facts["zero"] and facts["band_free"]:
            return dict(cfg=cfg, nk=nk, W=W, seed=seed, seqs=seqs, ref=ref, long=long, plants=plants, thr=thr, oracle=orc, per=per,
                        dense_D=dense, **facts)
        last = facts
    raise AssertionError("%s nk %d: no seed meets the conditions (last: %s)" % (cfg, nk, last))


# ---- 4. streams that are not a record's first -------------------------------------------------------------------------------------------
STREAMS_CFG = (3, 4, 7, 5)
STREAMS_NKS = (2, 65)
STREAMS_MIN_WINDOWS = 6300


def streams_genome(nk, P, seed):
    """One record of max(6300, 3 P + 300) windows and a short one.  The base window has period nk (base = u + u[:k], |u| = nk): its
    last randstrobe is its first again, so the two windows over a copy -- starts a + 1 and a + 2 for a copy at residue a -- hold the
    same items: a tie of exactly two.  Copies at residue t P - 2 (t = 1, 3: the tie just before the boundary between windows t P and
    t P + 1, the run of sub-threshold windows going on beyond it) and at 2 P - 1 (the tie ON the boundary: the last window of one
    stream and the first of the next)."""
    k = k_of(STREAMS_CFG)
    W = nk + k
    rng = _rng(SEED, 4, seed, nk, P)
    u = random_dna(rng, nk)
    base = (u * (k // nk + 2))[:W]
    nwin = max(STREAMS_MIN_WINDOWS, 3 * P + 300)
    a = bytearray(random_dna(rng, nwin + W))                          # a record of L residues has L - W windows
    for t, at in ((1, P - 2), (2, 2 * P - 1), (3, 3 * P - 2)):
        a[at:at + W] = base
    return [bytes(a), random_dna(rng, W + 100)], base


@functools.lru_cache(maxsize=None)
def streams_cell(nk, P=STREAM_WINDOWS):
    """Threshold: half-way above the distance of window P + 1, which holds all but one of the first copy's items."""
    cfg = STREAMS_CFG
    W = nk + k_of(cfg)
    last = None
    for seed in range(SHORT_SEEDS):
        seqs, base = streams_genome(nk, P, seed)
        ref = ref_of(family_table(base, cfg, FAMILY_N), FAMILY_N, cfg, W)
        o0 = oracle(seqs, ref, 0.0)
        per = split_dists(seqs, W, o0["dists_exact"])
        D = per[0]                                                        # D[w - 2]: window w
        vals = np.unique(np.concatenate(per))
        j = int(np.searchsorted(vals, max(int(D[t * P + 1 - 2]) for t in (1, 3))))
        if j + 1 >= vals.size:
            last = "the windows beyond the boundaries are at the largest distance"
            continue
        thr = thr_between(vals[j], vals[j + 1], ref)
        T = int_T(thr, ref)
        o = oracle(seqs, ref, thr)
        dips = [expected_dips(o["first_D"][r], per[r], T, W, ref["N"]) for r in range(len(seqs))]
        straddle = {t: next((d for d in dips[0] if d["start"] <= t * P and d["end"] >= t * P + 1), None) for t in (1, 2, 3)}
        tie = straddle[2]
        facts = dict(n_hits=len(o["exact"]), straddles=all(d is not None for d in straddle.values()),
                     tie_on_boundary=bool(tie and tie["argmin"] == 2 * P and tie["last_min"] == 2 * P + 1 and tie["nmin"] == 2),
                     band_free=band_free(np.concatenate(per), thr, ref), share=float(np.count_nonzero(D < T)) / D.size)
        if facts["n_hits"] >= 3 and facts["straddles"] and facts["tie_on_boundary"] and facts["band_free"] and facts["share"] < 0.2:
            return dict(cfg=cfg, nk=nk, W=W, P=P, seed=seed, seqs=seqs, ref=ref, thr=thr, T=T, oracle=o, per=per, dips=dips, straddle=straddle,
                        **facts)
        last = facts
    raise AssertionError("streams nk %d P %d: no seed meets the conditions (last: %s)" % (nk, P, last))


# ---- 5. the top of the 16-bit counters; 6. the ends of the integer range -----------------------------------------------------------------
TOP_N_ITEMS = 65_535
TOP_CFGS = ((2, 3, 5, 5), (3, 4, 7, 5), (1, 2, 4, 5))
TOP_RUN_EXTRA, TOP_TAIL, TOP_S1 = 200, 400, 3                             # S[1] = 3 N


@functools.lru_cache(maxsize=None)
def _top_genome(cfg):
    """A x (W + 200), a base window over C, G, T, 400 random residues: the permanent item is bin 0 and the windows of the leading run
    hold 65 535 copies of it (the whole low half-word of the dword whose high half-word counts bin 1).  The first seed is taken for
    which bin 1 -- a first strobe of A only, a second one ending in C -- is entered or left while bin 0 still counts 65 535 - 64 or
    more; the counts of the base window with S[1] = 3 per reference are the table's shape."""
    k = k_of(cfg)
    nk = TOP_N_ITEMS - 1
    W = nk + k
    for seed in range(SHORT_SEEDS):
        rng = _rng(SEED, 5, seed, cfg[0])
        base = np.frombuffer(b"CGT", dtype=np.uint8)[rng.integers(0, 3, size=W)].tobytes()
        seq = b"A" * (W + TOP_RUN_EXTRA) + base + random_dna(rng, TOP_TAIL)
        bins = so.strobe_bins(seq, *cfg)
        zeros = np.concatenate([[0], np.cumsum(bins == 0)])
        best = 0
        for p in np.flatnonzero(bins == 1).tolist():                       # enters at step i = p - nk + 1, leaves at step p + 1
            for i in (p - nk + 1, p + 1):
                if 1 <= i < len(seq) - W:                                 # the window before step i: items i - 1 .. i - 2 + nk, and bin 0
                    best = max(best, int(zeros[i - 1 + nk] - zeros[i - 1]) + 1)
        if best >= TOP_N_ITEMS - 64:
            shape = np.bincount(so.strobe_bins(base, *cfg), minlength=4 ** (2 * cfg[0])).astype(np.int64)
            assert shape[0] == 0 and shape[1] == 0 and int(shape.sum()) == TOP_N_ITEMS
            shape[1] = TOP_S1
            return dict(seed=seed, seq=seq, base=base, shape=shape, W=W, nk=nk, at=W + TOP_RUN_EXTRA, bin0_at_bin1=best)
    raise AssertionError("%s: no seed puts bin 1 next to a full bin 0" % (cfg,))


def top_dmax(cfg, N):
    return rc.dmax(_top_genome(cfg)["shape"] * np.int64(N), N, TOP_N_ITEMS)


def top_edge_N(cfg):
    """(edge-, edge+) of sum S^2 + N^2 n^2 < 2^61 for the table of top_cell at n = 65 535 items."""
    shape = _top_genome(cfg)["shape"]
    return rc.bisect_edge(lambda N: rc.d61(shape * np.int64(N), N, TOP_N_ITEMS))


@functools.lru_cache(maxsize=None)
def top_cell(cfg, N=FAMILY_N):
    """Threshold: N below the distance of the window 200 steps past the base window (off the lattice of D, whose steps are multiples
    of 2 N), so that the dip around the base window closes inside the record."""
    g = _top_genome(cfg)
    ref = ref_of(g["shape"] * np.int64(N), N, cfg, g["W"])
    seqs = [g["seq"]]
    o0 = oracle(seqs, ref, 0.0)
    D = np.asarray(o0["dists_exact"], dtype=np.int64)
    thr = float(int(D[g["at"] + 200 - 1]) - N) / scale_of(ref)
    o = oracle(seqs, ref, thr)
    dm = rc.dmax(ref["S"], N, TOP_N_ITEMS)
    return dict(cfg=cfg, N=N, W=g["W"], seqs=seqs, ref=ref, thr=thr, oracle=o, D=D, first_D=o0["first_D"], dmax=dm, at=g["at"],
                bin0_at_bin1=g["bin0_at_bin1"], band_free=band_free(D, thr, ref))


ENTRY_CFG = (2, 3, 5, 5)
ENTRY_BIN = 0x6C                                                          # first strobe CG, second TA


def entry_edge():
    """The largest S with S^2 + N^2 n^2 < 2^61 at N = 1, n = 2, and that S + 1."""
    return rc.bisect_edge(lambda S: S * S + 4 < 2 ** 61)


@functools.lru_cache(maxsize=None)
def entry_cell():
    """n = 2 items (W = k + 1), N = 1, one bin with the largest S the int64 range admits: D = S^2 + 2, + 4 and + 6 without the bin
    (the sliding and the permanent item apart or in one bin), (S - 1)^2 + 1 with one copy, (S - 2)^2 with two.  The genome plants
    the bin's randstrobe, CGxxTA with no score of 0 at offsets 4 and 5, singly and (a record that has it at position nk = 1) as both
    items.  Threshold: an eighth of the way down from one copy to two -- the guard band reaches 2^-30 of 2^61 = 2.15e9
    below the threshold and D moves by 2 S = 3.04e9 per copy, so one copy is above the threshold and two are clear of the band."""
    cfg = ENTRY_CFG
    k = k_of(cfg)
    W = k + 1
    S_lo, S_hi = entry_edge()
    S = np.zeros(4 ** (2 * cfg[0]), dtype=np.int64)
    S[ENTRY_BIN] = S_lo
    ref = ref_of(S, 1, cfg, W)
    for seed in range(SHORT_SEEDS):
        rng = _rng(SEED, 6, seed)
        unit = b"CGTATA"                                                  # CG + TA at offset 3; offsets 4, 5 (AT, TA): sums 9, 18
        a = bytearray(random_dna(rng, 900))
        for at in (100, 300, 500, 700):
            a[at:at + 12] = unit + unit
        b = bytearray(random_dna(rng, 400))
        b[0:18] = b"T" + unit + unit + b"GGGGG"                           # position 1: the bin is this record's permanent item
        b[200:212] = unit + unit
        seqs = [bytes(a), bytes(b), random_dna(rng, W), random_dna(rng, W - 1)]
        if int(so.strobe_bins(seqs[1], *cfg)[1]) != ENTRY_BIN:
            continue
        o0 = oracle(seqs, ref, 0.0)
        D = np.asarray(o0["dists_exact"], dtype=np.int64)
        one, two = (S_lo - 1) ** 2 + 1, (S_lo - 2) ** 2
        if not (np.any(D == one) and np.any(D == two)):
            continue
        thr = float(one - (one - two) // 8) / scale_of(ref)
        o = oracle(seqs, ref, thr)
        if len(o["exact"]) >= 1 and band_free(D, thr, ref):
            return dict(cfg=cfg, W=W, seqs=seqs, ref=ref, thr=thr, oracle=o, D=D, first_D=o0["first_D"], dmax=S_lo * S_lo + 4, S_lo=S_lo,
                        S_hi=S_hi, one=one, two=two)
    raise AssertionError("no seed gives the entry cell its windows")
