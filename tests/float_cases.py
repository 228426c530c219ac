"""General Float64 KFVs over the range kgma_set_refs accepts, for the Float64 form of the generic kernel and the generic chain
kernel.  Everything is seeded and small: five records per case (5000 residues, 3000, 600, exactly W, and W + 300).

A case is a dict: name, kind, k, W, nk (k-mers per window), records, kfv (dense: 4^k Float64; k >= 11: (keys, values) of its
non-zero entries), env (the switches the case runs under, on top of KGMA_KERNEL=generic / KGMA_CHAIN_GENERIC=1), cmode (where the
kernel keeps its counts under that env: tests/hash_model.py, geometry), base (the planted sequence), mut_at / exact_at (0-based
start of the planted mutated / exact copy in record 0) and refused (the KFV lies beyond the magnitude limit: no scan).

Records.  Record 0: a mutated copy of the base at 700 and an exact copy at 2050 -- the third window of the record's second stream
(streams hold at least 2048 windows).  Record 1: a poly-A run of W + 150 residues (plateaus of zero increments, pairs =
n (n - 1) / 2) and a run of 130 N.  Records 2 and 3: 600 and W residues.  Record 4 begins with the exact copy: the record's first
window, which no scan tests but kgma_get_first_window reports, and a stream -- of the scan and of the chain -- whose first distance
is noise.  (The device chain vouches for its binade decisions by comparing its value with the exact distance at every stream
start, relative to that distance; where that distance is noise it declines, a scan falls back to the host chain and
kgma_chain_values, which has no fallback, returns KGMA_E_UNSUPPORTED: seen on the device with the copy at window 2048 of record 0.)

KFV kinds:
  signed       log-odds-like, uniform in [-3, 3] (k = 8: on the k-mers of the records, 0 elsewhere; k = 11: sparse)
  wide         +-10^U(-8, 4), three entries -0.0, four 0.0, two subnormal
  nearcount    the k-mer counts of the base + 1e-9 U(-1, 1): the exact distance at the exact copy is ~1e-18 x entries, far below
               the rounding noise of any Float64 evaluation -- the computed value there is noise of either sign
  nearcount12  the same with noise 1e-12
  absorb       entries in [0, 2] and three of 5e8 + U(1, 31) on k-mers of the records (T...T, which the N run spells, among them):
               distances of ~7.5e17 / 2k whose ulp exceeds twice an ordinary increment.  (Three entries of 1e9 have sum ref^2 =
               3e18 > 2^61: kgma_set_refs refuses them.  And not 5e8 itself: that is a float32 number, and the case has to notice
               a table rounded to float32.)
  limit        the same with the three large entries at X, X - 1.5, X - 3 and X such that the magnitude kgma_set_refs tests,
               sum ref^2 + n^2 + 2 n max|ref| + 1, is 0.995 x 2^61: accepted, on a lattice of 2k (N = 1)
  over         ... 1.005 x 2^61: refused

Cells (k, W, env -> cmode): every kind at k = 3 and k = 6 / W = 305, signed and nearcount elsewhere."""
import functools
from fractions import Fraction

import numpy as np

from tests import float_exact as fx
from tests import hash_model as hm
from tests.helpers import kmer_values, mutate, random_dna

SEED = 9300
MUT_AT, EXACT_AT = 700, 2050
ALL_KINDS = ("signed", "wide", "nearcount", "nearcount12", "absorb", "limit", "over")
TWO_KINDS = ("signed", "nearcount")
CELLS = [  # (tag, k, W, env, kinds)
    ("k1-w40", 1, 40, {}, TWO_KINDS),
    ("k3-w50", 3, 50, {}, ALL_KINDS),
    ("k6-w305", 6, 305, {}, ALL_KINDS),
    ("k7-w120", 7, 120, {}, TWO_KINDS),
    ("k8-w300", 8, 300, {}, TWO_KINDS),
    ("k8-w300-global", 8, 300, {"KGMA_GENERIC_HASH": "0"}, TWO_KINDS),
    ("k11-w200", 11, 200, {}, TWO_KINDS),
    ("k11-w200-global", 11, 200, {"KGMA_WIDE_LDS_NK": "0"}, TWO_KINDS),
    ("k6-w40", 6, 40, {}, TWO_KINDS),
]
CMODE = {"k1-w40": 5, "k3-w50": 0, "k6-w305": 0, "k7-w120": 0, "k8-w300": 2, "k8-w300-global": 1, "k11-w200": 3, "k11-w200-global": 4,
         "k6-w40": 0}
LIMIT_FRACTION = {"limit": Fraction(995, 1000), "over": Fraction(1005, 1000)}
NOISE = {"nearcount": 1e-9, "nearcount12": 1e-12}


@functools.lru_cache(maxsize=None)
def _genome(k, W):
    rng = np.random.default_rng([SEED, k, W])
    base = random_dna(rng, W)
    r0 = bytearray(random_dna(rng, 5000))
    r0[MUT_AT:MUT_AT + W] = mutate(rng, base, 0.06)
    r0[EXACT_AT:EXACT_AT + W] = base
    r1 = bytearray(random_dna(rng, 3000))
    r1[400:400 + W + 150] = b"A" * (W + 150)
    r1[1500:1630] = b"N" * 130
    return base, (bytes(r0), bytes(r1), random_dna(rng, 600), random_dna(rng, W), base + random_dna(rng, 300))


def large_keys(k, W):
    """The three k-mers of the records that carry the large entries of absorb / limit / over: T...T (the N run), one of record 0
    and one of record 2."""
    _, recs = _genome(k, W)
    out = [4 ** k - 1]
    for seq, at in ((recs[0], 1200), (recs[2], 100)):
        km = kmer_values(seq, k).tolist()
        out.append(next(x for x in km[at:] if x not in out))
    return out


def limit_sum(kfv, nk) -> Fraction:
    """sum ref^2 + n^2 + 2 n max|ref| + 1 of a dense KFV, exactly: the magnitude kgma_set_refs holds below 2^61."""
    R = [Fraction(float(v)) for v in kfv]
    return sum((r * r for r in R), Fraction(0)) + nk * nk + 2 * nk * max(abs(r) for r in R) + 1


@functools.lru_cache(maxsize=None)
def _kfv(kind, k, W):
    rng = np.random.default_rng([SEED + 1, k, W, ALL_KINDS.index(kind)])
    base, recs = _genome(k, W)
    nk = W - k + 1
    if k >= hm.WIDE_MIN_K:                                          # sparse: the base's k-mers, k-mers of the records, absent ones
        parts = [kmer_values(base, k), kmer_values(recs[0][1000:1200], k), kmer_values(recs[2][:100], k), rng.integers(0, 4 ** k, size=40)]
        keys = np.unique(np.concatenate(parts))
        if kind == "signed":
            vals = rng.uniform(-3.0, 3.0, keys.size)
        else:
            cnt = dict(zip(*np.unique(kmer_values(base, k), return_counts=True)))
            vals = np.asarray([cnt.get(x, 0) for x in keys.tolist()], dtype=np.float64) + NOISE[kind] * rng.uniform(-1.0, 1.0, keys.size)
        assert np.all(vals != 0.0)
        return keys.astype(np.uint32), vals
    NB = 4 ** k
    if kind == "signed":
        v = rng.uniform(-3.0, 3.0, NB)
        if k >= 8:
            # (a profile's table: entries on the k-mers of the records -- some 9000 of 65536 -- and 0 elsewhere.  The bound's first
            #  term is (P + 5) u sum ref^2 / 4k: with all 4^8 entries set it is too wide to tell a float32 table from this one,
            #  tests/test_float_cases.py: test_bound_notices_wrong_inputs)
            keep = np.zeros(NB, dtype=bool)
            for seq in recs:
                keep[kmer_values(seq, k)] = True
            v[~keep] = 0.0
        return v
    if kind == "wide":
        v = rng.choice([-1.0, 1.0], NB) * 10.0 ** rng.uniform(-8.0, 4.0, NB)
        at = rng.choice(NB, size=9, replace=False)
        v[at[:3]] = -0.0
        v[at[3:7]] = 0.0
        v[at[7]] = 5e-324
        v[at[8]] = -2.5e-310
        return v
    if kind in NOISE:
        return np.bincount(kmer_values(base, k), minlength=NB).astype(np.float64) + NOISE[kind] * rng.uniform(-1.0, 1.0, NB)
    v = rng.uniform(0.0, 2.0, NB)
    big = large_keys(k, W)
    if kind == "absorb":
        v[big] = 5e8 + rng.uniform(1.0, 31.0, 3)
        return v
    # limit / over: 3 X^2 + 2 n X ~ fraction x 2^61 - (the rest); the host test holds the exact sum to its side of 2^61
    v[big] = 0.0
    rest = float(np.sum(v * v)) + float(nk) * nk + 1.0
    target = float(LIMIT_FRACTION[kind]) * 2.0 ** 61 - rest
    X = (-2.0 * nk + np.sqrt(4.0 * nk * nk + 12.0 * target)) / 6.0
    v[big] = [X, X - 1.5, X - 3.0]
    return v


def _case(tag, k, W, env, kind):
    base, recs = _genome(k, W)
    return dict(name=f"{kind}-{tag}", kind=kind, cell=tag, k=k, W=W, nk=W - k + 1, records=list(recs), kfv=_kfv(kind, k, W), env=dict(env),
                cmode=CMODE[tag], base=base, mut_at=MUT_AT, exact_at=EXACT_AT, refused=kind == "over")


@functools.lru_cache(maxsize=None)
def cases():
    out = [_case(tag, k, W, env, kind) for tag, k, W, env, kinds in CELLS for kind in kinds]
    for c in out:
        assert c["cmode"] == hm.geometry(c["k"], c["nk"], c["env"])[0], c["name"]
    return out


NAMES = [f"{kind}-{tag}" for tag, _, _, _, kinds in CELLS for kind in kinds]
SCAN_NAMES = [n for n in NAMES if not n.startswith("over-")]
OVER_NAMES = [n for n in NAMES if n.startswith("over-")]
NEARCOUNT_NAMES = [n for n in NAMES if n.startswith("nearcount")]
STREAM_1024_NAMES = [n for n in SCAN_NAMES if n.endswith(("-k3-w50", "-k6-w305", "-k8-w300", "-k11-w200"))]


def case(name):
    return next(c for c in cases() if c["name"] == name)


def is_sparse(c):
    return isinstance(c["kfv"], tuple)


def dense_of(c):
    """The case's KFV as {k-mer: float} of its non-zero entries (both forms)."""
    if is_sparse(c):
        return dict(zip(c["kfv"][0].tolist(), c["kfv"][1].tolist()))
    return {x: v for x, v in enumerate(c["kfv"].tolist()) if v != 0.0}


# ---- the exact reference, once per (kind, k, W) ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(kind, k, W):
    _, recs = _genome(k, W)
    kfv = _kfv(kind, k, W)
    R = fx.entries(kfv)
    return tuple(fx.scan(seq, kfv, k, W, R=R) for seq in recs)


def reference(c):
    """Per record the float_exact.Record of its windows (shared by every test that needs it; nobody writes to it)."""
    return _reference(c["kind"], c["k"], c["W"])


# ---- the reference's running Float64 value (the C oracle) ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_chain(kind, k, W):
    from oracle import oracle as orc
    _, recs = _genome(k, W)
    kfv = _kfv(kind, k, W)
    out = []
    for seq in recs:
        if isinstance(kfv, tuple):
            _, od = orc.single_scan_sparse([seq], kfv, k, W, 0.0, 50, return_dists=True)
            d1 = orc.kmer_dist_kfv_sparse(seq[:W], kfv, k)
        else:
            _, od = orc.single_scan([seq], kfv, k, W, 0.0, 50, return_dists=True)
            d1 = orc.kmer_dist_kfv(seq[:W], kfv, k)
        v = np.concatenate([[d1], od])
        v.setflags(write=False)
        out.append(v)
    return tuple(out)


def oracle_chain(c):
    """Per record the oracle's value at every window: the first window's direct distance, then the rolling chain."""
    return _oracle_chain(c["kind"], c["k"], c["W"])


def oracle_hits(c, thr, buff=50):
    from oracle import oracle as orc
    if is_sparse(c):
        return orc.single_scan_sparse(c["records"], c["kfv"], c["k"], c["W"], thr, buff)[0]
    return orc.single_scan(c["records"], c["kfv"], c["k"], c["W"], thr, buff)[0]


# ---- thresholds -------------------------------------------------------------------------------------------------------------------
def thr_mid(c) -> float:
    """The exact distance half way between the mutated copy's minimum and the median window."""
    ref = reference(c)
    W = c["W"]
    near = ref[0].exact[max(0, c["mut_at"] - W // 2):c["mut_at"] + W // 2 + 1]
    every = sorted(x for r in ref for x in r.exact)
    return float((min(near) + every[len(every) // 2]) / 2)


THR_AT_WINDOW = (0, 100)      # (record, 0-based window): thr_at is the device's distance there


def oracle_drift(c, thr) -> Fraction:
    """max |chain - exact| / max(exact, thr) over every window: what the chain replay's drift policy sees of the oracle."""
    worst = Fraction(0)
    t = Fraction(thr)
    for r, v in zip(reference(c), oracle_chain(c)):
        for e, x in zip(r.exact, v.tolist()):
            worst = max(worst, abs(Fraction(x) - e) / max(e, t))
    return worst
