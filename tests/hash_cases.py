"""Inputs computed to collide in the generic kernel's hash tables (tests/hash_model.py restates the tables; the hash is
home = (key * 2654435761) >> hshift on the device key).  Everything is seeded and small: records of at most 12 kb.

A case is a dict: name, family, k, nk (k-mers per window), ws, records, ref (the S/N KFV as the parity helpers take it: dense RV / S
at k <= 10, keys / vals / S at k >= 11), fref (a general Float64 KFV: the same entries perturbed; one case per family has one),
thr, env (the experiment switches the case runs under) and the floors its family has to reach in the model.

Families:
  long        records whose k-mers' homes fall, as often as a lookahead can arrange, into a narrow range of buckets that straddles the
              table's end: long probe paths that run from the last bucket round to bucket 0 (and many lanes of a step on one free
              entry: the contention cases are long-path records held to that floor)
  tomb        two such families A and B in the same buckets laid out A B A, and repeats with a period a little above / below n
  count       k = 10, n = 1983: a homopolymer run entered from a colliding region (key 0 lives in bucket 0, inside the cluster)
  limit       k = 11, n = 2048: a step that needs more than 8 x buckets iterations of the probe loop, the limit before it was derived
  rebuild     long-path records under KGMA_HASH_REBUILD = 1 / 7 and KGMA_HASH_LOG2M = 13, and a planted gene across a rebuild step
  short       n = 2, 33, 63 on colliding k-mers
  sparse      KFVs whose device keys share a home slot of the sparse KFV table (chains of 8 and 40, one past the last slot), 32 / 33
              entries, absent k-mers inside a chain, key 0 and 4^k - 1 inside a chain
"""
import functools
from collections import Counter

import numpy as np

from tests import hash_model as hm
from tests.helpers import kmer_values

SEED = 9100
N_REFS = 7
LETTERS = b"ACGT"


# ---- colliding sequence -------------------------------------------------------------------------------------------------------
def colliding_sequence(k, log2m, length, seed, share, look, avoid=frozenset(), centre=0):
    """`length` residues whose k-mers' home buckets (table of 2^log2m entries) fall into the buckets/share buckets around `centre`
    (default: astride the table's end) as often as a lookahead of `look` residues can arrange, never repeating a k-mer that is in
    the range (no short cycle) and using none of `avoid`.  Returns (sequence, the set of in-range k-mers used)."""
    rng = np.random.default_rng([SEED, k, log2m, length, seed])
    lgb = log2m - 2
    B = 1 << lgb
    Z = max(2, B // share)
    top = 2 * (k - 1)
    MULT, sh = hm.MULT, 32 - lgb
    used = set()

    def gain(key, path):
        if ((((key * MULT) & 0xFFFFFFFF) >> sh) - centre + Z // 2) % B >= Z:
            return 0
        return 0 if (key in used or key in avoid or key in path) else 1

    def best(key, depth, path):
        top_score = 0
        for c in range(4):
            nxt = (key >> 2) | (c << top)
            sc = gain(nxt, path)
            if depth > 1:
                sc += best(nxt, depth - 1, path + (nxt,))
            if sc > top_score:
                top_score = sc
        return top_score

    seq = [int(x) for x in rng.integers(0, 4, size=k - 1)]
    key = 0
    for c in seq:                                     # (k - 1 residues: the next one completes the first k-mer)
        key = (key >> 2) | (c << top)
    for _ in range(length - (k - 1)):
        scores = []
        for c in range(4):
            nxt = (key >> 2) | (c << top)
            scores.append(gain(nxt, ()) + (best(nxt, look - 1, (nxt,)) if look > 1 else 0))
        m = max(scores)
        c = int(rng.choice([i for i, s in enumerate(scores) if s == m]))
        key = (key >> 2) | (c << top)
        if gain(key, ()):
            used.add(key)
        seq.append(c)
    return bytes(LETTERS[c] for c in seq), used


# ---- KFVs ---------------------------------------------------------------------------------------------------------------------
def _sn_entries(base, k, seed):
    """{natural k-mer: S}: N_REFS copies of the base's counts, a third of them moved by a fraction of N_REFS (not a multiple of it),
    and a few k-mers the base does not hold -- the shape of the range cases' near_copies family."""
    rng = np.random.default_rng([SEED + 1, k, len(base), seed])
    c = Counter(kmer_values(base, k).tolist())
    S = {x: v * N_REFS for x, v in c.items()}
    keys = sorted(S)
    for x in rng.choice(keys, size=max(1, len(keys) // 3), replace=False).tolist():
        S[x] += int(rng.integers(0, N_REFS))
    for x in rng.integers(0, 4 ** k, size=6).tolist():
        S.setdefault(int(x), int(rng.integers(1, N_REFS)))
    return S


def _ref_of(S, k, ws):
    keys = np.asarray(sorted(S), dtype=np.int64)
    Sv = np.asarray([S[x] for x in keys.tolist()], dtype=np.int64)
    if k >= hm.WIDE_MIN_K:
        return dict(keys=keys.astype(np.uint32), S=Sv, N=N_REFS, vals=Sv * (1.0 / N_REFS), ws=ws, k=k)
    St = np.zeros(4 ** k, dtype=np.int64)
    St[keys] = Sv
    return dict(RV=St / float(N_REFS), S=St, N=N_REFS, ws=ws, k=k)


def _float_of(ref, seed):
    """The same entries moved by a relative 1e-7 ... 1e-3 (tests/test_gpu_wide.py: _float_kfvs, "perturbed")."""
    rng = np.random.default_rng([SEED + 2, ref["k"], ref["ws"], seed])
    v = ref["vals"] if "keys" in ref else ref["RV"]
    f = v * (1.0 + rng.uniform(-1.0, 1.0, v.size) * 10.0 ** rng.uniform(-7, -3, v.size))
    return (ref["keys"], f) if "keys" in ref else f


def _D_of(window, S, k):
    """D = sum_x (S[x] - N c[x])^2 of one window, from the entries."""
    c = Counter(kmer_values(window, k).tolist())
    return sum((S.get(x, 0) - N_REFS * c.get(x, 0)) ** 2 for x in set(S) | set(c))


def _thr(records, S, k, ws, at):
    """Half way between the planted window's distance and the smallest of a few other windows of the first record (one above the
    planted window's where those are no farther: repeats)."""
    seq = records[0]
    scale = 2.0 * k * N_REFS * N_REFS
    planted = _D_of(seq[at:at + ws], S, k)
    others = [_D_of(seq[p:p + ws], S, k) for p in range(0, len(seq) - ws + 1, max(1, (len(seq) - ws) // 7)) if abs(p - at) > ws // 2]
    lo = min(others) if others else 0
    return float(np.round(0.5 * (planted + lo) / scale if lo > planted else planted / scale + 1.0, 2))


def _case(name, family, k, nk, records, gene_at, env=None, with_float=False, floors=None, seed=0, S=None):
    ws = nk + k - 1
    if S is None:
        S = _sn_entries(records[0][gene_at:gene_at + ws], k, seed)
    ref = _ref_of(S, k, ws)
    return dict(name=name, family=family, k=k, nk=nk, ws=ws, records=records, ref=ref, fref=_float_of(ref, seed) if with_float else None,
                thr=_thr(records, S, k, ws, gene_at), env=dict(env or {}), floors=dict(floors or {}), gene_at=gene_at)


def _log2m(k, nk, env=None):
    return hm.geometry(k, min(nk, hm.HASH_MAX_NK) if k < hm.WIDE_MIN_K else nk, env)[1]


# ---- the families -------------------------------------------------------------------------------------------------------------
LONG = [  # (k, nk, share, look, k-mers of the record, env)
    (8, 282, 32, 3, 3000, None), (8, 448, 32, 3, 3200, None), (8, 449, 32, 3, 3200, None),
    (9, 1400, 32, 3, 7300, None), (9, 1401, 32, 3, 7300, None),
    (10, 1983, 64, 4, 9300, None), (10, 1984, 64, 4, 5000, None),
    (11, 289, 32, 3, 3000, None), (11, 2048, 32, 3, 7000, None),
    (12, 289, 32, 3, 3000, {"KGMA_WIDE_LDS_NK": "0"}),
    (15, 289, 32, 3, 3000, None),
]
LONG_FLOORS = dict(longest_walk=16, wraps=1)


@functools.lru_cache(maxsize=None)
def _long_record(k, nk, share, look, n_kmers, env_items=()):
    seq, _ = colliding_sequence(k, _log2m(k, nk, dict(env_items)), n_kmers + k - 1, 0, share, look)
    return seq


def _long_cases():
    out = []
    for k, nk, share, look, n_kmers, env in LONG:
        rec = _long_record(k, nk, share, look, n_kmers, tuple(sorted((env or {}).items())))
        hashed = hm.geometry(k, nk, env)[0] != 1
        out.append(_case(f"long-k{k}-n{nk}", "long" if hashed else "control", k, nk, [rec], nk + 300, env,
                         with_float=(k, nk) in ((8, 448), (11, 289)), floors=LONG_FLOORS if hashed else None))
    return out


def _contention_cases():
    out = []
    for k, nk in ((8, 448), (11, 289)):
        rec, _ = colliding_sequence(k, _log2m(k, nk), 2400 + k - 1, 1, 32, 4)
        out.append(_case(f"contention-k{k}-n{nk}", "contention", k, nk, [rec], nk + 200, floors=dict(contention=16), with_float=k == 8, seed=1))
    return out


def _tomb_cases():
    out = []
    for k, nk in ((8, 448), (11, 289)):
        lg = _log2m(k, nk)
        m = nk + 256
        A, usedA = colliding_sequence(k, lg, m, 2, 32, 3)
        Bq, _ = colliding_sequence(k, lg, m, 3, 32, 3, avoid=frozenset(usedA))
        t = nk // 3
        # (... and pieces of both a third of a window long, in turn: k-mers that come in again while their entry is live, behind
        #  the tombstones of what has left in the meantime)
        rec = A + Bq + A + (A[:t] + Bq[:t]) * 5
        out.append(_case(f"tomb-aba-k{k}-n{nk}", "tomb", k, nk, [rec], m + 50, floors=dict(tomb_claims=64, behind_tomb=1), with_float=k == 8, seed=2))
    k, nk = 8, 282
    for tag, period in (("above", nk + 5), ("below", nk - 5)):
        unit, _ = colliding_sequence(k, _log2m(k, nk), period, 4, 32, 3)
        flank = bytes(LETTERS[c] for c in np.random.default_rng([SEED, period]).integers(0, 4, size=1000).tolist())
        rec = flank[:500] + (unit * (2400 // period + 2))[:2400] + flank[500:]
        # (a period below n: every k-mer of the repeat is in every window inside it and its count goes between 1 and 2; the tombstones
        #  are those of the flank's k-mers, in front of entries that stay live for the whole repeat)
        floors = dict(tomb_claims=64, behind_tomb=1, **({} if period > nk else dict(peak_count=2)))
        out.append(_case(f"tomb-period-{tag}-k{k}-n{nk}", "tomb", k, nk, [rec], 100, floors=floors, seed=3))   # (the gene lies in the flank: the windows of an exact repeat tie with each other)
    return out


def _count_case():
    k, nk = 10, 1983
    rec = _long_record(10, 1983, 64, 4, 9300)
    cut = 3 * 1024 + 17
    rec = rec[:cut] + b"A" * (nk + 200) + rec[cut:cut + 2500]
    # (the window that holds nothing but the homopolymer: its one entry counts n, the most a count can reach -- see test_hash_cases)
    return _case("count-k10-n1983", "count", k, nk, [rec], cut - nk // 2, floors=dict(peak_count=nk), with_float=True, seed=4)


def _rebuild_cases():
    out = []
    r8 = _long_record(8, 282, 32, 3, 3000)[:2048 + 281 + 7]              # (one stream: 2048 windows)
    out.append(_case("rebuild-1-k8-n282", "rebuild", 8, 282, [r8], 282 + 300, {"KGMA_HASH_REBUILD": "1"},
                     floors=dict(LONG_FLOORS, rebuilds=20), with_float=True))
    out.append(_case("rebuild-log2m13-k8-n282", "rebuild", 8, 282, [colliding_sequence(8, 13, 2048 + 281 + 7, 5, 32, 3)[0]], 282 + 300,
                     {"KGMA_HASH_LOG2M": "13", "KGMA_HASH_REBUILD": "1"}, floors=dict(rebuilds=20), seed=5))
    out.append(_case("rebuild-7-k10-n1983", "rebuild", 10, 1983, [_long_record(10, 1983, 64, 4, 9300)], 1983 + 300, {"KGMA_HASH_REBUILD": "7"},
                     floors=dict(LONG_FLOORS, rebuilds=20)))
    # a gene (the KFV's own base) whose dip spans the stream's rebuild at step 20: windows 64 * 20 - 448 + 1 +- a few dozen
    k, nk = 8, 448
    rec = _long_record(8, 448, 32, 3, 3200)[:2048 + 447 + 7]
    out.append(_case("rebuild-gene-k8-n448", "rebuild", k, nk, [rec], 64 * 20 - nk - 10, floors=dict(rebuilds=1), seed=6))
    return out


def _short_cases():
    out = []
    for k in (8, 11):
        for nk in (2, 33, 63):
            rec, _ = colliding_sequence(k, _log2m(k, nk), 2300 + k - 1, 6, 128, 4)
            rec = rec[:1500] + rec[1200:1500] + rec[1500:]           # (a repeat: k-mers that leave and come back within a step or two)
            out.append(_case(f"short-k{k}-n{nk}", "short", k, nk, [rec], 700, floors=dict(longest_walk=4), with_float=(k, nk) == (8, 33), seed=7))
    return out


# ---- the sparse KFV table -----------------------------------------------------------------------------------------------------
def chain_keys(k, lg, slot, count, start, exclude=()):
    """`count` device keys whose home slot in a sparse table of 2^lg slots is `slot`, enumerated upwards from `start`."""
    out, key = [], start
    while len(out) < count:
        if hm.home(key, lg) == slot and key not in exclude and 0 < key < 4 ** k - 1:
            out.append(key)
        key += 1
    return out


def _sparse_case(name, k, nk, chains, fill_to, with_ends, seed, with_float=False):
    """chains: [(home slot, or None for the home slot of 4^k - 1; length)] in the table that fill_to entries get."""
    rng = np.random.default_rng([SEED + 3, k, fill_to, seed])
    lg = hm.sparse_log2(fill_to)
    P = 1 << lg
    KMAX = 4 ** k - 1
    start = (1 << 30) - (1 << 16) if k == 15 else 1 << (2 * k - 3)   # (k = 15: keys just below 2^30)
    members, used, spec = [], set(), []
    for slot, length in chains:
        if slot is None:
            slot = hm.home(KMAX, lg)
        ck = chain_keys(k, lg, slot, length, start, exclude=used)
        used.update(ck)
        members.append(ck)
        spec.append((slot, length))
    S = {}
    for ck in members:
        for key in ck:
            S[hm.natural_of_device_key(key, k)] = int(rng.integers(1, 4)) * N_REFS + int(rng.integers(0, N_REFS))
    if with_ends:
        S[0] = 3 * N_REFS + 2
        S[KMAX] = 5 * N_REFS + 1
    while len(S) < fill_to:
        S.setdefault(int(rng.integers(1, KMAX)), int(rng.integers(1, 3 * N_REFS)))
    assert len(S) == fill_to and hm.sparse_log2(len(S)) == lg
    present = set(hm.device_key_of_natural(x, k) for x in S)
    # absent k-mers whose home lies inside the first chain
    slot0, len0 = spec[0]
    absent = []
    for off in (0, 1, len0 // 2):
        absent += chain_keys(k, lg, (slot0 + off) % P, 2, start + (1 << 14), exclude=present)

    def spell(key):
        return bytes(LETTERS[(key >> (2 * j)) & 3] for j in range(k))
    # the record: the KFV's k-mers (twice, in two orders) and the absent ones, spelled out one after the other
    order = [hm.device_key_of_natural(x, k) for x in S]
    order = order + absent + [order[i] for i in rng.permutation(len(order)).tolist()] + absent[::-1]
    body = b"".join(spell(key) for key in order)
    if with_ends:
        body = body[:len(body) // 2] + b"A" * 40 + b"T" * 40 + b"N" * 30 + body[len(body) // 2:]
    filler = bytes(LETTERS[c] for c in rng.integers(0, 4, size=2 * nk + 600).tolist())
    rec = filler[:nk + 300] + body + filler[nk + 300:]
    ws = nk + k - 1
    at = nk + 300 + min(len(body) // 3, max(0, len(body) - ws))
    c = _case(name, "sparse", k, nk, [rec], at, with_float=with_float, seed=seed, S=S,
              floors=dict(chains=spec, absent=[int(x) for x in absent], wrap=any(s + n > P for s, n in spec)))
    c["sparse_lg"] = lg
    return c


def _limit_case():
    """k = 11, n = 2048 (4096 entries, 1024 buckets): a step of the warm-up whose probe loop runs for more than 8 x buckets iterations,
    the limit the kernel had before it was derived.  The record ends a few steps after that step."""
    k, nk = 11, 2048
    rec, _ = colliding_sequence(k, _log2m(k, nk), nk + 1300 + k - 1, 100, 32, 4)
    return _case("limit-k11-n2048", "limit", k, nk, [rec], 600, floors=dict(LONG_FLOORS, beyond_former_limit=True), seed=8)


def _sparse_cases():
    return [
        # 128 slots: a chain of 40 from slot 125 past the last slot (key 0 sits in slot 0, inside it) and one of 8 that ends in 4^k - 1
        _sparse_case("sparse-chains-k11", 11, 289, [(125, 40), (None, 7)], 60, True, 0, with_float=True),
        _sparse_case("sparse-chains-k15", 15, 289, [(125, 40), (None, 7)], 60, True, 1),
        # 32 / 33 entries: 64 / 128 slots, a chain of 8 that runs past the last slot in each
        _sparse_case("sparse-32-k12", 12, 289, [(61, 8)], 32, False, 2),
        _sparse_case("sparse-33-k12", 12, 289, [(125, 8)], 33, False, 3),
    ]


@functools.lru_cache(maxsize=None)
def cases():
    out = _long_cases() + _contention_cases() + _tomb_cases() + [_count_case(), _limit_case()] + _rebuild_cases() + _short_cases() + _sparse_cases()
    assert [c["name"] for c in out] == NAMES
    return out


def case(name):
    return next(c for c in cases() if c["name"] == name)


NAMES = ([f"long-k{k}-n{nk}" for k, nk, *_ in LONG] + ["contention-k8-n448", "contention-k11-n289", "tomb-aba-k8-n448", "tomb-aba-k11-n289",
         "tomb-period-above-k8-n282", "tomb-period-below-k8-n282", "count-k10-n1983", "limit-k11-n2048", "rebuild-1-k8-n282", "rebuild-log2m13-k8-n282",
         "rebuild-7-k10-n1983", "rebuild-gene-k8-n448"] + [f"short-k{k}-n{nk}" for k in (8, 11) for nk in (2, 33, 63)]
         + ["sparse-chains-k11", "sparse-chains-k15", "sparse-32-k12", "sparse-33-k12"])


def sparse_kfv_of(c, mutation=None):
    """The model's sparse KFV table of a case at k >= 11 (values: S), None below."""
    if "keys" not in c["ref"]:
        return None
    return hm.SparseKFV(c["ref"]["keys"].tolist(), c["ref"]["S"].tolist(), c["k"], mutation)
