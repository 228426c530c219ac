"""A lock-step model of the generic kernel's hash tables (kgma_generic.hip: Counts<2>, WCounts) and of the sparse KFV table
(kgma_api.cpp: set_refs_sparse_core; WCounts::lookup), in plain Python, written from the kernel's comments and code.

Geometry:  geometry() restates generic_set_mode / generic_set_wide, sparse_log2() the sparse table's size, stream_windows() the
stream length of a genome of a few kilobases (stream_length: every wave slot gets less than one stream's minimum, so
P = max(KGMA_STREAM_MIN_WINDOWS, 4 n rounded up to 64), and streams start on 64-window boundaries of the record).

The table:  M entries in buckets of four, linear probing over buckets.  An entry is never-used, a tombstone or live (key, count;
k >= 11: also the KFV's value, looked up when the entry is claimed).  A step of 64 lanes:
  (A) the probe loop: per iteration every unfinished entering search reads its bucket (all lanes read before any lane swaps), then
      the compare-and-swaps of the iteration happen one after the other, then every unfinished leaving search reads its bucket;
  (B) every acting lane reads its start-of-step counts, then adds / subtracts;  (C) a leaving lane whose entry is at 0 leaves a
      tombstone.
Which lane wins a compare-and-swap is not defined by the hardware: the model serialises them in lane order, or in reverse lane
order (order = -1); run_stream's caller compares the two (tests/test_hash_cases.py).

Lanes past the record's last k-mer read what follows the record in the 2-bit copy; their windows are not tested and the stream
ends with that step.  The model leaves those lanes out.

MUTATIONS names five one-line faults the model can be run with, to show which inputs notice them."""
from collections import Counter

MULT = 2654435761
HASH_MAX_NK = 1983                       # KGMA_HASH_MAX_NK: the 11-bit count field holds n + 64 <= 2047
WIDE_MIN_K = 11
WIDE_LDS_MAX_NK = 2048
WIDE_LDS_NK_CAP = 8192 - 64 - 1024 - 512
STREAM_MIN_WINDOWS = 2048
SP_EMPTY = 0xFFFFFFFF

MUTATIONS = ("no_wrap", "tomb_is_unused", "no_rescan", "rebuild_late", "lookup_first_slot")


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def geometry(k, nk, env=None):
    """(cmode, log2m, rebuild) of a launch whose longest window has nk k-mers, as generic_set_mode decides it."""
    env = env or {}
    if k == 1:
        return 5, 0, 0
    if k >= WIDE_MIN_K:
        lds_max = WIDE_LDS_MAX_NK
        if "KGMA_WIDE_LDS_NK" in env:
            lds_max = max(0, min(WIDE_LDS_NK_CAP, int(env["KGMA_WIDE_LDS_NK"])))
        lds = nk <= lds_max
        lg = 9
        while (1 << lg) - nk - 64 - (1 << lg) // 8 < 64 * (8 if lds else 16):
            lg += 1
        M = 1 << lg
        return (3 if lds else 4), lg, max(1, (M - nk - 64 - M // 8) // 64)
    if k <= 7:
        return 0, 0, 0
    if nk > HASH_MAX_NK or int(env.get("KGMA_GENERIC_HASH", "1")) == 0:
        return 1, 0, 0
    lg = 11 if nk <= 448 else (12 if nk <= 1400 else 13)
    if "KGMA_HASH_LOG2M" in env:
        lg = max(lg, min(13, int(env["KGMA_HASH_LOG2M"])))
    M = 1 << lg
    rebuild = max(1, (M - nk - 64 - M // 8) // 64)
    if "KGMA_HASH_REBUILD" in env:
        rebuild = max(1, min(rebuild, int(env["KGMA_HASH_REBUILD"])))
    return 2, lg, rebuild


def sparse_log2(entries):
    lg = 6
    while (1 << lg) < 2 * entries:
        lg += 1
    return lg


def stream_windows(nk_max):
    """Windows per stream of a small genome (its windows are fewer than the wave slots times the minimum below)."""
    return min(max(STREAM_MIN_WINDOWS, min((4 * nk_max + 63) // 64 * 64, 1 << 16)), 1 << 19)


PROBE_LIMIT_PASSES = 66                  # the kernel's: the probe loop gives up after this many iterations per bucket


def limit_of(log2m):
    """The probe loop's iteration limit (kgma_generic.hip derives it: 64 passes of the entering searches, 2 of the leaving ones)."""
    return PROBE_LIMIT_PASSES * ((1 << log2m) // 4)


def former_limit_of(log2m):
    """8 x buckets: the limit before it was derived.  Colliding inputs pass it (tests/hash_cases.py: the limit case)."""
    return 8 * ((1 << log2m) // 4)


# ---- keys ---------------------------------------------------------------------------------------------------------------------
_CODE = [3] * 256
for _c, _v in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
    _CODE[_c] = _v


def device_keys(seq, k):
    """The device key of every k-mer of seq: its first base in bits 0-1 (device_index_of)."""
    out, key, top = [], 0, 2 * (k - 1)
    for i, c in enumerate(seq):
        key = (key >> 2) | (_CODE[c] << top)
        if i >= k - 1:
            out.append(key)
    return out


def device_key_of_natural(v, k):
    key = 0
    for _ in range(k):
        key = (key << 2) | (v & 3)
        v >>= 2
    return key


def natural_of_device_key(key, k):
    return device_key_of_natural(key, k)            # (reversing the base order is its own inverse)


def home(key, log2_slots):
    return ((key * MULT) & 0xFFFFFFFF) >> (32 - log2_slots)


# ---- the sparse KFV table -----------------------------------------------------------------------------------------------------
class SparseKFV:
    """set_refs_sparse_core's insertion loop over the KFV's entries in increasing natural key order, and WCounts::lookup."""

    def __init__(self, natural_keys, values, k, mutation=None):
        assert list(natural_keys) == sorted(natural_keys)
        self.lg = sparse_log2(len(natural_keys))
        self.P = 1 << self.lg
        self.keys = [SP_EMPTY] * self.P
        self.vals = [0] * self.P
        self.displacement = {}                      # device key -> slots walked past at insertion
        self.wrapped = set()                        # device keys whose insertion passed from the last slot to slot 0
        self.mutation = mutation
        for nat, v in zip(natural_keys, values):
            key = device_key_of_natural(int(nat), k)
            h = home(key, self.lg)
            d = 0
            while self.keys[h] != SP_EMPTY:
                if h == self.P - 1:
                    self.wrapped.add(key)
                h = (h + 1) & (self.P - 1)
                d += 1
            self.keys[h], self.vals[h] = key, v
            self.displacement[key] = d
        self.true = dict(zip(self.keys, self.vals))
        self.true.pop(SP_EMPTY, None)
        self.longest_lookup = 0

    def lookup(self, key):
        h = home(key, self.lg)
        for it in range(self.P):
            kk = self.keys[h]
            if kk == key:
                self.longest_lookup = max(self.longest_lookup, it + 1)
                return self.vals[h]
            if kk == SP_EMPTY or self.mutation == "lookup_first_slot":
                self.longest_lookup = max(self.longest_lookup, it + 1)
                break
            h = (h + 1) & (self.P - 1)
        return 0


# ---- the count table ----------------------------------------------------------------------------------------------------------
UNUSED, TOMB = 0, 1                      # an entry's key word; a live entry holds key + 2


class _Search:
    __slots__ = ("key", "b", "home", "tomb", "slot", "done", "ins", "seen_tomb", "wrapped", "passes")

    def __init__(self, key, hb, on):
        self.key, self.b, self.home = key + 2, hb, hb
        self.tomb, self.slot, self.done, self.ins = -1, 0, not on, False
        self.seen_tomb = self.wrapped = False
        self.passes = 0


class Table:
    """One wave's table.  wide: WCounts (k >= 11), else Counts<2>."""

    def __init__(self, log2m, wide, order=1, mutation=None, kfv=None):
        self.M = 1 << log2m
        self.B = self.M // 4
        self.lgb = log2m - 2
        self.wide, self.order, self.mutation, self.kfv = wide, order, mutation, kfv
        # (no_wrap: a walk past the last bucket leaves the table; what lies behind it is never cleared)
        self.K = [UNUSED] * (2 * self.M)
        self.C = [0] * (2 * self.M)
        self.V = [0] * (2 * self.M)
        self.limit = PROBE_LIMIT_PASSES * self.B
        self.fault = False
        # contention: the most lanes of one step with different absent k-mers that tried the same entry; contention_iter: of those,
        # the most in one iteration of the probe loop (lanes reach their path's end together only from the same home bucket)
        self.stats = dict(longest_walk=0, wraps=0, tomb_claims=0, behind_tomb=0, contention=0, contention_iter=0, worst_iters=0,
                          peak_count=0, min_unused=self.M, rebuilds=0)

    def clear(self):
        self.K[:self.M] = [UNUSED] * self.M
        self.C[:self.M] = [0] * self.M

    def _next(self, b):
        return b + 1 if self.mutation == "no_wrap" else (b + 1) & (self.B - 1)

    def _found(self, s, b, j):
        s.slot, s.done = 4 * b + j, True
        st = self.stats
        walk = ((b - s.home) % self.B) + 1
        if walk > st["longest_walk"]:
            st["longest_walk"] = walk
        if s.wrapped:
            st["wraps"] += 1

    def probe2(self, ent, lea):
        """The searches of a step (or of a group of 64 of a rebuild): ent / lea are lists of _Search.  Returns the iterations."""
        K, B, st = self.K, self.B, self.stats
        unused_or_tomb = self.mutation == "tomb_is_unused"
        it = 0
        tried = {}                                      # entry -> the k-mers that tried to claim it in this loop
        act_e = [s for s in ent if not s.done]
        act_l = [s for s in lea if not s.done]
        while act_e or act_l:
            # entering searches: every lane reads, then the swaps one after the other
            swaps = []
            for s in act_e:
                b4 = 4 * s.b
                v = K[b4:b4 + 4]
                if s.key in v:
                    j = v.index(s.key)
                    if s.seen_tomb or TOMB in v[:j]:
                        st["behind_tomb"] += 1
                    self._found(s, s.b, j)
                    continue
                if s.tomb < 0 and TOMB in v:
                    s.tomb = b4 + v.index(TOMB)
                    s.seen_tomb = True
                free = (v[3] == UNUSED or TOMB in v) if unused_or_tomb else v[3] == UNUSED
                if not free:
                    nb = self._next(s.b)
                    if nb < s.b:
                        s.wrapped = True
                    s.b = nb
                    continue
                if UNUSED in v:
                    je = v.index(UNUSED)
                    target, expect = (s.tomb, TOMB) if s.tomb >= 0 else (b4 + je, UNUSED)
                else:                                   # (tomb_is_unused only: a bucket of tombstones and live entries)
                    target, expect = s.tomb, TOMB
                swaps.append((s, target, expect))
            if swaps:
                by_target = {}
                for s, target, _ in swaps:
                    by_target.setdefault(target, set()).add(s.key)
                    tried.setdefault(target, set()).add(s.key)
                worst = max(len(x) for x in by_target.values())
                if worst > st["contention_iter"]:
                    st["contention_iter"] = worst
                for s, target, expect in (swaps if self.order > 0 else reversed(swaps)):
                    old = K[target]
                    if old == expect:
                        K[target] = s.key
                        s.ins = True
                        if expect == TOMB:
                            st["tomb_claims"] += 1
                        self._found(s, target // 4, target & 3)
                    elif old == s.key or self.mutation == "no_rescan":
                        self._found(s, target // 4, target & 3)          # a lane with the same k-mer was first
                    else:                                                # lost to another k-mer: rescan
                        s.b, s.tomb, s.seen_tomb, s.wrapped = s.home, -1, False, False
                        s.passes += 1
            # leaving searches (present, or entered by a lower lane of this step when the window is shorter than a step)
            for s in act_l:
                b4 = 4 * s.b
                v = K[b4:b4 + 4]
                if s.key in v:
                    j = v.index(s.key)
                    if s.seen_tomb or TOMB in v[:j]:
                        st["behind_tomb"] += 1
                    self._found(s, s.b, j)
                    continue
                if TOMB in v:
                    s.seen_tomb = True
                if self.wide and v[3] == UNUSED:
                    s.b, s.seen_tomb, s.wrapped = s.home, False, False
                else:
                    nb = self._next(s.b)
                    if nb < s.b:
                        s.wrapped = True
                    s.b = nb
            it += 1
            if it > self.limit or any(s.b >= 2 * B for s in act_e + act_l):
                self.fault = True
                break
            act_e = [s for s in act_e if not s.done]
            act_l = [s for s in act_l if not s.done]
        if it > st["worst_iters"]:
            st["worst_iters"] = it
        if tried:
            st["contention"] = max(st["contention"], max(len(x) for x in tried.values()))
        return it

    def _claim_value(self, s):
        if s.ins and self.kfv is not None:
            self.V[s.slot] = self.kfv.lookup(s.key - 2)

    def rebuild(self, keys, b, nk):
        self.clear()
        self.stats["rebuilds"] += 1
        q1 = 64 * b
        q0 = max(0, q1 - nk) + (1 if self.mutation == "rebuild_late" else 0)
        for base in range(q0, q1, 64):
            grp = [_Search(keys[q], home(keys[q], self.lgb), True) for q in range(base, min(base + 64, q1))]
            self.probe2(grp, [])
            if self.fault:
                return
            for s in grp:
                self._claim_value(s)
                self.C[s.slot] += 1

    def step(self, kp, ks, actE, actL):
        """kp / ks / actE / actL per lane.  Returns per lane (cp, cs, vp, vl): the start-of-step counts and the cached values."""
        lgb = self.lgb
        ent = [_Search(kp[i], home(kp[i], lgb), actE[i]) for i in range(len(kp))]
        lea = [_Search(ks[i], home(ks[i], lgb), actL[i]) for i in range(len(kp))]
        its = self.probe2(ent, lea)
        if self.fault:
            return None, its
        for s in ent:
            self._claim_value(s)
        C, K, V = self.C, self.K, self.V
        out = [(C[e.slot] if actE[i] else 0, C[l.slot] if actL[i] else 0, V[e.slot] if actE[i] else 0, V[l.slot] if actL[i] else 0)
               for i, (e, l) in enumerate(zip(ent, lea))]
        for i, (e, l) in enumerate(zip(ent, lea)):
            if actE[i]:
                C[e.slot] += 1
            if actL[i]:
                C[l.slot] -= 1
        st = self.stats
        peak = max((C[e.slot] for i, e in enumerate(ent) if actE[i]), default=0)
        if peak > st["peak_count"]:
            st["peak_count"] = peak
        for i, l in enumerate(lea):
            if actL[i] and C[l.slot] == 0:
                K[l.slot] = TOMB
        unused = K[:self.M].count(UNUSED)
        if unused < st["min_unused"]:
            st["min_unused"] = unused
        return out, its

    def live(self):
        """{device key: count} of the live entries, and whether a key has two entries or a live entry counts 0."""
        d, bad = {}, False
        for x, c in zip(self.K, self.C):
            if x >= 2:
                if x - 2 in d or c <= 0:
                    bad = True
                d[x - 2] = d.get(x - 2, 0) + c
        return d, bad


def run_stream(keys, nk, log2m, rebuild, wide, order=1, mutation=None, kfv=None, n_pos=None, per_step=None):
    """One stream over the k-mers `keys` (device keys of its k-mer positions 0 ... : n_valid + nk - 1 of them, or more where the
    record goes on).  Returns (ok, stats): ok is False when a step ended with counts other than the window's true multiset, read a
    start-of-step count or a cached value other than the true one, or gave up.  per_step (a list) receives a dict per step."""
    t = Table(log2m, wide, order, mutation, kfv)
    n_pos = len(keys) if n_pos is None else n_pos
    n_blocks = (n_pos + 63) // 64
    window = Counter()
    ok = True
    truth = kfv.true if kfv is not None else None
    for b in range(n_blocks):
        lanes = range(64 * b, min(64 * b + 64, len(keys)))
        kp = [keys[p] for p in lanes]
        ks = [keys[p - nk] if p >= nk else keys[p] for p in lanes]
        haveL = [p >= nk for p in lanes]
        actE = [kp[i] != ks[i] or not haveL[i] for i in range(len(kp))]
        actL = [kp[i] != ks[i] and haveL[i] for i in range(len(kp))]
        if b > 0 and b % rebuild == 0:
            t.rebuild(keys, b, nk)
        before = dict(t.stats)
        out, its = t.step(kp, ks, actE, actL) if not t.fault else (None, 0)
        if t.fault:
            ok = False
            break
        for i, (cp, cs, vp, vl) in enumerate(out):
            if actE[i] and cp != window[kp[i]] or actL[i] and cs != window[ks[i]]:
                ok = False
            if truth is not None and (actE[i] and vp != truth.get(kp[i], 0) or actL[i] and vl != truth.get(ks[i], 0)):
                ok = False
        for i in range(len(kp)):
            if actE[i]:
                window[kp[i]] += 1
            if actL[i]:
                window[ks[i]] -= 1
                if window[ks[i]] == 0:
                    del window[ks[i]]
        live, bad = t.live()
        if bad or live != dict(window):
            ok = False
        if per_step is not None:
            per_step.append(dict(b=b, iters=its, tomb_claims=t.stats["tomb_claims"] - before["tomb_claims"],
                                 behind_tomb=t.stats["behind_tomb"] - before["behind_tomb"], wraps=t.stats["wraps"] - before["wraps"]))
    return ok, t.stats


def streams_of(seq, k, nk, P):
    """(keys, n_pos) of every stream of a record: stream t owns the windows t P ... of the record and reads its k-mers from there."""
    keys = device_keys(seq, k)
    nwin = len(keys) - nk + 1
    out = []
    for t0 in range(0, max(nwin, 0), P):
        n_valid = min(P, nwin - t0)
        n_pos = n_valid + nk - 1
        out.append((keys[t0:t0 + 64 * ((n_pos + 63) // 64)], n_pos))
    return out


def merge_stats(a, b):
    out = dict(a)
    for key, v in b.items():
        if key == "min_unused":
            out[key] = min(out[key], v)
        elif key in ("longest_walk", "contention", "contention_iter", "worst_iters", "peak_count"):
            out[key] = max(out[key], v)
        else:
            out[key] += v
    return out


def run_record(seq, k, nk, env=None, order=1, mutation=None, kfv=None, nk_mode=None):
    """Every stream of a record under the geometry of (k, nk_mode or nk, env).  Returns (ok, stats, per-stream rebuild counts)."""
    cmode, log2m, rebuild = geometry(k, nk_mode or nk, env)
    assert cmode in (2, 3, 4), "no hash table serves this case"
    P = stream_windows(nk_mode or nk)
    ok, stats, rebuilds = True, None, []
    for keys, n_pos in streams_of(seq, k, nk, P):
        o, s = run_stream(keys, nk, log2m, rebuild, cmode != 2, order, mutation, kfv, n_pos)
        ok = ok and o
        rebuilds.append(s["rebuilds"])
        stats = s if stats is None else merge_stats(stats, s)
    return ok, stats, rebuilds
