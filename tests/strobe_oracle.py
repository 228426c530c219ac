"""CPU restatement of the reference's strobemer engine, for the tests (a helper module, not a conftest).

Three pieces, read literally from the reference (src/StrobemerGMA/Strobemers.jl, StrobeRefGen.jl,
StrobeGenomeMiner.jl; src/Alignment.jl:83-111):

1. the randstrobe of the k = w_max + s - 1 residues at a position: `first` is the s-mer at offset 1, the score of
   offset i in w_min..w_max is (as_UInt(first) + as_UInt(s-mer at i)) % q, and because `min_score::Int = 2 << 63`
   is 0 and the test is `<=`, the chosen offset is the LAST offset whose score is 0, or w_min if none is.  The bin is
   first * 4^s + second (natural values, first base most significant);
2. gen_ref_ws_cons (strobemer method): summed bin counts times 1/N, windowsize = round(total / N), consensus as in
   the k-mer method;
3. StrobeGMA! per record: records shorter than the window are skipped (genome_pos does not advance); steps run over
   i = 1 .. L - W - 1; the strobemer leaving is the one starting at i, the one "entering" is read from
   view(seq, i+W-k : i+W), i.e. it starts at i + W - k -- the last one of the previous window.

Two results per record:
  exact: Python ints D = sum (S - N c)^2, the hit state machine on D against thr * 2 k N^2;
  float: the reference's sequential Float64 loop, first window summed left to right.
A hit is a dict(contig, cmi, lo, hi, genome_pos, D, dist); `lo:hi` is the candidate range before any alignment.  The
score gate of process_hit! does not feed back into the state machine (goal_ind and currminim are updated whether or
not the hit is kept): `accept(contig, cmi, lo, hi) -> bool` stands for the gate and only decides whether a candidate is
emitted.  `gate_feeds_back=True` is the COUNTERFACTUAL in which a rejected candidate leaves goal_ind alone -- not the
reference; tests use it to show that an input tells the two apart.
"""
from __future__ import annotations

from fractions import Fraction
from typing import List, Sequence, Tuple

import numpy as np

_CODE = np.full(256, -1, dtype=np.int64)
for _ch, _v in (("A", 0), ("C", 1), ("G", 2), ("T", 3), ("N", 3)):
    _CODE[ord(_ch)] = _v
    _CODE[ord(_ch.lower())] = _v


class BadBase(KeyError):
    pass


def check_params(s: int, w_min: int, w_max: int, q: int) -> None:
    if s < 1 or w_min < 1 or w_min > w_max or q < 1:
        raise ValueError(f"invalid randstrobe parameters s={s}, w_min={w_min}, w_max={w_max}, q={q}")


def strobe_bins(seq: bytes, s: int, w_min: int, w_max: int, q: int, n_lookup: int = None) -> np.ndarray:
    """Bin (0-based) of the randstrobe starting at every position of `seq` that has k residues to its right.
    Residues beyond `n_lookup` (default: all) are never looked up: a bad one there is read as 0."""
    return strobe_bins_offsets(seq, s, w_min, w_max, q, n_lookup)[0]


def strobe_bins_offsets(seq: bytes, s: int, w_min: int, w_max: int, q: int, n_lookup: int = None) -> Tuple[np.ndarray, np.ndarray]:
    """(bins, offsets): strobe_bins and, per position, the 1-based offset w_min..w_max the second s-mer was taken from (the last
    one of score 0; w_min where none scores 0, which a look at (first + second) % q tells apart)."""
    check_params(s, w_min, w_max, q)
    k = w_max + s - 1
    codes = _CODE[np.frombuffer(seq, dtype=np.uint8)].copy()
    n_lookup = len(seq) if n_lookup is None else n_lookup
    bad = np.nonzero(codes[:n_lookup] < 0)[0]
    if bad.size:
        raise BadBase(f"residue {seq[bad[0]:bad[0] + 1]!r} at position {int(bad[0]) + 1}")
    codes[codes < 0] = 0
    n = codes.size - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    ns = codes.size - s + 1
    smer = np.zeros(ns, dtype=np.int64)
    for j in range(s):
        smer = smer * 4 + codes[j:j + ns]
    first = smer[:n]
    second = smer[w_min - 1:w_min - 1 + n].copy()
    offset = np.full(n, w_min, dtype=np.int64)
    for i in range(w_min, w_max + 1):                   # ascending: the last offset of score 0 wins
        cand = smer[i - 1:i - 1 + n]
        zero = (first + cand) % q == 0
        second = np.where(zero, cand, second)
        offset = np.where(zero, i, offset)
    return first * 4 ** s + second, offset


def get_strobe_2_mer(seq: bytes, s: int = 2, w_min: int = 3, w_max: int = 5, q: int = 5, withGap: bool = True) -> bytes:
    check_params(s, w_min, w_max, q)
    codes = _CODE[np.frombuffer(seq, dtype=np.uint8)]
    val = lambda a: int(sum(int(c) << (2 * (s - 1 - j)) for j, c in enumerate(codes[a:a + s])))
    first = val(0)
    ind = w_min
    for i in range(w_min, w_max + 1):
        if (first + val(i - 1)) % q <= 0:
            ind = i
    a, b = seq[:s], seq[ind - 1:ind - 1 + s]
    if not withGap:
        return a + b
    return a + b"-" * (ind - s - 1) + b + b"-" * (len(seq) - ind - s + 1)


def strobe_count(seq: bytes, s: int = 2, w_min: int = 3, w_max: int = 5, q: int = 5) -> np.ndarray:
    return np.bincount(strobe_bins(seq, s, w_min, w_max, q), minlength=4 ** (2 * s)).astype(np.int64)


def _julia_round(x: float) -> int:
    return int(np.rint(x))


def gen_ref(seqs: Sequence[bytes], s: int, w_min: int, w_max: int, q: int) -> Tuple[np.ndarray, int, np.ndarray, int]:
    """(KFV Float64, windowsize, S int64, N) of the strobemer gen_ref_ws_cons."""
    S = np.zeros(4 ** (2 * s), dtype=np.int64)
    total = 0
    for seq in seqs:
        S += strobe_count(seq, s, w_min, w_max, q)
        total += len(seq)
    N = len(seqs)
    inv = 1.0 / N
    return S.astype(np.float64) * inv, _julia_round(total * inv), S, N


def scan_record(seq: bytes, ref: np.ndarray, S: np.ndarray, N: int, s: int, w_min: int, w_max: int, q: int, W: int,
                thr: float, buff: int, contig: int = 0, genome_pos: int = 0, return_dists: bool = False, accept=None,
                gate_feeds_back: bool = False):
    """One record with L >= W.  Returns dict(exact=[hits], float=[hits], D1, d1, dists_exact=[D...], dists_float=[...])."""
    k = w_max + s - 1
    L = len(seq)
    assert L >= W > k
    bins = strobe_bins(seq, s, w_min, w_max, q, n_lookup=max(W, L - 2)).tolist()
    NB = 4 ** (2 * s)
    cnt = np.bincount(np.asarray(bins[:W - k + 1], dtype=np.int64), minlength=NB)
    # exact first window
    Sl = [int(x) for x in S]
    D = int(sum((Sl[x] - N * int(cnt[x])) ** 2 for x in range(NB)))
    # Float64 first window: (1/(2k)) * sqeuclidean(refVec, counts), summed left to right
    refl = [float(x) for x in ref]
    acc = 0.0
    for x in range(NB):
        t = refl[x] - float(cnt[x])
        acc += t * t
    kd = (1 / (2 * k)) * acc
    SF = 1 / k
    ci = [int(x) for x in cnt]
    cf = [float(x) for x in cnt]
    scale = 2 * k * N * N
    T = Fraction(thr) * scale
    T = T.numerator // T.denominator + (1 if T.numerator % T.denominator else 0)      # D < thr*scale  <=>  D < ceil(.)
    twoN = 2 * N
    out = {"D1": D, "d1": kd, "exact": [], "float": []}
    dE: List[int] = []
    dF: List[float] = []
    # state machines (exact / float)
    eCMI, estop, emin, egoal = 2, True, D, 0
    fCMI, fstop, fmin, fgoal, fminD = 2, True, kd, 0, D

    def emit(lst, CMI, dist, Dv):
        lo, hi = max(CMI - buff, 1), min(CMI + W - 1 + buff, L)
        ok = accept is None or accept(contig, CMI, lo, hi)
        if ok:
            lst.append(dict(contig=contig, cmi=CMI, lo=lo, hi=hi, genome_pos=genome_pos, D=Dv, dist=dist))
        return ok or not gate_feeds_back

    off = W - k
    for i in range(1, L - W):
        l = bins[i - 1]
        r = bins[i - 1 + off]
        if l != r:
            kd += SF * (1 + cf[r] + refl[l] - refl[r] - cf[l])
            D += twoN * (Sl[l] - Sl[r] - N * (ci[l] - 1 - ci[r]))
            ci[l] -= 1; ci[r] += 1
            cf[l] -= 1; cf[r] += 1
        if return_dists:
            dE.append(D); dF.append(kd)
        # exact
        if D < T:
            if D < emin:
                emin = D; eCMI = i; estop = False
        elif not estop:
            estop = True
            eCMI += 1
            if eCMI > egoal:
                if emit(out["exact"], eCMI, emin / scale, emin):
                    egoal = eCMI + W - 1
                emin = D
        # float
        if kd < thr:
            if kd < fmin:
                fmin = kd; fminD = D; fCMI = i; fstop = False
        elif not fstop:
            fstop = True
            fCMI += 1
            if fCMI > fgoal:
                if emit(out["float"], fCMI, fmin, fminD):
                    fgoal = fCMI + W - 1
                fmin = kd; fminD = D
    out["dists_exact"] = dE
    out["dists_float"] = dF
    return out


def scan(seqs: Sequence[bytes], ref: np.ndarray, S: np.ndarray, N: int, s: int, w_min: int, w_max: int, q: int, W: int,
         thr: float, buff: int, return_dists: bool = False, accept=None, gate_feeds_back: bool = False):
    """All records.  Returns dict(exact, float: hit lists; first_D: per record (-1 = skipped); per_record: list of
    (exact hits, float hits) per record; dists_exact / dists_float when asked)."""
    res = {"exact": [], "float": [], "first_D": [], "first_d": [], "per_record": [], "dists_exact": [], "dists_float": []}
    genome_pos = 0
    for c, seq in enumerate(seqs):
        if len(seq) < W:
            res["first_D"].append(-1); res["first_d"].append(None); res["per_record"].append(([], []))
            continue
        r = scan_record(seq, ref, S, N, s, w_min, w_max, q, W, thr, buff, c, genome_pos, return_dists, accept, gate_feeds_back)
        res["exact"] += r["exact"]; res["float"] += r["float"]
        res["first_D"].append(r["D1"]); res["first_d"].append(r["d1"])
        res["per_record"].append((r["exact"], r["float"]))
        res["dists_exact"] += r["dists_exact"]; res["dists_float"] += r["dists_float"]
        genome_pos += len(seq)
    return res


def window_counts_direct(seq: bytes, s: int, w_min: int, w_max: int, q: int, W: int, i: int) -> np.ndarray:
    """The reference's count vector after step i (0 = the first window), by running its update literally."""
    k = w_max + s - 1
    bins = strobe_bins(seq, s, w_min, w_max, q)
    cnt = np.bincount(bins[:W - k + 1], minlength=4 ** (2 * s)).astype(np.int64)
    for j in range(1, i + 1):
        l, r = bins[j - 1], bins[j - 1 + W - k]
        if l != r:
            cnt[l] -= 1; cnt[r] += 1
    return cnt
