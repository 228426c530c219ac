"""Case builders of the position-weight-matrix search tests (tests/test_pwm_host.py checks that every list hits what it is for;
tests/test_gpu_pwm.py runs them on the device with the library's real geometry).

A case is a Case(name, matrices, thresholds, records, aim): `aim` says what the case is for in a form the host test checks --
"hits": (matrix, record, start) triples the oracle must report, "absent": triples it must not, "none": the list is empty,
"many": it has more entries than that."""
from typing import NamedTuple

import numpy as np

from tests import pwm_oracle as po

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
LENGTHS = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64)
HOST_GEOMETRY = (1, 2048, 8192)       # (lane_starts, wave_starts, wg_starts) the host test builds the seam cases with


class Case(NamedTuple):
    name: str
    matrices: list
    thresholds: list
    records: list
    aim: dict


def rand_dna(rng, n) -> bytes:
    return BASES[rng.integers(0, 4, size=n)].tobytes()


def rand_matrix(rng, m, lo=-300, hi=300, constant=()) -> np.ndarray:
    """m rows of weights in lo ... hi, every row with one strict maximum; the rows of `constant` are four equal weights."""
    W = rng.integers(lo, hi, size=(m, 4)).astype(np.int64)
    for i in range(m):
        W[i, int(rng.integers(0, 4))] = hi + 1 + int(rng.integers(0, 20))
        if i in constant:
            W[i, :] = int(rng.integers(lo, hi))
    return W


def best_site(W) -> bytes:
    """The top-scoring sequence (the first maximum of every row)."""
    return BASES[np.asarray(W).argmax(axis=1)].tobytes()


def score(W, site: bytes) -> int:
    return int(po.profile_rows(W, site)[0])


def plant(text: bytearray, start0: int, site: bytes) -> None:
    assert 0 <= start0 and start0 + len(site) <= len(text), (start0, len(site), len(text))
    text[start0:start0 + len(site)] = site


# ---- lengths ---------------------------------------------------------------------------------------------------------------------
def length_cases():
    out = []
    for m in LENGTHS:
        rng = np.random.default_rng(100 + m)
        W = rand_matrix(rng, m, constant=(1, 2, 7, 30, 31, 40) if m >= 5 else ())
        site = best_site(W)
        big = bytearray(rand_dna(rng, 3001))
        plant(big, 1500, site)
        extra = rand_dna(rng, 1)
        recs = [bytes(big), site[:-1], site, site + extra, extra + site]
        recs = [r for r in recs if r]                                  # (m = 1: no record of m - 1 residues)
        thr = po.highest(W) - (0 if m <= 3 else 250)                   # (short matrices hit often as it is)
        at = {r: c for c, r in enumerate(recs)}
        out.append(Case(f"m{m}", [W], [thr], recs,
                        {"hits": [(0, 0, 1501), (0, at[site], 1), (0, at[site + extra], 1), (0, at[extra + site], 2)]}))
    return out


def tiny_records_case():
    rng = np.random.default_rng(7)
    recs = [rand_dna(rng, int(n)) for n in rng.integers(1, 4, size=300)]
    W = np.array([[2, 0, 0, 1], [0, 3, 1, 0]], dtype=np.int64)
    want = next(c for c, r in enumerate(recs) if r[:2] == b"AC")
    return Case("tiny_records", [W, W[:1]], [4, 2], recs, {"hits": [(0, want, 1)], "many": 20})


def empty_cases():
    rng = np.random.default_rng(8)
    W = rand_matrix(rng, 20)
    text = rand_dna(rng, 5000)
    return [Case("above_the_highest", [W], [po.highest(W) + 1], [text], {"none": True}),
            Case("nothing_reaches_it", [W], [po.highest(W)], [text], {"none": True}),
            Case("int32_max", [W], [2 ** 31 - 1], [text], {"none": True}),
            Case("records_shorter_than_the_matrix", [W], [po.lowest(W) + 1], [text[:19], text[:1], text[:7]], {"none": True})]


# ---- seams -----------------------------------------------------------------------------------------------------------------------
def seam_boundaries(lane_starts, wave_starts, wg_starts):
    return {"word32": 32, "word64": 64, "lane": max(2, lane_starts), "wave": wave_starts, "wg": wg_starts, "wg2": 2 * wg_starts}


def seam_cases(lane_starts, wave_starts, wg_starts, m=12):
    """Per boundary B: one record per offset o = -m ... +1 with the top-scoring site at the 0-based start B + o (the 1-based
    start B + o + 1), so a site begins at, ends at and lies across every multiple; one record with the site at its last possible
    start; and two records that hold the two halves of a site at their common end, which is no hit."""
    out = []
    for name, B in seam_boundaries(lane_starts, wave_starts, wg_starts).items():
        rng = np.random.default_rng(B)
        W = rand_matrix(rng, m, constant=(4, 5))
        site = best_site(W)
        recs, hits = [], []
        for o in range(-m, 2):
            if B + o < 0:
                continue
            t = bytearray(rand_dna(rng, B + 40 + int(rng.integers(0, 30))))
            plant(t, B + o, site)
            hits.append((0, len(recs), B + o + 1))
            recs.append(bytes(t))
        t = bytearray(rand_dna(rng, B + m))                             # its last possible start is the 0-based B
        plant(t, B, site)
        hits.append((0, len(recs), B + 1))
        recs.append(bytes(t))
        left, right = bytearray(rand_dna(rng, B + 5)), bytearray(rand_dna(rng, 50))
        left[-5:], right[:m - 5] = site[:5], site[5:]
        absent = [(0, len(recs), B + 1)]
        recs += [bytes(left), bytes(right)]
        out.append(Case(f"{name}_seam", [W], [po.highest(W) - 150], recs, {"hits": hits, "absent": absent}))
    return out


# ---- arithmetic ------------------------------------------------------------------------------------------------------------------
def arithmetic_cases():
    rng = np.random.default_rng(9)
    out = []
    text = rand_dna(rng, 4000)
    lo64, hi64 = np.full((64, 4), -32768, dtype=np.int64), np.full((64, 4), 32767, dtype=np.int64)
    out.append(Case("all_lowest_weights", [lo64], [64 * -32768 + 1], [text], {"none": True}))
    out.append(Case("all_highest_weights", [hi64], [64 * 32767 + 1], [text], {"none": True}))
    ext = lo64.copy()
    ext[np.arange(64), rng.integers(0, 4, size=64)] = 32767
    t = bytearray(text)
    plant(t, 1000, best_site(ext))
    near = bytearray(best_site(ext))
    near[17] = BASES[(int(np.argmax(ext[17])) + 1) % 4]
    plant(t, 2000, bytes(near))
    out.append(Case("extreme_weights_top", [ext, ext], [64 * 32767, 64 * 32767 - 65535], [bytes(t)],
                    {"hits": [(0, 0, 1001), (1, 0, 1001), (1, 0, 2001)], "absent": [(0, 0, 2001)]}))
    out.append(Case("extreme_weights_lowest_plus_one", [ext], [64 * -32768 + 1], [bytes(t)[:2500]], {"hits": [(0, 0, 1001)], "many": 2000}))
    W = rand_matrix(rng, 17, constant=(3,))
    site = bytearray(best_site(W))
    site[5] = BASES[int(np.argsort(W[5])[1])]
    s = score(W, bytes(site))
    t = bytearray(b"".join(BASES[np.asarray(W).argmin(axis=1)].tobytes() for _ in range(40)))
    plant(t, 333, bytes(site))
    out.append(Case("threshold_is_the_score", [W, W], [s, s + 1], [bytes(t)], {"hits": [(0, 0, 334)], "absent": [(1, 0, 334)]}))
    neg = -np.abs(rand_matrix(rng, 9, lo=-500, hi=-1)) - 1
    t = bytearray(rand_dna(rng, 3000))
    plant(t, 77, best_site(neg))
    out.append(Case("negative_thresholds", [neg, neg], [po.highest(neg), po.highest(neg) - 300], [bytes(t)], {"hits": [(0, 0, 78), (1, 0, 78)], "many": 3}))
    one = np.repeat(rng.integers(-50, 50, size=(39, 1)), 4, axis=1).astype(np.int64)
    one[20] = [-7, 11, -7, 3]
    out.append(Case("one_row_is_not_constant", [one], [po.highest(one)], [rand_dna(rng, 2000) + b"NNNCNN" + rand_dna(rng, 30)], {"many": 400}))
    three = np.repeat(rng.integers(-50, 50, size=(10, 1)), 4, axis=1).astype(np.int64)
    three[np.arange(10), rng.integers(0, 4, size=10)] -= 1             # constant but for the base that sets the minimum (and N)
    t = bytearray(rand_dna(rng, 3000))
    plant(t, 500, best_site(three))
    t[1000:1012] = b"N" * 12
    out.append(Case("constant_but_for_the_minimum", [three, three], [po.highest(three), po.highest(three) - 1], [bytes(t)],
                    {"hits": [(0, 0, 501), (1, 0, 501)], "absent": [(1, 0, 1001)], "many": 100}))
    return out


# ---- alphabet --------------------------------------------------------------------------------------------------------------------
def alphabet_cases():
    rng = np.random.default_rng(10)
    out = []
    W = rand_matrix(rng, 14)
    W[:, 3] = W.max(axis=1) + 5                                         # T is the best base of every row
    site = best_site(W)
    assert site == b"T" * 14
    t = bytearray(rand_dna(rng, 3000).replace(b"TTT", b"TAT"))
    plant(t, 400, site)
    plant(t, 800, site[:6] + b"N" + site[7:])                           # a site only if N were T
    plant(t, 1200, b"N" * 14)
    plant(t, 1600, b"NNNN" + site + b"NNNN")
    plant(t, 2000, site.lower())
    t[2200:2300] = bytes(t[2200:2300]).lower()
    out.append(Case("n_is_not_t", [W], [po.highest(W)], [bytes(t)],
                    {"hits": [(0, 0, 401), (0, 0, 1605), (0, 0, 2001)], "absent": [(0, 0, 801), (0, 0, 1201)]}))
    low = bytes(t).lower()
    out.append(Case("lower_case", [W], [po.highest(W) - 400], [low, low.upper()[:1000] + low[1000:]], {"hits": [(0, 0, 401), (0, 1, 2001)], "many": 6}))
    M = rand_matrix(rng, 8)
    t2 = bytearray(rand_dna(rng, 1500))
    t2[:20] = b"N" * 20
    t2[-20:] = b"N" * 20
    t2[700:760] = b"N" * 60
    plant(t2, 20, best_site(M))
    plant(t2, 692, best_site(M))
    plant(t2, 760, best_site(M))
    plant(t2, 1500 - 28, best_site(M))
    out.append(Case("runs_of_n", [M], [po.highest(M) - 200], [bytes(t2), b"N" * 100, b"N" * 7],
                    {"hits": [(0, 0, 21), (0, 0, 693), (0, 0, 761), (0, 0, 1473)], "absent": [(0, 0, 700), (0, 1, 1)]}))
    return out


# ---- batch -----------------------------------------------------------------------------------------------------------------------
def batch_case():
    rng = np.random.default_rng(11)
    ms = (1, 6, 13, 24, 39, 40, 57, 64)
    mats = [rand_matrix(rng, m, constant=range(7, 30) if m == 39 else (2,) if m > 6 else ()) for m in ms]
    recs = [bytearray(rand_dna(rng, n)) for n in (9000, 50, 2600, 12)]
    hits = []
    for i, W in enumerate(mats):
        plant(recs[0], 300 + 900 * i, best_site(W))
        hits.append((i, 0, 301 + 900 * i))
    plant(recs[2], 2600 - 64, best_site(mats[7]))
    hits.append((7, 2, 2600 - 63))
    thr = [po.highest(W) - d for W, d in zip(mats, (0, 100, 300, 500, 700, 900, 1100, 1300))]
    return Case("batch_of_eight", mats, thr, [bytes(r) for r in recs], {"hits": hits, "many": 30})


def host_cases():
    return (length_cases() + [tiny_records_case()] + empty_cases() + seam_cases(*HOST_GEOMETRY) + arithmetic_cases() + alphabet_cases()
            + [batch_case()])
