"""Case builders of the codon-weight-matrix search tests (tests/test_codon_host.py checks that every list hits what it is for;
tests/test_gpu_codon.py runs them on the device with the library's real geometry).

A case is a Case(name, matrices, thresholds, records, aim): the matrices are CODON matrices, (m, 65); `aim` says what the case is
for in a form the host test checks -- "hits": (matrix, record, start) triples the oracle must report, "absent": triples it must
not, "none": the list is empty, "many": it has more entries than that."""
from typing import NamedTuple

import numpy as np

from tests import codon_oracle as co

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
LENGTHS = (1, 2, 21, 22, 63, 64)
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
    """m rows of 65 weights in lo ... hi, every row with one strict maximum among its 64 codons and the ambiguous entry at the
    row's minimum; the rows of `constant` are 65 equal weights."""
    W = rng.integers(lo, hi, size=(m, 65)).astype(np.int64)
    for i in range(m):
        W[i, int(rng.integers(0, 64))] = hi + 1 + int(rng.integers(0, 20))
        W[i, 64] = W[i, :64].min()
        if i in constant:
            W[i, :] = int(rng.integers(lo, hi))
    return W


def codon_text(c: int) -> bytes:
    return bytes([b"ACGT"[c >> 4], b"ACGT"[(c >> 2) & 3], b"ACGT"[c & 3]])


def best_site(W) -> bytes:
    """The top-scoring sequence (the first maximum of every row among the 64 codons)."""
    return b"".join(codon_text(int(c)) for c in np.asarray(W)[:, :64].argmax(axis=1))


def worst_site(W) -> bytes:
    return b"".join(codon_text(int(c)) for c in np.asarray(W)[:, :64].argmin(axis=1))


def plant(text: bytearray, start0: int, site: bytes) -> None:
    assert 0 <= start0 and start0 + len(site) <= len(text), (start0, len(site), len(text))
    text[start0:start0 + len(site)] = site


# ---- lengths ---------------------------------------------------------------------------------------------------------------------
def length_cases():
    """Per m: a long record with a site in its middle and one at its last valid start, and records of 3m - 1, 3m, 3m + 1 and
    3m + 2 residues that hold the site (but for the first, which is too short for any start)."""
    out = []
    for m in LENGTHS:
        rng = np.random.default_rng(200 + m)
        W = rand_matrix(rng, m, constant=(1, 2, 7, 30, 31, 40) if m >= 21 else ())
        site = best_site(W)
        big = bytearray(rand_dna(rng, 3001))
        plant(big, 1500, site)
        plant(big, 3001 - 3 * m, site)                                 # the last valid start
        x1, x2 = rand_dna(rng, 1), rand_dna(rng, 2)
        recs = [bytes(big), site[:-1], site, x1 + site, site + x2, x2 + site]
        thr = co.highest(W) - (0 if m <= 2 else 250)                   # (short matrices hit often as it is)
        out.append(Case(f"m{m}", [W], [thr], recs,
                        {"hits": [(0, 0, 1501), (0, 0, 3001 - 3 * m + 1), (0, 2, 1), (0, 3, 2), (0, 4, 1), (0, 5, 3)], "absent": [(0, 1, 1)]}))
    return out


def tiny_records_case():
    rng = np.random.default_rng(7)
    recs = [rand_dna(rng, int(n)) for n in rng.integers(1, 6, size=300)]
    W = np.zeros((1, 65), dtype=np.int64)
    W[0, co.codon_index(b"ACG")] = 3
    W[0, co.codon_index(b"TAC")] = 2
    want = next(c for c, r in enumerate(recs) if r[:3] == b"ACG")
    return Case("tiny_records", [W, np.concatenate([W, W])], [2, 99], recs, {"hits": [(0, want, 1)], "many": 5})


def empty_cases():
    rng = np.random.default_rng(8)
    W = rand_matrix(rng, 20)
    text = rand_dna(rng, 5000)
    return [Case("above_the_highest", [W], [co.highest(W) + 1], [text], {"none": True}),
            Case("nothing_reaches_it", [W], [co.highest(W)], [text], {"none": True}),
            Case("int32_max", [W], [2 ** 31 - 1], [text], {"none": True}),
            Case("records_shorter_than_the_site", [W], [co.lowest(W) + 1], [text[:59], text[:1], text[:7]], {"none": True})]


# ---- seams -----------------------------------------------------------------------------------------------------------------------
def seam_boundaries(lane_starts, wave_starts, wg_starts):
    return {"lane": max(2, lane_starts), "row": 64 * lane_starts, "wave": wave_starts, "wg": wg_starts, "wg2": 2 * wg_starts}


def seam_cases(lane_starts, wave_starts, wg_starts, m=5):
    """Per boundary B: one record per offset o = -3m ... +3 with the top-scoring site at the 0-based start B + o (the 1-based
    start B + o + 1), so in each of the three frames a site begins at, ends at and lies across every multiple; one record with
    the site at its last possible start; and two records that hold the two halves of a site at their common end, no hit."""
    out = []
    for name, B in seam_boundaries(lane_starts, wave_starts, wg_starts).items():
        rng = np.random.default_rng(B)
        W = rand_matrix(rng, m, constant=(3,))
        site = best_site(W)
        recs, hits = [], []
        for o in range(-3 * m, 4):
            if B + o < 0:
                continue
            t = bytearray(rand_dna(rng, B + 40 + int(rng.integers(0, 30))))
            plant(t, B + o, site)
            hits.append((0, len(recs), B + o + 1))
            recs.append(bytes(t))
        t = bytearray(rand_dna(rng, B + 3 * m))                         # its last possible start is the 0-based B
        plant(t, B, site)
        hits.append((0, len(recs), B + 1))
        recs.append(bytes(t))
        left, right = bytearray(rand_dna(rng, B + 7)), bytearray(rand_dna(rng, 50))
        left[-7:], right[:3 * m - 7] = site[:7], site[7:]
        absent = [(0, len(recs), B + 1)]
        recs += [bytes(left), bytes(right)]
        out.append(Case(f"{name}_seam", [W], [co.highest(W) - 150], recs, {"hits": hits, "absent": absent}))
    return out


# ---- arithmetic ------------------------------------------------------------------------------------------------------------------
def arithmetic_cases():
    rng = np.random.default_rng(9)
    out = []
    text = rand_dna(rng, 4000)
    lo64, hi64 = np.full((64, 65), -32768, dtype=np.int64), np.full((64, 65), 32767, dtype=np.int64)
    out.append(Case("all_lowest_weights", [lo64], [64 * -32768 + 1], [text], {"none": True}))
    out.append(Case("all_highest_weights", [hi64], [64 * 32767 + 1], [text], {"none": True}))
    ext = lo64.copy()
    ext[np.arange(64), rng.integers(0, 64, size=64)] = 32767
    t = bytearray(text)
    plant(t, 1000, best_site(ext))
    near = bytearray(best_site(ext))
    near[3 * 17:3 * 17 + 3] = codon_text((int(np.argmax(ext[17, :64])) + 1) % 64)
    plant(t, 2000, bytes(near))
    out.append(Case("extreme_weights_top", [ext, ext], [64 * 32767, 64 * 32767 - 65535], [bytes(t)],
                    {"hits": [(0, 0, 1001), (1, 0, 1001), (1, 0, 2001)], "absent": [(0, 0, 2001)]}))
    out.append(Case("extreme_weights_lowest_plus_one", [ext], [64 * -32768 + 1], [bytes(t)[:2500]], {"hits": [(0, 0, 1001)], "many": 1000}))   # (1 - (63/64)^64 = 0.63 of the 2309 starts hold a top codon)
    W = rand_matrix(rng, 17, constant=(3,))
    site = bytearray(best_site(W))
    site[15:18] = codon_text(int(np.argsort(W[5, :64])[-2]))
    s = co.score_at(W, bytes(site), 1)
    t = bytearray(worst_site(W) * 40)
    plant(t, 333, bytes(site))
    out.append(Case("threshold_is_the_score", [W, W], [s, s + 1], [bytes(t)], {"hits": [(0, 0, 334)], "absent": [(1, 0, 334)]}))
    neg = -np.abs(rand_matrix(rng, 9, lo=-500, hi=-1)) - 1
    t = bytearray(rand_dna(rng, 3000))
    plant(t, 77, best_site(neg))
    out.append(Case("negative_thresholds", [neg, neg], [co.highest(neg), co.highest(neg) - 300], [bytes(t)], {"hits": [(0, 0, 78), (1, 0, 78)]}))
    one = np.repeat(rng.integers(-50, 50, size=(39, 1)), 65, axis=1).astype(np.int64)
    one[20, :] = -7
    one[20, [co.codon_index(b"TGG"), co.codon_index(b"ATG")]] = 11
    t = bytearray(rand_dna(rng, 2000) + b"NNNTGGNN" + rand_dna(rng, 130))
    plant(t, 500, b"TGG")
    out.append(Case("one_row_is_not_constant", [one], [co.highest(one)], [bytes(t)], {"hits": [(0, 0, 501 - 60), (0, 0, 2004 - 60)], "many": 30}))
    only_n = np.repeat(rng.integers(-50, 50, size=(6, 1)), 65, axis=1).astype(np.int64)
    only_n[2, 64] -= 1                                                  # constant but for the ambiguous entry
    t = bytearray(rand_dna(rng, 600))
    t[300] = ord("N")
    out.append(Case("constant_but_for_the_ambiguous_entry", [only_n], [co.highest(only_n)], [bytes(t)],
                    {"hits": [(0, 0, 1), (0, 0, 292), (0, 0, 296)], "absent": [(0, 0, 293), (0, 0, 294), (0, 0, 295)], "many": 500}))
    return out


# ---- alphabet --------------------------------------------------------------------------------------------------------------------
def alphabet_cases():
    rng = np.random.default_rng(10)
    out = []
    W = rand_matrix(rng, 6)
    W[:, 63] = W.max(axis=1) + 5                                        # TTT is the best codon of every row
    site = best_site(W)
    assert site == b"T" * 18
    t = bytearray(rand_dna(rng, 3000).replace(b"TTT", b"TAT"))
    plant(t, 400, site)
    for k in range(3):                                                  # a site only if N were T: N at each codon position
        plant(t, 800 + 100 * k, site[:6 + k] + b"N" + site[7 + k:])
    plant(t, 1200, b"N" * 18)
    plant(t, 1600, b"NNNN" + site + b"NNNN")
    plant(t, 2000, site.lower())
    t[2200:2300] = bytes(t[2200:2300]).lower()
    out.append(Case("n_is_not_t", [W], [co.highest(W)], [bytes(t)],
                    {"hits": [(0, 0, 401), (0, 0, 1605), (0, 0, 2001)], "absent": [(0, 0, 801), (0, 0, 901), (0, 0, 1001), (0, 0, 1201)]}))
    # the ambiguous entry is a weight like any other: here it is the best one, and the hits are the starts whose six codons all
    # touch the run of 18 N at the 0-based 1200 ... 1217: the 0-based starts 1198 ... 1202
    Wn = W.copy()
    Wn[:, 64] = Wn.max(axis=1) + 1
    out.append(Case("n_scores_its_own_entry", [Wn], [co.highest(Wn)], [bytes(t)],
                    {"hits": [(0, 0, s) for s in range(1199, 1204)], "absent": [(0, 0, 401), (0, 0, 1198), (0, 0, 1204)]}))
    low = bytes(t).lower()
    out.append(Case("lower_case", [W], [co.highest(W) - 300], [low, low.upper()[:1000] + low[1000:]], {"hits": [(0, 0, 401), (0, 1, 2001)], "many": 3}))
    M = rand_matrix(rng, 4)
    t2 = bytearray(rand_dna(rng, 1500))
    t2[:20] = b"N" * 20
    t2[-20:] = b"N" * 20
    t2[700:760] = b"N" * 60
    plant(t2, 20, best_site(M))
    plant(t2, 688, best_site(M))
    plant(t2, 760, best_site(M))
    plant(t2, 1500 - 32, best_site(M))
    out.append(Case("runs_of_n", [M], [co.highest(M) - 200], [bytes(t2), b"N" * 100, b"N" * 7],
                    {"hits": [(0, 0, 21), (0, 0, 689), (0, 0, 761), (0, 0, 1469)], "absent": [(0, 0, 700), (0, 1, 1)]}))
    return out


# ---- batch -----------------------------------------------------------------------------------------------------------------------
def rand_profile(rng, m, lo=-300, hi=300) -> np.ndarray:
    """An (m, 21) amino-acid profile, every row with one strict maximum among the 20 amino acids and the stop at the minimum."""
    P = rng.integers(lo, hi, size=(m, 21)).astype(np.int64)
    for i in range(m):
        P[i, int(rng.integers(0, 20))] = hi + 1 + int(rng.integers(0, 20))
        P[i, 20] = lo - 1
    return P


def batch_case():
    """Eight amino-acid profiles folded for both strands: sixteen codon matrices, (2 i) the plus and (2 i + 1) the minus one
    of profile i; each profile's best site lies once on each strand of the first record."""
    rng = np.random.default_rng(11)
    ms = (1, 2, 5, 8, 13, 21, 40, 64)
    profs = [rand_profile(rng, m) for m in ms]
    recs = [bytearray(rand_dna(rng, n)) for n in (9000, 50, 2600, 12)]
    mats, hits = [], []
    for i, P in enumerate(profs):
        plus, minus = co.fold(P), co.fold(P, minus=True)
        mats += [plus, minus]
        plant(recs[0], 300 + 1000 * i, best_site(plus))
        plant(recs[0], 300 + 1000 * i + 3 * 64 + 5, best_site(minus))
        hits += [(2 * i, 0, 301 + 1000 * i), (2 * i + 1, 0, 301 + 1000 * i + 3 * 64 + 5)]
    plant(recs[2], 2600 - 192, best_site(mats[14]))
    hits.append((14, 2, 2600 - 191))
    thr = [co.highest(W) - d for W, d in zip(mats, (0, 0, 0, 0, 300, 300, 500, 500, 700, 700, 900, 900, 1100, 1100, 1300, 1300))]
    return Case("batch_of_eight_on_both_strands", mats, thr, [bytes(r) for r in recs], {"hits": hits, "many": 30}), profs


# ---- the family: a position weight matrix of 3 m rows as a codon matrix ------------------------------------------------------------
def codon_matrix_of_pwm(W) -> np.ndarray:
    """row_i[c] = W[3i][b0] + W[3i + 1][b1] + W[3i + 2][b2]; the ambiguous entry is never read on an N-free text (0)."""
    W = np.asarray(W).astype(np.int64)
    assert W.shape[0] % 3 == 0 and W.shape[1] == 4
    out = np.zeros((W.shape[0] // 3, 65), dtype=np.int64)
    for i in range(out.shape[0]):
        for c in range(64):
            out[i, c] = W[3 * i, c >> 4] + W[3 * i + 1, (c >> 2) & 3] + W[3 * i + 2, c & 3]
    return out


def host_cases():
    return (length_cases() + [tiny_records_case()] + empty_cases() + seam_cases(*HOST_GEOMETRY) + arithmetic_cases() + alphabet_cases()
            + [batch_case()[0]])
