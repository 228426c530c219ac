"""CPU statement of the position-weight-matrix search (kgma_pwm_match / api.pwmMatch), in numpy.

A matrix is m rows of four integer weights in the order A, C, G, T.  Laid at the 1-based start s of a record t[1..L] with
s + m - 1 <= L it scores score(s) = sum_i W[i][t[s + i]]; case is folded and a genome N scores the row's minimum.  Every s with
score(s) >= threshold is a hit; no hit spans two records.  The profile is stated twice -- a loop over the rows, and one gather over
a sliding view of the record -- and tests/test_pwm_host.py holds each against the other."""
import json
import os
from fractions import Fraction

import numpy as np

from tests.motif_oracle import IUPAC, LOCI_RSSD_D1

_CODES = np.full(256, 255, dtype=np.uint8)
for _i, _ch in enumerate(b"ACGTN"):
    _CODES[_ch] = _CODES[bytes([_ch]).lower()[0]] = _i
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _bytes(x) -> bytes:
    return x.encode() if isinstance(x, str) else bytes(x)


def matrix(W) -> np.ndarray:
    W = np.asarray(W)
    if W.ndim != 2 or W.shape[1] != 4 or not 1 <= W.shape[0] <= 64 or W.dtype.kind not in "iu":
        raise ValueError("a matrix has 1 ... 64 rows of four integers")
    W = W.astype(np.int64)
    if (W < -32768).any() or (W > 32767).any():
        raise ValueError("weight outside -32768 ... 32767")
    return W


def residue_codes(seq) -> np.ndarray:
    """A 0, C 1, G 2, T 3, N 4, either case."""
    c = _CODES[np.frombuffer(_bytes(seq), dtype=np.uint8)]
    if (c == 255).any():
        raise ValueError("genome residue outside A/C/G/T/N")
    return c


def with_n(W) -> np.ndarray:
    """The matrix with a fifth column: what a genome N scores, the row's minimum."""
    W = matrix(W)
    return np.concatenate([W, W.min(axis=1, keepdims=True)], axis=1)


def lowest(W) -> int:
    return int(matrix(W).min(axis=1).sum())


def highest(W) -> int:
    return int(matrix(W).max(axis=1).sum())


def revcomp_matrix(W) -> np.ndarray:
    """Rows reversed, A <-> T and C <-> G swapped."""
    return matrix(W)[::-1, ::-1].copy()


def revcomp_text(seq) -> bytes:
    return _bytes(seq).translate(_COMP)[::-1]


def profile_rows(W, seq) -> np.ndarray:
    """score(s) for s = 1 ... L - m + 1 (empty when the matrix is longer than the record): row by row."""
    W5, c = with_n(W), residue_codes(seq)
    n = c.size - W5.shape[0] + 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    out = np.zeros(n, dtype=np.int64)
    for i in range(W5.shape[0]):
        out += W5[i][c[i:i + n]]
    return out


def profile_gather(W, seq) -> np.ndarray:
    """The same profile as one gather over the sliding view of the record."""
    W5, c = with_n(W), residue_codes(seq)
    m = W5.shape[0]
    if c.size < m:
        return np.zeros(0, dtype=np.int64)
    view = np.lib.stride_tricks.sliding_window_view(c, m)                  # [start, row]
    return W5[np.arange(m)[None, :], view].sum(axis=1, dtype=np.int64)


def find(W, seq, threshold):
    """[(start, score)] of one record, 1-based, ascending."""
    threshold = int(threshold)
    if threshold <= lowest(W):
        raise ValueError("the threshold must exceed the sum of the row minima")
    p = profile_rows(W, seq)
    idx = np.flatnonzero(p >= threshold)
    return list(zip((idx + 1).tolist(), p[idx].tolist()))


def match_list(matrices, records, thresholds):
    """(matrix, record, start, score), 0-based matrix and record, sorted by (matrix, record, start): what
    kgma_get_pwm_matches returns."""
    if isinstance(thresholds, int):
        thresholds = [thresholds] * len(matrices)
    return [(i, c, s, k) for i, (W, t) in enumerate(zip(matrices, thresholds)) for c, r in enumerate(records) for s, k in find(W, r, t)]


def api_list(W, records, threshold, strand="+"):
    """(record, lo, hi, strand, score) sorted by (record, lo, strand): api.pwmMatch_batch without the identifier."""
    m = matrix(W).shape[0]
    out = []
    if strand != "-":
        out += [(c, s, s + m - 1, "+", k) for c, r in enumerate(records) for s, k in find(W, r, threshold)]
    if strand != "+":
        out += [(c, s, s + m - 1, "-", k) for c, r in enumerate(records) for s, k in find(revcomp_matrix(W), r, threshold)]
    return sorted(out, key=lambda t: (t[0], t[1], t[3]))


# ---- the host mathematics around a matrix, stated independently of kmergma_amd.api ---------------------------------------------

def from_sequences(seqs, pseudocount=1.0, background=(.25, .25, .25, .25), scale=100) -> np.ndarray:
    """Log-odds matrix of equal-length A/C/G/T sites: rint(scale * log2(((count + pseudocount * bg) / (n + pseudocount)) / bg))."""
    rows = [_bytes(s).upper() for s in seqs]
    n, m = len(rows), len(rows[0])
    W = np.zeros((m, 4), dtype=np.int64)
    for i in range(m):
        for b, ch in enumerate(b"ACGT"):
            count = sum(1 for r in rows if r[i] == ch)
            W[i, b] = int(np.rint(scale * np.log2(((count + pseudocount * background[b]) / (n + pseudocount)) / background[b])))
    return W


def from_motif(motif):
    """(0/1 matrix, informative): weight 1 where the IUPAC symbol's set holds the base, four 0 for N."""
    sets = [IUPAC[chr(ch).upper()] for ch in _bytes(motif)]
    W = np.array([[0, 0, 0, 0] if s == 15 else [(s >> b) & 1 for b in range(4)] for s in sets], dtype=np.int64)
    return W, sum(1 for s in sets if s != 15)


def score_distribution(W, background=None) -> dict:
    """{score: probability} for independent bases: exact Fractions with the uniform background (None), floats otherwise."""
    bg = [Fraction(1, 4)] * 4 if background is None else [float(x) for x in background]
    dist = {0: Fraction(1) if background is None else 1.0}
    for row in matrix(W).tolist():
        nxt = {}
        for s, p in dist.items():
            for b in range(4):
                nxt[s + row[b]] = nxt.get(s + row[b], 0) + p * bg[b]
        dist = nxt
    return dist


def threshold(W, pvalue, background=None) -> int:
    """The smallest integer t with P(score >= t) <= pvalue; one above the highest score when no score is that rare."""
    dist = score_distribution(W, background)
    pvalue = Fraction(pvalue) if background is None else float(pvalue)
    t, tail = max(dist) + 1, 0
    for s in sorted(dist, reverse=True):
        tail += dist[s]
        if tail > pvalue:
            break
        t = s
    # (between two attainable scores every t has the tail of the next attainable one above it: the smallest such t follows
    #  the last score whose tail is too large)
    below = [s for s in dist if s < t]
    return max(below) + 1 if below else t


# ---- tests/golden/pwm.json -------------------------------------------------------------------------------------------------------
GOLDEN_PVALUES = ("1e-4", "1e-6", "1e-8")
RSS_LEN = 39
MADE_BY = "python -m tests.pwm_oracle"


def read_fasta_sequences(path):
    """The records' residues (plain reader: '>' starts a record)."""
    seqs, cur = [], None
    with open(path, "rb") as f:
        for line in f:
            line = line.strip()
            if line.startswith(b">"):
                cur = []
                seqs.append(cur)
            elif line and cur is not None:
                cur.append(line)
    return [b"".join(s) for s in seqs]


def loci_sites(records):
    """The seven 23-spacer recombination signal sequences behind the seven V genes of tests/data/Loci.fasta."""
    return [records[c][s - 1:s - 1 + RSS_LEN].upper() for c, s, _ in LOCI_RSSD_D1]


def make_golden(records, only_record=None):
    sites = loci_sites(records)
    W = from_sequences(sites)
    out = {"made_by": MADE_BY, "fasta": "tests/data/Loci.fasta", "sites": [s.decode() for s in sites], "matrix": W.tolist(),
           "lowest": lowest(W), "highest": highest(W), "thresholds": {}, "hits": {}}
    for p in GOLDEN_PVALUES:
        t = threshold(W, Fraction(p))
        out["thresholds"][p] = t
        hits = [[c, lo, hi, st, k] for c, lo, hi, st, k in api_list(W, records, t, "both")] if only_record is None else \
            [[only_record, lo, hi, st, k] for _, lo, hi, st, k in api_list(W, [records[only_record]], t, "both")]
        out["hits"][p] = hits
    return out


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    golden = make_golden(read_fasta_sequences(os.path.join(root, "tests", "data", "Loci.fasta")))
    with open(os.path.join(root, "tests", "golden", "pwm.json"), "w") as f:
        json.dump(golden, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("range", golden["lowest"], "...", golden["highest"])
    for p in GOLDEN_PVALUES:
        print(p, "threshold", golden["thresholds"][p], "hits", len(golden["hits"][p]), golden["hits"][p] if p != "1e-4" else "")
