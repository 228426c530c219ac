"""The hit aligner's model, stated on its own: what kgma_align.hip and kgma_align_host.cpp must compute.

Written from the definition below, not from either implementation (neither a trace matrix nor their H/D/I recurrence appears here).

The model.  The consensus `a` (length m >= 1) is aligned globally against the segment `b` (length n).
  * codes: A/C/G/T in either case are 0..3; N and every other byte are 4;
  * substitution scores: equal bases +5, different bases -4, N-N -1, N-base -2;
  * a gap of length L scores gap_open + L * gap_extend, both scores <= 0;
  * runs of unaligned segment residues ('D') before the first or after the last consensus position are free.
So the optimum is the best ordinary global affine-gap score of `a` against any substring b[s:e], the empty one included.

  optimum_bruteforce   exactly that sentence, cell by cell, for tiny inputs;
  optimum              one vectorised row per consensus position, any size;
  rescore              the score of a given CIGAR under the model, after checking that it is a well-formed alignment of a and b.
A CIGAR consumes the consensus with '=', 'X', 'I' and the segment with '=', 'X', 'D' (BioAlignments' orientation for
pairalign(SemiGlobalAlignment(), consensus, segment)).
"""
import re

import numpy as np

NEG = -(1 << 60)          # "no alignment ends here"; far below any score, far above int64's minimum

_CODE = np.full(256, 4, dtype=np.int64)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i   # lower case

SUB = np.full((5, 5), -4, dtype=np.int64)
SUB[np.arange(4), np.arange(4)] = 5
SUB[4, :] = SUB[:, 4] = -2
SUB[4, 4] = -1
_SUB_ROWS = SUB.tolist()


def codes(s: bytes) -> np.ndarray:
    return _CODE[np.frombuffer(bytes(s), dtype=np.uint8)]


def _global_all_ends(sa, sb, go, ge):
    """Ordinary global Gotoh DP of the coded consensus sa against sb, cell by cell.  Returns, for every e, the global score of sa
    against sb[:e] (cell (m, e) of a global DP is by definition the global score against that prefix).  Three states: M ends in an
    aligned pair, X in a consensus residue against a gap, Y in a segment residue against a gap."""
    m, n = len(sa), len(sb)
    sub = _SUB_ROWS
    M = [[NEG] * (n + 1) for _ in range(m + 1)]
    X = [[NEG] * (n + 1) for _ in range(m + 1)]
    Y = [[NEG] * (n + 1) for _ in range(m + 1)]
    M[0][0] = 0
    for i in range(1, m + 1):
        X[i][0] = go + i * ge
    for j in range(1, n + 1):
        Y[0][j] = go + j * ge
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            M[i][j] = max(M[i - 1][j - 1], X[i - 1][j - 1], Y[i - 1][j - 1]) + sub[sa[i - 1]][sb[j - 1]]
            X[i][j] = max(max(M[i - 1][j], Y[i - 1][j]) + go + ge, X[i - 1][j] + ge)
            Y[i][j] = max(max(M[i][j - 1], X[i][j - 1]) + go + ge, Y[i][j - 1] + ge)
    return [max(M[m][e], X[m][e], Y[m][e]) for e in range(n + 1)]


def optimum_bruteforce(a: bytes, b: bytes, go: int, ge: int) -> int:
    """max over all substrings b[s:e] (the empty one included) of the global affine-gap score of a against b[s:e].  For m, n <= ~10."""
    assert go <= 0 and ge <= 0 and len(a) >= 1
    sa, sb = codes(a).tolist(), codes(b).tolist()
    best = go + len(a) * ge                                   # the empty substring: the consensus against one gap
    for s in range(len(b) + 1):
        best = max(best, max(_global_all_ends(sa, sb[s:], go, ge)))
    return best


def optimum(a: bytes, b: bytes, go: int, ge: int) -> int:
    """The same optimum for any size, one vectorised row of the segment per consensus position.

    Per row i, over columns j = 0..n:
      ins[j]   best alignment of a[:i] with some b[s:j] that ends with a[i-1] against a gap;
      match[j] ... that ends with a[i-1] paired with b[j-1];
      Ht       max(match, ins);
      D[j]     ... that ends with b[j-1] against a gap = max over j' < j of Ht[j'] - open - (j - j') * ext: a horizontal gap is
               opened once, from an alignment that does not itself end in one (merging two gaps never costs more, as go <= 0), so
               a prefix maximum of Ht[j'] + j' * ext does it;
      H        max(Ht, D).
    Row 0 is all zero (an unaligned prefix of b is free); on the last row trailing gaps are free, so D is the plain prefix maximum."""
    assert go <= 0 and ge <= 0 and len(a) >= 1
    op, ex = -int(go), -int(ge)
    ca, cb = codes(a), codes(b)
    m, n = len(ca), len(cb)
    subrows = np.concatenate([np.full((5, 1), NEG, dtype=np.int64), SUB[:, cb]], axis=1)   # column 0 pairs with nothing
    jx = np.arange(n + 1, dtype=np.int64) * ex
    H = np.zeros(n + 1, dtype=np.int64)
    ins = np.full(n + 1, NEG, dtype=np.int64)
    Hd = np.empty(n + 1, dtype=np.int64)                      # H of the row above, shifted one column right
    Hd[0] = NEG
    D = np.empty(n + 1, dtype=np.int64)
    D[0] = NEG
    for i in range(1, m + 1):
        np.maximum(H - (op + ex), ins - ex, out=ins)
        Hd[1:] = H[:-1]
        np.maximum(Hd + subrows[ca[i - 1]], ins, out=H)      # H holds Ht from here
        if i < m:
            D[1:] = np.maximum.accumulate(H + jx)[:-1]
            D[1:] -= jx[1:] + op
        else:
            D[1:] = np.maximum.accumulate(H)[:-1]
        np.maximum(H, D, out=H)
    return int(H[n])


_RUN = re.compile(r"(\d+)([=XDI])")


def runs(cigar: str):
    """[(length, op)] of a CIGAR; the string must be exactly what those runs spell, every run non-empty."""
    out = [(int(x), o) for x, o in _RUN.findall(cigar)]
    assert "".join(f"{x}{o}" for x, o in out) == cigar, f"CIGAR {cigar!r} does not round-trip"
    assert all(x >= 1 for x, _ in out), f"CIGAR {cigar!r} has an empty run"
    return out


def rescore(cigar: str, a: bytes, b: bytes, go: int, ge: int) -> int:
    """Score of `cigar` as an alignment of a against b under the model; AssertionError if it is not a well-formed one."""
    rr = runs(cigar)
    assert all(rr[k][1] != rr[k + 1][1] for k in range(len(rr) - 1)), f"CIGAR {cigar!r}: adjacent runs of one op"
    ca, cb = codes(a), codes(b)
    m, n = len(ca), len(cb)
    i = j = 0
    score = 0
    for L, o in rr:
        if o in "=X":
            assert i + L <= m and j + L <= n, f"CIGAR {cigar!r} runs off a sequence"
            x, y = ca[i:i + L], cb[j:j + L]
            same = (x == y) & (x < 4)
            assert bool(same.all()) if o == "=" else not bool(same.any()), f"CIGAR {cigar!r}: '{o}' run at ({i}, {j}) mislabels a pair"
            score += int(SUB[x, y].sum())
            i += L
            j += L
        elif o == "I":
            assert i + L <= m, f"CIGAR {cigar!r} runs off the consensus"
            score += go + L * ge
            i += L
        else:
            assert j + L <= n, f"CIGAR {cigar!r} runs off the segment"
            if 0 < i < m:
                score += go + L * ge
            j += L
    assert (i, j) == (m, n), f"CIGAR {cigar!r} consumes ({i}, {j}) of ({m}, {n})"
    return score
