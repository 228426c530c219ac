"""The Float64 KFV scan in exact arithmetic, and an a-priori bound on what Float64 may make of it.  Plain Python: `fractions`, no
numpy arithmetic, nothing from the library under test, nothing from the oracle.

Every Float64 entry of a KFV is the rational it is.  For the windows q = 0, 1, ... of a record (W residues each, n = W - k + 1 k-mers)

  exact[q] = (1 / 2k) sum_x (ref[x] - c_q[x])^2,

computed once from the first window's counts and then incrementally: with l the k-mer that leaves and r the one that enters,
nothing happens if l == r, else exact += (1 / k) ((1 + c[r]) + ref[l] - ref[r] - c[l]) with the counts of the window before the
step -- the update of src/GenomeMiner.jl:66-77 without its roundings.  Residues through the reference's code table (A0 C1 G2 T3,
N -> T, either case; natural k-mer value, first base most significant).

The bound, from exact quantities of the same pass and never from the code under test (u = 2^-53, SF = 1 / k, P = non-zero
entries of the KFV):

  A_q      = sum ref^2 + 2 sum_{p in window q} |ref[K_p]| + n + 2 pairs_q         (pairs_q = sum_x c_q[x] (c_q[x] - 1) / 2)
  M_i      = (1 + c[r]) + |ref[l]| + |ref[r]| + c[l] of the step into window i, 0 if l == r
  bound[q] = u [ (max(P, n) + 5) (SF / 2) max_{i <= q} A_i + (q + 4) SF sum_{i <= q} M_i ]

It holds for the first-window identity SF/2 ((sum ref^2 - 2 sum_p ref[K_p]) + (n + 2 pairs)) of a stream that starts at any
window i <= q plus a sum, in any order, of that stream's increments -- and for the reference's left-to-right first window plus its
serial chain ("The Float64 scan in exact arithmetic", has the derivation).  It does not know the stream length or the
shape of a prefix tree, and it is not tuned: a value outside it is a finding about the code or about the derivation.

A KFV is a dense sequence of 4^k floats or a pair (keys, values) of its non-zero entries (natural k-mer values)."""
from fractions import Fraction

U = Fraction(1, 2 ** 53)

_CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3, ord("N"): 3}


def kmers(seq: bytes, k: int, n_as: int = 3):
    """Natural value of the k-mer at every position of seq (n_as: the code N takes; the library's is 3 = T)."""
    code = dict(_CODE)
    code[ord("N")] = n_as
    c = [code[b & 0xDF] for b in seq]
    out = []
    if len(c) < k:
        return out
    v = 0
    mask = 4 ** k - 1
    for j, x in enumerate(c):
        v = ((v << 2) | x) & mask
        if j >= k - 1:
            out.append(v)
    return out


def entries(kfv) -> dict:
    """{natural k-mer value: Fraction} of the KFV's non-zero entries (-0.0 is zero)."""
    if isinstance(kfv, tuple):
        keys, vals = kfv
        return {int(x): Fraction(float(v)) for x, v in zip(keys, vals) if float(v) != 0.0}
    return {x: Fraction(float(v)) for x, v in enumerate(kfv) if float(v) != 0.0}


class Record:
    """exact[q], bound[q] (Fractions) of every window of one record; inc[q] the exact increment into window q (inc[0] = 0) and
    A[q], M[q] the magnitudes the bound is made of."""
    __slots__ = ("exact", "bound", "inc", "A", "M")

    def __init__(self):
        self.exact, self.bound, self.inc, self.A, self.M = [], [], [], [], []


def scan(seq: bytes, kfv, k: int, W: int, n_as: int = 3, R=None) -> Record:
    """The windows of one record (none if it is shorter than W).  R: entries(kfv), for callers with many records."""
    out = Record()
    n = W - k + 1
    if len(seq) < W or n < 1:
        return out
    R = entries(kfv) if R is None else R
    get = R.get
    Z = Fraction(0)
    P = len(R)
    sum_r2 = sum((r * r for r in R.values()), Z)
    km = kmers(seq, k, n_as)
    cnt = {}
    for x in km[:n]:
        cnt[x] = cnt.get(x, 0) + 1
    tot = sum_r2                                                   # sum_x (ref[x] - c[x])^2 of the window in hand
    for x, c in cnt.items():
        r = get(x, Z)
        tot += (r - c) ** 2 - r * r
    absw = sum((abs(get(x, Z)) for x in km[:n]), Z)
    pairs = sum(c * (c - 1) // 2 for c in cnt.values())
    sf = Fraction(1, k)
    lead = (max(P, n) + 5) * sf / 2
    max_a = sum_r2 + 2 * absw + n + 2 * pairs
    sum_m = Z
    out.exact.append(tot / (2 * k)); out.inc.append(Z); out.A.append(max_a); out.M.append(Z)
    out.bound.append(U * (lead * max_a + 4 * sf * sum_m))
    for q in range(1, len(seq) - W + 1):
        l, r = km[q - 1], km[q - 1 + n]
        inc = m = Z
        if l != r:
            cp, cs = cnt.get(r, 0), cnt[l]
            rl, rr = get(l, Z), get(r, Z)
            inc = ((1 + cp) + rl - rr - cs) * sf
            m = (1 + cp) + abs(rl) + abs(rr) + cs
            cnt[r] = cp + 1
            cnt[l] = cs - 1
            pairs += cp - (cs - 1)
            absw += abs(rr) - abs(rl)
            tot += 2 * k * inc
            sum_m += m
        a = sum_r2 + 2 * absw + n + 2 * pairs
        if a > max_a:
            max_a = a
        out.exact.append(tot / (2 * k)); out.inc.append(inc); out.A.append(a); out.M.append(m)
        out.bound.append(U * (lead * max_a + (q + 4) * sf * sum_m))
    return out


def window(seq: bytes, kfv, k: int, W: int, q: int, n_as: int = 3, R=None, sum_r2=None) -> Fraction:
    """exact[q] from scratch: the counts of window q alone (R: entries(kfv), sum_r2: the sum of their squares, for callers with many
    windows -- an entry the window does not touch contributes its square)."""
    R = entries(kfv) if R is None else R
    tot = sum((r * r for r in R.values()), Fraction(0)) if sum_r2 is None else sum_r2
    cnt = {}
    for x in kmers(seq[q:q + W], k, n_as):
        cnt[x] = cnt.get(x, 0) + 1
    for x, c in cnt.items():
        r = R.get(x, Fraction(0))
        tot += (r - c) * (r - c) - r * r
    return tot / (2 * k)


def lattice(dist: float, scale: float) -> int:
    """round-half-up of the Float64 product dist * scale: the integer the host keeps for a Float64 distance."""
    x = Fraction(dist * scale) + Fraction(1, 2)
    return x.numerator // x.denominator


def ulp(x: Fraction) -> Fraction:
    """The spacing of the Float64 numbers at |x| (normal range)."""
    x = abs(x)
    if x == 0:
        return Fraction(1, 2 ** 1074)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    return Fraction(2) ** (max(e, -1022) - 52)
