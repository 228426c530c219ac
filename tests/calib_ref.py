"""Plain-Python reference for the calibration entry points (kgma_window_dists, kgma_mutation_dists): Python integers and
`fractions`, no numpy arithmetic, nothing from the library under test and nothing from kmergma_amd.api.

  D(seq, S, N, k)            sum_x (S[x] - N c[x])^2 of the whole sequence, c its k-mer counts (residues through the reference's
                             code table: A0 C1 G2 T3, N -> 3, either case; natural k-mer value, first base most significant)
  window_D(seq, S, N, k, W)  D of every window of W residues of seq, in order of their start
  mutate(seq, rate, seed, stream)   the mutation rule of kgma.h, restated from its text
  float_dist(seq, ref, k)    (1 / 2k) sum_x (ref[x] - c[x])^2 as an exact Fraction of the Float64 entries
"""
from fractions import Fraction

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3, ord("N"): 3}
# mutation_dict, src/DistanceTesting.jl:38-42
MUT = {"A": "CGT", "C": "AGT", "G": "CAT", "T": "CGA"}


def codes(seq: bytes):
    return [CODE[b & 0xDF] for b in seq]


def kmers(seq: bytes, k: int):
    """Natural value of the k-mer at every position of seq."""
    c = codes(seq)
    out = []
    for j in range(len(c) - k + 1):
        v = 0
        for t in range(k):
            v = v * 4 + c[j + t]
        out.append(v)
    return out


def counts(seq: bytes, k: int) -> dict:
    c = {}
    for v in kmers(seq, k):
        c[v] = c.get(v, 0) + 1
    return c


def sum_sq(S) -> int:
    return sum(int(x) * int(x) for x in S)


def D(seq: bytes, S, N: int, k: int, sumS2=None) -> int:
    """sum_x (S[x] - N c[x])^2 over all 4^k k-mers (S a sequence of 4^k integers, natural order)."""
    tot = sum_sq(S) if sumS2 is None else sumS2
    for x, cx in counts(seq, k).items():
        Sx = int(S[x])
        tot += (Sx - N * cx) ** 2 - Sx * Sx
    return tot


def window_D(seq: bytes, S, N: int, k: int, W: int):
    """D of the windows seq[s : s + W], s = 0 ... len - W, by sliding the counts (exact integers throughout)."""
    if len(seq) < W:
        return []
    N = int(N)
    Sl = [int(x) for x in S]
    km = kmers(seq, k)
    nk = W - k + 1
    c = {}
    d = sum_sq(Sl)

    def add(x, delta, d):
        old = c.get(x, 0)
        new = old + delta
        c[x] = new
        return d + (Sl[x] - N * new) ** 2 - (Sl[x] - N * old) ** 2

    for x in km[:nk]:
        d = add(x, 1, d)
    out = [d]
    for s in range(1, len(seq) - W + 1):
        d = add(km[s - 1], -1, d)
        d = add(km[s + nk - 1], 1, d)
        out.append(d)
    return out


def mix64(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def trial_key(seed: int, i: int, r: int, t: int) -> int:
    K = seed & M64
    for idx in (i, r, t):
        K = mix64((K + G * (idx + 1)) & M64)
    return K


def rate_P(rate: float) -> int:
    """floor(rate * 2^53), exactly."""
    return int(Fraction(rate) * (1 << 53))


def mutate(seq: bytes, rate: float, seed: int = 42, stream=(0, 0, 0)) -> bytes:
    K, P = trial_key(seed, *stream), rate_P(rate)
    out = bytearray(seq)
    for j, b in enumerate(seq):
        base = chr(b & 0xDF)
        if base not in MUT:
            raise KeyError(base)
        z = mix64((K + G * (j + 1)) & M64)
        if (z >> 11) < P:
            out[j] = ord(MUT[base][((z & 0x7FF) * 3) >> 11])
    return bytes(out)


def sum_ref2(ref) -> Fraction:
    return sum((Fraction(float(r)) ** 2 for r in ref), Fraction(0))


def float_dist(seq: bytes, ref, k: int, sumR2=None) -> Fraction:
    """(1 / 2k) sum_x (ref[x] - c[x])^2, every Float64 entry of `ref` taken as the rational it is (sumR2: sum_ref2(ref), for
    callers with many sequences -- the bins the sequence does not touch contribute ref[x]^2)."""
    tot = sum_ref2(ref) if sumR2 is None else sumR2
    for x, cx in counts(seq, k).items():
        r = Fraction(float(ref[x]))
        tot += (r - cx) ** 2 - r * r
    return tot / (2 * k)


# ---- the exact-integer oracle's D of every window (the one function here that is not plain Python: it only calls the oracle) ------

def oracle_D(seqs, S, N, k, W):
    """Per record the list [D1] + Dout of the exact-integer oracle: D of every window (empty for a record shorter than W)."""
    from oracle import oracle as orc
    _, Dout, D1 = orc.single_scan_int(list(seqs), S, N, k, W, 0, return_D=True)
    out, at = [], 0
    for c, s in enumerate(seqs):
        n = len(s) - W + 1
        if n < 1:
            out.append([])
            continue
        out.append([int(D1[c])] + Dout[at:at + n - 1].tolist())
        at += n - 1
    assert at == len(Dout)
    return out
