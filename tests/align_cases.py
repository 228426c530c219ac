"""Inputs shared by the aligner's CPU tests (tests/test_align_host.py) and GPU tests (tests/test_gpu_align.py)."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def rand_seq(rng, n, alphabet=b"ACGT"):
    al = np.frombuffer(bytes(alphabet), dtype=np.uint8)
    return al[rng.integers(0, len(al), size=int(n))].tobytes()


def mutated(rng, cons, flank=99):
    """`cons` with a few substitutions / N, up to three indels of 1-29 residues, and 0..flank random residues on each side.
    Never empty."""
    g = bytearray(cons)
    for _ in range(int(rng.integers(0, 2 + len(g) // 25))):
        g[int(rng.integers(0, len(g)))] = b"ACGTN"[int(rng.integers(0, 5))]
    for _ in range(int(rng.integers(0, 4))):
        p, L = int(rng.integers(0, len(g) + 1)), int(rng.integers(1, 30))
        if rng.random() < 0.5 and len(g) > L:
            del g[p:p + L]
        else:
            g[p:p] = rand_seq(rng, L)
    return rand_seq(rng, rng.integers(0, flank + 1)) + bytes(g) + rand_seq(rng, rng.integers(0, flank + 1))


def with_n(s, positions):
    g = bytearray(s)
    for p in positions:
        g[p:p] = b"N"
    return bytes(g)


def low_complexity_cases():
    """(consensus, segment) pairs where nearly every DP cell is a tie, or where the alphabet's edges show: homopolymers, (AC)^r
    against (AC)^s with N inserted, segments of only N, lower and mixed case, bytes outside ACGTN (they count as N)."""
    rng = np.random.default_rng(417)
    c40 = rand_seq(rng, 40)
    c70 = rand_seq(rng, 70)
    cases = [
        (b"A" * 20, b"A" * 50), (b"A" * 50, b"A" * 20), (b"A" * 7, b"A" * 7), (b"A" * 30, b"C" * 30),
        (b"A" * 64, b"A" * 65), (b"A" * 65, b"A" * 64), (b"A" * 10, b"T" * 3 + b"A" * 4 + b"T" + b"A" * 9 + b"T" * 2),
        (b"AC" * 5, with_n(b"AC" * 9, [4, 11])), (b"AC" * 9, with_n(b"AC" * 5, [3])),
        (b"AC" * 32, with_n(b"AC" * 40, [1, 30, 31, 64])), (b"AC" * 33, with_n(b"AC" * 20, [0, 20, 41])),
        (b"AC" * 32, b"CA" * 32), (with_n(b"AC" * 12, [6, 7]), b"AC" * 14),
        (c40, b"N" * 60), (c40, b"N"), (b"N" * 10, b"N" * 25), (b"N" * 25, b"N" * 10), (b"N" * 5, c40),
        (c70, c70.lower()), (c70.lower(), mutated(rng, c70, 20)), (c70, mutated(rng, c70, 20).lower()),
        (c70, bytes(x | 32 if k % 3 == 0 else x for k, x in enumerate(mutated(rng, c70, 20)))),
        (c70, c70[:20] + b"R" + c70[21:40] + b"--" + c70[40:] + b"-"), (c70[:30] + b"R-" + c70[32:], b"-" + c70 + b"RR"),
        (b"R" * 6, b"N" * 4 + b"-" * 4), (b"ACGTNacgtn", b"acgtnACGTN"),
        # the smallest inputs on which the order match > deletion > insertion and the `>=` of the extend flags decide the CIGAR
        (b"A", b"AA"), (b"AA", b"A"), (b"A", b"AAC"), (b"A", b"C"), (b"A", b"CCC"),
    ]
    return cases


LOW_COMPLEXITY_GAPS = [(-69, -1), (-200, -1), (-5, -3), (-69, -5), (0, -1), (-3, -1), (0, -2)]
