"""Case lists shared by the k-mer distance matrix's CPU tests (tests/test_kmat_host.py: the model on them, non-vacuity) and GPU
tests (tests/test_gpu_kmat.py).  A matrix case is (k, seqs_a, seqs_b) -- lists of bytes, seqs_b None meaning B = A.  The kernel's
constants are restated here; the shapes are the smallest at which kgma_kmat.hip can go wrong."""
import numpy as np

from kmergma_amd import fasta
from tests import align_cases as ac

TILE = {1: 16, 2: 16, 3: 16, 4: 16, 5: 16, 6: 8, 7: 4, 8: 1, 9: 1, 10: 1}      # kmat_tile(k) (kgma_device.h): sequences of B per workgroup
LDS_K_MAX = 7                   # count tables in LDS up to here, one global table per workgroup above
WAVES = 4                       # KGMA_KMAT_THREADS / 64: the rows of a chunk go to the waves in turn
MIN_ROWS = 64                   # KGMA_KMAT_MIN_ROWS: a second chunk needs more rows of A than this
MAX_LEN = 32767                 # KGMA_KMAT_MAX_LEN
MAX_NEAR = 128                  # KGMA_KMAT_MAX_NEAR
D_MAX = 2 * MAX_LEN * MAX_LEN   # 2 147 352 578: A x 32767 against C x 32767 at k = 1
KS = list(range(1, 11))
FORM_LDS, FORM_GLOBAL = 0, 1


def form_of(k):
    return FORM_LDS if k <= LDS_K_MAX else FORM_GLOBAL


def length_case(k):
    """A: lengths 0, k - 1, k, k + 1 and those giving 63, 64, 65, 128, 129 k-mers (the lane loop's edges); B: 2 T + 1 sequences
    (two full tiles and a tail of one) whose lengths include 0, k - 1 and k, some of them relatives of A's."""
    rng = np.random.default_rng(1000 + k)
    lens = [0, k - 1, k, k + 1] + [nk + k - 1 for nk in (63, 64, 65, 128, 129)]
    A = [ac.rand_seq(rng, n) for n in lens]
    nb = 2 * TILE[k] + 1
    B = [ac.rand_seq(rng, n) for n in ([0, k - 1, k] + rng.integers(1, 150, size=nb).tolist())[:nb]]
    B[-1] = A[-1][3:] + b"ACGT"                    # (the tail tile holds a near relative: a nearest reference other than index 0)
    if nb > 4:
        B[3] = A[5]
    return k, A, B


TILE_KS = [5, 6, 7, 8]          # T = 16, 8, 4 and the global form


def tile_case(k):
    """70 rows of A (two chunks of 35: every wave's row loop wraps, and the second chunk's rows do not start at 0) against
    2 T + 1 sequences of B, of which the GPU test takes the first 1, T - 1, T, T + 1 and all."""
    rng = np.random.default_rng(2000 + k)
    B = [ac.rand_seq(rng, n) for n in rng.integers(k, 90, size=2 * TILE[k] + 1)]
    A = [ac.rand_seq(rng, n) for n in rng.integers(0, 90, size=70)]
    assert len(A) > MIN_ROWS and (len(A) + 1) // 2 > WAVES
    return k, A, B


def tile_widths(k):
    T = TILE[k]
    return sorted({n for n in (1, T - 1, T, T + 1, 2 * T + 1) if n >= 1})


def long_cases():
    """One sequence of 32767 residues on either side, in both forms."""
    rng = np.random.default_rng(32767)
    long = ac.rand_seq(rng, MAX_LEN)
    other = ac.rand_seq(rng, MAX_LEN, b"ACGTN")
    short = [ac.rand_seq(rng, 300), long[500:900]]
    return [(6, [long] + short, [other, long] + short), (9, [short[1], long], [long, short[0]])]


def counter_cases():
    """The counters' edges.  k = 1: A x 32767 and C x 32767 share a dword and give the largest D there is; A x 16000 + C x 16000
    fills both halves of one dword.  Homopolymers at k = 7 and k = 10: one counter takes every k-mer of the sequence."""
    a, c = b"A" * MAX_LEN, b"C" * MAX_LEN
    both = b"A" * 16000 + b"C" * 16000
    homo = [b"A" * MAX_LEN, b"T" * 5000, b"N" * 5000, b"g" * 77, b"A" * 6]
    return [(1, [a, c, both], None), (1, [a, c, both], [c, a, both, b"G"]), (2, [a, both], [both, c]),
            (7, homo, None), (10, homo, homo[::-1])]


def alphabet_cases():
    """Lower case, N counted as T, and N only against T only (D = 0)."""
    rng = np.random.default_rng(7)
    s = ac.rand_seq(rng, 200, b"ACGTN")
    t = ac.rand_seq(rng, 180, b"acgtnACGTN")
    A = [s, s.lower(), s.replace(b"N", b"T"), t, b"N" * 50, b"n" * 50]
    B = [t.upper().replace(b"N", b"T"), b"T" * 50, s, b"t" * 50]
    return [(k, A, B) for k in (3, 6, 8)]


def matrix_cases():
    return ([length_case(k) for k in KS] + long_cases() + counter_cases() + alphabet_cases())


def bad_cases():
    """(k, seqs_a, seqs_b, words the error must contain): a bad residue in A, in B, in both (A is reported), inside the first
    k - 1 residues of a sequence shorter than k, and in the last sequence of a tail tile."""
    rng = np.random.default_rng(99)
    good = [ac.rand_seq(rng, n) for n in (40, 7, 130, 64)]
    badA = list(good); badA[2] = good[2][:77] + b"R" + good[2][78:]
    short = list(good); short[1] = b"AC-"                        # 3 residues at k = 6: nothing is counted, the residue is still looked up
    many = [ac.rand_seq(rng, 30) for _ in range(17)]
    many[16] = many[16][:29] + b"x"
    out = []
    for k in (6, 9):
        out += [(k, badA, good, ("A sequence 2", "position 78")), (k, good, badA, ("B sequence 2", "position 78")),
                (k, badA, short, ("A sequence 2", "position 78")), (k, short, good, ("A sequence 1", "position 3")),
                (k, good, short, ("B sequence 1", "position 3")), (k, good, many, ("B sequence 16", "position 30")),
                (k, badA, None, ("A sequence 2", "position 78"))]
    return out


def nearest_cases():
    """(k, seqs_a, seqs_b, n_nears).  Duplicate references (exact ties, ordered by index), n_b of 63, 64, 65 and 200 (the select
    kernel's lane loop), n_near of 1, n_b and 128, and rows in which every D is equal."""
    rng = np.random.default_rng(128)
    genes = [ac.rand_seq(rng, 120) for _ in range(7)]
    out = []
    for nb in (63, 64, 65, 200):
        B = [genes[int(i)] if rng.random() < 0.5 else ac.mutated(rng, genes[int(i)], 10) for i in rng.integers(0, 7, size=nb)]
        B[nb - 1] = B[0] = genes[3]                               # a tie between the first and the last column
        A = [genes[3], ac.mutated(rng, genes[5], 20), b"", ac.rand_seq(rng, 90), genes[0][:60] + genes[6][60:]]
        out.append((6, A, B, sorted({1, 2, min(nb, MAX_NEAR)})))
    same = [genes[1]] * 130
    out.append((6, [genes[1], genes[2], b"AC"], same, [1, 128]))   # every D of a row equal: the first n_near indices
    out.append((9, [genes[0], genes[4]], [genes[4], genes[0], genes[4], genes[0].lower()], [1, 4]))
    return out


def record_case():
    """Records of a genome, ranges on them -- at record starts and ends, empty ones, whole records -- and a B list.  Record 2
    holds a residue outside the alphabet that no range covers."""
    rng = np.random.default_rng(404)
    gene = ac.rand_seq(rng, 150)
    recs = [ac.rand_seq(rng, 400), ac.rand_seq(rng, 30) + gene + ac.rand_seq(rng, 220, b"ACGTN"), b"ACGT*ACGTACGTAAC", b"G",
            ac.mutated(rng, gene, 25).lower()]
    L = [len(r) for r in recs]
    ranges = [(0, 1, 1), (0, 1, 0), (0, L[0], L[0]), (0, L[0] + 1, L[0]), (0, 1, L[0]), (1, 31, 180), (1, L[1] - 99, L[1]), (2, 1, 4),
              (2, 6, L[2]), (3, 1, 1), (4, 1, L[4]), (1, 31, 180), (4, 5, 4), (1, 1, 64 + 5), (1, 2, 65 + 5)]
    B = [gene, ac.mutated(rng, gene, 0), ac.rand_seq(rng, 90), recs[0][100:300], b"", b"ACG"]
    bad_range = (2, 3, 7)
    return recs, ranges, B, bad_range


def ranges_text(recs, ranges, revcomp=False):
    src = [fasta.reverse_complement(r) for r in recs] if revcomp else recs
    return [src[c][lo - 1:hi] for c, lo, hi in ranges]


# ---- the prescreen on the fixture genes ---------------------------------------------------------------------------------
FIXTURE_QUERIES = 12
FIXTURE_RATE, FIXTURE_FLANK = 0.05, 50


def fixture_queries(genes, n=FIXTURE_QUERIES, seed=84):
    """(indices, queries): a fixed, seeded subset of the reference genes, each substituted at 5 % with 50 random residues either
    side."""
    rng = np.random.default_rng(seed)
    pick = sorted(rng.choice(len(genes), size=n, replace=False).tolist())
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for i in pick:
        a = np.frombuffer(bytes(genes[i]).upper(), dtype=np.uint8).copy()
        hit = rng.random(a.size) < FIXTURE_RATE
        a[hit] = bases[rng.integers(0, 4, size=int(hit.sum()))]
        out.append(ac.rand_seq(rng, FIXTURE_FLANK) + a.tobytes() + ac.rand_seq(rng, FIXTURE_FLANK))
    return pick, out


def small_screen_case():
    """A small batch for the screened assignment under every gap model: 9 references (two of them identical, one in lower case)
    and 6 queries; n_near = 4, top = 2."""
    rng = np.random.default_rng(4242)
    genes = [ac.rand_seq(rng, 80) for _ in range(4)]
    refs = [genes[0], ac.mutated(rng, genes[0], 0), genes[1], genes[2], genes[1], genes[3], genes[2].lower(), ac.rand_seq(rng, 60),
            ac.mutated(rng, genes[3], 0)]
    queries = [ac.rand_seq(rng, 20) + genes[1] + ac.rand_seq(rng, 11), ac.mutated(rng, genes[0], 30), genes[2][5:70], ac.mutated(rng, genes[3], 15),
               ac.rand_seq(rng, 100), genes[2]]
    return refs, queries
