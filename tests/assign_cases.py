"""Case lists shared by the assignment's CPU tests (tests/test_assign_host.py: the model on them, non-vacuity) and GPU tests
(tests/test_gpu_assign.py).  A case is (refs, queries): lists of bytes.  Sequences come from tests/align_cases.py's helpers."""
import numpy as np

from tests import align_cases as ac

GAPS = [(-69, -1), (-200, -1), (-5, -3), (-69, -5), (0, -1)]     # the five gap models of tests/test_gpu_align.py
STRIP_M = [1, 2, 63, 64, 65, 128, 129]
PAIRS_PER_LAUNCH = 1 << 16      # KGMA_ASSIGN_PAIRS_PER_LAUNCH (kgma_device.h): pairs of one score launch
MAX_LEN = 8191                  # KGMA_ASSIGN_MAX_LEN


def query_of_length(rng, ref, n):
    """A mutated copy of `ref` cut or padded to n residues where n >= m/2, random sequence otherwise."""
    if 2 * n < len(ref):
        return ac.rand_seq(rng, n)
    s = ac.mutated(rng, ref, flank=0)
    if len(s) < n:
        left = int(rng.integers(0, n - len(s) + 1))
        return ac.rand_seq(rng, left) + s + ac.rand_seq(rng, n - len(s) - left)
    off = int(rng.integers(0, len(s) - n + 1))
    return s[off:off + n]


def strip_case(m):
    """R = 5 references of different lengths -- m first, then the next four of STRIP_M in cyclic order, each a relative of the
    first where it is long enough -- against queries whose lengths sit around the 64 lanes and around m."""
    rng = np.random.default_rng(500 + m)
    k = STRIP_M.index(m)
    lens = [STRIP_M[(k + d) % len(STRIP_M)] for d in range(5)]
    first = ac.rand_seq(rng, m)
    refs = [first] + [query_of_length(rng, first, L) for L in lens[1:]]
    assert [len(r) for r in refs] == lens and len(set(lens)) == 5
    ns = sorted({n for n in (1, 2, 63, 64, 65, 127, 129, m - 1, m, m + 1) if n >= 1})
    queries = [query_of_length(rng, refs[j % 5], n) for j, n in enumerate(ns)]
    assert [len(q) for q in queries] == ns
    return refs, queries


def tie_case():
    """References 1 and 3 are byte-identical; reference 4 is the same gene in lower case -- other bytes, the same codes, so the
    same score against every query by construction.  0 and 2 are mutated copies.  The queries hold the gene, whole or in part."""
    rng = np.random.default_rng(1313)
    gene = ac.rand_seq(rng, 90)
    m0 = bytearray(gene); m0[10] = ord("N"); m0[50:53] = b""
    m2 = bytearray(gene); m2[70:70] = b"ACGTAC"
    refs = [bytes(m0), gene, bytes(m2), gene, gene.lower()]
    queries = [ac.rand_seq(rng, 30) + gene + ac.rand_seq(rng, 17), gene, gene[5:80], ac.mutated(rng, gene, 40), gene[:60] + gene[63:]]
    return refs, queries


def alphabet_cases():
    """align_cases.low_complexity_cases() in groups of eight: a group's consensus sequences are the references, its segments the
    queries (every reference against every query of its group)."""
    cases = ac.low_complexity_cases()
    return [([a for a, _ in cases[i:i + 8]], [b for _, b in cases[i:i + 8]]) for i in range(0, len(cases), 8)]


def chunked_case():
    """260 queries x 253 references = 65780 pairs, more than one score launch holds; the sequences are drawn from a few tiny ones
    (so the model stays cheap and equal scores abound)."""
    rng = np.random.default_rng(65536)
    small_r = [bytes([a]) for a in b"ACGT"] + [bytes([a, b]) for a in b"ACGT" for b in b"ACGT"]
    small_q = small_r + [bytes([a, b, c]) for a in b"ACGN" for b in b"ACGT" for c in b"ACGT"]
    refs = [small_r[int(i)] for i in rng.integers(0, len(small_r), size=253)]
    queries = [small_q[int(i)] for i in rng.integers(0, len(small_q), size=260)]
    assert len(refs) * len(queries) > PAIRS_PER_LAUNCH
    return refs, queries


def long_query_case():
    """One 8191-residue query among 40 short ones, against two references of 64: the long one runs in another length class."""
    rng = np.random.default_rng(8191)
    refs = [ac.rand_seq(rng, 64), ac.rand_seq(rng, 64)]
    queries = [query_of_length(rng, refs[j % 2], int(n)) for j, n in enumerate([1, 2, 64, 65, 200, 255, 256, 300] + rng.integers(1, 400, size=32).tolist())]
    long = bytearray(ac.rand_seq(rng, MAX_LEN))
    long[3000:3064] = refs[1]
    long[7000:7030] = refs[0][:30]
    queries.insert(17, bytes(long))
    assert len(queries) == 41 and sum(len(q) == MAX_LEN for q in queries) == 1
    return refs, queries


def long_ref_case():
    """An 8191-residue reference (128 strips) and a short one against a 70-residue query cut from the long one."""
    rng = np.random.default_rng(70)
    long = ac.rand_seq(rng, MAX_LEN)
    return [long, long[4000:4060]], [long[4000:4070], ac.mutated(rng, long[100:160], 5)]


def record_case():
    """Records for the ranges source -- one of a single residue -- and ranges at their first and last residues."""
    rng = np.random.default_rng(77)
    gene = ac.rand_seq(rng, 120)
    refs = [gene, ac.mutated(rng, gene, 0), ac.rand_seq(rng, 70)]
    recs = [ac.rand_seq(rng, 333), ac.rand_seq(rng, 41) + ac.mutated(rng, gene, 0) + ac.rand_seq(rng, 301), b"G",
            ac.mutated(rng, gene, 0) + ac.rand_seq(rng, 97) + refs[2], ac.mutated(rng, gene, 30)]
    L = [len(r) for r in recs]
    ranges = [(1, 1, L[1]), (1, 1, 200), (1, 42, 42 + 170), (1, L[1] - 256, L[1]), (0, 1, 1), (0, L[0], L[0]), (0, 7, 333), (2, 1, 1),
              (3, 1, 140), (3, L[3] - 69, L[3]), (3, 1, L[3]), (4, 1, L[4]), (1, 42, 42 + 170), (4, 3, L[4] - 1), (0, 1, 1)]
    return refs, recs, ranges


def all_model_lists():
    """Every (refs, queries) list above, for the non-vacuity checks."""
    refs, recs, ranges = record_case()
    out = [strip_case(m) for m in STRIP_M] + [tie_case()] + alphabet_cases() + [long_query_case(), (refs, [recs[c][lo - 1:hi] for c, lo, hi in ranges])]
    return out
