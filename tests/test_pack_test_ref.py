"""The exactness argument of the in-pack granule test, on the CPU: the candidate set of tests/filter_ref.py (per record, positions
behind the record's last k-mer counting 0) is a plain prefix-sum difference over the GLOBAL block array of the laid-out genome, and
the kernel's walk over it -- chunks of 128 blocks, two per lane, runs of R units primed with the chunk in front -- finds exactly
that set.  Layouts: records shorter than a block, shorter than a unit, exactly one unit long; several records in one unit; a
record that ends in low sums 32 words in front of one that starts with a gene."""
import functools

import numpy as np
import pytest

from tests import filter_cases as fc
from tests import filter_ref, pack_test_ref as ptr
from tests.helpers import kmer_values, mutate, random_dna

NBLK63_NK = 16 * 62 - 14                                               # (nk + 14) // 16 + 1 = 63, the most launch_filter admits
NKS = tuple(fc.NKS) + (NBLK63_NK,)
UNIT = 32 * ptr.UNIT_WORDS


@functools.lru_cache(maxsize=None)
def case(k, nk):
    """(contigs, S, W, U, marks) for one (k, nk); marks name the records the assertions look at."""
    W = nk + k - 1
    rng = np.random.default_rng([7100, k, nk])
    gene = random_dna(rng, W)
    S = np.zeros(4 ** k, dtype=np.int64)
    for _ in range(7):
        S += np.bincount(kmer_values(mutate(rng, gene, 0.03), k), minlength=4 ** k)
    S = np.minimum(S, 255)
    S[kmer_values(b"A" * k, k)[0]] = 0                                  # a poly-A tail sums to 0
    U = int(0.6 * S[kmer_values(gene, k)].sum())
    contigs, marks = [], {}

    def rec(L, at=(), name=None):
        a = bytearray(random_dna(rng, L))
        for pos in at:
            a[pos:pos + W] = gene
        if name:
            marks[name] = len(contigs)
        contigs.append(bytes(a))

    rec(10, name="sub_block")                                          # shorter than a block
    rec(3)                                                             # shorter than k
    rec(W + 700, at=(700,), name="sub_unit")                            # shorter than a unit (for the short windows), gene on its end
    rec(max(UNIT, W), at=(0, max(UNIT, W) - W), name="one_unit")        # exactly one unit long where the window allows
    for L in (40, 70, 33, W + 20, 95, W, 64):                           # several records in one unit
        rec(L, at=(L - W,) if L >= W else ())
    low = bytearray(random_dna(rng, W + 300))
    low[-(W // 2 + 40):] = b"A" * (W // 2 + 40)                         # ends in sums of 0 ...
    marks["low_tail"] = len(contigs)
    contigs.append(bytes(low))
    rec(W + 50, at=(0,), name="gene_first")                             # ... 32 words in front of a gene on a record's first residue
    L = 3 * UNIT + 1234
    rec(L, at=(UNIT - W // 2, 2 * UNIT - 5, L - W), name="long")        # genes across unit (and, at R = 1, run) boundaries
    return contigs, S, W, U, marks


@pytest.mark.parametrize("run", [1, 2, 3])
@pytest.mark.parametrize("nk", NKS)
@pytest.mark.parametrize("k", [5, 6])
def test_walk_equals_the_per_record_reference(k, nk, run):
    contigs, S, W, U, marks = case(k, nk)
    want = filter_ref.candidates(contigs, S, k, W, U)
    got, counts = ptr.candidates(contigs, S, k, W, U, run)
    assert np.array_equal(got, want)
    assert np.array_equal(ptr.candidates_direct(contigs, S, k, W, U), want)
    assert counts["primed"] == counts["runs"] - 1 and counts["runs"] > 3   # more runs than waves: a wave primes more than once
    have = set(map(tuple, want.tolist()))
    for name in ("sub_unit", "one_unit", "gene_first", "long"):
        assert any(c == marks[name] for c, _ in have), name
    assert (marks["gene_first"], 0) in have
    # the record in front ends in zeros: its last granules are none, whatever stands 64 blocks on
    c = marks["low_tail"]
    ng = (len(contigs[c]) - W + 1 + 15) // 16
    assert (c, ng - 1) not in have
    assert not any(c == marks["sub_block"] for c, _ in have)


def test_both_parities_and_the_widest_sum():
    nblks = sorted({ptr.nblk_of(nk) for nk in NKS})
    assert nblks == [2, 3, 4, 8, 19, 25, 63]
    assert {n & 1 for n in nblks} == {0, 1}


def test_the_pad_is_what_keeps_records_apart():
    """With a pad shorter than nblk - 1 blocks the global difference would see the next record: the constant the kernel relies on."""
    assert 2 * ptr.PAD_WORDS >= 62
    k, nk = 5, NBLK63_NK
    contigs, S, W, U, marks = case(k, nk)
    arr, offs = ptr.global_blocks(contigs, S, k)
    c = marks["low_tail"]
    end = 2 * offs[c] + 2 * ((len(contigs[c]) + 31) // 32)              # first pad block behind the record
    assert np.all(arr[end:end + 64] == 0) and arr[2 * offs[c + 1]] > 0
