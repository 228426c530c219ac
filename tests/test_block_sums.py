"""The block sums of tests/sums_ref.py against the prefilter's granule sums (tests/filter_ref.py) and against the definition at a
record's end.  No GPU: both sides are numpy."""
import numpy as np
import pytest

from tests import filter_cases as fc
from tests import filter_ref, sums_ref
from tests.helpers import kmer_values, random_dna

CELLS = [(k, nk) for k in fc.KS for nk in fc.NKS]


@pytest.mark.parametrize("k,nk", CELLS, ids=["k%d-nk%d" % c for c in CELLS])
def test_granule_sums_are_sums_of_blocks(k, nk):
    """A granule's sum is the sum of nblk consecutive block sums, whatever the record's length modulo 16 and 32."""
    ref = fc.family(k, 7, nk)
    W, nblk = ref["ws"], fc.nblk_of(nk)
    rng = np.random.default_rng([6401, k, nk])
    for L in [W, W + 1, W + 15, W + 16, W + 17, W + 31, W + 32, 3 * W + 5, 5000 + int(rng.integers(0, 32))]:
        seq = random_dna(rng, L)
        bs = sums_ref.block_sums(seq, ref["S"], k)
        want = filter_ref.granule_sums(seq, ref["S"], k, W)
        ng = want.size
        assert ng == (L - W + 1 + 15) // 16
        ext = np.concatenate([bs, np.zeros(ng + nblk, dtype=np.int64)])
        got = np.asarray([ext[g:g + nblk].sum() for g in range(ng)])
        assert np.array_equal(got, want), (L, np.nonzero(got != want)[0][:4])


@pytest.mark.parametrize("k", fc.KS)
def test_mask_at_the_record_end(k):
    """Positions behind the record's last k-mer count as 0: every length modulo 16, and records shorter than k."""
    ref = fc.family(k, 7, 100)
    S = ref["S"]
    rng = np.random.default_rng([6402, k])
    for r in range(16):
        for L in (160 + r, 176 + r):                                  # (an even and an odd number of whole blocks before the end)
            seq = random_dna(rng, L)
            bs = sums_ref.block_sums(seq, S, k)
            assert bs.size == 2 * ((L + 31) // 32)
            vals = S[kmer_values(seq, k)]
            assert vals.size == L - k + 1 and bs.sum() == vals.sum()
            last = (L - k) // 16                                         # block of the last k-mer
            assert bs[last] == vals[16 * last:].sum()
            assert not bs[last + 1:].any()
            for b in range(last):
                assert bs[b] == vals[16 * b:16 * b + 16].sum()
    for L in range(0, k):
        bs = sums_ref.block_sums(random_dna(rng, L), S, k)
        assert bs.size == 2 * ((L + 31) // 32) and not bs.any()


def test_codes_of_n_and_lower_case():
    """N reads as T and lower case as upper case, as in the 2-bit genome copy."""
    ref = fc.family(6, 7, 17)
    a = sums_ref.block_sums(b"acgtnACGTN" * 7, ref["S"], 6)
    b = sums_ref.block_sums(b"ACGTTACGTT" * 7, ref["S"], 6)
    assert np.array_equal(a, b)
