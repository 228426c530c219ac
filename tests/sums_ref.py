"""numpy restatement of the block sums that the step's pack writes for the prefilter (kmergma.jl_amd/csrc/kgma_filter.hip:
pack_sums_kernel; include/kgma.h: kgma_get_block_sums), shared by test_block_sums.py and test_gpu_fused_sums.py.

Block b of a record holds the 16 positions 16 b ... 16 b + 15 (one dword of the 2-bit genome copy); its sum is the sum of S over the
k-mers that start there and are k-mers of the record (position <= len - k).  A record has 2 * ceil(len / 32) blocks."""
import numpy as np

from tests.helpers import kmer_values


def n_blocks(length: int) -> int:
    return 2 * ((length + 31) // 32)


def block_sums(seq: bytes, S, k: int) -> np.ndarray:
    """One sum per block of `seq` (S in natural k-mer order, as tests.helpers.kmer_values indexes it)."""
    nb = n_blocks(len(seq))
    v = np.zeros(16 * nb, dtype=np.int64)
    if len(seq) < k:                                                   # no k-mer: every block is 0
        return v.reshape(nb, 16).sum(axis=1)
    sv = np.asarray(S, dtype=np.int64)[kmer_values(seq, k)]          # one value per k-mer position 0 ... len - k
    v[:sv.size] = sv
    return v.reshape(nb, 16).sum(axis=1)
