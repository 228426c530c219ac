"""numpy restatement of the granule test that the step's sums-only pack makes itself (kmergma.jl_amd/csrc/kgma_filter.hip:
pack_sums_kernel<K, false, true>), shared by test_pack_test_ref.py (CPU) and test_gpu_pack_test.py.

The block sums of a laid-out genome are ONE array over all blocks (dwords of the 2-bit copy): a record's sums (tests/sums_ref.py) from
block 2 * word_off on, 0 everywhere else.  Records lie PAD_WORDS = 32 words = 64 zero blocks apart and nblk - 1 <= 62, so the sum of
the nblk blocks from a granule's first block never reaches the next record: the candidates are a prefix-sum difference over the
global array, and only the label (record, granule) and the test 0 <= granule < ceil(nwin / 16) are per record.

The walk is the kernel's: units of 128 words in two chunks of 64; lane l of a chunk holds its blocks 2l and 2l + 1; a prefix over
the lane pairs with a carry mod 2^32; with nblk = 2a + b the lower end of element q of lane l is element (q - b) & 1 of lane
l - a - [q < b], of this chunk or the one before.  A wave takes runs of R consecutive units, dealt round-robin over the waves, and
primes a run with the chunk in front of it, of which it emits nothing."""
import numpy as np

from tests import sums_ref

LEAD_PAD_WORDS = 8
PAD_WORDS = 32
TAIL_PAD_WORDS = 253 * 2 + 128
UNIT_WORDS = 128
CHUNK_BLOCKS = 128
M32 = (1 << 32) - 1


def nblk_of(nk: int) -> int:
    return (nk + 14) // 16 + 1


def layout(lengths):
    """(word_off per record, total_words) as the resident genome lays records out."""
    offs, w = [], LEAD_PAD_WORDS
    for L in lengths:
        offs.append(w)
        w += (L + 31) // 32 + PAD_WORDS
    return offs, w + TAIL_PAD_WORDS


def global_blocks(contigs, S, k):
    """(block array over the whole layout, word_off per record)."""
    offs, total = layout([len(c) for c in contigs])
    n_units = (total + UNIT_WORDS - 1) // UNIT_WORDS
    arr = np.zeros(2 * n_units * UNIT_WORDS, dtype=np.int64)           # (whole units: words past the genome count 0)
    for c, seq in zip(offs, contigs):
        s = sums_ref.block_sums(seq, S, k)
        arr[2 * c:2 * c + s.size] = s
    return arr, offs


def unit_of(record_word_off: int, pos: int) -> int:
    """The unit that holds 0-based position `pos` of a record."""
    return (record_word_off + pos // 32) // UNIT_WORDS


def candidates_direct(contigs, S, k, W, U):
    """The exactness argument alone: global prefix differences, labels, validity -- no chunks, no runs."""
    arr, offs = global_blocks(contigs, S, k)
    nblk = nblk_of(W - k + 1)
    P = np.concatenate([[0], np.cumsum(arr)])
    out = []
    for c, (woff, seq) in enumerate(zip(offs, contigs)):
        nwin = len(seq) - W + 1
        ng = (nwin + 15) // 16 if nwin > 0 else 0
        B = 2 * woff + np.arange(ng)
        g = np.nonzero(P[B + nblk] - P[B] >= U)[0]
        out.append(np.stack([np.full(g.size, c, dtype=np.int64), g.astype(np.int64)], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int64)


def candidates(contigs, S, k, W, U, run, n_waves=3):
    """The kernel's walk.  Returns the sorted (record, granule) array and a dict of counts (units, primed chunks, runs per wave)."""
    arr, offs = global_blocks(contigs, S, k)
    lens = [len(c) for c in contigs]
    nblk = nblk_of(W - k + 1)
    assert 1 <= nblk <= 63
    a, b = nblk >> 1, nblk & 1
    n_units = arr.size // (2 * UNIT_WORDS)
    n_runs = (n_units + run - 1) // run
    lane = np.arange(64)
    woffs = np.asarray(offs, dtype=np.int64)
    ngs = np.asarray([((L - W + 1) + 15) // 16 if L >= W else 0 for L in lens], dtype=np.int64)
    found, primed = [], 0

    def chunk(state, first_block, emit):
        s = arr[first_block:first_block + CHUNK_BLOCKS].reshape(64, 2)
        I1 = (np.cumsum(s.sum(axis=1)) + state["carry"]) & M32
        state["carry"] = int(I1[63])
        I = np.stack([(I1 - s[:, 1]) & M32, I1], axis=1)               # inclusive prefix at the lane's two blocks
        R = np.stack([I[:, (0 - b) & 1], I[:, (1 - b) & 1]], axis=1)   # what the lane offers the reader of its element q
        for q in range(2):
            back = a + (1 if q < b else 0)
            offered = np.where(lane + back < 64, R[:, q], state["prev"][:, q])
            lo = offered[(lane - back) & 63]
            cand = ((I[:, q] - lo) & M32) >= U
            if emit:
                for l in np.nonzero(cand)[0]:
                    B = first_block + 2 * int(l) + q - (nblk - 1)     # the granule's first block
                    if B < 0:
                        continue
                    c = int(np.searchsorted(2 * woffs, B, side="right")) - 1
                    if c >= 0 and 0 <= B - 2 * woffs[c] < ngs[c]:
                        found.append((c, int(B - 2 * woffs[c])))
        state["prev"] = R

    for w in range(min(n_waves, n_runs)):
        state = dict(carry=0, prev=np.zeros((64, 2), dtype=np.int64))   # (the carry runs on from run to run: only differences count)
        for r in range(w, n_runs, n_waves):
            u0 = r * run
            if u0 > 0:
                chunk(state, 2 * UNIT_WORDS * (u0 - 1) + CHUNK_BLOCKS, False)
                primed += 1
            for u in range(u0, min(u0 + run, n_units)):
                chunk(state, 2 * UNIT_WORDS * u, True)
                chunk(state, 2 * UNIT_WORDS * u + CHUNK_BLOCKS, True)
    out = np.asarray(sorted(found), dtype=np.int64).reshape(-1, 2)
    assert len(set(found)) == len(found)                               # every candidate granule once
    return out, dict(units=n_units, primed=primed, runs=n_runs)
