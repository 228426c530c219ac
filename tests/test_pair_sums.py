"""numpy restatements of the arithmetic of kmergma.jl_amd/csrc/kgma_filter.hip's fused pack and sum-reading filter, against the
references the GPU tests use (tests/sums_ref.py, tests/filter_ref.py).  No GPU.

* pack_sums_kernel's fast path: the pair table P[y] = S[y & KM] + S[(y >> 2) & KM] over the (k + 1)-mers and the eight reads per
  dword of the 2-bit copy at the even positions, the address cut out one bit low (d0 << 1, d0 >> (2i - 1), or the funnel shift of
  the next dword over d0 by 2i - 1), the last pairs reading into the next dword;
* pack_word_2bit's encoder: (x >> 1) & 7 without a case fold, the two byte tables, the dot product with {1, 4, 16, 64};
* filter_sums_kernel's indexing: four blocks per lane, the serial prefix and the scan of the lane totals, the (qa, qb) split of
  nblk, the source lane and element of a bound's lower end with the source choosing the iteration, the transposition of the four
  ballots into entries of 64 consecutive granules."""
import numpy as np
import pytest

from tests import filter_ref, sums_ref
from tests.helpers import random_dna

U32 = np.uint64(0xFFFFFFFF)


def device_order(S, k):
    """S in the 2-bit copy's index order (first residue in the lowest bits) from S in natural order (first residue highest)."""
    x = np.arange(4 ** k)
    nat = np.zeros_like(x)
    for j in range(k):
        nat |= ((x >> (2 * j)) & 3) << (2 * (k - 1 - j))
    return np.asarray(S, dtype=np.int64)[nat]


def codes_of(seq):
    t = np.full(256, 3, dtype=np.uint64)
    for ch, v in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
        t[ch] = v
    return t[np.frombuffer(seq, dtype=np.uint8)]


def dwords_of(seq):
    """The 2-bit copy of a sequence of a multiple of 16 residues: residue t of a dword at bits 2t."""
    c = codes_of(seq).reshape(-1, 16)
    return (c << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint64)


def pair_table(Sdev, k):
    KM = 4 ** k - 1
    y = np.arange(4 ** (k + 1))
    return (Sdev[y & KM] + Sdev[(y >> 2) & KM]).astype(np.uint16)


def pair_sums(d, P, k):
    """ps_sum16_pairs on every dword of d but the last (d1: the next dword)."""
    M2 = np.uint64(((1 << (2 * (k + 1))) - 1) << 1)
    d0, d1 = d[:-1], d[1:]
    total = np.zeros(d0.size, dtype=np.int64)
    for i in range(0, 16, 2):
        if i == 0:
            y2 = (d0 << np.uint64(1)) & U32
        elif 2 * i + 2 * (k + 1) <= 32:
            y2 = d0 >> np.uint64(2 * i - 1)
        else:
            y2 = (((d1 << np.uint64(32)) | d0) >> np.uint64(2 * i - 1)) & U32          # v_alignbit_b32
        off = (y2 & M2).astype(np.int64)
        assert not (off & 1).any()
        total += P[off >> 1]                                            # (a 2-byte read at byte offset `off`)
    return total


S_KINDS = ("random", "all255", "zero")


@pytest.mark.parametrize("kind", S_KINDS)
@pytest.mark.parametrize("k", [5, 6])
def test_pair_sums_are_block_sums(k, kind):
    rng = np.random.default_rng([7101, k, S_KINDS.index(kind)])
    S = dict(random=rng.integers(0, 256, size=4 ** k), all255=np.full(4 ** k, 255), zero=np.zeros(4 ** k, dtype=np.int64))[kind]
    P = pair_table(device_order(S, k), k)
    assert P.dtype == np.uint16 and int(P.max()) == (510 if kind == "all255" else int(P.max())) and int(P.max()) <= 510
    seq = random_dna(rng, 16 * 4096) + b"acgtnACGTNnnnnNN" * 8 + random_dna(rng, 16 * 8)
    got = pair_sums(dwords_of(seq), P, k)
    want = sums_ref.block_sums(seq, S, k)[:got.size]                    # (every k-mer that starts before the last dword is one of seq)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:4]
    assert int(got.max()) <= 4080 and (kind != "all255" or (got == 4080).all())
    # two neighbouring sums in one dword, as the kernel stores them: neither reaches the other's half
    lo, hi = got[0:-1:2], got[1::2]
    packed = lo | (hi << 16)
    assert np.array_equal(packed & 0xFFFF, lo) and np.array_equal(packed >> 16, hi)


def _perm(hi, lo, sel):
    """v_perm_b32 for selector bytes 0 ... 7: byte j of the result is byte sel_j of the 8 bytes {hi, lo}."""
    src = (int(hi) << 32) | int(lo)
    out = 0
    for j in range(4):
        s = (sel >> (8 * j)) & 0xFF
        assert s < 8
        out |= ((src >> (8 * s)) & 0xFF) << (8 * j)
    return out


def _ps_code(ch):
    ch &= 0xDF
    return (1 if ch == ord("C") else 0) | (2 if ch == ord("G") else 0) | (3 if ch in (ord("T"), ord("N")) else 0)


def test_dot_product_encoder_every_byte_every_position():
    letters = set(b"ACGTNacgtn")
    filler = b"AcgT"
    for pos in range(4):
        for v in range(256):
            b = bytearray(filler); b[pos] = v
            x = int.from_bytes(bytes(b), "little")
            sel = (x >> 1) & 0x07070707
            letter = _perm(0x4E000000, 0x47544341, sel)
            code = _perm(0x03000000, 0x02030100, sel)
            diff = (x ^ letter) & 0xDFDFDFDF
            byte = sum(((code >> (8 * j)) & 0xFF) * w for j, w in enumerate((1, 4, 16, 64)))     # v_dot4_u32_u8 with 0x40100401
            if v in letters:
                assert diff == 0, (pos, v)
                assert byte == sum(_ps_code(c) << (2 * j) for j, c in enumerate(b)), (pos, v)
                assert byte < 256
            else:
                assert diff != 0, (pos, v)
                assert (diff >> (8 * pos)) & 0xFF, (pos, v)                # (in the byte of the residue itself)


def test_dot_product_chain_joins_four_bytes():
    """r = dot(c3); r = dot(c2) + (r << 8); ...: the dword of the copy, first residue lowest."""
    rng = np.random.default_rng(7102)
    seq = random_dna(rng, 16 * 64)
    want = dwords_of(seq)
    c = codes_of(seq).reshape(-1, 4, 4).astype(np.int64)               # dword of the copy, dword of four residues, residue
    byte = (c * np.array([1, 4, 16, 64])).sum(axis=2)
    r = byte[:, 3]
    for j in (2, 1, 0):
        r = byte[:, j] + (r << 8)
    assert np.array_equal(r.astype(np.uint64), want)


# ---- filter_sums_kernel ----------------------------------------------------------------------------------------------------------

def walk_stream(bs, g0, n_valid, nblk, U, nvb):
    """One wave on one stream: bs the record's block sums (as stored: uint16), g0 the stream's first granule, nvb the number of
    blocks of the stream that hold a k-mer of the record.  Returns the entries (gbase, mask) in the kernel's order."""
    lane = np.arange(64)
    qa, qb = nblk >> 2, nblk & 3
    ng = (n_valid + 15) >> 4
    nb = ng + nblk - 1
    ext = np.concatenate([np.asarray(bs, dtype=np.int64), np.full(nb + 512, 12345, dtype=np.int64)])   # (what lies behind the record is not 0)
    carry, prevR, out = 0, np.zeros((4, 64), dtype=np.int64), []
    for it in range((nb + 255) >> 8):
        jb = (it << 8) + 4 * lane
        s = np.stack([ext[g0 + jb + q] for q in range(4)])
        if (it << 8) + 256 > nvb:
            s = np.where(jb[None, :] + np.arange(4)[:, None] < nvb, s, 0)
        p = np.cumsum(s, axis=0)
        top = (np.cumsum(p[3]) + carry) & 0xFFFFFFFF                     # f_incl_scan over the lane totals, plus the carry
        carry = int(top[63])
        base = (top - p[3]) & 0xFFFFFFFF
        I = np.stack([(base + p[0]) & 0xFFFFFFFF, (base + p[1]) & 0xFFFFFFFF, (base + p[2]) & 0xFFFFFFFF, top])
        R = np.stack([I[(q - qb) & 3] for q in range(4)])
        m = []
        for q in range(4):
            back = qa + (1 if q < qb else 0)
            offered = np.where(lane + back < 64, R[q], prevR[q])           # the SOURCE lane chooses
            lo = offered[(lane - back) & 63]                                # ds_bpermute
            gl = jb + q - (nblk - 1)
            ok = (gl >= 0) & (gl < ng) & (((I[q] - lo) & 0xFFFFFFFF) >= U)
            m.append(sum(1 << int(l) for l in np.nonzero(ok)[0]))
        prevR = R
        if any(m):
            for e in range(4):
                me = sum(((m[j & 3] >> (16 * e + (j >> 2))) & 1) << j for j in range(64))
                if me:
                    out.append((g0 + (it << 8) + 64 * e - (nblk - 1), me))
    return out


def walk_record(seq, S, k, W, U, P):
    """The candidate granules of one record through walk_stream, the record cut into streams of P windows as the host cuts it."""
    nwin = len(seq) - W + 1
    nblk = (W - k + 1 + 14) // 16 + 1
    bs = sums_ref.block_sums(seq, S, k)
    assert int(bs.max(initial=0)) <= 4080
    got = []
    for t in range((max(nwin, 0) + P - 1) // P):
        g0 = t * P // 16
        rem = len(seq) - k - 16 * g0
        nvb = 0 if rem < 0 else (rem >> 4) + 1
        for gbase, mask in walk_stream(bs, g0, min(P, nwin - t * P), nblk, U, nvb):
            got += [gbase + j for j in range(64) if (mask >> j) & 1]
    return np.asarray(sorted(got), dtype=np.int64)


NBLKS = (1, 2, 3, 4, 5, 19, 25, 63)


@pytest.mark.parametrize("nblk", NBLKS)
def test_four_blocks_per_lane_indexing(nblk):
    k = 5
    nk = 1 if nblk == 1 else 16 * (nblk - 1) - 3
    assert (nk + 14) // 16 + 1 == nblk
    W = nk + k - 1
    rng = np.random.default_rng([7103, nblk])
    S = rng.integers(0, 256, size=4 ** k)
    # stream lengths: one iteration and a bit, several iterations that are no multiple of 256 blocks, exactly 256 granules
    for L, P in ((W + 16 * 300 + 5, 1 << 16), (W + 16 * 1500 + 11, 64 * 77), (W + 16 * 256 - 1, 1 << 16), (W + 16 * 700, 64 * 16), (W + 3, 64)):
        seq = random_dna(rng, L)
        gs = filter_ref.granule_sums(seq, S, k, W)
        for quant in (0.5, 0.97):
            U = int(np.quantile(gs, quant))
            want = filter_ref.candidates([seq], S, k, W, U)[:, 1]
            assert 0 < want.size
            got = walk_record(seq, S, k, W, U, P)
            assert np.array_equal(got, want), (L, P, U, got[:5], want[:5])
