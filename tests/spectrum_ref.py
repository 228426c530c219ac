"""A plain model of kgma_genome_kmer_count (include/kgma.h): ranges, the three flags, n_skipped and the bad-base rule, written
for clarity, not speed.  It imports nothing from the library or the oracle.

    counts, skipped = kmer_count(records, k, ranges, flags)

records: bytes per record; ranges: (record 0-based, lo, hi 1-based inclusive; hi = lo - 1 is empty).  A byte outside A/C/G/T/N
among the residues a range covers raises BadBase(record, position) -- the smallest (record, position) over all ranges -- unless
SKIP_N is set."""
import numpy as np

SKIP_N, SKIP_MASKED, BY_START = 1, 2, 4
ALL_FLAGS = (0, 1, 2, 3, 4, 5, 6, 7)

CODE = np.full(256, -1, dtype=np.int64)          # the reference's table: A0 C1 G2 T3, N -> 3, either case
for _ch, _c in ((b"A", 0), (b"C", 1), (b"G", 2), (b"T", 3), (b"N", 3)):
    CODE[_ch[0]] = CODE[_ch.lower()[0]] = _c
IS_BASE = np.zeros(256, dtype=bool)              # A/C/G/T in either case
IS_BASE[list(b"ACGTacgt")] = True
IS_LOWER = np.zeros(256, dtype=bool)
IS_LOWER[ord("a"):ord("z") + 1] = True


class BadBase(KeyError):
    def __init__(self, record, position):
        super().__init__(f"record {record} position {position}")
        self.record, self.position = record, position


def considered_starts(L, k, lo, hi, by_start):
    """(first, last) considered start, 1-based inclusive (last < first: none)."""
    return (lo, min(hi, L - k + 1)) if by_start else (lo, hi - k + 1)


def covered(L, k, lo, hi, by_start):
    """(first, last) residue the range covers, 1-based inclusive (last < first: none)."""
    if hi < lo:
        return lo, lo - 1
    return (lo, min(hi + k - 1, L)) if by_start else (lo, hi)


def first_bad(records, k, ranges, flags):
    """The smallest (record, position) of a byte outside A/C/G/T/N among the covered residues, or None."""
    best = None
    for c, lo, hi in ranges:
        a, b = covered(len(records[c]), k, lo, hi, bool(flags & BY_START))
        seg = np.frombuffer(records[c], dtype=np.uint8)[a - 1:b]
        bad = np.flatnonzero(CODE[seg] < 0)
        if bad.size:
            key = (c, a + int(bad[0]))
            best = key if best is None or key < best else best
    return best


def kmer_count(records, k, ranges, flags=0):
    records = [bytes(r) for r in records]
    ranges = [(int(c), int(lo), int(hi)) for c, lo, hi in ranges]
    for c, lo, hi in ranges:
        assert 0 <= c < len(records) and lo >= 1 and hi <= len(records[c]) and hi >= lo - 1, (c, lo, hi)
    if not flags & SKIP_N:
        bad = first_bad(records, k, ranges, flags)
        if bad is not None:
            raise BadBase(*bad)
    counts = np.zeros((len(ranges), 4 ** k), dtype=np.int64)
    skipped = np.zeros(len(ranges), dtype=np.int64)
    weights = 4 ** np.arange(k - 1, -1, -1, dtype=np.int64)
    for r, (c, lo, hi) in enumerate(ranges):
        first, last = considered_starts(len(records[c]), k, lo, hi, bool(flags & BY_START))
        n = last - first + 1
        if hi < lo or n <= 0:
            continue
        seg = np.frombuffer(records[c], dtype=np.uint8)[first - 1:last + k - 1]
        win = np.lib.stride_tricks.sliding_window_view(seg, k)               # [n, k]
        assert win.shape[0] == n
        skip = np.zeros(n, dtype=bool)
        if flags & SKIP_N:
            skip |= ~IS_BASE[win].all(axis=1)
        if flags & SKIP_MASKED:
            skip |= IS_LOWER[win].any(axis=1)
        codes = np.where(CODE[win] < 0, 3, CODE[win])                        # (only under SKIP_N, where such a start is skipped)
        value = (codes * weights).sum(axis=1)
        counts[r] = np.bincount(value[~skip], minlength=4 ** k)
        skipped[r] = int(skip.sum())
    return counts, skipped


def n_considered(records, k, ranges, flags):
    out = []
    for c, lo, hi in ranges:
        first, last = considered_starts(len(records[c]), k, lo, hi, bool(flags & BY_START))
        out.append(0 if hi < lo else max(0, last - first + 1))
    return np.asarray(out, dtype=np.int64)


def reverse_complement(seq: bytes) -> bytes:
    return bytes(seq).translate(bytes.maketrans(b"ACGTacgtNn", b"TGCAtgcaNn"))[::-1]
