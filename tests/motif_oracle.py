"""CPU statement of the motif search (kgma_motif_match / api.motifMatch), in numpy.

Every residue and every motif symbol is a 4-bit set of bases (bit 0 A, 1 C, 2 G, 3 T; N = all four).  A position matches when
the residue's set is a subset of the symbol's set, so a base matches a symbol that contains it and a genome N matches only a
motif N.  mism(s) is the number of non-matching positions of the motif laid at start s, summed position by position; start s
(1-based) is a match iff s + m - 1 <= L and mism(s) <= max_mismatch.  No match spans two records."""
import numpy as np

IUPAC = {"A": 1, "C": 2, "G": 4, "T": 8, "R": 5, "Y": 10, "S": 6, "W": 9, "K": 12, "M": 3, "B": 14, "D": 13, "H": 11, "V": 7, "N": 15}
_COMP = bytes.maketrans(b"ATCGMKRYVBHDatcgmkryvbhd", b"TAGCKMYRBVDHtagckmyrbvdh")

_SETS = np.zeros(256, dtype=np.uint8)
for _ch, _s in IUPAC.items():
    _SETS[ord(_ch)] = _SETS[ord(_ch.lower())] = _s
_GENOME_OK = np.zeros(256, dtype=bool)
for _ch in b"ACGTNacgtn":
    _GENOME_OK[_ch] = True


# tests/data/Loci.fasta: the summed length of the records before each record, the seven V-gene loci of tests/golden/scan.json, and
# the matches (0-based record, start, mismatches) of the two recombination signal sequences with one mismatch on the plus strand
LOCI_CUM = [0, 121478, 221227, 444023]
LOCI_GENES = [8543, 20425, 221912, 234018, 450875, 467930, 477868]
LOCI_RSSD_D1 = [(0, 8839, 0), (0, 20721, 1), (2, 981, 0), (2, 13087, 1), (3, 7148, 1), (3, 24206, 1), (3, 34138, 0)]
LOCI_RSSV_D1 = [(0, 59186, 1), (0, 82730, 1), (2, 51945, 1), (2, 75561, 1)]


def _bytes(x) -> bytes:
    return x.encode() if isinstance(x, str) else bytes(x)


def motif_sets(motif) -> np.ndarray:
    m = _bytes(motif)
    if not 1 <= len(m) <= 64:
        raise ValueError("a motif has 1 ... 64 symbols")
    s = _SETS[np.frombuffer(m, dtype=np.uint8)]
    if (s == 0).any():
        raise ValueError("motif symbol outside the IUPAC alphabet")
    return s


def residue_sets(seq) -> np.ndarray:
    b = np.frombuffer(_bytes(seq), dtype=np.uint8)
    if not _GENOME_OK[b].all():
        raise ValueError("genome residue outside A/C/G/T/N")
    return _SETS[b]


def revcomp(motif) -> bytes:
    return _bytes(motif).translate(_COMP)[::-1]


def mism_profile(motif, seq) -> np.ndarray:
    """mism(s) for s = 1 ... L - m + 1 (empty when the motif is longer than the record)."""
    ms, rs = motif_sets(motif), residue_sets(seq)
    n = rs.size - ms.size + 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    out = np.zeros(n, dtype=np.int64)
    for j in range(ms.size):
        out += (rs[j:j + n] & ~ms[j] & 15) != 0
    return out


def find(motif, seq, d):
    """[(start, mismatches)] of one record, 1-based, ascending."""
    d = int(d)
    if not 0 <= d <= 15 or d >= int((motif_sets(motif) != 15).sum()):
        raise ValueError("max_mismatch must be 0 ... 15 and smaller than the number of informative positions")
    p = mism_profile(motif, seq)
    idx = np.flatnonzero(p <= d)
    return list(zip((idx + 1).tolist(), p[idx].tolist()))


def match_list(motifs, records, ds):
    """(motif, record, start, mismatches), 0-based motif and record, sorted by (motif, record, start): what
    kgma_get_motif_matches returns."""
    if isinstance(ds, int):
        ds = [ds] * len(motifs)
    return [(i, c, s, k) for i, (m, d) in enumerate(zip(motifs, ds)) for c, r in enumerate(records) for s, k in find(m, r, d)]


def api_list(motif, records, d, strand="+"):
    """(record, lo, hi, strand, mismatches) sorted by (record, lo, strand): api.motifMatch_batch without the identifier."""
    m = len(_bytes(motif))
    out = []
    if strand != "-":
        out += [(c, s, s + m - 1, "+", k) for c, r in enumerate(records) for s, k in find(motif, r, d)]
    if strand != "+":
        out += [(c, s, s + m - 1, "-", k) for c, r in enumerate(records) for s, k in find(revcomp(motif), r, d)]
    return sorted(out, key=lambda t: (t[0], t[1], t[3]))
