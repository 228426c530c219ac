"""CPU restatement of the reference's exact search, for the tests (a helper module, not a conftest).

The reference (src/ExactMatch.jl) repeats BioSequences' `findfirst(ExactSearchQuery(q), view(seq, start:end))`: symbol equality
on DNAAlphabet{4} after case folding, so N matches only N and an IUPAC code only itself.  On case-folded bytes that is
`bytes.find`.  FindAllOverlap (:33-43) restarts one symbol behind a match's first symbol, FindAll (:20-30) one behind its last.
Coordinates are 1-based and inclusive.
"""
ALPHABET = frozenset(b"ACGTMRWSYKVHDBN-")


def fold(seq) -> bytes:
    """Case-folded residue bytes; ValueError for a symbol outside the 16-symbol alphabet."""
    s = (seq.encode() if isinstance(seq, str) else bytes(seq)).upper()
    if not ALPHABET.issuperset(s):
        i = next(i for i, ch in enumerate(s) if ch not in ALPHABET)
        raise ValueError(f"symbol {i + 1} ({s[i:i + 1]!r}) is outside the DNA alphabet")
    return s


def find_all_folded(q: bytes, s: bytes, overlap: bool = True):
    out, start = [], 0
    while True:
        i = s.find(q, start)
        if i < 0:
            return out
        out.append((i + 1, i + len(q)))
        start = i + 1 if overlap else i + len(q)


def find_all(query, seq, overlap: bool = True):
    """All matches of `query` in ONE sequence as 1-based (lo, hi) pairs; [] if none."""
    q = fold(query)
    if not q:
        raise ValueError("empty query")
    return find_all_folded(q, fold(seq), overlap)


def match_list(queries, records, overlap: bool = True):
    """The complete sorted list of (query, record, start) triples -- 0-based query and record, 1-based start -- that
    kgma_get_matches returns for these queries over these records."""
    folded = [fold(s) for s in records]
    out = []
    for qi, q in enumerate(queries):
        fq = fold(q)
        if not fq:
            raise ValueError("empty query")
        for ci, s in enumerate(folded):
            out.extend((qi, ci, lo) for lo, _ in find_all_folded(fq, s, overlap))
    return out
