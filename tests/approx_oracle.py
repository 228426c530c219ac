"""CPU statement of the edit-distance search (kgma_approx_match / api.approxMatch), in numpy; no library code.

Every residue and every query symbol is a 4-bit set of bases (bit 0 A, 1 C, 2 G, 3 T; N = all four).  A residue matches a symbol
when its set is a subset of the symbol's set: a base matches a symbol that contains it, a genome N matches only a query N.

For a record t[1..L] and a query q[1..m], score(j) = min over 1 <= s <= j + 1 of ed(q, t[s..j]) with unit costs -- Sellers'
semi-global dynamic programme: C[0][j] = 0, C[i][0] = i, C[i][j] = min(C[i-1][j-1] + (0 if match else 1), C[i][j-1] + 1,
C[i-1][j] + 1), score(j) = C[m][j].  An end j with score(j) <= e is a matching end; its start is the largest s with
ed(q, t[s..j]) == score(j).  A run is a maximal set of consecutive matching ends; its best end has the smallest score, on a tie
the smallest end.  Nothing spans two records.

The second statement, `bitvector_scores`, is Myers' bit-vector recurrence in Python integers (the search form the device kernel
runs); tests/test_approx_host.py holds it equal to `scores`.

`python -m tests.approx_oracle` writes tests/golden/approx.json from tests/data/Loci.fasta."""
import functools
import json
import os

import numpy as np

IUPAC = {"A": 1, "C": 2, "G": 4, "T": 8, "R": 5, "Y": 10, "S": 6, "W": 9, "K": 12, "M": 3, "B": 14, "D": 13, "H": 11, "V": 7, "N": 15}
_COMP = bytes.maketrans(b"ATCGMKRYVBHDatcgmkryvbhd", b"TAGCKMYRBVDHtagckmyrbvdh")
MAX_LEN, MAX_EDITS = 64, 15

# the recombination signal sequences of src/RSS.jl:11-15 (12- and 23-nt spacer)
HumanRSSV = b"CACAGTG" + b"N" * 12 + b"ACAAAAACC"
HumanRSSD = b"CACAGTG" + b"N" * 23 + b"ACAAAAACC"

_SETS = np.zeros(256, dtype=np.uint8)
for _ch, _s in IUPAC.items():
    _SETS[ord(_ch)] = _SETS[ord(_ch.lower())] = _s
_GENOME_OK = np.zeros(256, dtype=bool)
for _ch in b"ACGTNacgtn":
    _GENOME_OK[_ch] = True


def _bytes(x) -> bytes:
    return x.encode() if isinstance(x, str) else bytes(x)


def query_sets(query) -> np.ndarray:
    q = _bytes(query)
    if not 1 <= len(q) <= MAX_LEN:
        raise ValueError("a query has 1 ... 64 symbols")
    s = _SETS[np.frombuffer(q, dtype=np.uint8)]
    if (s == 0).any():
        raise ValueError("query symbol outside the IUPAC alphabet")
    return s


def residue_sets(seq) -> np.ndarray:
    b = np.frombuffer(_bytes(seq), dtype=np.uint8)
    if not _GENOME_OK[b].all():
        raise ValueError("genome residue outside A/C/G/T/N")
    return _SETS[b]


def check_edits(query, e) -> int:
    e = int(e)
    if not 0 <= e <= MAX_EDITS or e >= int((query_sets(query) != 15).sum()):
        raise ValueError("max_edits must be 0 ... 15 and smaller than the number of informative symbols")
    return e


def revcomp(query) -> bytes:
    return _bytes(query).translate(_COMP)[::-1]


def _cost_columns(qs: np.ndarray) -> dict:
    """Per residue set r the substitution costs of the query's symbols: 0 where r is a subset of the symbol's set."""
    return {r: ((r & ~qs & 15) != 0).astype(np.int64) for r in (1, 2, 4, 8, 15)}


def scores(query, text) -> np.ndarray:
    """score(j) for j = 1 ... L: Sellers' dynamic programme, column by column."""
    qs, rs = query_sets(query), residue_sets(text)
    m = qs.size
    cost = _cost_columns(qs)
    i = np.arange(m + 1, dtype=np.int64)
    col = i.copy()                                    # C[.][0]
    out = np.zeros(rs.size, dtype=np.int64)
    x = np.zeros(m + 1, dtype=np.int64)
    for j, r in enumerate(rs.tolist()):
        x[0] = 0
        np.minimum(col[:-1] + cost[r], col[1:] + 1, out=x[1:])     # diagonal and horizontal moves
        col = np.minimum.accumulate(x - i) + i                      # the vertical chain C[i-1][j] + 1
        out[j] = col[m]
    return out


def bitvector_scores(query, text, first: int = 0, fresh_at: int = 0) -> np.ndarray:
    """The same scores by the bit-vector recurrence (Myers 1999, the search form: the horizontal delta of row 0 is 0).
    Scores of the columns first .. L - 1 (0-based) from a FRESH state (Pv = ones, Mv = 0, score = m) at column fresh_at <= first:
    with the defaults, score(j) for every j."""
    qs, rs = query_sets(query), residue_sets(text)
    m = qs.size
    mask = (1 << m) - 1
    peq = {r: sum(1 << i for i in range(m) if (r & ~int(qs[i]) & 15) == 0) for r in (1, 2, 4, 8, 15)}
    Pv, Mv, score = mask, 0, m
    out = np.zeros(rs.size - first, dtype=np.int64)
    for j, r in enumerate(rs[fresh_at:].tolist(), start=fresh_at):
        Eq = peq[r]
        Xv = Eq | Mv
        Xh = ((((Eq & Pv) + Pv) & mask) ^ Pv) | Eq
        Ph = Mv | (~(Xh | Pv) & mask)
        Mh = Pv & Xh
        score += (Ph >> (m - 1)) & 1
        score -= (Mh >> (m - 1)) & 1
        Ph = (Ph << 1) & mask
        Mh = (Mh << 1) & mask
        Pv = Mh | (~(Xv | Ph) & mask)
        Mv = Ph & Xv
        if j >= first:
            out[j - first] = score
    return out


def restarted_scores(query, text, e, tile) -> np.ndarray:
    """What a search gives whose state is made fresh m + e columns before every `tile` ends (or at the record's first residue):
    per tile the scores of its own ends."""
    m, L = len(_bytes(query)), len(_bytes(text))
    parts = [bitvector_scores(query, _bytes(text)[:min(L, a + tile)], a, max(0, a - (m + e))) for a in range(0, L, tile)]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


def ends(query, text, e):
    """[(end, score)] of one record, 1-based, ascending: the matching ends."""
    e = check_edits(query, e)
    sc = scores(query, text)
    idx = np.flatnonzero(sc <= e)
    return list(zip((idx + 1).tolist(), sc[idx].tolist()))


def edit_distances_to_end(query, window) -> np.ndarray:
    """ed(q, t[s..j]) for every start s of the window t[j-n+1..j], s = j + 1 (the empty substring, index 0), j, ..., j - n + 1:
    one global dynamic programme of the reversed query against t[j], t[j-1], ..."""
    qs, rs = query_sets(query)[::-1], residue_sets(window)[::-1]
    m = qs.size
    cost = _cost_columns(qs)
    i = np.arange(m + 1, dtype=np.int64)
    col = i.copy()
    out = np.zeros(rs.size + 1, dtype=np.int64)
    out[0] = m
    x = np.zeros(m + 1, dtype=np.int64)
    for c, r in enumerate(rs.tolist(), start=1):
        x[0] = c                                                    # (anchored: the whole substring is aligned)
        np.minimum(col[:-1] + cost[r], col[1:] + 1, out=x[1:])
        col = np.minimum.accumulate(x - i) + i
        out[c] = col[m]
    return out


@functools.lru_cache(maxsize=1 << 16)
def _shortest_best(query: bytes, window: bytes) -> int:
    d = edit_distances_to_end(query, window)
    return int(np.flatnonzero(d == d.min())[0])


def start_of(query, text, j) -> int:
    """The largest s with ed(q, t[s..j]) == score(j).  Every candidate start is tried: a substring of more than 2m residues is
    more than m edits from the query, and score(j) <= m (the empty substring).  (The answer depends on the 2m residues before
    the end alone, and is remembered for them.)"""
    q, t = _bytes(query), _bytes(text)
    return j + 1 - _shortest_best(q, t[max(0, j - 2 * len(q)):j])


def runs_best(matching):
    """[(end, score)] ascending -> the best end of every run of consecutive ends: the smallest score, on a tie the smallest end."""
    out, i = [], 0
    while i < len(matching):
        k = i
        while k + 1 < len(matching) and matching[k + 1][0] == matching[k][0] + 1:
            k += 1
        out.append(min(matching[i:k + 1], key=lambda t: (t[1], t[0])))
        i = k + 1
    return out


def find(query, text, e, best_only=True):
    """[(start, end, edits)] of one record."""
    found = ends(query, text, e)
    if best_only:
        found = runs_best(found)
    return [(start_of(query, text, j), j, k) for j, k in found]


def search(queries, records, max_edits, best_only=True):
    """(query, record, start, end, edits), 0-based query and record, sorted by (query, record, end): what
    kgma_get_approx_matches returns."""
    if isinstance(max_edits, int):
        max_edits = [max_edits] * len(queries)
    return [(i, c, s, j, k) for i, (q, e) in enumerate(zip(queries, max_edits)) for c, r in enumerate(records)
            for s, j, k in find(q, r, e, best_only)]


def api_list(query, records, e, strand="+", all_ends=False):
    """(record, lo, hi, strand, edits) sorted by (record, lo, strand): api.approxMatch_batch without the identifier."""
    out = []
    if strand != "-":
        out += [(c, s, j, "+", k) for c, r in enumerate(records) for s, j, k in find(query, r, e, not all_ends)]
    if strand != "+":
        out += [(c, s, j, "-", k) for c, r in enumerate(records) for s, j, k in find(revcomp(query), r, e, not all_ends)]
    return sorted(out, key=lambda t: (t[0], t[1], t[3], t[2]))


# ---- tests/golden/approx.json ---------------------------------------------------------------------------------------------------
GOLDEN_MOTIFS = {"HumanRSSD": HumanRSSD, "HumanRSSV": HumanRSSV}
GOLDEN_EDITS = (0, 1, 2)
MADE_BY = "python -m tests.approx_oracle"


def read_fasta_sequences(path):
    """The records' residues (plain reader: '>' starts a record)."""
    seqs, cur = [], None
    with open(path, "rb") as f:
        for line in f:
            line = line.strip()
            if line.startswith(b">"):
                cur = []
                seqs.append(cur)
            elif line and cur is not None:
                cur.append(line)
    return [b"".join(s) for s in seqs]


def golden_entry(query, records, e):
    """One (motif, e, strand) entry: all ends and the best end of every run as [record, start, end, edits]."""
    out = {"all": [], "best": []}
    for c, r in enumerate(records):
        found = ends(query, r, e)
        out["all"] += [[c, start_of(query, r, j), j, k] for j, k in found]
        out["best"] += [[c, start_of(query, r, j), j, k] for j, k in runs_best(found)]
    return out


def make_golden(records):
    out = {"made_by": MADE_BY, "fasta": "tests/data/Loci.fasta", "entries": {}}
    for name, motif in GOLDEN_MOTIFS.items():
        for e in GOLDEN_EDITS:
            for strand, q in (("+", motif), ("-", revcomp(motif))):
                out["entries"][f"{name}|{e}|{strand}"] = golden_entry(q, records, e)
    return out


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    golden = make_golden(read_fasta_sequences(os.path.join(root, "tests", "data", "Loci.fasta")))
    with open(os.path.join(root, "tests", "golden", "approx.json"), "w") as f:
        json.dump(golden, f, indent=0, separators=(",", ":"))
        f.write("\n")
    for key, v in golden["entries"].items():
        print(key, len(v["all"]), "ends,", len(v["best"]), "runs")
