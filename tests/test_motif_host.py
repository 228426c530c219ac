"""Motif search without a GPU: the numpy oracle (tests/motif_oracle.py) against a naive double loop, RSS_dist and the RSS
constants as src/RSS.jl has them, reverse-complemented IUPAC motifs, the argument errors of the public functions (raised before
any device is touched), and the facts about tests/data/Loci.fasta that DESIGN.md section 5d quotes -- computed by the oracle AND
spelled out as literals."""
import os

import numpy as np
import pytest

from kmergma_amd import _lib, api, fasta
from tests import motif_oracle as mo
from tests.conftest import DATA

LOCI = os.path.join(DATA, "Loci.fasta")
CUM, RSSD_D1, RSSV_D1 = mo.LOCI_CUM, mo.LOCI_RSSD_D1, mo.LOCI_RSSV_D1


def naive(motif, seq, d):
    """The semantics word for word: per start, per position, set containment."""
    sets = mo.IUPAC
    m, s = motif.upper(), seq.upper()
    out = []
    for st in range(len(s) - len(m) + 1):
        k = 0
        for j in range(len(m)):
            r, q = s[st + j], m[j]
            if r == "N":
                ok = q == "N"
            else:
                ok = bool(sets[q] & sets[r])
            k += 0 if ok else 1
        if k <= d:
            out.append((st + 1, k))
    return out


def test_oracle_against_naive_loop():
    rng = np.random.default_rng(7)
    syms = "ACGTRYSWKMBDHVN"
    for _ in range(60):
        L = int(rng.integers(1, 120))
        seq = "".join(rng.choice(list("ACGTNacgtn"), size=L, p=[.2, .2, .2, .2, .05, .03, .03, .03, .03, .03]))
        m = int(rng.integers(1, 20))
        motif = "".join(rng.choice(list(syms + syms.lower()), size=m))
        inf = sum(1 for ch in motif.upper() if ch != "N")
        if inf == 0:
            continue
        d = int(rng.integers(0, min(inf, api.MOTIF_MAX_MISMATCH + 1)))
        assert api._motif_bytes(motif, d) == motif.encode()               # (the public functions accept what the oracle accepts)
        assert mo.find(motif, seq, d) == naive(motif, seq, d)
    assert mo.find("T", "ANNA", 0) == [] and mo.find("NA", "ANNA", 0) == [(3, 0)]                # N under T, N under N
    assert mo.find("TN", "ANNATN", 0) == [(5, 0)] and mo.find("AN", "ccanna", 0) == [(3, 0)]
    assert mo.find("R", "AGCTN", 0) == [(1, 0), (2, 0)]
    assert mo.find("ACGT", "ACG", 0) == []                                 # longer than the record
    with pytest.raises(ValueError):
        mo.find("AXA", "AAAA", 0)
    with pytest.raises(ValueError):
        mo.find("ACG", "AARA", 0)
    with pytest.raises(ValueError):
        mo.find("ANN", "AAAA", 1)


def test_match_list_order():
    recs = [b"ACGTACGT", b"ttacg"]
    rss = b"CACAGTG" + b"ACGTACGTACGT" + b"ACAAAAACC"
    assert mo.match_list([api.HumanRSSV, api.HumanRSSD], [b"tt" + rss + b"a", rss], [0, 1]) == [(0, 0, 3, 0), (0, 1, 1, 0)]
    assert mo.match_list([b"ACG", b"TW"], recs, [1, 0]) == [
        (0, 0, 1, 0), (0, 0, 5, 0), (0, 1, 3, 0), (1, 0, 4, 0), (1, 1, 1, 0), (1, 1, 2, 0)]
    assert mo.api_list(b"ACG", recs, 0, "both") == [(0, 1, 3, "+", 0), (0, 2, 4, "-", 0), (0, 5, 7, "+", 0), (0, 6, 8, "-", 0),
                                                     (1, 3, 5, "+", 0)]


def test_rss_constants():
    assert api.HumanRSSV == b"CACAGTG" + b"N" * 12 + b"ACAAAAACC" and len(api.HumanRSSV) == 28
    assert api.HumanRSSD == b"CACAGTG" + b"N" * 23 + b"ACAAAAACC" and len(api.HumanRSSD) == 39
    assert api.MOTIF_MAX_LEN == 64 and api.MOTIF_MAX_MISMATCH == 15


def test_rss_dist_known_answers():
    assert api.RSS_dist(b"ACGT", b"ACGT") == 0 and api.RSS_dist("ACGT", "AGGA") == 2 and api.RSS_dist("acgt", "ACGT") == 0
    assert api.RSS_dist(b"AC", b"ACGT") == 0                                 # only RSS1's positions are compared
    perfect = b"CACAGTG" + b"ACGTACGTACGT" + b"ACAAAAACC"
    assert api.RSS_dist(perfect) == 12                                       # the quirk: every N of the spacer counts
    assert api.RSS_dist(api.HumanRSSV) == 0 and api.RSS_dist(api.HumanRSSD, api.HumanRSSD) == 0
    assert api.RSS_dist(b"CACAGTG" + b"N" * 12 + b"ACAAAAACG") == 1
    with pytest.raises(IndexError):
        api.RSS_dist(api.HumanRSSD)                                          # 39 symbols against HumanRSSV's 28
    with pytest.raises(IndexError):
        api.RSS_dist(b"ACGT", b"ACG")


def test_reverse_complemented_iupac_motifs():
    assert fasta.reverse_complement(b"ACGTRYSWKMBDHVN") == b"NBDHVKMWSRYACGT" == mo.revcomp(b"ACGTRYSWKMBDHVN")
    assert fasta.reverse_complement(api.HumanRSSD) == b"GGTTTTTGT" + b"N" * 23 + b"CACTGTG"
    # the minus strand of a motif on a sequence = the plus strand on the reverse-complemented sequence, mirrored
    rng = np.random.default_rng(11)
    seq = bytes(rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=400, p=[.24, .24, .24, .24, .04]))
    for motif, d in ((b"RYN", 0), (b"ACNNGT", 1), (b"WSKMB", 2), (b"ACGT", 1)):
        minus = [(s, k) for s, k in mo.find(mo.revcomp(motif), seq, d)]
        plus_rc = mo.find(motif, fasta.reverse_complement(seq), d)
        assert sorted((len(seq) - (s + len(motif) - 1) + 1, k) for s, k in plus_rc) == minus
    both = mo.api_list(b"ACGT", [seq], 1, "both")                            # its own reverse complement: reported twice
    assert [t for t in both if t[3] == "+"] == [(c, lo, hi, "+", k) for c, lo, hi, _, k in both if _ == "-"]


BAD = [(b"", 0), (b"A" * 65, 0), (b"ACXG", 0), (b"AC-G", 0), (b"ACGT", 4), (b"ACGT", 7), (b"ANNT", 2), (b"NNNN", 0), (b"N", 0),
       (b"ACGTACGTACGTACGTACGT", 16), (b"ACGT", -1)]


@pytest.mark.parametrize("fn", [lambda m, d: api.motifMatch(m, b"ACGTACGT", max_mismatch=d),
                                lambda m, d: api.motifMatch(m, LOCI, max_mismatch=d),
                                lambda m, d: api.motifMatch_batch([b"ACG", m], LOCI, max_mismatch=[0, d]),
                                lambda m, d: api.findRSS(LOCI, m, d)])
def test_argument_errors_need_no_device(fn):
    for motif, d in BAD:
        with pytest.raises(ValueError):
            fn(motif, d)
    with pytest.raises(TypeError):
        fn(1234, 0)


def test_more_argument_errors_need_no_device():
    with pytest.raises(ValueError):
        api.motifMatch(b"ACGT", b"ACGTACGT", strand="x")
    with pytest.raises(ValueError):
        api.findRSS(LOCI, strand="plus")
    with pytest.raises(ValueError):
        api.motifMatch_batch([b"ACG", b"ACGT"], LOCI, max_mismatch=[0])
    with pytest.raises(TypeError):
        api.motifMatch(b"ACGT", 3.5)


def test_bindings_declare_the_entry_points():
    assert {"kgma_motif_match", "kgma_get_motif_matches"} <= set(_lib.EXPORTS)
    assert _lib.MOTIF_HIT_DTYPE.itemsize == 24 and _lib.C.sizeof(_lib.KgmaMotifHit) == 24
    assert [_lib.MOTIF_HIT_DTYPE.fields[n][1] for n in ("motif", "contig", "start", "mismatches")] == [0, 4, 8, 16]
    L = _lib.load()
    assert L.kgma_motif_match and L.kgma_get_motif_matches


# ---- the fixture ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seqs(loci):
    return [r.sequence for r in loci]


def _triples(motif, seqs, d):
    return [(c, s, k) for _, c, s, k in mo.match_list([motif], seqs, d)]


def test_fixture_rssd(seqs):
    assert _triples(api.HumanRSSD, seqs, 1) == RSSD_D1
    assert _triples(mo.revcomp(api.HumanRSSD), seqs, 1) == []
    assert len(mo.api_list(api.HumanRSSD, seqs, 2, "both")) == 14
    assert len(mo.api_list(api.HumanRSSD, seqs, 3, "both")) == 30


def test_fixture_rssv(seqs):
    assert _triples(api.HumanRSSV, seqs, 0) == []
    assert _triples(api.HumanRSSV, seqs, 1) == RSSV_D1
    assert len(mo.api_list(api.HumanRSSV, seqs, 2, "both")) == 8
    assert len(mo.api_list(api.HumanRSSV, seqs, 3, "both")) == 23


def test_fixture_rss_behind_every_golden_locus(seqs, golden):
    assert [sum(len(s) for s in seqs[:c]) for c in range(4)] == CUM
    want = mo.LOCI_GENES
    assert golden["scan"]["single_align"]["hit_loci"] == want
    starts = [CUM[c] + s for c, s, _ in _triples(api.HumanRSSD, seqs, 1)]
    diffs = [s - l for s, l in zip(starts, want)]                           # one-to-one, in order
    assert len(starts) == 7 and all(293 <= x <= 299 for x in diffs), diffs
