"""Host side of strand=: the complement map, the strand field of the headers, the coordinate map, argument checking, and the
library's ABI for kgma_genome_revcomp.  No GPU."""
import ctypes
import os
import re

import pytest

from kmergma_amd import _lib, api, fasta, headers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(b"A", b"T"), (b"C", b"G"), (b"M", b"K"), (b"R", b"Y"), (b"V", b"B"), (b"H", b"D")]
SELF = b"WSN-"
ALPHABET = b"ACGTMRWSYKVHDBN-acgtmrwsykvhdbn"


def test_reverse_complement_pairs_and_case():
    rc = fasta.reverse_complement
    for a, b in PAIRS:
        assert rc(a) == b and rc(b) == a
        assert rc(a.lower()) == b.lower() and rc(b.lower()) == a.lower()
    for ch in SELF:
        assert rc(bytes([ch])) == bytes([ch]) and rc(bytes([ch]).lower()) == bytes([ch]).lower()


def test_reverse_complement_is_an_involution_over_the_alphabet():
    rc = fasta.reverse_complement
    assert rc(rc(ALPHABET)) == ALPHABET
    assert rc(ALPHABET) == bytes(rc(bytes([c]))[0] for c in reversed(ALPHABET))
    every = bytes(range(256))
    assert rc(rc(every)) == every


def test_reverse_complement_leaves_other_bytes_alone():
    rc = fasta.reverse_complement
    letters = set(b"ATCGMKRYVBHDatcgmkryvbhd")
    for c in range(256):
        if c not in letters:
            assert rc(bytes([c])) == bytes([c])
    assert rc(b"AX*Uu.c") == b"g.uU*XT"
    assert rc(b"") == b""


def test_reverse_complement_example():
    assert fasta.reverse_complement(b"AACGTNnRyKM-") == b"-KMrYnNACGTT"
    assert isinstance(fasta.reverse_complement(bytearray(b"ACG")), bytes)


def test_headers_plus_is_unchanged_and_minus_appends_the_field():
    want = "JQ684648.1 | dist = 9.21 | MatchPos = 20380:20768 | GenomePos = 0 | Len = 389"     # __graft_entry__.smoke
    args = ("JQ684648.1", 9.2123, 20380, 20768, 0)
    assert headers.single_header(*args) == want
    assert headers.single_header(*args, strand="+") == want
    assert headers.single_header(*args, strand="-") == want + " | Strand = -"
    assert headers.single_header(*args, False, strand="-") == "JQ684648.1 | dist = 9.21 | MatchPos = 20380:20768 | Len = 389 | Strand = -"
    omn = ("id", 12.5, 3, 10, 20, 7)
    plain = "id | Dist = 12.5 | KFV = 3 | MatchPos = 10:20 | GenomePos = 7 | Len = 11"
    assert headers.omn_header(*omn) == plain == headers.omn_header(*omn, strand="+")
    assert headers.omn_header(*omn, strand="-") == plain + " | Strand = -"
    with pytest.raises(ValueError):
        headers.single_header(*args, strand="both")


def test_coordinate_map():
    L = 121478
    assert api.strand_range(L, 85654, 86042) == (35437, 35825)
    assert api.strand_range(L, *api.strand_range(L, 85654, 86042)) == (85654, 86042)
    assert api.strand_range(L, 1, L) == (1, L)
    assert api.strand_range(L, 1, 1) == (L, L) and api.strand_range(L, L, L) == (1, 1)
    # the range keeps its length, and it names the same residues: s[lo-1:hi] reversed is rc-string[lo'-1:hi']
    s = b"AACCGGTTACGTNACGATCG"
    r = fasta.reverse_complement(s)
    for lo, hi in [(1, 4), (3, 17), (20, 20), (1, 20)]:
        lo2, hi2 = api.strand_range(len(s), lo, hi)
        assert hi2 - lo2 == hi - lo
        assert r[lo2 - 1:hi2] == fasta.reverse_complement(s[lo - 1:hi])


@pytest.mark.parametrize("call", [
    lambda: api.ac_gma_testing(genome_path="no such file", refVec=[0.0] * 7, k=99, strand="x", resultVec=[]),
    lambda: api.record_KmerGMA(record=fasta.Record("r", b"ACGT"), refVec=[0.0] * 7, k=99, resultVec_vec=[[]], strand="x"),
    lambda: api.Omn_KmerGMA(genome_path="no such file", refVecs=[[0.0] * 7], windowsizes=[5], resultVec=[], k=99, strand="x"),
    lambda: api.StrobeGMA(genome_path="no such file", refVec=[0.0] * 7, s=99, strand="x"),
    lambda: api.findGenes(genome_path="no such file", ref_path="no such file", k=99, strand="x"),
    lambda: api.findGenes_cluster_mode(genome_path="no such file", ref_path="no such file", k=99, strand="x"),
    lambda: api.Strobemer_findGenes(genome_path="no such file", ref_path="no such file", s=99, strand="x"),
    lambda: api.findGenes(genome_path="no such file", ref_path="no such file", strand="minus"),
    lambda: api.findGenes(genome_path="no such file", ref_path="no such file", strand=None),
])
def test_bad_strand_is_refused_before_anything_else(call, monkeypatch):
    """The other arguments are invalid too (missing files, k and s no engine serves) and there may be no GPU: the strand
    check comes first, before references are read and before a context is made."""
    def no_context(*a, **k):
        raise AssertionError("a device context was asked for")
    monkeypatch.setattr(api, "default_context", no_context)
    with pytest.raises(ValueError, match="strand"):
        call()


def test_revcomp_is_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "kgma.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+kgma_genome_revcomp\s*\(\s*kgma_ctx\s*\*\s*ctx\s*,\s*const\s+kgma_genome\s*\*\s*g\s*,\s*kgma_genome\s*\*\*\s*out\s*\)\s*;", code)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("kgma_genome_revcomp", "kgma_genome_revcomp_into"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name), f"libkgma.so does not export {name}"
        assert name in _lib.EXPORTS
    assert hasattr(_lib.Genome, "revcomp")
    # null arguments: KGMA_E_ARG, no device needed
    L = _lib.load()
    out = ctypes.c_void_p()
    assert L.kgma_genome_revcomp(None, None, ctypes.byref(out)) == _lib.KGMA_E_ARG
