"""Exact search without a GPU: the reference's own expected values (tests/golden/exact.json) hold for the CPU oracle
(tests/exact_oracle.py) in both overlap modes, fasta_id_to_cumulative_len_dict gives the reference's dictionary, and the
argument errors of the public functions are raised before any device is touched."""
import json
import os

import pytest

from kmergma_amd import _lib, api, fasta
from tests import exact_oracle as eo
from tests.conftest import DATA, GOLDEN


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLDEN, "exact.json")) as fh:
        return json.load(fh)


def _reader_result(query, recs, overlap=True):
    """exactMatch over a FASTA reader (src/ExactMatch.jl:100-121) on the oracle."""
    out = {}
    for r in recs:
        m = eo.find_all(query, r.sequence, overlap)
        if m:
            out[r.identifier] = m
    return out or "no match"


def _golden_query(g, recs):
    if "query" in g:
        return g["query"].encode()
    f = g["query_from"]
    return recs[f["record"] - 1].sequence[f["lo"] - 1:f["hi"]]


def test_oracle_single_sequence_goldens(gold):
    for g in gold["single_seq"]:
        got = eo.find_all(g["query"], g["subject"], g["overlap"]) or None
        assert got == (None if g["expect"] is None else [tuple(x) for x in g["expect"]])


def test_oracle_reader_goldens(gold):
    for g in gold["reader"]:
        recs = fasta.read_fasta(os.path.join(DATA, g["fasta"]))
        got = _reader_result(_golden_query(g, recs), recs)
        want = g["expect"] if isinstance(g["expect"], str) else {k: [tuple(x) for x in v] for k, v in g["expect"].items()}
        assert got == want


def test_oracle_overlap_modes():
    assert [lo for lo, _ in eo.find_all("AAAA", "A" * 10, True)] == [1, 2, 3, 4, 5, 6, 7]
    assert [lo for lo, _ in eo.find_all("AAAA", "A" * 10, False)] == [1, 5]
    assert eo.find_all("GAGAG", "GAGAGAGAGAG", True) == [(1, 5), (3, 7), (5, 9), (7, 11)]
    assert eo.find_all("GAGAG", "GAGAGAGAGAG", False) == [(1, 5), (7, 11)]


def test_oracle_symbol_equality():
    assert eo.find_all("T", "ANNA") == [] and eo.find_all("N", "ATTA") == []
    assert eo.find_all("AN", "ccanna") == [(3, 4)]
    assert eo.find_all("R", "ARGAN") == [(2, 2)] and eo.find_all("A", "RRR") == []
    assert eo.find_all("acgt", "ttACgTaa") == [(3, 6)]
    with pytest.raises(ValueError):
        eo.find_all("AXA", "AAAA")
    with pytest.raises(ValueError):
        eo.find_all("", "AAAA")


def test_match_list_is_sorted_and_complete():
    recs = [b"ACGTACGT", b"ttacg", b"AC"]
    assert eo.match_list([b"ACG", b"T"], recs) == [(0, 0, 1), (0, 0, 5), (0, 1, 3), (1, 0, 4), (1, 0, 8), (1, 1, 1), (1, 1, 2)]


def test_cumulative_len_dict_golden(gold):
    g = gold["cumulative_len"]
    assert api.fasta_id_to_cumulative_len_dict(os.path.join(DATA, g["fasta"])) == g["expect"]
    with pytest.raises(TypeError):
        api.fasta_id_to_cumulative_len_dict(42)


@pytest.mark.parametrize("fn", [lambda q: api.exactMatch(q, b"ACGT"), lambda q: api.exactMatch(q, os.path.join(DATA, "Loci.fasta")),
                                lambda q: api.exactMatch_batch([b"ACG", q], os.path.join(DATA, "Loci.fasta"))])
def test_argument_errors_need_no_device(fn):
    with pytest.raises(ValueError):
        fn(b"")
    with pytest.raises(ValueError):
        fn("ACXGT")
    with pytest.raises(ValueError):
        fn(fasta.Record("q", b"AC GT"))
    with pytest.raises(TypeError):
        fn(1234)


def test_invalid_subject_type():
    with pytest.raises(TypeError):
        api.exactMatch(b"ACGT", 3.5)


def test_bindings_declare_the_entry_points():
    assert {"kgma_exact_match", "kgma_get_matches"} <= set(_lib.EXPORTS)
    assert _lib.MATCH_DTYPE.itemsize == 16 and _lib.C.sizeof(_lib.KgmaMatch) == 16
    L = _lib.load()
    assert L.kgma_exact_match and L.kgma_get_matches
