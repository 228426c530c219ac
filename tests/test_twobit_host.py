"""The host parser of .2bit files (kgma_twobit.cpp) through its context-free entry kgma_twobit_inspect, and the reference
writer / reader of tests/twobit_ref.py: no GPU.  Every rejection the parser promises is provoked on files derived from a good one."""
import struct

import numpy as np
import pytest

from kmergma_amd import _lib, api
from tests import twobit_ref as tb

E_ARG, E_UNSUPPORTED = _lib.KGMA_E_ARG, _lib.KGMA_E_UNSUPPORTED

# one record `chr1` = ACGTNNacgtA, made by hand from the format's description
HAND = bytes.fromhex("4327411a 00000000 01000000 00000000" "04 63687231 19000000"
                     "0b000000 01000000 04000000 02000000 01000000 06000000 04000000 00000000 9c09c8")


def rand_seq(rng, n, n_runs=0, mask_runs=0) -> bytes:
    a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()
    for _ in range(n_runs if n else 0):
        s = int(rng.integers(0, n)); a[s:s + int(rng.integers(1, 40))] = ord("N")
    for _ in range(mask_runs if n else 0):
        s = int(rng.integers(0, n)); a[s:s + int(rng.integers(1, 60))] |= 0x20
    return a.tobytes()


def good_records():
    """A few records of different name lengths (one name empty, one record empty), with N runs and mask runs; the last one
    has packed bytes, so every byte of the file is needed."""
    rng = np.random.default_rng(20)
    return [("chr1", rand_seq(rng, 1003, 3, 5)), ("", rand_seq(rng, 64, 1, 1)), ("empty", b""), ("scaffold_17", rand_seq(rng, 7)),
            ("chrM", rand_seq(rng, 333, 2, 2))]


def inspect_bytes(tmp_path, data: bytes, name="f.2bit"):
    p = tmp_path / name
    p.write_bytes(data)
    return _lib.twobit_inspect(str(p))


def patched(data: bytes, off: int, fmt: str, value) -> bytes:
    b = bytearray(data)
    struct.pack_into(fmt, b, off, value)
    return bytes(b)


def record_offsets(data: bytes, version: int):
    """File offset of every record (from the index) and of the index entries' offset fields."""
    count = struct.unpack_from("<I", data, 8)[0]
    pos, recs, fields = 16, [], []
    for _ in range(count):
        pos += 1 + data[pos]
        fields.append(pos)
        recs.append(struct.unpack_from("<Q" if version == 1 else "<I", data, pos)[0])
        pos += 8 if version == 1 else 4
    return recs, fields


def malformed_files():
    """[(label, bytes, status, words the message must hold)]: the whole malformed set (the stand-alone sanitizer run of the parser
    reads the same files)."""
    out = []
    for version in (0, 1):
        recs = good_records()
        good = tb.twobit_bytes(recs, version)
        for cut in tb.field_boundaries(recs, version):
            out.append((f"v{version}-cut-{cut}", good[:cut], E_ARG, ()))
        offs, fields = record_offsets(good, version)
        r1 = offs[0]                                                   # record 0: dnaSize 1003, N blocks, mask blocks
        nn = struct.unpack_from("<I", good, r1 + 4)[0]
        m_at = r1 + 8 + 8 * nn
        mm = struct.unpack_from("<I", good, m_at)[0]
        assert nn >= 1 and mm >= 1
        out += [
            (f"v{version}-nstart", patched(good, r1 + 8, "<I", 1003), E_ARG, ("record 0", "nBlock")),
            (f"v{version}-nsize", patched(good, r1 + 8 + 4 * nn, "<I", 0xFFFFFFFF), E_ARG, ("record 0", "nBlock")),
            (f"v{version}-mstart", patched(good, m_at + 4, "<I", 0xFFFFFFF0), E_ARG, ("record 0", "maskBlock")),
            (f"v{version}-msize", patched(good, m_at + 4 + 4 * mm, "<I", 1004), E_ARG, ("record 0", "maskBlock")),
            (f"v{version}-ncount", patched(good, r1 + 4, "<I", 0x40000000), E_ARG, ("record 0", "nBlock")),
            (f"v{version}-mcount", patched(good, m_at, "<I", 0xFFFFFFFF), E_ARG, ("record 0", "maskBlock")),
            (f"v{version}-dnasize", patched(good, offs[4], "<I", 0xFFFFFFFF), E_ARG, ("record 4",)),
            (f"v{version}-offset", patched(good, fields[3], "<I", len(good) + 1), E_ARG, ("record 3", "offset")),
            (f"v{version}-count-huge", patched(good, 8, "<I", 0xFFFFFFFF), E_ARG, ("sequenceCount",)),
            (f"v{version}-count-index", patched(good, 8, "<I", 1000), E_ARG, ()),
            (f"v{version}-signature", patched(good, 0, "<I", 0x1A412744), E_ARG, ("signature",)),
            (f"v{version}-swapped", good[3::-1] + good[4:], E_UNSUPPORTED, ("signature", "swapped")),
            (f"v{version}-version2", patched(good, 4, "<I", 2), E_UNSUPPORTED, ("version",)),
        ]
        if version == 1:
            out.append(("v1-offset-2^63", patched(good, fields[2], "<Q", 1 << 63), E_ARG, ("record 2", "offset")))
            out.append(("v1-offset-max", patched(good, fields[2], "<Q", (1 << 64) - 1), E_ARG, ("record 2", "offset")))
    # a record whose packed bases would end exactly one byte behind the file
    one = tb.twobit_bytes([("x", b"ACGTA")])
    out.append(("packed-short", one[:-1], E_ARG, ("record 0", "packedDna")))
    return out


def good_files():
    """[(label, bytes)]: files the parser accepts."""
    out = [("hand", HAND), ("none-v0", tb.twobit_bytes([], 0)), ("none-v1", tb.twobit_bytes([], 1))]
    for version in (0, 1):
        out.append((f"good-v{version}", tb.twobit_bytes(good_records(), version)))
    out.append(("unnormalised", tb.twobit_bytes([UNNORMALISED])))
    return out


def test_hand_made_file_pins_the_encoding(tmp_path):
    assert len(HAND) == 60
    assert tb.read_twobit(HAND) == [("chr1", b"ACGTNNacgtA")]
    assert tb.read_twobit(HAND, mask=False) == [("chr1", b"ACGTNNACGTA")]
    assert inspect_bytes(tmp_path, HAND) == dict(version=0, n_records=1, total_bases=11, n_blocks=1, mask_blocks=1, packed_bytes=3)
    # the writer makes the same bytes of the same record
    assert tb.twobit_bytes([("chr1", b"ACGTNNacgtA")]) == HAND


@pytest.mark.parametrize("version", [0, 1])
def test_writer_reader_round_trip(tmp_path, version):
    rng = np.random.default_rng(5)
    recs = good_records() + [(f"r{n}", rand_seq(rng, n, 2, 3)) for n in (1, 2, 3, 4, 5, 255, 256, 4097)]
    recs += [("allN", b"N" * 37), ("alln", b"n" * 9), ("lower", b"acgtn" * 5)]
    data = tb.twobit_bytes(recs, version)
    assert tb.read_twobit(data) == [(n, s) for n, s in recs]
    assert tb.read_twobit(data, mask=False) == [(n, s.upper()) for n, s in recs]
    info = inspect_bytes(tmp_path, data)
    assert info["version"] == version and info["n_records"] == len(recs)
    assert info["total_bases"] == sum(len(s) for _, s in recs)
    assert info["packed_bytes"] == sum((len(s) + 3) // 4 for _, s in recs)
    assert info["n_blocks"] == sum(len(tb.runs((np.frombuffer(s, np.uint8) | 0x20) == ord("n"))) for _, s in recs)
    assert info["mask_blocks"] == sum(len(tb.runs(np.frombuffer(s, np.uint8) >= ord("a"))) for _, s in recs)


def test_versions_agree(tmp_path):
    recs = good_records()
    v0, v1 = tb.twobit_bytes(recs, 0), tb.twobit_bytes(recs, 1)
    assert len(v1) == len(v0) + 4 * len(recs)
    assert tb.read_twobit(v0) == tb.read_twobit(v1)
    a, b = inspect_bytes(tmp_path, v0, "a.2bit"), inspect_bytes(tmp_path, v1, "b.2bit")
    assert a.pop("version") == 0 and b.pop("version") == 1 and a == b


def test_writer_refuses_other_symbols():
    for seq in (b"ACGU", b"ACG-T", b"ACGR", b"AC GT", b"ACGT\n"):
        with pytest.raises(ValueError):
            tb.twobit_bytes([("x", seq)])


def test_no_records(tmp_path):
    for version in (0, 1):
        info = inspect_bytes(tmp_path, tb.twobit_bytes([], version))
        assert info == dict(version=version, n_records=0, total_bases=0, n_blocks=0, mask_blocks=0, packed_bytes=0)


_MALFORMED = malformed_files()


@pytest.mark.parametrize("label,data,status,words", _MALFORMED, ids=[m[0] for m in _MALFORMED])
def test_rejections(tmp_path, label, data, status, words):
    with pytest.raises(_lib.KgmaError) as e:
        inspect_bytes(tmp_path, data)
    assert e.value.status == status, e.value.message
    assert e.value.message
    for w in words:
        assert w in e.value.message, (w, e.value.message)


def test_truncations_cover_every_field():
    # the four header fields, every index entry's three, every record's nine (fields of zero length share their cut with the next)
    recs = good_records()
    data = tb.twobit_bytes(recs, 0)
    cuts = tb.field_boundaries(recs, 0)
    offs, fields = record_offsets(data, 0)
    assert cuts[:5] == [0, 4, 8, 12, 16] and cuts[-1] < len(data)
    for off, fld in zip(offs, fields):
        nn = struct.unpack_from("<I", data, off + 4)[0]
        mm = struct.unpack_from("<I", data, off + 8 + 8 * nn)[0]
        packed = off + 16 + 8 * nn + 8 * mm
        assert {fld, off, off + 4, off + 8, off + 8 + 8 * nn, packed - 4} <= set(cuts)
        assert packed in cuts or packed == len(data) or off == offs[2]   # (the empty record's packed bases begin where the next record does)


def test_missing_file_and_null_arguments(tmp_path):
    with pytest.raises(_lib.KgmaError) as e:
        _lib.twobit_inspect(str(tmp_path / "absent.2bit"))
    assert e.value.status == E_ARG and "absent.2bit" in e.value.message
    with pytest.raises(_lib.KgmaError) as e:
        _lib.twobit_inspect(str(tmp_path))                             # a directory
    assert e.value.status == E_ARG
    L = _lib.load()
    assert L.kgma_twobit_inspect(None, None, None, 0) == E_ARG


# blocks as a careless writer may leave them: unsorted, overlapping, adjacent, empty, repeated
UNNORMALISED = ("messy", b"ACGT" * 50,
                [(100, 10), (10, 5), (15, 5), (12, 1), (50, 0), (105, 20), (199, 1), (0, 0), (10, 5)],   # -> [10,20) [100,125) [199,200)
                [(0, 200), (5, 5), (200, 0)])                                                              # -> [0,200)


def test_block_lists_are_normalised(tmp_path):
    info = inspect_bytes(tmp_path, tb.twobit_bytes([UNNORMALISED]))
    assert info["n_blocks"] == 3 and info["mask_blocks"] == 1
    # already normalised lists keep their counts: adjacent-but-one blocks stay apart
    rec = ("tidy", b"ACGT" * 50, [(0, 1), (2, 1), (4, 196)], [(1, 1), (3, 1)])
    info = inspect_bytes(tmp_path, tb.twobit_bytes([rec]))
    assert info["n_blocks"] == 3 and info["mask_blocks"] == 2
    # a block may end exactly at dnaSize, and an empty block may sit there too
    rec = ("edge", b"ACGTA", [(4, 1), (5, 0)], [(0, 5)])
    assert inspect_bytes(tmp_path, tb.twobit_bytes([rec]))["n_blocks"] == 1


def test_sniffing_and_the_length_dict(tmp_path):
    recs = good_records()
    for version in (0, 1):
        p = tmp_path / f"genome_v{version}.fa"                         # (the name says FASTA: the content decides)
        p.write_bytes(tb.twobit_bytes(recs, version))
        assert _lib.is_twobit(str(p))
        d = api.fasta_id_to_cumulative_len_dict(str(p))
        want, total = {}, 0
        for name, seq in recs:
            want[name] = total
            total += len(seq)
        assert d == want
    fa = tmp_path / "genome.2bit"                                      # (and the other way round)
    fa.write_bytes(b">a desc\nACGT\n>b\nAC\n")
    assert not _lib.is_twobit(str(fa))
    assert api.fasta_id_to_cumulative_len_dict(str(fa)) == {"a desc": 0, "b": 4}
    empty = tmp_path / "empty.fa"
    empty.write_bytes(b"")
    assert not _lib.is_twobit(str(empty))
    bad = tmp_path / "bad.2bit"
    bad.write_bytes(tb.twobit_bytes(recs)[:40])
    with pytest.raises(_lib.KgmaError):
        api.fasta_id_to_cumulative_len_dict(str(bad))
