"""Reference writer and reader of UCSC .2bit files in plain NumPy, written from the format's description:

    header   signature 0x1A412743, version (0: 32-bit record offsets, 1: 64-bit), sequenceCount, reserved = 0
    index    sequenceCount x { nameSize (1 byte), name, offset of the record from the start of the file }
    record   dnaSize, nBlockCount, nBlockStarts[], nBlockSizes[], maskBlockCount, maskBlockStarts[], maskBlockSizes[],
             reserved = 0, packedDna: ceil(dnaSize / 4) bytes, four bases per byte, first base in the two most significant
             bits, T = 0, C = 1, A = 2, G = 3, last byte zero-padded

all integers 32-bit little endian, starts 0-based.  Residue i decodes to N inside an N block, else to the letter of its code,
then to lower case inside a mask block.  The reader shares no packing code with the writer: the writer packs four columns of
a reshaped code array with shifts, the reader indexes byte i // 4 and shifts by 6 - 2 (i % 4) per residue.
"""
from __future__ import annotations

import struct

import numpy as np

SIGNATURE = 0x1A412743
_ALLOWED = np.zeros(256, dtype=bool)
_ALLOWED[np.frombuffer(b"ACGTNacgtn", dtype=np.uint8)] = True
_CODE = np.zeros(256, dtype=np.uint8)            # T = 0 (and N, as faToTwoBit packs it), C = 1, A = 2, G = 3
for _ch, _c in ((b"Cc", 1), (b"Aa", 2), (b"Gg", 3)):
    _CODE[np.frombuffer(_ch, dtype=np.uint8)] = _c


def runs(flag: np.ndarray) -> list:
    """[(start, size)] of the maximal runs of True in a boolean array."""
    f = np.concatenate(([False], np.asarray(flag, dtype=bool), [False]))
    edges = np.flatnonzero(f[1:] != f[:-1])
    return [(int(a), int(b - a)) for a, b in zip(edges[0::2], edges[1::2])]


def pack_record(seq: bytes, n_blocks=None, mask_blocks=None) -> bytes:
    """One record's bytes from dnaSize on.  Blocks are (start, size) pairs; None: the runs of N/n, of lower case, in seq."""
    a = np.frombuffer(bytes(seq), dtype=np.uint8)
    if not _ALLOWED[a].all():
        bad = int(np.flatnonzero(~_ALLOWED[a])[0])
        raise ValueError(f"symbol {bad + 1} ({bytes(seq)[bad:bad + 1]!r}) is not one of ACGTNacgtn")
    if n_blocks is None:
        n_blocks = runs((a | 0x20) == ord("n"))
    if mask_blocks is None:
        mask_blocks = runs(a >= ord("a"))
    codes = np.zeros((a.size + 3) // 4 * 4, dtype=np.uint8)
    codes[:a.size] = _CODE[a]
    q = codes.reshape(-1, 4)
    packed = (q[:, 0] << 6) | (q[:, 1] << 4) | (q[:, 2] << 2) | q[:, 3]
    out = [struct.pack("<I", a.size)]
    for blocks in (n_blocks, mask_blocks):
        out.append(struct.pack("<I", len(blocks)))
        out.append(np.asarray([s for s, _ in blocks], dtype="<u4").tobytes())
        out.append(np.asarray([n for _, n in blocks], dtype="<u4").tobytes())
    out.append(struct.pack("<I", 0))
    out.append(packed.astype(np.uint8).tobytes())
    return b"".join(out)


def twobit_bytes(records, version: int = 0) -> bytes:
    """The file for records = [(name, seq)] or [(name, seq, n_blocks, mask_blocks)] (explicit (start, size) lists are written
    as given: unsorted, overlapping or empty blocks included; seq then only supplies the packed codes)."""
    if version not in (0, 1):
        raise ValueError("version 0 or 1")
    recs = [(r[0].encode() if isinstance(r[0], str) else bytes(r[0]), r[1], *(r[2:] if len(r) > 2 else (None, None))) for r in records]
    for name, *_ in recs:
        if len(name) > 255:
            raise ValueError("a record name holds at most 255 bytes")
    off_size = 8 if version == 1 else 4
    pos = 16 + sum(1 + len(name) + off_size for name, *_ in recs)
    bodies, index = [], []
    for name, seq, nb, mb in recs:
        body = pack_record(seq, nb, mb)
        index.append(bytes([len(name)]) + name + struct.pack("<Q" if version == 1 else "<I", pos))
        bodies.append(body)
        pos += len(body)
    return struct.pack("<IIII", SIGNATURE, version, len(recs), 0) + b"".join(index) + b"".join(bodies)


def write_twobit(path, records, version: int = 0) -> None:
    with open(path, "wb") as fh:
        fh.write(twobit_bytes(records, version))


def field_boundaries(records, version: int = 0) -> list:
    """Every offset of twobit_bytes(records, version) at which a field begins (the file's length is not one of them)."""
    off_size = 8 if version == 1 else 4
    cuts = [0, 4, 8, 12]
    pos = 16
    names = [(r[0].encode() if isinstance(r[0], str) else bytes(r[0])) for r in records]
    for name in names:
        cuts += [pos, pos + 1, pos + 1 + len(name)]
        pos += 1 + len(name) + off_size
    for r in records:
        body = pack_record(r[1], *(r[2:] if len(r) > 2 else (None, None)))
        nn = struct.unpack_from("<I", body, 4)[0]
        mm = struct.unpack_from("<I", body, 8 + 8 * nn)[0]
        rel = [0, 4, 8, 8 + 4 * nn, 8 + 8 * nn, 12 + 8 * nn, 12 + 8 * nn + 4 * mm, 12 + 8 * nn + 8 * mm, 16 + 8 * nn + 8 * mm]
        cuts += [pos + x for x in rel]
        pos += len(body)
    return sorted(set(c for c in cuts if c < pos))


# ---- the reader ---------------------------------------------------------------------------------------------------------------
_LETTERS = np.frombuffer(b"TCAG", dtype=np.uint8)


def read_twobit(data, mask: bool = True) -> list:
    """[(name, residues)] decoded from a .2bit file given as bytes or as a path."""
    if not isinstance(data, (bytes, bytearray)):
        with open(data, "rb") as fh:
            data = fh.read()
    sig, version, count, _ = struct.unpack_from("<IIII", data, 0)
    if sig != SIGNATURE or version > 1:
        raise ValueError("not a .2bit file of version 0 or 1 in this byte order")
    pos, entries = 16, []
    for _ in range(count):
        n = data[pos]
        name = bytes(data[pos + 1:pos + 1 + n])
        pos += 1 + n
        if version == 1:
            off = struct.unpack_from("<Q", data, pos)[0]; pos += 8
        else:
            off = struct.unpack_from("<I", data, pos)[0]; pos += 4
        entries.append((name, off))
    out = []
    for name, off in entries:
        size = struct.unpack_from("<I", data, off)[0]
        lists, p = [], off + 4
        for _ in range(2):
            cnt = struct.unpack_from("<I", data, p)[0]
            starts = np.frombuffer(data, dtype="<u4", count=cnt, offset=p + 4).astype(np.int64)
            sizes = np.frombuffer(data, dtype="<u4", count=cnt, offset=p + 4 + 4 * cnt).astype(np.int64)
            lists.append((starts, sizes))
            p += 4 + 8 * cnt
        p += 4                                                          # reserved
        raw = np.frombuffer(data, dtype=np.uint8, count=(size + 3) // 4, offset=p)
        i = np.arange(size, dtype=np.int64)
        text = _LETTERS[(raw[i >> 2] >> (6 - 2 * (i & 3)).astype(np.uint8)) & 3].copy()
        for s, n in zip(*lists[0]):
            text[s:s + n] = ord("N")
        if mask:
            for s, n in zip(*lists[1]):
                text[s:s + n] |= 0x20
        out.append((name.decode(), text.tobytes()))
    return out
