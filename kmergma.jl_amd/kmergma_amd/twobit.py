"""Host-side view of a UCSC .2bit file's index: record names and lengths (fasta_id_to_cumulative_len_dict).  The sequence data
never pass through Python: kgma_genome_from_2bit_file ships the packed bytes to the device (include/kgma.h)."""
from __future__ import annotations

import struct

from . import _lib


def twobit_names_and_lengths(path) -> list:
    """[(name, dnaSize)] of the records of a .2bit file, in file order.  The library's parser validates the whole file first
    (kgma_twobit_inspect: KgmaError with its status and message for a file it refuses), so every offset read here is inside
    the file."""
    info = _lib.twobit_inspect(path)
    off_fmt = "<Q" if info["version"] == 1 else "<I"
    out = []
    with open(path, "rb") as fh:
        fh.seek(16)
        index = []
        for _ in range(info["n_records"]):
            n = fh.read(1)[0]
            name = fh.read(n).decode("utf-8", "replace")
            index.append((name, struct.unpack(off_fmt, fh.read(struct.calcsize(off_fmt)))[0]))
        for name, off in index:
            fh.seek(off)
            out.append((name, struct.unpack("<I", fh.read(4))[0]))
    return out
