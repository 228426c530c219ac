"""The genome code of kgma_api.cpp where the other tests do not reach: every construction path across the 32 MiB boundary
of the staging buffers, and the state of a context after an ingest has failed."""
import numpy as np
import pytest

from kmergma_amd import _lib
from tests import twobit_ref as tb
from tests.helpers import hit_key, random_dna

pytestmark = pytest.mark.gpu

MIB = 1 << 20


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gene(data_dir, alp_ref):
    """One reference gene cut to the window size: a hit of the fixture reference wherever it is written."""
    import os
    from kmergma_amd import fasta
    return fasta.read_fasta(os.path.join(data_dir, "Alp_V_ref.fasta"))[3].sequence.upper()[:alp_ref["ws"]]


def _fasta_text(records, width=60) -> bytes:
    parts = []
    for i, seq in enumerate(records):
        parts.append(b">rec%d\n" % i)
        a = np.frombuffer(seq, dtype=np.uint8)
        full = len(a) // width
        lines = np.full((full, width + 1), ord("\n"), dtype=np.uint8)
        lines[:, :width] = a[:full * width].reshape(full, width)
        parts.append(lines.tobytes())
        if len(a) > full * width:
            parts.append(a[full * width:].tobytes() + b"\n")
    return b"".join(parts)


def test_every_construction_path_across_a_staging_boundary(ctx, alp_ref, gene, tmp_path):
    """Record lengths against the text layout (a record's slot is its length rounded up to 32, and 32 more): the first slot ends
    exactly on the 32 MiB boundary of a staging buffer, the padding of the second straddles the next one, then a short, an empty
    and a mid-sized record.  Lower-case and N runs sit around text offsets 32 MiB and 64 MiB.  The 60-column FASTA text of the
    same records crosses the boundaries at other places.  genome_from_host, genome_from_fasta(bytes) and genome_from_fasta(path)
    must hold the same records, and one scan must find the same hits in all three -- among them two genes poked in next to text
    offset 32 MiB: one ending 100 bases before the end of record 0, one beginning 100 bases into record 1."""
    rng = np.random.default_rng(3207)
    lens = [32 * MIB - 40, 32 * MIB - 20, 5, 0, 3 * MIB + 1]
    records = []
    for L in lens:
        a = bytearray(random_dna(rng, L))
        if L > 1000:
            a[:30] = b"N" * 30                                          # runs at both ends of the long records: the text
            a[30:70] = bytes(a[30:70]).lower()                          # around offsets 32 MiB and 64 MiB (+ 32)
            a[L - 40:] = b"N" * 40
            a[L - 90:L - 40] = bytes(a[L - 90:L - 40]).lower()
        records.append(bytes(a))
    text = _fasta_text(records)
    assert len(text) > 64 * MIB
    path = tmp_path / "boundary.fasta"
    path.write_bytes(text)
    ws = alp_ref["ws"]
    ctx.set_refs(6, [alp_ref["RV"]], [ws], [30.0], [alp_ref["N"]])
    results = []
    for source in ("host", "fasta bytes", "fasta path"):
        g = ctx.genome_from_host(records) if source == "host" else ctx.genome_from_fasta(text if source == "fasta bytes" else str(path))
        try:
            assert g.n_contigs == len(records), source
            for c, seq in enumerate(records):
                assert g.contig_len(c) == len(seq), (source, c)
                assert g.fetch(c, 1, len(seq)) == seq, (source, c)
            g.poke(0, lens[0] - 100 - len(gene) + 1, gene)
            g.poke(1, 101, gene)
            g.repack()
            ctx.scan(g, _lib.MODE_SINGLE, 50, 0, 0, None)
            results.append(([hit_key(h) for h in ctx.hits()], np.array(ctx.first_window(1))))
        finally:
            g.free()
    hits0, first0 = results[0]
    assert {h[0] for h in hits0} >= {0, 1}, "the two poked genes were not found"
    for hits, first in results[1:]:
        assert hits == hits0
        assert np.array_equal(first, first0)


def test_a_failed_ingest_leaves_the_context_whole(ctx, alp_ref, gene, tmp_path):
    """An ingest that fails half way gives back everything it took: the device bytes the context reports for the same scan of the
    same genome are what they were before, and that scan finds the same hits.  (The context keeps the FASTA ingest's device scratch
    between calls by design, so a FASTA ingest of the same size has succeeded before the count is taken.)"""
    rng = np.random.default_rng(77)
    ws = alp_ref["ws"]
    contigs = [random_dna(rng, 5000) + gene + random_dna(rng, 3000), random_dna(rng, 700)]
    ctx.set_refs(6, [alp_ref["RV"]], [ws], [30.0], [alp_ref["N"]])

    def scan():
        g = ctx.genome_from_host(contigs)
        try:
            ctx.scan(g, _lib.MODE_SINGLE, 50, 0, 0, None)
            return [hit_key(h) for h in ctx.hits()], ctx.stats()["device_bytes"]
        finally:
            g.free()

    ctx.genome_from_fasta(b">a\nACGTACGTACGT\n").free()
    hits_before, bytes_before = scan()
    assert len(hits_before) >= 1
    with pytest.raises(_lib.KgmaError):
        ctx.genome_from_fasta(b"ACGT\n>late\nACGT\n")
    assert scan() == (hits_before, bytes_before)
    short = tb.twobit_bytes([("x", b"ACGTA")])[:-1]                     # tests/test_twobit_host.py's "packed-short"
    p = tmp_path / "short.2bit"
    p.write_bytes(short)
    with pytest.raises(_lib.KgmaError):
        ctx.genome_from_2bit(str(p))
    assert scan() == (hits_before, bytes_before)
