""".2bit ingest on the device (kgma_genome_from_2bit_file / twobit_unpack_kernel) against the NumPy reader of tests/twobit_ref.py.
Every comparison is exact: the residue text of every record, names, lengths; then the search entry points on a .2bit path and
on one resident genome against the FASTA path.

The kernel's sizes (kgma_device.h / kgma_twobit.hip): a lane writes chunks of 16 residues, a workgroup passes of 256 x 16 = 4096,
a tile is 4 passes = 16384 bytes of a record's slot, and a tile keeps up to 1024 blocks of a list in LDS."""
import os
import struct

import numpy as np
import pytest

from kmergma_amd import _lib, api
from tests import twobit_ref as tb
from tests.conftest import DATA
from tests.motif_oracle import LOCI_RSSD_D1
from tests.test_twobit_host import rand_seq

pytestmark = pytest.mark.gpu
CHUNK, PASS, TILE, LDS_BLOCKS = 16, 4096, 16384, 1024
LOCI = os.path.join(DATA, "Loci.fasta")
REF = os.path.join(DATA, "Alp_V_ref.fasta")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def device_text(ctx, path, mask=True):
    """[(name, residues)] of a .2bit file as the device holds it, after the checks every genome gets."""
    g = ctx.genome_from_2bit(str(path), mask=mask)
    try:
        n = g.n_contigs
        lens = [g.contig_len(c) for c in range(n)]
        assert g.total_bases == sum(lens)
        out = [(g.header(c), g.fetch(c, 1, lens[c])) for c in range(n)]
        # one gather for all records gives the same bytes
        assert g.fetch_batch([(c, 1, lens[c]) for c in range(n)]) == [s for _, s in out]
        if g.total_bases:
            ctx.motif_match(g, [b"ACGTACGTAC"], [0])                   # (raises BadBaseError if first_bad reports anything)
        return out
    finally:
        g.free()


def check(ctx, tmp_path, records, version=0, name="t.2bit"):
    """Write `records`, read them back through the device, compare with the reference reader (and, for records without
    explicit block lists, with the sequences themselves)."""
    p = tmp_path / name
    data = tb.twobit_bytes(records, version)
    p.write_bytes(data)
    want = tb.read_twobit(data)
    got = device_text(ctx, p)
    assert [n for n, _ in got] == [n for n, _ in want]
    assert [len(s) for _, s in got] == [len(s) for _, s in want]
    for (n, a), (_, b) in zip(got, want):
        if a != b:
            x, y = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
            i = int(np.flatnonzero(x != y)[0])
            raise AssertionError(f"record {n!r}: residue {i} of {len(a)} is {a[i:i + 1]!r}, want {b[i:i + 1]!r}; {int((x != y).sum())} differ")
    for r, (_, s) in zip(records, want):
        if len(r) == 2:
            assert s == r[1]
    assert device_text(ctx, p, mask=False) == [(n, s.upper()) for n, s in want]
    return want


def packed_phases(data: bytes) -> set:
    """File offset mod 4 of every non-empty record's packed bases (version 0)."""
    count = struct.unpack_from("<I", data, 8)[0]
    pos, out = 16, set()
    for _ in range(count):
        pos += 1 + data[pos]
        off = struct.unpack_from("<I", data, pos)[0]
        pos += 4
        size = struct.unpack_from("<I", data, off)[0]
        nn = struct.unpack_from("<I", data, off + 4)[0]
        mm = struct.unpack_from("<I", data, off + 8 + 8 * nn)[0]
        if size:
            out.add((off + 16 + 8 * nn + 8 * mm) % 4)
    return out


LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, PASS - 1, PASS, PASS + 1, TILE - 1, TILE, TILE + 1,
           4 * TILE - 1, 4 * TILE, 4 * TILE + 1, 100003]


@pytest.mark.parametrize("version", [0, 1])
def test_record_lengths_in_one_file(ctx, tmp_path, version):
    rng = np.random.default_rng(11)
    recs = [("c" * (1 + i % 7) + str(n), rand_seq(rng, n, 2, 4)) for i, n in enumerate(LENGTHS)]
    if version == 0:
        assert packed_phases(tb.twobit_bytes(recs)) == {0, 1, 2, 3}
    check(ctx, tmp_path, recs, version)


def test_versions_give_equal_genomes(ctx, tmp_path):
    rng = np.random.default_rng(12)
    recs = [("a", rand_seq(rng, 5000, 3, 9)), ("bb", b""), ("ccc", rand_seq(rng, 33, 1, 1))]
    assert check(ctx, tmp_path, recs, 0, "v0.2bit") == check(ctx, tmp_path, recs, 1, "v1.2bit")


def test_no_records_and_empty_records(ctx, tmp_path):
    assert check(ctx, tmp_path, []) == []
    assert check(ctx, tmp_path, [], 1) == []
    assert check(ctx, tmp_path, [("only", b"")]) == [("only", b"")]
    rng = np.random.default_rng(13)
    recs = [("e0", b""), ("a", rand_seq(rng, 70, 1, 1)), ("e1", b""), ("e2", b""), ("b", rand_seq(rng, TILE + 3, 1, 1)), ("e3", b"")]
    check(ctx, tmp_path, recs)


def edge_records(kind: str):
    """Blocks of one kind ("n": N blocks, "m": mask blocks) with a start and an end at every offset 0 ... 16 around a chunk
    boundary (all pairs), a pass boundary and a tile boundary (every start with a far end, every end with a far start, and
    one-base blocks)."""
    rng = np.random.default_rng(14)
    recs = []

    def add(L, s, e):
        blocks = [(s, e - s)]
        recs.append((f"{kind}{L}_{s}_{e}", rand_seq(rng, L), blocks if kind == "n" else [], [] if kind == "n" else blocks))

    B = 2 * CHUNK
    for s in range(B - 8, B + 9):
        for e in range(s + 1, B + 9 + 1):
            add(4 * CHUNK + 3, s, e)
    for B in (PASS, TILE):
        L = TILE + 4 * CHUNK + 1
        for d in range(-8, 9):
            add(L, B + d, L - 5)          # a start at every offset, far end
            add(L, 3, B + d)              # an end at every offset, far start
            add(L, B + d, B + d + 1)      # one base
    return recs


@pytest.mark.parametrize("kind", ["n", "m"])
def test_block_edges(ctx, tmp_path, kind):
    check(ctx, tmp_path, edge_records(kind))


def test_block_shapes(ctx, tmp_path):
    rng = np.random.default_rng(15)
    L = TILE + 77
    s = lambda n=L: rand_seq(rng, n)
    recs = [
        ("none", s(), [], []),
        ("one_n", s(), [(100, 1)], []), ("one_m", s(), [], [(100, 1)]),
        ("whole_n", s(), [(0, L)], []), ("whole_m", s(), [], [(0, L)]), ("whole_both", s(), [(0, L)], [(0, L)]),
        ("first_n", s(), [(0, 1)], []), ("first_m", s(), [], [(0, 3)]),
        ("last_n", s(), [(L - 1, 1)], []), ("last_m", s(), [], [(L - 20, 20)]),
        ("n_in_m", s(), [(1000, 10)], [(990, 40)]), ("m_in_n", s(), [(990, 40)], [(1000, 10)]),
        ("overlap_nm", s(), [(1000, 30)], [(1015, 30)]), ("overlap_mn", s(), [(1015, 30)], [(1000, 30)]),
        ("same", s(), [(TILE - 3, 9)], [(TILE - 3, 9)]),
        # eight blocks of a list in one chunk, and chunks between blocks
        ("dense", s(), [(i, 1) for i in range(0, 64, 2)], [(i, 1) for i in range(1, 64, 2)]),
        # unsorted / overlapping lists reach the kernel normalised
        ("messy", s(), [(500, 10), (20, 5), (25, 5), (505, 20), (40, 0)], [(300, 100), (0, 50), (350, 10)]),
    ]
    # the two padding bits of the last packed byte (3, 2, 1 padding positions) under a mask block / an N block that ends at dnaSize
    for pad, n in ((3, 5), (2, 6), (1, 7), (3, TILE + 1), (2, TILE + 2), (1, PASS + 3)):
        recs.append((f"pad{pad}_m{n}", b"G" * n, [], [(n - 2 if n > 2 else 0, 2 if n > 2 else n)]))
        recs.append((f"pad{pad}_n{n}", b"G" * n, [(n - 1, 1)], []))
        recs.append((f"pad{pad}_{n}", b"G" * n, [], []))
    check(ctx, tmp_path, recs)


@pytest.mark.parametrize("kind", ["n", "m"])
def test_every_other_base(ctx, tmp_path, kind):
    """40 000 bases with every other base in a block: 20 000 blocks, 8192 of them in a tile (the lists stay in global memory
    and every chunk meets eight blocks)."""
    rng = np.random.default_rng(16)
    blocks = [(i, 1) for i in range(1, 40000, 2)]
    rec = ("alt", rand_seq(rng, 40000), blocks if kind == "n" else [], [] if kind == "n" else blocks)
    other = ("alt0", rand_seq(rng, 40000), [(i, 1) for i in range(0, 40000, 2)] if kind == "m" else [(7, 3)],
             [(i, 1) for i in range(0, 40000, 2)] if kind == "n" else [(7, 3)])
    check(ctx, tmp_path, [rec, other])


def test_lds_threshold(ctx, tmp_path):
    """Tiles with LDS_BLOCKS - 1, LDS_BLOCKS and LDS_BLOCKS + 1 blocks of a list: the last takes the lists from global memory."""
    rng = np.random.default_rng(17)
    recs = []
    for n in (LDS_BLOCKS - 1, LDS_BLOCKS, LDS_BLOCKS + 1):
        blocks = [(3 * i + 1, 2) for i in range(n)]                    # all inside the first tile
        blocks2 = [(TILE + 5 * i, 3) for i in range(n)]                # all inside the second
        recs.append((f"n{n}", rand_seq(rng, 2 * TILE + 9), blocks, blocks2))
        recs.append((f"m{n}", rand_seq(rng, 2 * TILE + 9), blocks2, blocks))
    check(ctx, tmp_path, recs)


def test_random_genome(ctx, tmp_path):
    rng = np.random.default_rng(18)
    recs = []
    for i, n in enumerate((120000, 50001, 29999)):                     # 200 kb
        nb = [(int(a), int(b)) for a, b in zip(rng.integers(0, n - 500, size=12), rng.integers(0, 500, size=12))]
        mb = [(int(a), int(b)) for a, b in zip(rng.integers(0, n - 900, size=n // 600), rng.integers(0, 900, size=n // 600))]
        recs.append((f"chr{i + 1}", rand_seq(rng, n), nb, mb))
    check(ctx, tmp_path, recs)


# ---- downstream: the search entry points on a .2bit path and on a resident genome ---------------------------------------------
@pytest.fixture(scope="module")
def loci_2bit(tmp_path_factory, loci):
    p = tmp_path_factory.mktemp("twobit") / "Loci.2bit"
    assert all(set(r.sequence) <= set(b"ACGT") for r in loci)
    tb.write_twobit(p, [(r.identifier, r.sequence) for r in loci])
    return str(p)


def pairs(records):
    return [(r.description, r.sequence) for r in records]


@pytest.fixture(scope="module")
def path_results(ctx, loci_2bit):
    """The FASTA path's results, computed once: findGenes with and without alignment, and the cluster mode."""
    fg = {al: api.findGenes(genome_path=LOCI, ref_path=REF, k=6, KmerDistThr=30.0, do_align=al, strand="both", verbose=False, ctx=ctx)
          for al in (True, False)}
    cl = api.findGenes_cluster_mode(genome_path=LOCI, ref_path=REF, k=6, KmerDistThrs=[30.0] * 8, strand="both", verbose=False, ctx=ctx)
    assert len(fg[True][0]) >= 7 and len(cl[0]) >= 7
    return fg, cl


def test_find_genes_on_a_2bit_path(ctx, loci_2bit, path_results):
    fg, cl = path_results
    for al in (True, False):
        got = api.findGenes(genome_path=loci_2bit, ref_path=REF, k=6, KmerDistThr=30.0, do_align=al, strand="both", verbose=False, ctx=ctx)
        assert pairs(got[0]) == pairs(fg[al][0])
    got = api.findGenes_cluster_mode(genome_path=loci_2bit, ref_path=REF, k=6, KmerDistThrs=[30.0] * 8, strand="both", verbose=False, ctx=ctx)
    assert pairs(got[0]) == pairs(cl[0])


def test_motif_and_exact_match_on_a_2bit_path(ctx, loci, loci_2bit, path_results):
    ids = [r.identifier for r in loci]
    assert api.motifMatch(api.HumanRSSD, loci_2bit, max_mismatch=1, strand="both", ctx=ctx) == \
        [(c, ids[c], s, s + 38, "+", k) for c, s, k in LOCI_RSSD_D1]
    assert api.findRSS(loci_2bit, ctx=ctx) == api.findRSS(LOCI, ctx=ctx)
    gene = path_results[0][False][0][0].sequence                       # the first gene the scan finds, as it lies in the fixture
    want = api.exactMatch(gene, LOCI, ctx=ctx)
    assert isinstance(want, dict) and sum(len(v) for v in want.values()) >= 1
    assert api.exactMatch(gene, loci_2bit, ctx=ctx) == want
    assert api.fasta_id_to_cumulative_len_dict(loci_2bit) == {r.identifier: v for r, v in
                                                              zip(loci, api.fasta_id_to_cumulative_len_dict(LOCI).values())}


@pytest.mark.parametrize("source", ["2bit", "fasta"])
def test_scans_on_one_resident_genome(ctx, loci, loci_2bit, path_results, source):
    fg, cl = path_results
    g = ctx.genome_from_2bit(loci_2bit) if source == "2bit" else ctx.genome_from_fasta(LOCI)
    try:
        for _ in range(2):
            got = api.findGenes(genome_path=g, ref_path=REF, k=6, KmerDistThr=30.0, do_align=False, strand="both", verbose=False, ctx=ctx)
            assert pairs(got[0]) == pairs(fg[False][0])
            got = api.findGenes_cluster_mode(genome_path=g, ref_path=REF, k=6, KmerDistThrs=[30.0] * 8, strand="both", verbose=False, ctx=ctx)
            assert pairs(got[0]) == pairs(cl[0])
        got = api.findGenes(genome_path=g, ref_path=REF, k=6, KmerDistThr=30.0, do_align=True, strand="+", verbose=False, ctx=ctx)
        assert pairs(got[0]) == [p for p in pairs(fg[True][0]) if "Strand = -" not in p[0]]
        # still open, still the same text
        assert g.n_contigs == len(loci)
        for c, r in enumerate(loci):
            assert g.fetch(c, 1, len(r.sequence)) == r.sequence
        view = api._GenomeView(ctx, g)
        view.free()                                                    # (not owned: stays open)
        assert g.fetch(0, 1, 10) == loci[0].sequence[:10]
    finally:
        g.free()


def test_a_malformed_file_raises_and_the_context_lives_on(ctx, tmp_path):
    good = tb.twobit_bytes([("a", b"ACGTNNacgtA"), ("b", b"acgt" * 9)])
    for label, data, status in (("cut", good[:-3], _lib.KGMA_E_ARG), ("swapped", good[3::-1] + good[4:], _lib.KGMA_E_UNSUPPORTED),
                                ("version", good[:4] + struct.pack("<I", 7) + good[8:], _lib.KGMA_E_UNSUPPORTED),
                                ("fasta", b">a\nACGT\n", _lib.KGMA_E_ARG)):
        p = tmp_path / f"{label}.2bit"
        p.write_bytes(data)
        with pytest.raises(_lib.KgmaError) as e:
            ctx.genome_from_2bit(str(p))
        assert e.value.status == status and label + ".2bit" in e.value.message
    with pytest.raises(_lib.KgmaError) as e:
        ctx.genome_from_2bit(str(tmp_path / "absent.2bit"))
    assert e.value.status == _lib.KGMA_E_ARG
    # a byte-swapped file is not mistaken for FASTA by the sniffing helper either
    with pytest.raises(_lib.KgmaError) as e:
        ctx.genome_from_path(str(tmp_path / "swapped.2bit"))
    assert e.value.status == _lib.KGMA_E_UNSUPPORTED
    assert check(ctx, tmp_path, [("a", b"ACGTNNacgtA"), ("b", b"acgt" * 9)]) == [("a", b"ACGTNNacgtA"), ("b", b"acgt" * 9)]
    assert ctx.twobit_unpack_ms() > 0
