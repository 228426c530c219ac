"""kgma_genome_revcomp (revcomp_kernel) and strand= through the API, on the device.

Every comparison is exact: the kernel against the host statement of the complement map (fasta.reverse_complement), the scans of a
device-made reverse genome against the scans of the same text ingested from the host (array equality of hits, dips, first
windows and distances), the API's minus strand against the CPU oracle on host-reversed records (compared as
__graft_entry__.smoke compares: coordinates equal, the header's rounded distance equal).
"""
import os
import re

import numpy as np
import pytest

from kmergma_amd import _lib, align, api, fasta, headers
from kmergma_amd.fasta import reverse_complement
from oracle import oracle as orc
from tests.conftest import DATA

pytestmark = pytest.mark.gpu

# lane (16 B), block pair (32 B), pass (4096 B) and tile (16384 B) boundaries of the kernel, and the record tails around them
LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8193, 16383, 16384, 16385,
           100003]
SYMBOLS = np.frombuffer(b"ACGTNacgtnMRWSYKVHDBmrwsykvhdb-", dtype=np.uint8)
LOCI = os.path.join(DATA, "Loci.fasta")
MINI = os.path.join(DATA, "Alp_V_locus.fasta")
REF = os.path.join(DATA, "Alp_V_ref.fasta")
OMN_THR = [37, 33, 38, 34, 28]
# the reverse-strand hits of Loci.fasta at k = 6, W = 389, thr = 30, buff = 50 (0-based record, forward range)
MINUS_30 = [(0, 35437, 35825), (2, 32774, 33162), (2, 27816, 28204)]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def rev_loci(loci):
    return [reverse_complement(r.sequence) for r in loci]


@pytest.fixture(scope="module")
def minus_oracle(alp_ref, rev_loci):
    """oracle.single_scan over the host-reversed records of Loci.fasta, per threshold (computed once)."""
    return {thr: orc.single_scan(rev_loci, alp_ref["RV"], 6, alp_ref["ws"], thr, 50)[0] for thr in (30.0, 33.5)}


def _records(g):
    return [g.fetch(c, 1, g.contig_len(c)) for c in range(g.n_contigs)]


def _check_revcomp(ctx, seqs):
    g = ctx.genome_from_host(seqs)
    r = g.revcomp()
    rr = r.revcomp()
    try:
        assert r.n_contigs == len(seqs) and [r.contig_len(c) for c in range(r.n_contigs)] == [len(s) for s in seqs]
        assert r.total_bases == g.total_bases
        got = _records(r)
        for c, (a, s) in enumerate(zip(got, seqs)):
            assert a == reverse_complement(s), f"record {c} of length {len(s)}"
        assert _records(rr) == list(seqs)
        assert _records(g) == list(seqs)              # the source is left as it was
    finally:
        rr.free(); r.free(); g.free()


def test_kernel_against_the_host_map(ctx):
    rng = np.random.default_rng(20261018)
    seqs = [SYMBOLS[rng.integers(0, SYMBOLS.size, size=L)].tobytes() for L in LENGTHS]
    odd = bytearray(SYMBOLS[rng.integers(0, SYMBOLS.size, size=300)].tobytes())
    odd[0:1] = b"X"; odd[17:18] = b"*"; odd[150:152] = b"x@"; odd[299:300] = b"*"
    seqs.insert(7, bytes(odd))
    seqs.append(bytes(range(256)) * 3)                # every byte value: only the 24 letters of the map change
    _check_revcomp(ctx, seqs)


@pytest.mark.parametrize("L", [1, 16, 17, 4097])
def test_single_record_at_buffer_offset_zero(ctx, L):
    rng = np.random.default_rng(L)
    _check_revcomp(ctx, [SYMBOLS[rng.integers(0, SYMBOLS.size, size=L)].tobytes()])


def test_no_records_and_empty_records(ctx):
    _check_revcomp(ctx, [])
    _check_revcomp(ctx, [b""])
    _check_revcomp(ctx, [b"", b"", b"ACGTN", b""])


def _fields(a):
    return a[[n for n in a.dtype.names if n != "reserved"]]


def _scan_all(ctx, g, mode, flags, m):
    ctx.scan(g, mode, 50, 0, flags, None)
    out = dict(hits=_fields(ctx.hits_array()).copy(), dips=_fields(ctx.dips_array()).copy(),
               first=[ctx.first_window(j + 1).copy() for j in range(m)])
    if flags & _lib.F_RETURN_DISTS:
        out["dists"] = [ctx.dists(j + 1).copy() for j in range(m)]
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        if isinstance(a[key], list):
            assert len(a[key]) == len(b[key])
            for x, y in zip(a[key], b[key]):
                assert np.array_equal(x, y), key
        else:
            assert np.array_equal(a[key], b[key]), key


def test_layout_and_padding_scans_equal_a_host_ingested_reverse(ctx, alp_ref, alp_clusters, loci, rev_loci):
    """The device-made reverse genome is an ordinary genome: every engine gives on it what it gives on the same text ingested
    from the host (whose padding kgma_genome_from_host zeroes)."""
    seqs = [bytearray(r.sequence) for r in loci]
    seqs[0][1000:1040] = b"N" * 40; seqs[1][5:6] = b"N"; seqs[2][70000:70700] = b"n" * 700; seqs[-1][-3:] = b"NNN"
    seqs = [bytes(s) for s in seqs]
    g = ctx.genome_from_host(seqs)
    dev = g.revcomp()
    host = ctx.genome_from_host([reverse_complement(s) for s in seqs])
    try:
        ctx.set_refs(6, [alp_ref["RV"]], [alp_ref["ws"]], [30.0], [alp_ref["N"]])
        a = _scan_all(ctx, host, _lib.MODE_SINGLE, _lib.F_RETURN_DISTS, 1)
        b = _scan_all(ctx, dev, _lib.MODE_SINGLE, _lib.F_RETURN_DISTS, 1)
        assert len(a["hits"]) > 0 and a["dists"][0].size > 400000
        _same(a, b)
        c = alp_clusters
        ctx.set_refs(6, c["KFVs"], c["ws"], OMN_THR, c["N"])
        a = _scan_all(ctx, host, _lib.MODE_OMN, _lib.F_RETURN_DISTS, len(c["ws"]))
        b = _scan_all(ctx, dev, _lib.MODE_OMN, _lib.F_RETURN_DISTS, len(c["ws"]))
        assert len(a["hits"]) > 0
        _same(a, b)
        rev0 = reverse_complement(seqs[0])
        queries = [rev0[85653:86042], rev0[:40], rev0[-25:], b"N" * 40, b"ACGTACGT", rev_loci[2][194592:194981]]
        ctx.exact_match(host, queries)
        ma = ctx.matches().copy()
        ctx.exact_match(dev, queries)
        mb = ctx.matches().copy()
        assert ma.size >= 4 and np.array_equal(ma, mb)
    finally:
        host.free(); dev.free(); g.free()


def test_headers_survive(ctx):
    g = ctx.genome_from_fasta(LOCI)
    r = g.revcomp()
    try:
        assert g.n_contigs == r.n_contigs == 4
        assert [r.header(c) for c in range(4)] == [g.header(c) for c in range(4)]
        assert all(r.header(c) for c in range(4))
    finally:
        r.free(); g.free()
    h = ctx.genome_from_host([b"ACGT"])               # no headers: none appear
    r = h.revcomp()
    try:
        with pytest.raises(_lib.KgmaError):
            r.header(0)
    finally:
        r.free(); h.free()


def test_bad_base_turns_up_mirrored(ctx, alp_ref):
    rng = np.random.default_rng(5)
    L, p = 3001, 1234                                  # 1-based forward position of the X
    clean = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=L)].tobytes()
    bad = bytearray(clean); bad[p - 1:p] = b"X"
    ctx.set_refs(6, [alp_ref["RV"]], [alp_ref["ws"]], [30.0], [alp_ref["N"]])
    for seq, raises in ((bytes(bad), True), (clean, False)):
        g = ctx.genome_from_host([clean, seq])
        r = g.revcomp()
        try:
            if raises:
                with pytest.raises(_lib.BadBaseError) as e:
                    ctx.scan(r, _lib.MODE_SINGLE, 50, 0, 0, None)
                assert f"record 1 position {L - p + 1}" in str(e.value)
                assert r.fetch(1, L - p + 1, 1) == b"X"
            else:
                ctx.scan(r, _lib.MODE_SINGLE, 50, 0, 0, None)
        finally:
            r.free(); g.free()


def _minus_expected(loci, rev_loci, ohits):
    """Records the API must return for the oracle's hits on the reversed records."""
    out = []
    for h in ohits:
        c = h["contig"]
        lo, hi = api.strand_range(len(rev_loci[c]), h["lo"], h["hi"])
        hdr = headers.single_header(loci[c].identifier, h["dist"], lo, hi, h["genome_pos"], strand="-")
        out.append((hdr, rev_loci[c][h["lo"] - 1:h["hi"]], lo + h["genome_pos"], (c, lo, hi)))
    return out


@pytest.mark.parametrize("thr, n_hits", [(30.0, 3), (33.5, 50)])
def test_minus_strand_equals_the_oracle_on_reversed_records(ctx, alp_ref, loci, rev_loci, minus_oracle, thr, n_hits):
    res, loc = [], []
    api.ac_gma_testing(genome_path=LOCI, refVec=alp_ref["RV"], consensus_refseq=alp_ref["cons"], windowsize=alp_ref["ws"],
                       thr=thr, do_align=False, resultVec=res, get_hit_loci=True, hit_loci_vec=loc, n_refs=alp_ref["N"],
                       ctx=ctx, strand="-")
    want = _minus_expected(loci, rev_loci, minus_oracle[thr])
    assert len(want) == n_hits
    assert [r.description for r in res] == [w[0] for w in want]
    assert [r.sequence for r in res] == [w[1] for w in want]
    assert loc == [w[2] for w in want]
    assert all(r.description.endswith(" | Strand = -") for r in res)
    for r, w in zip(res, want):
        c, lo, hi = w[3]
        assert r.sequence == reverse_complement(loci[c].sequence[lo - 1:hi])
    if thr == 30.0:
        assert [w[3] for w in want] == MINUS_30


def _ranges(recs):
    out = []
    for r in recs:
        m = re.search(r"MatchPos = (\d+):(\d+)", r.description)
        out.append((r.description.split(" | ")[0], int(m.group(1)), int(m.group(2))))
    return out


def _write_rc(path_in, path_out):
    recs = fasta.read_fasta(path_in)
    with open(path_out, "wb") as fh:
        for r in recs:
            s = reverse_complement(r.sequence)
            fh.write(b">" + r.description.encode() + b"\n")
            for i in range(0, len(s), 70):
                fh.write(s[i:i + 70] + b"\n")
    return {r.identifier: len(r.sequence) for r in recs}


def _assert_mirror(fwd, minus, lens):
    """`fwd`: the plus-strand records of a file; `minus`: the minus-strand records of its reverse complement."""
    assert len(fwd) == len(minus) and len(fwd) > 0
    assert [r.sequence for r in minus] == [r.sequence for r in fwd]
    for (ida, lo, hi), (idb, lo2, hi2) in zip(_ranges(fwd), _ranges(minus)):
        assert ida == idb and (lo2, hi2) == api.strand_range(lens[ida], lo, hi)
    for a, b in zip(fwd, minus):
        assert b.description.endswith(" | Strand = -") and not a.description.endswith("Strand = -")
        strip = lambda d: re.sub(r"MatchPos = \d+:\d+", "", d.replace(" | Strand = -", ""))
        assert strip(a.description) == strip(b.description)       # identifier, distance, KFV, GenomePos, Len


def test_symmetry_findgenes(ctx, tmp_path):
    rc_file = str(tmp_path / "loci_rc.fasta")
    lens = _write_rc(LOCI, rc_file)
    fwd = api.findGenes(genome_path=LOCI, ref_path=REF, KmerDistThr=30, verbose=False, ctx=ctx)[0]
    minus = api.findGenes(genome_path=rc_file, ref_path=REF, KmerDistThr=30, verbose=False, ctx=ctx, strand="-")[0]
    _assert_mirror(fwd, minus, lens)


def test_symmetry_cluster_mode(ctx, golden, tmp_path):
    g = golden["scan"]["findGenes_cluster_mode"]
    rc_file = str(tmp_path / "mini_rc.fasta")
    lens = _write_rc(MINI, rc_file)
    kw = dict(ref_path=REF, KmerDistThrs=g["KmerDistThrs"], buffer=g["buffer"], verbose=False, ctx=ctx)
    fwd = api.findGenes_cluster_mode(genome_path=MINI, **kw)[0]
    assert [r.description for r in fwd] == g["headers"]
    minus = api.findGenes_cluster_mode(genome_path=rc_file, strand="-", **kw)[0]
    _assert_mirror(fwd, minus, lens)


@pytest.mark.parametrize("thr", [30, 40])
def test_symmetry_strobemers(ctx, tmp_path, thr):
    rc_file = str(tmp_path / "mini_rc.fasta")
    lens = _write_rc(MINI, rc_file)
    fwd = api.Strobemer_findGenes(genome_path=MINI, ref_path=REF, KmerDistThr=thr, verbose=False, ctx=ctx)[0]
    minus = api.Strobemer_findGenes(genome_path=rc_file, ref_path=REF, KmerDistThr=thr, verbose=False, ctx=ctx, strand="-")[0]
    _assert_mirror(fwd, minus, lens)


def test_both_is_plus_then_minus(ctx, alp_ref, loci):
    kw = dict(genome_path=LOCI, refVec=alp_ref["RV"], consensus_refseq=alp_ref["cons"], windowsize=alp_ref["ws"], thr=30.0,
              do_align=True, get_hit_loci=True, do_return_dists=True, do_return_align=True, n_refs=alp_ref["N"], ctx=ctx)

    def call(**extra):
        out = dict(resultVec=[], hit_loci_vec=[], dist_vec=[], result_align_vec=[])
        api.ac_gma_testing(**kw, **out, **extra)
        return out

    none, plus, minus, both = call(), call(strand="+"), call(strand="-"), call(strand="both")
    for key in none:
        assert none[key] == plus[key], key
        assert both[key] == plus[key] + minus[key], key
    assert len(plus["resultVec"]) == 7 and len(minus["resultVec"]) == 3
    assert len(both["dist_vec"]) == 2 * len(plus["dist_vec"]) == 2 * 484127
    # loci and alignment ranges of the minus part are forward coordinates: they name the listed genes
    assert len(minus["hit_loci_vec"]) == 3 and len(minus["result_align_vec"]) == 3
    for rec, locus, al, (c, lo, hi) in zip(minus["resultVec"], minus["hit_loci_vec"], minus["result_align_vec"], MINUS_30):
        m = re.search(r"MatchPos = (\d+):(\d+) \| GenomePos = (\d+)", rec.description)
        alo, ahi, gpos = int(m.group(1)), int(m.group(2)), int(m.group(3))
        assert locus == alo + gpos
        # the aligned range is the listed (unaligned) range of the gene, in forward coordinates; first / last are relative to the
        # gene-oriented segment, so the hit's range follows from them in reversed coordinates, as the reference maps them
        # (max(lo + first - 1, 1) : min(lo + last - 1, L), Alignment.jl:46), and then through the coordinate map
        assert al[0] == c and (al[2], al[3]) == (lo, hi)
        L = len(loci[c].sequence)
        rlo, _ = api.strand_range(L, lo, hi)
        assert (alo, ahi) == api.strand_range(L, max(rlo + al[4] - 1, 1), min(rlo + al[5] - 1, L))


def test_both_in_cluster_mode_per_kfv(ctx, alp_clusters):
    c = alp_clusters
    m = len(c["ws"])

    def call(strand):
        out = dict(resultVec=[], hit_loci_vec=[], dist_vec_vec=[[] for _ in range(m)])
        api.Omn_KmerGMA(genome_path=MINI, refVecs=c["KFVs"], windowsizes=c["ws"], consensus_seqs=c["cons"], thr_vec=OMN_THR,
                        n_refs=c["N"], get_hit_loci=True, do_return_dists=True, ctx=ctx, strand=strand, **out)
        return out

    plus, minus, both = call("+"), call("-"), call("both")
    assert both["resultVec"] == plus["resultVec"] + minus["resultVec"]
    assert both["hit_loci_vec"] == plus["hit_loci_vec"] + minus["hit_loci_vec"]
    for j in range(m):
        assert both["dist_vec_vec"][j] == plus["dist_vec_vec"][j] + minus["dist_vec_vec"][j]
        assert len(minus["dist_vec_vec"][j]) == len(plus["dist_vec_vec"][j]) > 0


def test_caller_supplied_aligner_gets_gene_oriented_segments(ctx, alp_ref, loci, rev_loci):
    seen = []

    def aligner(cons, segment, gap_open, gap_extend):
        seen.append(bytes(segment))
        return align.align_range(cons, segment, gap_open, gap_extend)

    kw = dict(refVec=alp_ref["RV"], consensus_refseq=alp_ref["cons"], windowsize=alp_ref["ws"], thr=30.0, do_align=True,
              get_hit_loci=True, do_return_align=True, n_refs=alp_ref["N"], ctx=ctx, strand="-")
    dev = dict(resultVec=[], hit_loci_vec=[], result_align_vec=[])
    api.ac_gma_testing(genome_path=LOCI, **kw, **dev)
    for source in (LOCI, list(loci)):                  # a FASTA path, and records given from host memory
        seen.clear()
        host = dict(resultVec=[], hit_loci_vec=[], result_align_vec=[])
        api.ac_gma_testing(genome_path=source, aligner=aligner, **kw, **host)
        assert host == dev
        assert len(seen) == 3
        for seg, (c, lo, hi) in zip(seen, MINUS_30):     # the listed ranges are the candidate ranges the engine aligns
            rlo, rhi = api.strand_range(len(rev_loci[c]), lo, hi)
            assert seg == rev_loci[c][rlo - 1:rhi] == reverse_complement(loci[c].sequence[lo - 1:hi])
