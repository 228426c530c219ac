"""The sparse step pack (kgma_api.cpp: kgma_genome::inter_state, ensure_inter, pack_candidate_blocks, pack_record_blocks;
kgma_filter.hip: pack_sums_kernel<K, false>; switch KGMA_SPARSE_PACK): a step whose pack carries the block sums writes the 2-bit
copy of the genome only in the pack blocks (1024 plane words, 32 768 residues) that its candidate streams and chained records read,
and leaves the genome PARTIAL; every other reader of the copy completes it first.

What is checked: a sparse step gives what the step with the full pack gives, in every field the fused-sums tests compare (their
helpers are used), and what the oracle gives; with KGMA_SPARSE_POISON=1 -- the copy filled with a byte pattern before the step
packs its blocks -- it still does, so nothing reads a block that was not packed; every family of call that reads the copy after
a poisoned sparse step gives what it gives after a full step; so do text changes, the filter's fallbacks, a genome with a
bit-plane copy, and the sums-only form of the pack loop through the layout of test_gpu_pack_loop.py.

The genome is laid out against the pack blocks; test_layout asserts the places the cases rely on."""
import functools

import numpy as np
import pytest

from kmergma_amd import _lib
from oracle import oracle as orc
from tests import filter_cases as fc
from tests import strobe_cases as sc
from tests import filter_ref, sums_ref
from tests import test_gpu_fused_sums as fu
from tests import test_gpu_pack_loop as pl
from tests.helpers import hit_key, mutate, random_dna
from tests.test_gpu_pack_pairs import CONTIG_PAD_WORDS, LEAD_PAD_WORDS, UNIT_WORDS, word_offsets

pytestmark = pytest.mark.gpu

BUFF = fu.BUFF
PRESUMMED = _lib.FILTER_FORM_PRESUMMED
FULL, PARTIAL = _lib.INTER_FULL, _lib.INTER_PARTIAL
BLOCK_WORDS = 1024                      # PACK_BLOCK_WORDS (kgma_kernels.hip)
TAIL_PAD_WORDS = pl.TAIL_PAD_WORDS
NK = 100                                # k-mers of a window: W = NK + k - 1
N = 7
KS = (5, 6)
CHAIN = _lib.F_CHAIN_REPLAY


@pytest.fixture(autouse=True)
def _small_genomes(monkeypatch):
    monkeypatch.setenv("KGMA_FILTER_MIN_WINDOWS", "1")
    monkeypatch.setenv("KGMA_FILTER", "1")
    monkeypatch.setenv("KGMA_FUSE_SUMS", "1")
    for name in ("KGMA_OVERLAP", "KGMA_PACK_WGS", "KGMA_SPARSE_PACK", "KGMA_SPARSE_POISON", "KGMA_CHAIN", "KGMA_KERNEL", "KGMA_FILTER_CAP"):
        monkeypatch.delenv(name, raising=False)


# ---- the layout ------------------------------------------------------------------------------------------------------------------
# (record: words, residues missing from its last word)
RECORDS = [
    (BLOCK_WORDS - LEAD_PAD_WORDS + 1, 27),   # 0: ends 5 residues into block 1
    (1, 12),                                  # 1: one word, no window
    (2 * BLOCK_WORDS - 1090, 4),              # 2: ends 4 residues before the end of block 1
    (BLOCK_WORDS, 0),                         # 3: exactly one block long (it lies across blocks 2 | 3)
    (2 * BLOCK_WORDS, 0),                     # 4: exactly two blocks long; the same gene twice: chained
    (4 * BLOCK_WORDS, 0),                     # 5: blocks 5 ... 9; a gene across the edge 6 | 7 is the only reader of block 7; none of block 8
    (1000, 9),                                # 6: the genome's last record, its end in the last, partial block
]


def lengths():
    return [32 * w - miss for w, miss in RECORDS]


def total_words(lens):
    return word_offsets(lens)[1] + TAIL_PAD_WORDS


def block_of_residue(off, c, pos):
    return (off[c] + pos // 32) // BLOCK_WORDS


def plants_of(lens, W):
    """(record, 0-based window, what it is there for)."""
    off, _ = word_offsets(lens)
    edge4 = 32 * (4 * BLOCK_WORDS - off[4])                             # the residue of record 4 at which block 4 starts
    return [
        (0, lens[0] - W, "record 0's last window: its stream runs across the block edge 0 | 1 and over record 1's lead padding"),
        (2, 0, "a record's first window"),
        (2, lens[2] - W, "a record's last window, a few residues before a block's end"),
        (3, 0, "first window of the record of one block"),
        (3, lens[3] - W, "... and its last"),
        (4, edge4 - W // 2, "across a block edge inside a record"),
        (4, 50_000, "the same gene a second time"),
        (6, 0, "first window of the last record"),
        (6, lens[6] - W, "the genome's last window, in its last, partial block"),
        # (a dip at a record's first window is never tested and one on its last residues never closes: these give hits)
        (0, 20_000, "inside block 0"), (2, 5_000, "inside block 1"), (3, 15_000, "inside block 2"), (6, 10_000, "inside block 9"),
        (5, 1_000, "inside block 5"),
        (5, 32 * (7 * BLOCK_WORDS - off[5]) - W // 2, "across the block edge 6 | 7: no other stream starts in or reaches block 7"),
    ]


@pytest.mark.parametrize("k", KS)
def test_layout(k):
    """(no GPU work)"""
    lens = lengths()
    W = NK + k - 1
    off, end = word_offsets(lens)
    words = [(L + 31) // 32 for L in lens]
    assert sum(lens) < 1_000_000
    assert off[0] == LEAD_PAD_WORDS and off[2] == 1090 and BLOCK_WORDS % UNIT_WORDS == 0
    assert words[1] == 1 and lens[1] < W                                            # one word
    assert lens[3] == 32 * BLOCK_WORDS and lens[4] == 64 * BLOCK_WORDS              # exactly one block, exactly two
    last0 = off[0] * 32 + lens[0]                                                   # (global residue index behind the record)
    assert last0 - 32 * BLOCK_WORDS == 5                                            # ends 5 residues into block 1
    last2 = off[2] * 32 + lens[2]
    assert 2 * 32 * BLOCK_WORDS - last2 == 4                                        # ends 4 residues before block 1's end
    assert off[1] // BLOCK_WORDS == 1 and off[1] - (off[0] + words[0]) == CONTIG_PAD_WORDS
    tw = total_words(lens)
    n_blocks = -(-tw // BLOCK_WORDS)
    assert tw % BLOCK_WORDS != 0                                                    # the last block is partial
    assert (off[6] + words[6] - 1) // BLOCK_WORDS == n_blocks - 1                   # ... and holds the last record's end
    P = plants_of(lens, W)
    assert block_of_residue(off, 6, P[8][1]) == n_blocks - 1
    # block 8 lies inside record 5, thousands of words from its ends and from any plant: no step reads it unless it chains record 5;
    # block 7 is read by the one stream that starts in block 6
    assert off[5] // BLOCK_WORDS == 5 and (off[5] + words[5]) // BLOCK_WORDS == 9
    assert all(block_of_residue(off, c, pos + W + 256) != 8 and block_of_residue(off, c, pos - 256) != 8 for c, pos, _ in P)
    starts_in_7 = [(c, pos) for c, pos, _ in P if block_of_residue(off, c, max(pos - 128, 0)) == 7]
    assert not starts_in_7 and (block_of_residue(off, 5, P[-1][1]), block_of_residue(off, 5, P[-1][1] + W)) == (6, 7)
    c, pos, _ = P[5]
    assert block_of_residue(off, c, pos) + 1 == block_of_residue(off, c, pos + W - 1) == 4
    assert block_of_residue(off, 0, P[0][1]) == 0 and block_of_residue(off, 0, lens[0] - 1) == 1
    for c, pos, _ in P:
        assert 0 <= pos and pos + W <= lens[c]


@functools.lru_cache(maxsize=None)
def case(k):
    """What the tests of one k share, computed once and never modified."""
    ref = fc.family(k, N, NK)
    W = ref["ws"]
    lens = lengths()
    rng = np.random.default_rng([9901, k])
    arrs = [bytearray(random_dna(rng, L)) for L in lens]
    twice = mutate(rng, ref["base"], 0.04)[:W]
    plants = []
    for c, pos, what in plants_of(lens, W):
        arrs[c][pos:pos + W] = twice if c == 4 else mutate(rng, ref["base"], 0.04)[:W]
        plants.append((c, pos))
    contigs = [bytes(a) for a in arrs]
    D = fc.exact_D(contigs, ref["S"], N, k, W)
    # the threshold: on the distance of a window of record 4 (the nearest to the usual one, on a gene's flank), so that the window
    # is in the guard band and the record is chained whatever its two equal minima do
    scale = 2.0 * k * N * N
    s4 = int(np.argmin(np.abs(D[4][1:] - fc.threshold(D, plants, k, N) * scale))) + 1
    thr = float(D[4][s4]) / scale
    T, T_hi = filter_ref.threshold_band(thr, k, N)
    assert T == D[4][s4] <= T_hi and thr > fc.planted_max(D, plants, k, N)
    sums = [sums_ref.block_sums(c, ref["S"], k) for c in contigs]
    ohits, _ = orc.single_scan(contigs, ref["RV"], k, W, thr, BUFF)
    return dict(ref=ref, W=W, lens=lens, contigs=contigs, plants=plants, thr=thr, sums=sums, ohits=ohits,
                n_blocks=-(-total_words(lens) // BLOCK_WORDS))


class Run:
    """A context with the case's references and genome."""

    def __init__(self, c, k, contigs=None):
        self.ctx = _lib.Context(0)
        self.g = None
        try:
            self.ctx.set_refs(k, [c["ref"]["RV"]], [c["W"]], [c["thr"]], [N])
            self.g = self.ctx.genome_from_host(c["contigs"] if contigs is None else contigs)
        except Exception:
            self.close()
            raise

    def step(self, flags=0):
        self.ctx.step_hits(self.g, _lib.MODE_SINGLE, BUFF, 0, flags)
        state = self.g.inter_state()
        out = fu._collect(self.ctx, self.g, True, self.g.n_contigs)
        out["state"], out["demand"] = state
        out["chain_pairs"] = self.ctx.stats()["n_chain_pairs"]
        return out

    def close(self):
        if self.g is not None:
            self.g.free()
        self.ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def one_step(monkeypatch, c, k, flags, sparse, poison=False, chain_host=False, contigs=None):
    monkeypatch.setenv("KGMA_SPARSE_PACK", "1" if sparse else "0")
    monkeypatch.setenv("KGMA_SPARSE_POISON", "1" if poison else "0")
    if chain_host:
        monkeypatch.setenv("KGMA_CHAIN", "host")
    else:
        monkeypatch.delenv("KGMA_CHAIN", raising=False)
    with Run(c, k, contigs) as r:
        return r.step(flags)


_FULL_STEPS = {}


def full_step(monkeypatch, k, flags):
    """The step with KGMA_SPARSE_PACK=0 (computed once per (k, flags), never modified)."""
    if (k, flags) not in _FULL_STEPS:
        _FULL_STEPS[(k, flags)] = one_step(monkeypatch, case(k), k, flags, False)
    return _FULL_STEPS[(k, flags)]


def check_sparse_step(c, k, flags, on, off):
    assert off["state"] == FULL and off["demand"] == 0
    assert on["state"] == PARTIAL
    assert on["demand"] > 0
    if not flags & CHAIN:                                               # (a chained record's blocks are counted on top of the candidates')
        assert on["demand"] <= c["n_blocks"] - 1                        # block 8: test_layout
    assert on["fs"]["ran"] == 1 and on["fs"]["fell_back"] == 0, on["fs"]
    want_form = fc.form_of(k, int(np.max(c["ref"]["S"]))) | PRESUMMED
    assert on["fs"]["form"] == want_form and off["fs"]["form"] == want_form
    fu._check_sums(on["sums"], c["sums"])                               # (first: a wrong sum names its block)
    fu._check_sums(off["sums"], c["sums"])
    fu._same(on, off)
    have = set(map(tuple, on["cand"].tolist()))
    assert all((r, s // 16) in have for r, s in c["plants"])
    if flags & CHAIN:
        assert on["chain_pairs"] >= 1 and on["chain_pairs"] == off["chain_pairs"]
        assert [hit_key(h) for h in on["hits"]] == [hit_key(h) for h in c["ohits"]]
    assert len(on["hits"]) >= 5


# ---- 1, 2: equality, and only packed blocks are read -----------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, CHAIN], ids=["plain", "chain"])
@pytest.mark.parametrize("k", KS)
def test_sparse_step_equals_full_step_and_oracle(monkeypatch, k, flags):
    c = case(k)
    check_sparse_step(c, k, flags, one_step(monkeypatch, c, k, flags, True), full_step(monkeypatch, k, flags))


@pytest.mark.parametrize("chain", ["none", "device", "host"])
@pytest.mark.parametrize("k", KS)
def test_poisoned_sparse_step(monkeypatch, k, chain):
    """The copy is filled with a byte pattern behind the sums-only pack: a read of a block nobody packed changes a result."""
    c = case(k)
    flags = 0 if chain == "none" else CHAIN
    on = one_step(monkeypatch, c, k, flags, True, poison=True, chain_host=chain == "host")
    check_sparse_step(c, k, flags, on, full_step(monkeypatch, k, flags))


# ---- 3: every later reader -------------------------------------------------------------------------------------------------------

def _scan(r, flags=0):
    r.ctx.scan(r.g, _lib.MODE_SINGLE, BUFF, 0, flags, None)
    return dict(hits=r.ctx.hits(), dips=r.ctx.dips(), D1=r.ctx.first_window(1).tolist(), att=r.ctx.att().tolist(), name=r.ctx.kernel_name())


def _ranges(c):
    """Ranges of the genome around the plants (record, 1-based lo, hi)."""
    W = c["W"]
    rec = [p[0] for p in c["plants"]]
    lo = [p[1] + 1 for p in c["plants"]]
    return rec, lo, [x + W - 1 for x in lo]


def reader_scan(monkeypatch, r, c, k):
    return _scan(r)


def reader_bitslice(monkeypatch, r, c, k):
    monkeypatch.setenv("KGMA_KERNEL", "bitslice")
    out = _scan(r)
    assert out["name"].startswith("scan_kernel")
    return out


def reader_generic(monkeypatch, r, c, k):
    monkeypatch.setenv("KGMA_KERNEL", "generic")
    out = _scan(r)
    assert out["name"].startswith("gen_kernel")
    return out


def reader_strobe(monkeypatch, r, c, k):
    cfg = (2, 3, 5, 5)
    ref = sc.ref_of(sc.disc_table(2), sc.DISC_N, cfg, 60)
    r.ctx.set_strobe_ref(*cfg, ref["RV"], ref["W"], 1.0, ref["N"])
    r.ctx.strobe_scan(r.g, BUFF, 0, None, -69, -5, 0)
    return dict(hits=r.ctx.hits(), dips=r.ctx.dips(), D1=r.ctx.first_window(1).tolist(), name=r.ctx.kernel_name())


def reader_both_strands(monkeypatch, r, c, k):
    rc = r.g.revcomp()
    try:
        r.ctx.scan(rc, _lib.MODE_SINGLE, BUFF, 0, 0, None)
        minus = dict(hits=r.ctx.hits(), D1=r.ctx.first_window(1).tolist())
        assert rc.inter_state()[0] == FULL
    finally:
        rc.free()
    return dict(minus=minus, plus=_scan(r))


def reader_exact(monkeypatch, r, c, k):
    qs = [c["contigs"][rec][pos:pos + 24] for rec, pos in c["plants"]] + [b"ACGTACGTACGTAC", c["contigs"][6][-17:]]
    r.ctx.exact_match(r.g, qs, True)
    out = r.ctx.matches().tolist()
    assert len(out) >= len(qs) - 1
    return out


def reader_motif(monkeypatch, r, c, k):
    r.ctx.motif_match(r.g, [c["contigs"][3][:20], b"ACGTNNRYACGT"], [2, 1])
    return r.ctx.motif_matches().tolist()


def reader_window_and_mutation_dists(monkeypatch, r, c, k):
    rec, lo, _ = _ranges(c)
    D, dist = r.ctx.window_dists(r.g, 1, rec, lo)
    Dm, distm = r.ctx.mutation_dists([c["ref"]["base"]], 1, [0.0, 0.05], 3, 11)
    return dict(D=D.tolist(), dist=dist.tolist(), Dm=Dm.tolist(), distm=distm.tolist())


def _refs_for_assign(c):
    rng = np.random.default_rng(9902)
    return [c["ref"]["base"], mutate(rng, c["ref"]["base"], 0.2), random_dna(rng, c["W"])]


def reader_assign(monkeypatch, r, c, k):
    rec, lo, hi = _ranges(c)
    out, scores = r.ctx.assign_ranges(r.g, _refs_for_assign(c), rec, lo, hi)
    return dict(out=out.tolist(), scores=scores.tolist())


def reader_assign_screened(monkeypatch, r, c, k):
    rec, lo, hi = _ranges(c)
    out, cand, scores = r.ctx.assign_ranges_screened(r.g, _refs_for_assign(c), rec, lo, hi, n_near=2)
    return dict(out=out.tolist(), cand=cand.tolist(), scores=scores.tolist())


def reader_kmat(monkeypatch, r, c, k):
    rec, lo, hi = _ranges(c)
    D, dist = r.ctx.kmer_dist_matrix_ranges(r.g, rec, lo, hi, _refs_for_assign(c), k)
    return dict(D=D.tolist(), dist=dist.tolist())


def reader_landscape(monkeypatch, r, c, k):
    r.ctx.scan(r.g, _lib.MODE_SINGLE, BUFF, 0, _lib.F_RETURN_DISTS, None)
    bmin, barg, off = r.ctx.dist_bins(1, 512)
    below, dips = r.ctx.dist_sweep([0.5 * c["thr"], c["thr"], 2.0 * c["thr"]], 1)
    assert below[-1] > 0
    return dict(bmin=bmin.tolist(), barg=barg.tolist(), off=off.tolist(), below=below.tolist(), dips=dips.tolist())


def reader_chain_values(monkeypatch, r, c, k):
    return dict(many=r.g.chain_values(4, 1, [(1, 3), (40_000, 40_010)]).tolist(), first=r.g.chain_values(2, 1, [(1, 1)]).tolist())


# (reads_copy: the call reads the 2-bit copy or the planes, so it completes the copy itself; the others read the residue text alone
#  and leave the state as it is -- the plain scan that follows every reader then completes it)
READERS = [
    ("scan", reader_scan, True), ("bitslice", reader_bitslice, True), ("generic", reader_generic, True), ("strobe", reader_strobe, True),
    ("both_strands", reader_both_strands, True), ("exact", reader_exact, True), ("motif", reader_motif, True),
    ("window_mutation_dists", reader_window_and_mutation_dists, False), ("assign", reader_assign, False),
    ("assign_screened", reader_assign_screened, False), ("kmat", reader_kmat, False), ("landscape", reader_landscape, True),
    ("chain_values", reader_chain_values, True),
]


@pytest.mark.parametrize("name,reader,reads_copy", READERS, ids=[x[0] for x in READERS])
@pytest.mark.parametrize("k", KS)
def test_reader_after_a_poisoned_sparse_step(monkeypatch, k, name, reader, reads_copy):
    c = case(k)
    got = []
    for sparse in (True, False):
        monkeypatch.setenv("KGMA_SPARSE_PACK", "1" if sparse else "0")
        monkeypatch.setenv("KGMA_SPARSE_POISON", "1" if sparse else "0")
        monkeypatch.delenv("KGMA_KERNEL", raising=False)
        with Run(c, k) as r:
            r.ctx.step_hits(r.g, _lib.MODE_SINGLE, BUFF, 0, 0)
            assert r.g.inter_state()[0] == (PARTIAL if sparse else FULL)
            out = reader(monkeypatch, r, c, k)
            if reads_copy:
                assert r.g.inter_state()[0] == FULL
            monkeypatch.delenv("KGMA_KERNEL", raising=False)
            if name == "strobe":
                r.ctx.set_refs(k, [c["ref"]["RV"]], [c["W"]], [c["thr"]], [N])
            after = _scan(r)                                            # every sequence ends in a reader of the copy
            assert r.g.inter_state() == (FULL, 0)
            got.append((out, after))
    assert got[0][0] == got[1][0]
    assert got[0][1] == got[1][1]
    assert len(got[0][1]["hits"]) >= 5


# ---- 4: text changes -------------------------------------------------------------------------------------------------------------

def _poked(c, k):
    gene = mutate(np.random.default_rng([9903, k]), c["ref"]["base"], 0.03)[:c["W"]]
    a = bytearray(c["contigs"][0]); a[9_000:9_000 + c["W"]] = gene        # (no candidate stream of the first step is near)
    return (0, 9_001, gene), [bytes(a)] + c["contigs"][1:]


@pytest.mark.parametrize("k", KS)
def test_poke_then_plain_scan_without_repack(monkeypatch, k):
    c = case(k)
    poke, _ = _poked(c, k)
    got = []
    for sparse in (True, False):
        monkeypatch.setenv("KGMA_SPARSE_PACK", "1" if sparse else "0")
        monkeypatch.setenv("KGMA_SPARSE_POISON", "1" if sparse else "0")
        with Run(c, k) as r:
            r.step(0)
            r.g.poke(*poke)
            assert r.g.inter_state()[0] == FULL                         # completed from the old text, before the text changed
            got.append(_scan(r))
    assert got[0] == got[1]


@pytest.mark.parametrize("k", KS)
def test_poke_then_step(monkeypatch, k):
    c = case(k)
    poke, contigs2 = _poked(c, k)
    monkeypatch.setenv("KGMA_SPARSE_PACK", "1")
    monkeypatch.setenv("KGMA_SPARSE_POISON", "1")
    with Run(c, k) as r:
        first = r.step(CHAIN)
        r.g.poke(*poke)
        second = r.step(CHAIN)
    assert first["state"] == PARTIAL and second["state"] == PARTIAL
    ohits, _ = orc.single_scan(contigs2, c["ref"]["RV"], k, c["W"], c["thr"], BUFF)
    assert [hit_key(h) for h in second["hits"]] == [hit_key(h) for h in ohits]
    assert len(second["hits"]) == len(first["hits"]) + 1
    fu._check_sums(second["sums"], [sums_ref.block_sums(x, c["ref"]["S"], k) for x in contigs2])


# ---- 5: fallbacks inside a sparse step -------------------------------------------------------------------------------------------

def _unfiltered(monkeypatch, c, k, contigs):
    monkeypatch.setenv("KGMA_FILTER", "0")
    try:
        with Run(c, k, contigs) as r:
            r.ctx.step_hits(r.g, _lib.MODE_SINGLE, BUFF, 0, 0)
            return dict(hits=r.ctx.hits(), dips=r.ctx.dips(), D1=r.ctx.first_window(1).tolist(), att=r.ctx.att().tolist())
    finally:
        monkeypatch.setenv("KGMA_FILTER", "1")


def _fallback(monkeypatch, c, k, contigs, reason):
    want = _unfiltered(monkeypatch, c, k, contigs)
    monkeypatch.setenv("KGMA_SPARSE_PACK", "1")
    monkeypatch.setenv("KGMA_SPARSE_POISON", "1")
    with Run(c, k, contigs) as r:
        first = r.step(0)
        second = r.step(0)
    assert first["fs"]["ran"] == 1 and first["fs"]["fell_back"] == 1 and first["fs"]["reason"] == reason, first["fs"]
    assert first["fs"]["form"] & PRESUMMED
    assert first["state"] == FULL                                       # one full pack, once
    for s in (first, second):
        assert dict(hits=s["hits"], dips=s["dips"], D1=s["D1"].tolist(), att=s["att"].tolist()) == want
    assert second["fs"]["reason"] == _lib.FILTER_REMEMBERED and not second["fs"]["form"] & PRESUMMED
    assert second["state"] == FULL
    assert len(want["hits"]) >= 1


@pytest.mark.parametrize("k", KS)
def test_fallback_overflow(monkeypatch, k):
    monkeypatch.setenv("KGMA_FILTER_CAP", "2")
    c = case(k)
    _fallback(monkeypatch, c, k, None, _lib.FILTER_OVERFLOW)


@pytest.mark.parametrize("k", KS)
def test_fallback_fraction(monkeypatch, k):
    """A tandem run of the base over most of a record: the candidate streams pass FILTER_MAX_FRACTION of the windows."""
    c = case(k)
    W = c["W"]
    rng = np.random.default_rng([9904, k])
    run = c["ref"]["base"][:W] * 300
    contigs = [random_dna(rng, 10_000), random_dna(rng, 3_000) + run + random_dna(rng, 3_000)]
    assert len(run) > 0.6 * sum(len(x) for x in contigs)                # (FILTER_MAX_FRACTION is 0.5)
    _fallback(monkeypatch, c, k, contigs, _lib.FILTER_FRACTION)


# ---- 6: a genome with a plane copy -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_genome_with_bit_planes_packs_in_full(monkeypatch, k):
    c = case(k)
    got = []
    for sparse in (True, False):
        monkeypatch.setenv("KGMA_SPARSE_PACK", "1" if sparse else "0")
        monkeypatch.setenv("KGMA_SPARSE_POISON", "1" if sparse else "0")
        with Run(c, k) as r:
            monkeypatch.setenv("KGMA_KERNEL", "bitslice")
            _scan(r)                                                    # (makes the bit-plane copy)
            monkeypatch.delenv("KGMA_KERNEL")
            poke, _ = _poked(c, k)
            r.g.poke(*poke)
            step = r.step(0)
            assert (step["state"], step["demand"]) == (FULL, 0)
            assert step["fs"]["form"] & PRESUMMED
            monkeypatch.setenv("KGMA_KERNEL", "bitslice")
            planes = _scan(r)                                           # the planes the step's pack wrote
            monkeypatch.delenv("KGMA_KERNEL")
            assert planes["name"].startswith("scan_kernel")
            got.append((step, planes))
    fu._same(got[0][0], got[1][0])
    assert got[0][1] == got[1][1]
    assert len(got[0][1]["hits"]) >= 5


# ---- 7: the pack loop, sums-only form --------------------------------------------------------------------------------------------

def _loop_step(monkeypatch, c, k, sparse):
    monkeypatch.setenv("KGMA_SPARSE_PACK", "1" if sparse else "0")
    ctx = _lib.Context(0)
    g = None
    try:
        ctx.set_refs(k, [c["ref"]["RV"]], [c["ref"]["ws"]], [c["thr"]], [c["ref"]["N"]])
        g = ctx.genome_from_host(c["contigs"])
        ctx.step_hits(g, _lib.MODE_SINGLE, BUFF, 0, 0)
        state = g.inter_state()[0]
        return fu._collect(ctx, g, True, len(c["contigs"])), state
    finally:
        if g is not None:
            g.free()
        ctx.close()


@pytest.mark.parametrize("wgs", [1, 2, None], ids=["wgs1", "wgs2", "default"])
@pytest.mark.parametrize("k", KS)
def test_pack_loop_sums_only_form(monkeypatch, k, wgs):
    """The layout of test_gpu_pack_loop.py (13 or 14 units per wave at one workgroup): the sums-only form's sums, candidates and
    results are the storing form's and the reference's."""
    if wgs is not None:
        monkeypatch.setenv("KGMA_PACK_WGS", str(wgs))
    c = pl.case(k, "long")
    (on, s_on), (off, s_off) = _loop_step(monkeypatch, c, k, True), _loop_step(monkeypatch, c, k, False)
    assert (s_on, s_off) == (PARTIAL, FULL)
    assert on["fs"]["form"] & PRESUMMED and off["fs"]["form"] & PRESUMMED
    fu._check_sums(on["sums"], c["sums"])
    fu._check_sums(off["sums"], c["sums"])
    fu._same(on, off)
    assert np.array_equal(on["cand"], c["cand"])


@pytest.mark.parametrize("k", KS)
def test_pack_loop_sums_only_illegal_byte(monkeypatch, k):
    """One illegal byte in the second and in the last unit a wave takes at one workgroup: first_bad -- the status, the record and
    the position -- is the storing form's."""
    monkeypatch.setenv("KGMA_PACK_WGS", "1")
    c = pl.case(k, "long")
    lens, contigs, ref = c["lens"], c["contigs"], c["ref"]
    off, _ = word_offsets(lens)
    n = pl.n_units(lens)
    last = max(u for u in range(n) if pl.unit_kind(u, lens, k)[:2] == (13, "fast"))
    second = last % pl.WAVES + pl.WAVES
    assert last + pl.WAVES >= n and pl.unit_kind(second, lens, k)[:2] == (0, "fast")
    spots = [(0, 32 * (second * UNIT_WORDS - off[0]) + 1234), (13, 32 * (last * UNIT_WORDS - off[13]) + 4001)]
    ctx = _lib.Context(0)
    g = None
    try:
        ctx.set_refs(k, [ref["RV"]], [ref["ws"]], [c["thr"]], [ref["N"]])
        g = ctx.genome_from_host(contigs)

        def step(sparse):
            monkeypatch.setenv("KGMA_SPARSE_PACK", "1" if sparse else "0")
            try:
                ctx.step_hits(g, _lib.MODE_SINGLE, BUFF, 0, 0)
            except _lib.KgmaError as e:
                return e.status, e.message
            return 0, ""

        for bad in ([spots[0]], [spots[1]], spots):
            for r, pos in bad:
                g.poke(r, pos + 1, b"X")
            on, off_ = step(True), step(False)
            for r, pos in bad:
                g.poke(r, pos + 1, contigs[r][pos:pos + 1])
            assert on == off_, (bad, on, off_)
            assert on[0] == _lib.KGMA_E_BADBASE and "record %d position %d" % (bad[0][0], bad[0][1] + 1) in on[1], (bad, on)
        assert step(True) == (0, "")                                    # restored
        assert g.inter_state()[0] == PARTIAL
        clean = fu._collect(ctx, g, True, len(contigs))
        fu._check_sums(clean["sums"], c["sums"])
        assert np.array_equal(clean["cand"], c["cand"])
    finally:
        if g is not None:
            g.free()
        ctx.close()
