"""The fused pack's pair table and dot-product encoder and the sum-reading filter's four blocks per lane (kgma_filter.hip:
pack_sums_kernel, filter_sums_kernel; kgma_pack.h: pack_word_2bit) where they can go wrong: every case runs the step with the sums
fused into the pack and with KGMA_FUSE_SUMS=0 and compares the two in every field, the sums read back with tests/sums_ref.py and
the candidate granules with tests/filter_ref.py, the way test_gpu_fused_sums.py does (its helpers are used here).

The pack takes units of 128 plane words (4096 residues) of the GLOBAL word array: a genome starts with LEAD_PAD_WORDS words of
padding and every record is followed by CONTIG_PAD_WORDS (kgma_api.cpp: genome_layout), so the records below get the lengths that
put their ends where a unit ends."""
import functools
import re

import numpy as np
import pytest

from kmergma_amd import _lib
from tests import filter_cases as fc
from tests import filter_ref, sums_ref
from tests import test_gpu_fused_sums as fu
from tests.helpers import kmer_values, mutate, random_dna

pytestmark = pytest.mark.gpu

LEAD_PAD_WORDS, CONTIG_PAD_WORDS, UNIT_WORDS = 8, 32, 128
PRESUMMED = _lib.FILTER_FORM_PRESUMMED


@pytest.fixture(autouse=True)
def _small_genomes(monkeypatch):
    monkeypatch.setenv("KGMA_FILTER_MIN_WINDOWS", "1")
    monkeypatch.setenv("KGMA_FILTER", "1")
    monkeypatch.delenv("KGMA_OVERLAP", raising=False)


def word_offsets(lengths):
    """The global word index of every record's first word, and of the word behind the last record's padding."""
    off, at = [], LEAD_PAD_WORDS
    for L in lengths:
        off.append(at)
        at += (L + 31) // 32 + CONTIG_PAD_WORDS
    return off, at


def _thr(contigs, ref, plants, k):
    D = fc.exact_D(contigs, ref["S"], ref["N"], k, ref["ws"])
    return fc.threshold(D, plants, k, ref["N"])


def _compare(monkeypatch, contigs, ref, thr, k):
    """Fused on against off (every field, the form, the sums against sums_ref) and the candidates against filter_ref."""
    sums = [sums_ref.block_sums(c, ref["S"], k) for c in contigs]
    on = fu._on_off(monkeypatch, contigs, ref, thr, k, ref["ws"], None, sums, all_flags=(0,))
    T, T_hi = filter_ref.threshold_band(thr, k, ref["N"])
    U = filter_ref.bound_U(ref["S"], ref["N"], k, ref["ws"], T, T_hi)
    assert on["fs"]["bound"] == U
    assert np.array_equal(on["cand"], filter_ref.candidates(contigs, ref["S"], k, ref["ws"], U))
    return on


# ---- unit edges ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [5, 6])
def test_records_that_end_around_a_units_end(monkeypatch, k):
    """Records of 4096 m + r residues counted from a unit's start, r in {0, k - 2, k - 1, k, 31, 32, 33}: the last whole unit is just
    not fast (fewer than k - 1 residues behind it) and just fast; the halo's residues are the record's last; the pair at positions
    14, 15 of a word's second dword reads the next word across a chunk boundary (word 63 -> 64) and across the unit's end."""
    ref = fc.family(k, 7, 100)
    W = ref["ws"]
    rng = np.random.default_rng([7201, k])
    contigs, plants, at = [], [], LEAD_PAD_WORDS
    for m, r in [(2, 0), (2, k - 2), (3, k - 1), (2, k), (2, 31), (3, 32), (2, 33)]:
        head = (-at) % UNIT_WORDS                                      # words up to the next unit's start
        L = 32 * (head + UNIT_WORDS * m) + r
        a = bytearray(random_dna(rng, L))
        for pos in (32 * head + 4096 - W // 2, L - W):                  # a gene across a unit's start and on the record's last residue
            a[pos:pos + W] = mutate(rng, ref["base"], 0.04)[:W]
            plants.append((len(contigs), pos))
        contigs.append(bytes(a))
        at += (L + 31) // 32 + CONTIG_PAD_WORDS
    off, _ = word_offsets([len(c) for c in contigs])
    for c, (m, r) in zip(range(len(contigs)), [(2, 0), (2, k - 2), (3, k - 1), (2, k), (2, 31), (3, 32), (2, 33)]):
        assert (off[c] + len(contigs[c]) // 32) % UNIT_WORDS == (1 if r >= 32 else 0) and len(contigs[c]) % 4096 % 32 == r % 32
    assert sum(len(c) for c in contigs) < 1_000_000
    on = _compare(monkeypatch, contigs, ref, _thr(contigs, ref, plants, k), k)
    have = set(map(tuple, on["cand"].tolist()))
    assert all((c, s // 16) in have for c, s in plants)


# ---- maximal sums ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [5, 6])
def test_maximal_sums(monkeypatch, k):
    """S = 255 on every k-mer of the gene and on three entries in ten of the rest: pair sums of 510 and runs of neighbouring block
    sums of 4080, which must stay inside their halves of the dword the pack stores; the filter still takes the byte form."""
    nk, N = 284, 255
    W = nk + k - 1
    rng = np.random.default_rng([7202, k])
    base = random_dna(rng, W)
    S = np.where(rng.random(4 ** k) < 0.3, 255, 0).astype(np.int64)
    S[kmer_values(base, k)] = 255
    ref = fc.ref_from_S(S, N, k, W, base)
    a = bytearray(random_dna(rng, 60_000))
    plants = [(0, pos) for pos in (100, 4096 * 3 + 8 * 32 - 150, 30_000, 60_000 - W)]
    for _, pos in plants:
        a[pos:pos + W] = base
    contigs = [bytes(a), base + random_dna(rng, 77)]
    plants.append((1, 0))
    sums = sums_ref.block_sums(contigs[0], S, k)
    full = np.nonzero(sums == 4080)[0]
    assert full.size > 40 and (np.diff(full) == 1).sum() > 30          # neighbours at the maximum
    on = _compare(monkeypatch, contigs, ref, _thr(contigs, ref, plants, k), k)
    assert on["fs"]["form"] == fc.form_of(k, 255) | PRESUMMED == (1 | 32 << 8 | PRESUMMED)
    have = set(map(tuple, on["cand"].tolist()))
    assert all((c, s // 16) in have for c, s in plants)


# ---- letter case -----------------------------------------------------------------------------------------------------------------

def test_letter_case_and_n_runs(monkeypatch):
    """Lower-case and mixed-case full words inside fast units (no case fold before the table index), N and n runs on a unit's first
    and last word."""
    k = 6
    ref = fc.family(k, 7, 100)
    W = ref["ws"]
    rng = np.random.default_rng(7203)
    head = (-LEAD_PAD_WORDS) % UNIT_WORDS                                # the record's words before its first whole unit
    u = lambda n: 32 * (head + UNIT_WORDS * n)                            # residue at which unit n of the record starts
    a = bytearray(random_dna(rng, u(6) + 500))
    plants = []
    for pos in (u(1) + 1000, u(2) + 40, u(3) - W // 2):
        a[pos:pos + W] = mutate(rng, ref["base"], 0.04)[:W]
        plants.append((0, pos))
    a[u(1) + 900:u(1) + 1400] = bytes(a[u(1) + 900:u(1) + 1400]).lower()                        # over a gene
    mixed = np.frombuffer(bytes(a[u(2):u(2) + 640]), dtype=np.uint8) | (rng.integers(0, 2, size=640).astype(np.uint8) << 5)
    a[u(2):u(2) + 640] = mixed.tobytes()
    a[u(4) - 10:u(4) + 32] = b"N" * 42                                                            # a unit's last word into the next one's first
    a[u(5) - 32:u(5)] = b"n" * 32
    a[u(5):u(5) + 32] = b"nN" * 16
    contigs = [bytes(a)]
    on = _compare(monkeypatch, contigs, ref, _thr([contigs[0].upper()], ref, plants, k), k)
    assert len(on["hits"]) >= 3


# ---- illegal bytes ---------------------------------------------------------------------------------------------------------------

def test_every_byte_value_in_a_fast_unit(monkeypatch):
    """One context, one genome: every byte value in turn in a fast-path unit.  The ten letters are accepted (the step's results
    are the unfused step's); every other value is KGMA_E_BADBASE with the record and position the unfused step names."""
    k = 6
    ref = fc.family(k, 7, 100)
    rng = np.random.default_rng(7204)
    head = (-LEAD_PAD_WORDS) % UNIT_WORDS
    contigs = [random_dna(rng, 500), random_dna(rng, 32 * (head + UNIT_WORDS * 3) + 100)]
    off, _ = word_offsets([len(c) for c in contigs])
    u1 = 32 * ((-off[1]) % UNIT_WORDS + UNIT_WORDS)                      # record 1's second whole unit
    a = bytearray(contigs[1])
    a[100:100 + ref["ws"]] = mutate(rng, ref["base"], 0.04)[:ref["ws"]]
    contigs[1] = bytes(a)
    thr = _thr(contigs, ref, [(1, 100)], k)
    letters = set(b"ACGTNacgtn")
    ctx = _lib.Context(0)
    g = None
    try:
        ctx.set_refs(k, [ref["RV"]], [ref["ws"]], [thr], [ref["N"]])
        g = ctx.genome_from_host(contigs)

        def step(fuse):
            monkeypatch.setenv("KGMA_FUSE_SUMS", "1" if fuse else "0")
            try:
                ctx.step_hits(g, _lib.MODE_SINGLE, fu.BUFF, 0, 0)
            except _lib.KgmaError as e:
                return e.status, e.message
            return 0, (ctx.hits(), ctx.filter_candidates().tolist(), ctx.filter_stats()["form"] & PRESUMMED)

        for v in range(256):
            pos = u1 + 37 + 13 * v                                      # (moves through the unit's words and dwords)
            assert pos < u1 + 4096
            g.poke(1, pos + 1, bytes([v]))
            on, off_ = step(True), step(False)
            g.poke(1, pos + 1, contigs[1][pos:pos + 1])
            if v in letters:
                assert on[0] == 0 and off_[0] == 0, (v, on, off_)
                assert on[1][:2] == off_[1][:2] and on[1][2] == PRESUMMED and off_[1][2] == 0, v
            else:
                assert on == off_, (v, on, off_)
                assert on[0] == _lib.KGMA_E_BADBASE and "record 1 position %d" % (pos + 1) in on[1], (v, on)
        assert step(True)[0] == 0                                       # restored
    finally:
        if g is not None:
            g.free()
        ctx.close()


# ---- single candidate granules at every place of a wave iteration ---------------------------------------------------------------

BIG = 20_000_000
RESIDUES = (0, 1, 3, 63, 64, 127, 128, 255)
RUN_GRANULES = 320


@functools.lru_cache(maxsize=None)
def _big_record():
    return random_dna(np.random.default_rng(7205), BIG)


@pytest.mark.parametrize("nk", [17, 18, 34, 284], ids=lambda nk: "nblk%d" % fc.nblk_of(nk))
def test_candidate_granule_at_every_place_of_an_iteration(monkeypatch, nk):
    """filter_sums_kernel takes 256 blocks per wave iteration, and the host cuts a genome into (CUs not reserved x streams per CU)
    streams of at least 2048 windows, 128 granules.  kgma_set_reserved_cus takes half of the CUs at most, which leaves 4096 streams
    on a device of 256 CUs, so a stream of more than 256 granules needs 17 M windows: this one test takes a record of 20 Mb with
    half of the CUs reserved (the stream length is asserted), learns the stream length from a first step, and then pokes exact
    copies of the gene where the candidate granule's index within its stream is 0, 1, 3, 63, 64, 127, 128 and 255 mod 256, in
    streams 1, 2, ..., and a tandem run of 320 consecutive candidate granules, which crosses an iteration and a stream's end.  nk
    gives nblk = 2, 3, 4, 19: every nblk % 4 (which element of the source lane a bound reads), source lane l and l - 1 (qa = 0)
    and further back."""
    k, N = 6, 7
    ref = fc.family(k, N, nk)
    W, base = ref["ws"], ref["base"]
    assert fc.nblk_of(nk) in (2, 3, 4, 19)
    seq = _big_record()
    vals = kmer_values(base, k)
    D_plant = int(((ref["S"] - N * np.bincount(vals, minlength=4 ** k)) ** 2).sum())
    thr = round(1.25 * D_plant / (2.0 * k * N * N) + 0.05, 2)
    T, T_hi = filter_ref.threshold_band(thr, k, N)
    U = filter_ref.bound_U(ref["S"], N, k, W, T, T_hi)
    nwin = BIG - W + 1

    def plan(n_streams):
        """(pokes, the granules they make candidates) for the stream length the host chose."""
        P = -(-(-(-nwin // n_streams)) // 64) * 64                      # (streams start on 64-window boundaries)
        assert -(-nwin // P) == n_streams and P // 16 > 256, (n_streams, P)
        pokes, plants = [], []
        for t, r in enumerate(RESIDUES, start=1):
            for rep in range(1 if r + 256 >= P // 16 else 2):           # the residue in the stream's first and second iteration
                gr = t * (P // 16) + r + 256 * rep
                pokes.append((16 * gr + 5, base))
                plants.append(gr)
        run_at = 16 * (20 * (P // 16) + 100) + 3                        # from granule 100 of stream 20 on
        pokes.append((run_at, base * (-(-(16 * RUN_GRANULES + W) // W))))
        return pokes, plants

    def run(fuse):
        monkeypatch.setenv("KGMA_FUSE_SUMS", "1" if fuse else "0")
        ctx = _lib.Context(0)
        g = None
        try:
            with pytest.raises(_lib.KgmaError) as too_many:             # (the message names the most that can be reserved: half)
                ctx.set_reserved_cus(1 << 20)
            ctx.set_reserved_cus(int(re.search(r"0\.\.(\d+)", too_many.value.message).group(1)))
            ctx.set_refs(k, [ref["RV"]], [W], [thr], [N])
            g = ctx.genome_from_host([seq])
            ctx.step_hits(g, _lib.MODE_SINGLE, fu.BUFF, 0, 0)
            pokes, plants = plan(ctx.stats()["n_tiles"])
            for pos, data in pokes:
                g.poke(0, pos + 1, data)
            ctx.step_hits(g, _lib.MODE_SINGLE, fu.BUFF, 0, 0)
            return fu._collect(ctx, g, False, 1), pokes, plants
        finally:
            if g is not None:
                g.free()
            ctx.close()

    (on, pokes, plants), (off, pokes_off, _) = run(True), run(False)
    assert pokes == pokes_off
    a = bytearray(seq)
    for pos, data in pokes:
        a[pos:pos + len(data)] = data
    assert on["fs"]["ran"] == 1 and on["fs"]["fell_back"] == 0 and on["fs"]["bound"] == U, on["fs"]
    assert on["fs"]["form"] == fc.form_of(k, int(ref["S"].max())) | PRESUMMED and off["fs"]["form"] == fc.form_of(k, int(ref["S"].max()))
    fu._same(on, off)
    assert np.array_equal(on["cand"], filter_ref.candidates([bytes(a)], ref["S"], k, W, U))
    have = set(on["cand"][:, 1].tolist())
    assert all(gr in have for gr in plants)
    assert fc.longest_run(on["cand"]) >= 300
    assert len(on["hits"]) >= len(plants)


# ---- a stream whose sums start off an 8-byte boundary ----------------------------------------------------------------------------

def test_stream_at_an_odd_word(monkeypatch):
    """filter_sums_kernel loads a lane's four sums (uint16) as 8 bytes at bsum + 2 * word_base + ...: 4-byte aligned for every
    stream, 8-byte aligned only at an even word.  Short records of an odd number of words ahead of the long one put it at an odd
    word (checked on the layout; streams are a multiple of 64 windows, two words, long, so all of the record's streams are)."""
    k = 6
    ref = fc.family(k, 7, 100)
    W = ref["ws"]
    rng = np.random.default_rng(7206)
    lengths = [W + 3, 33, 160, 100_000, 32 * 6, 70_000]
    off, _ = word_offsets(lengths)
    assert off[3] % 2 == 1 and off[5] % 2 == 0 and off[0] % 2 == 0
    contigs, plants = [], []
    for c, L in enumerate(lengths):
        a = bytearray(random_dna(rng, L))
        if L >= W:
            for pos in sorted({0, L // 3, L - W}):
                a[pos:pos + W] = mutate(rng, ref["base"], 0.04)[:W]
                plants.append((c, pos))
        contigs.append(bytes(a))
    on = _compare(monkeypatch, contigs, ref, _thr(contigs, ref, plants, k), k)
    have = set(map(tuple, on["cand"].tolist()))
    assert all((c, s // 16) in have for c, s in plants)
