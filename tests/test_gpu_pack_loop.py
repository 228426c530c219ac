"""The fused pack's steady loop (kgma_filter.hip: pack_sums_kernel): a wave keeps the record of its units in scalar registers and
looks it up again only when a unit starts at or past the next record, and it takes the next unit's loads over between encoding a
unit and storing it.  Both only show once a wave takes several units, which on a small genome needs the grid capped:
KGMA_PACK_WGS=1 gives 16 waves whose successive units are 16 units (65 536 residues) apart, 2 gives 32 waves, 32 units apart; by
default the genomes here give every wave one unit at most.

Every case runs the step fused and with KGMA_FUSE_SUMS=0 and compares every field, the sums read back with tests/sums_ref.py and
the candidate granules with tests/filter_ref.py (the helpers of test_gpu_fused_sums.py; the layout constants of
test_gpu_pack_pairs.py).  The sums depend on every encoded residue, so they hold the 2-bit copy to account as well."""
import functools

import numpy as np
import pytest

from kmergma_amd import _lib
from tests import filter_cases as fc
from tests import filter_ref, sums_ref
from tests import test_gpu_fused_sums as fu
from tests.helpers import mutate, random_dna
from tests.test_gpu_pack_pairs import CONTIG_PAD_WORDS, LEAD_PAD_WORDS, UNIT_WORDS, word_offsets

pytestmark = pytest.mark.gpu

TAIL_PAD_WORDS = 2 * 253 + 128          # behind the last record's padding (kgma_api.cpp: KGMA_TILE_WORDS + 128)
WAVES = 16                              # of a workgroup
STRIDE = WAVES * UNIT_WORDS             # words between a wave's successive units at KGMA_PACK_WGS=1
NK = 100                                # k-mers of a window: W = NK + k - 1


@pytest.fixture(autouse=True)
def _small_genomes(monkeypatch):
    monkeypatch.setenv("KGMA_FILTER_MIN_WINDOWS", "1")
    monkeypatch.setenv("KGMA_FILTER", "1")
    monkeypatch.delenv("KGMA_OVERLAP", raising=False)
    monkeypatch.delenv("KGMA_PACK_WGS", raising=False)


# ---- the layout ------------------------------------------------------------------------------------------------------------------

def G(i):
    """The first word of the i-th unit of wave 0 at KGMA_PACK_WGS=1."""
    return STRIDE * i


# The first word of every record; a record ends 32 words of padding before the next one starts.  What wave 0 meets at one
# workgroup, unit by unit, is in the comments and asserted in test_layout.
STARTS = [
    LEAD_PAD_WORDS,                     # 0: G(0) starts in the lead padding; G(1) ... G(4) inside record 0
    G(4) + 848,                         # 1: G(5) inside the next record
    G(5) + 300,                         # 2: one word
    G(5) + 333,                         # 3: two words (shorter than W)
    G(5) + 367,                         # 4: one word
    G(5) + 400,                         # 5: 20 words (shorter than a unit)
    G(5) + 452,                         # 6: one word
    G(5) + 485,                         # 7: three words (shorter than W)
    G(5) + 520,                         # 8: G(6) inside it, six records on; its last word is G(7) - 11
    G(7) + 22,                          # 9: G(7) starts in the padding behind record 8; record 9's last word is G(8) + 4
    G(8) + 37,                          # 10: one word
    G(8) + 70,                          # 11: ten words; G(8)'s unit holds the ends of records 9, 10 and 11 ...
    G(8) + 112,                         # 12: ... and record 12's first words; G(9) inside it; its last word is G(10) + 50
    G(10) + 83,                         # 13: G(11), G(12) inside it; G(13) in the padding behind it, the genome's last
]
LAST_WORDS = 6000                       # record 13's length in words


def lengths():
    out = []
    for c, s in enumerate(STARTS):
        words = STARTS[c + 1] - s - CONTIG_PAD_WORDS if c + 1 < len(STARTS) else LAST_WORDS
        out.append(32 * words - (7 * c + 3) % 32)                      # (the last word partial, a different fill per record)
    return out


def unit_kind(u, lens, k):
    """What unit u is to the pack: (record the lookup gives, 'fast' | 'lead' | 'pad' | 'slow', record ends inside the unit)."""
    off, end = word_offsets(lens)
    total = end + TAIL_PAD_WORDS
    g0 = u * UNIT_WORDS
    c = max([i for i in range(len(off)) if off[i] <= g0], default=0)
    w0 = g0 - off[c]
    ends = sum(1 for i in range(len(off)) if g0 <= off[i] + (lens[i] + 31) // 32 - 1 < g0 + UNIT_WORDS)
    if w0 < 0:
        return c, "lead", ends
    if g0 + UNIT_WORDS <= total and (w0 + UNIT_WORDS) * 32 + (k - 1) <= lens[c]:
        return c, "fast", ends
    return c, ("pad" if w0 * 32 >= lens[c] else "slow"), ends


def n_units(lens):
    return -(-(word_offsets(lens)[1] + TAIL_PAD_WORDS) // UNIT_WORDS)


@pytest.mark.parametrize("k", [5, 6])
def test_layout(k):
    """(no GPU work: the places the cases below rely on)"""
    lens = lengths()
    W = NK + k - 1
    off, _ = word_offsets(lens)
    assert off == STARTS and sum(lens) < 2_000_000
    kinds = [unit_kind(WAVES * i, lens, k) for i in range(14)]
    assert kinds[0] == (0, "lead", 0)                                               # starts in the lead padding
    assert kinds[1:5] == [(0, "fast", 0)] * 4                                       # the same record four times
    assert kinds[5] == (1, "fast", 0)                                               # the next record
    assert kinds[6] == (8, "fast", 0)                                               # several records further on
    assert [lens[c] <= 32 for c in range(2, 8)] == [True, False, True, False, True, False]
    assert all(lens[c] < UNIT_WORDS * 32 for c in range(2, 8)) and lens[3] < W and lens[7] < W and lens[5] > W
    assert kinds[7] == (8, "pad", 0)                                                # starts in the padding behind a record
    assert kinds[8] == (9, "slow", 3)                                               # the ends of three records
    assert kinds[9] == (12, "fast", 0) and kinds[10] == (12, "slow", 1) and kinds[11] == (13, "fast", 0)
    assert kinds[12] == (13, "fast", 0) and kinds[13] == (13, "pad", 0)             # the wave's last unit: behind the last record
    n = n_units(lens)
    assert WAVES * 13 < n < WAVES * 14 and n % WAVES != 0                           # some waves are an iteration short
    # two workgroups: wave 0 goes lead -> record 0 (twice) -> record 8 -> three ends -> slow -> record 13
    assert [unit_kind(2 * WAVES * i, lens, k)[:2] for i in range(7)] == [(0, "lead"), (0, "fast"), (0, "fast"), (8, "fast"), (9, "slow"), (12, "slow"), (13, "fast")]
    # by default every wave has one unit at most (the grid is one workgroup per 16 units)
    small = small_lengths()
    assert n_units(small) < WAVES and unit_kind(n_units(small) - 1, small, k)[1] == "pad"


def small_lengths():
    return [20_000, 40, 9_000]


def build(k, lens, seed):
    """(contigs, plants, ref): random records of the given lengths; genes across the boundary between two units (of different
    waves at any grid), on records' last residues and inside a record shorter than a unit."""
    ref = fc.family(k, 7, NK)
    W = ref["ws"]
    rng = np.random.default_rng([seed, k])
    off, _ = word_offsets(lens)
    arrs = [bytearray(random_dna(rng, L)) for L in lens]
    plants = []

    def plant(c, pos):
        assert 0 <= pos and pos + W <= lens[c]
        arrs[c][pos:pos + W] = mutate(rng, ref["base"], 0.04)[:W]
        plants.append((c, pos))

    def unit_start(c, u):                                               # the residue of record c at which unit u starts
        return 32 * (u * UNIT_WORDS - off[c])

    plant(0, unit_start(0, 2) - W // 2)                                 # across units 1 | 2
    for c in range(len(lens)):
        if lens[c] > 4 * W:
            plant(c, lens[c] - W)                                       # on the record's last residues
    if len(lens) > 13:
        plant(0, unit_start(0, 18) - W // 3)                            # across units 17 | 18: the second units of waves 1 and 2
        plant(5, 200)
        plant(13, unit_start(13, 11 * WAVES + 1) - 5)
        # lower-case and N words inside fast units, before and behind the word-by-word unit G(10): they stay fast
        a, at = arrs[12], unit_start(12, 9 * WAVES)
        a[at + 64:at + 160] = bytes(a[at + 64:at + 160]).lower()
        a[at + 4096 - 32:at + 4096] = b"N" * 32
        a, at = arrs[13], unit_start(13, 11 * WAVES)
        a[at:at + 32] = b"nN" * 16
        a[at + 2000:at + 2100] = bytes(a[at + 2000:at + 2100]).lower()
    return [bytes(a) for a in arrs], plants, ref


@functools.lru_cache(maxsize=None)
def case(k, which):
    """What the tests of one genome and k share, computed once and never modified."""
    lens = lengths() if which == "long" else small_lengths()
    contigs, plants, ref = build(k, lens, 8101 if which == "long" else 8102)
    D = fc.exact_D([c.upper() for c in contigs], ref["S"], ref["N"], k, ref["ws"])
    thr = fc.threshold(D, plants, k, ref["N"])
    T, T_hi = filter_ref.threshold_band(thr, k, ref["N"])
    U = filter_ref.bound_U(ref["S"], ref["N"], k, ref["ws"], T, T_hi)
    return dict(contigs=contigs, plants=plants, ref=ref, thr=thr, U=U, lens=lens,
                sums=[sums_ref.block_sums(c, ref["S"], k) for c in contigs],
                cand=filter_ref.candidates(contigs, ref["S"], k, ref["ws"], U))


def _compare(monkeypatch, c, k, wgs):
    if wgs is not None:
        monkeypatch.setenv("KGMA_PACK_WGS", str(wgs))
    on = fu._on_off(monkeypatch, c["contigs"], c["ref"], c["thr"], k, c["ref"]["ws"], None, c["sums"], all_flags=(0,))
    assert on["fs"]["bound"] == c["U"]
    assert np.array_equal(on["cand"], c["cand"])
    have = set(map(tuple, on["cand"].tolist()))
    assert all((r, s // 16) in have for r, s in c["plants"])
    W = c["ref"]["ws"]                                                  # (a gene on a record's last residues has no rise behind it)
    assert len(on["hits"]) >= sum(1 for r, s in c["plants"] if s + W < c["lens"][r])
    return on


# ---- the cases -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wgs", [1, 2, None], ids=["wgs1", "wgs2", "default"])
@pytest.mark.parametrize("k", [5, 6])
def test_a_waves_successive_units(monkeypatch, k, wgs):
    """The layout of test_layout at one workgroup (a wave takes 13 or 14 units), at two, and at the default grid."""
    _compare(monkeypatch, case(k, "long"), k, wgs)


@pytest.mark.parametrize("wgs", [1, None], ids=["wgs1", "default"])
@pytest.mark.parametrize("k", [5, 6])
def test_fewer_units_than_waves(monkeypatch, k, wgs):
    """A genome of fewer than 16 units: waves with exactly one unit, and waves with none."""
    _compare(monkeypatch, case(k, "small"), k, wgs)


@pytest.mark.parametrize("k", [5, 6])
def test_illegal_byte_in_a_waves_second_and_last_unit(monkeypatch, k):
    """One illegal byte in the second and in the last unit a wave takes at one workgroup (both fast units, the last one the wave's
    last iteration): KGMA_E_BADBASE with the record and position the unfused step names; with the bytes restored the step is clean
    and its sums are the reference's."""
    monkeypatch.setenv("KGMA_PACK_WGS", "1")
    c = case(k, "long")
    lens, contigs, ref = c["lens"], c["contigs"], c["ref"]
    off, _ = word_offsets(lens)
    n = n_units(lens)
    last = max(u for u in range(n) if unit_kind(u, lens, k)[:2] == (13, "fast"))
    wave = last % WAVES
    second = wave + WAVES
    assert last + WAVES >= n and unit_kind(second, lens, k)[:2] == (0, "fast")
    spots = [(0, 32 * (second * UNIT_WORDS - off[0]) + 1234), (13, 32 * (last * UNIT_WORDS - off[13]) + 4001)]
    ctx = _lib.Context(0)
    g = None
    try:
        ctx.set_refs(k, [ref["RV"]], [ref["ws"]], [c["thr"]], [ref["N"]])
        g = ctx.genome_from_host(contigs)

        def step(fuse):
            monkeypatch.setenv("KGMA_FUSE_SUMS", "1" if fuse else "0")
            try:
                ctx.step_hits(g, _lib.MODE_SINGLE, fu.BUFF, 0, 0)
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
        clean = fu._collect(ctx, g, True, len(contigs))
        fu._check_sums(clean["sums"], c["sums"])
        assert np.array_equal(clean["cand"], c["cand"])
    finally:
        if g is not None:
            g.free()
        ctx.close()
