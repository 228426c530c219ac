"""The inputs shared by test_strobe_calib_host.py (CPU) and test_gpu_strobe_calib.py: genomes, tables and window lists for the
strobemer calibration calls.  Nothing here calls the library under test; expected values come from tests/strobe_calib_ref.py.
Tables are strobe_cases.disc_table (N = 7, every bin non-zero, neighbouring bins and a bin's own first strobe told apart), so a
randstrobe counted in the wrong bin, a missing permanent item or a wrong one changes D."""
import functools

import numpy as np

from tests import strobe_cases as sc
from tests import strobe_calib_ref as scr
from tests.helpers import random_dna

SEED = 9300
DEFAULT_SETS = (((1, 2, 4, 5), 60), ((2, 3, 5, 5), 120), ((3, 4, 7, 5), 150))
STRIDE_CFG = (2, 3, 5, 5)
STRIDE_ITEMS = (2, 63, 64, 65, 255, 256, 257, 1025)
ONEBIN_ITEMS = 65_535


def _rng(*key):
    return np.random.default_rng([SEED] + [int(x) for x in key])


def disc_ref(cfg, W):
    return sc.ref_of(sc.disc_table(cfg[0]), sc.DISC_N, cfg, W)


def parity_sets():
    """(cfg, W): default-like parameters, and every edge set of strobe_cases (k = 16, w_min = 1, a zero score in every word of the
    modulus mask, ...) at 41 items per window."""
    return list(DEFAULT_SETS) + [(cfg, sc.k_of(cfg) + sc.SELECT_NK) for cfg, _sums, _seed in sc.SELECT_SETS]


@functools.lru_cache(maxsize=None)
def parity_case(cfg, W):
    """Three records cut from strobe_cases.select_genome: one longer than W (1300 residues: 'GA' + a run of N, a lower-case stretch,
    a homopolymer), one of exactly W + 1 and one of exactly W residues (over a homopolymer each)."""
    seed = next((sd for c, _u, sd in sc.SELECT_SETS if c == cfg), 0)
    g = sc.select_genome(seed)
    seqs = [g[0][600:1900], g[1][280:280 + W + 1], g[2][480:480 + W]]
    assert [len(x) for x in seqs] == [1300, W + 1, W] and b"N" in seqs[0] and seqs[0] != seqs[0].upper()
    return dict(cfg=cfg, W=W, seqs=seqs, ref=disc_ref(cfg, W))


def all_starts(seqs, W):
    c, s = [], []
    for i, r in enumerate(seqs):
        v = scr.valid_starts(len(r), W)
        c += [i] * len(v)
        s += list(v)
    return c, s


@functools.lru_cache(maxsize=None)
def stride_case(n_items):
    """W - k + 1 = n_items at s = 2; a record of W + 300 residues and one of W + 1; starts 1, 2 and L - W (and 1 of the short one)."""
    cfg = STRIDE_CFG
    W = n_items + sc.k_of(cfg) - 1
    rng = _rng(2, n_items)
    seqs = [random_dna(rng, W + 300), random_dna(rng, W + 1)]
    return dict(cfg=cfg, W=W, seqs=seqs, ref=disc_ref(cfg, W), contig=[0, 0, 0, 1], start=[1, 2, 300, 1])


@functools.lru_cache(maxsize=None)
def onebin_case():
    """65 535 randstrobes in ONE bin (a homopolymer record): the sum of the items' counts is n^2 = 4 294 836 225, beyond int32 and
    within 131 071 of 2^32; every lane's partial sum of it (n / 256 items of count n) is beyond 2^31 / 128 already."""
    cfg = STRIDE_CFG
    W = ONEBIN_ITEMS + sc.k_of(cfg) - 1
    seqs = [b"A" * (W + 3)]
    S = sc.disc_table(cfg[0]).copy()
    S[0] = 31
    return dict(cfg=cfg, W=W, seqs=seqs, ref=sc.ref_of(S, sc.DISC_N, cfg, W), contig=[0, 0, 0], start=[1, 2, 3])


@functools.lru_cache(maxsize=None)
def list_case():
    """Three records; lower case and N residues in the first, windows in all three."""
    cfg, W = (2, 3, 5, 5), 90
    rng = _rng(4)
    a = bytearray(random_dna(rng, 900))
    a[100:160] = bytes(a[100:160]).lower()
    a[300:420] = b"N" * 120
    a[500:503] = b"nnn"
    seqs = [bytes(a), random_dna(rng, 400), random_dna(rng, 250)]
    return dict(cfg=cfg, W=W, seqs=seqs, ref=disc_ref(cfg, W))


BAD_POS = 40                                   # 0-based residue of the bad symbol in bad_case's record 1


@functools.lru_cache(maxsize=None)
def bad_case():
    """cfg (2, 3, 5, 5), W = 46: k = 6, the permanent item is the randstrobe at 0-based residue 40 and reads residues 40 .. 45.
    Record 0 is clean; record 1 (300 residues) has an X at residue BAD_POS = 40: inside the first window and inside the permanent
    item of every later one, and outside residues q - 1 .. q + W - 2 (0-based) of every window with start q >= 42; record 2 (30
    residues) is shorter than W; record 3 (300 residues) has an X at residue 200."""
    cfg, W = (2, 3, 5, 5), 46
    rng = _rng(5)
    b = bytearray(random_dna(rng, 300))
    b[BAD_POS] = ord("X")
    d = bytearray(random_dna(rng, 300))
    d[200] = ord("X")
    seqs = [random_dna(rng, 300), bytes(b), random_dna(rng, 30), bytes(d)]
    return dict(cfg=cfg, W=W, seqs=seqs, ref=disc_ref(cfg, W))


MUT_RATES = (0.0, 0.0125, 0.5, 1.0)
MUT_TRIALS = 3
MUT_SEED = 42
MUT_SETS = ((1, 2, 4, 5), (2, 3, 5, 5), (3, 4, 7, 5))


@functools.lru_cache(maxsize=None)
def mutation_case(cfg):
    """Two sequences (700 residues with a lower-case stretch, 333 residues) and a table; also sequences of k - 1, k and k + 1."""
    k = sc.k_of(cfg)
    rng = _rng(6, cfg[0])
    a = bytearray(random_dna(rng, 700))
    a[50:90] = bytes(a[50:90]).lower()
    seqs = [bytes(a), random_dna(rng, 333)]
    short = [random_dna(rng, k - 1), random_dna(rng, k), random_dna(rng, k + 1)]
    return dict(cfg=cfg, seqs=seqs, short=short, ref=disc_ref(cfg, k + 1))
