"""Host side of threshold calibration (no GPU): the plain-Python reference against the oracle, api.mutate_seq against the
reference's restatement of the mutation rule, sample_window_starts, and the off-lattice rule against the guard band of
kgma_set_refs (threshold_band: T = ceil(thr scale (1 - 2^-30)), T_hi = floor(thr scale (1 + 2^-30)))."""
import math
from fractions import Fraction

import numpy as np
import pytest

from kmergma_amd import api
from tests import calib_ref as cr
from tests.helpers import random_dna


def test_reference_D_equals_oracle(alp_ref, alp_locus):
    seqs = [r.sequence for r in alp_locus]
    want = cr.oracle_D(seqs, alp_ref["S"], alp_ref["N"], 6, alp_ref["ws"])
    assert sum(len(w) for w in want) > 1000
    for s, w in zip(seqs, want):
        assert cr.window_D(s, alp_ref["S"], alp_ref["N"], 6, alp_ref["ws"]) == w
    # (and the whole-sequence form agrees with the sliding one)
    s = seqs[0]
    W = alp_ref["ws"]
    for st in (0, 1, 777, len(s) - W):
        assert cr.D(s[st:st + W], alp_ref["S"], alp_ref["N"], 6) == want[0][st]


# ---- api.mutate_seq ---------------------------------------------------------------------------------------------------------

SEQ = random_dna(np.random.default_rng(11), 997) + b"acgtacgtttgacca"


@pytest.mark.parametrize("rate", [0.0, 2.0 ** -53, 0.0125, 0.25, 0.5, 1.0])
@pytest.mark.parametrize("stream", [(0, 0, 0), (3, 1, 2), (83, 80, 41)])
def test_mutate_seq_equals_reference(rate, stream):
    assert api.mutate_seq(SEQ, rate, seed=7, stream=stream) == cr.mutate(SEQ, rate, 7, stream)
    assert api.mutate_seq(SEQ, rate, stream=stream) == cr.mutate(SEQ, rate, 42, stream)


def test_mutate_seq_rates_0_and_1():
    assert api.mutate_seq(SEQ, 0.0) == SEQ
    out = api.mutate_seq(SEQ, 1.0)
    assert len(out) == len(SEQ)
    for a, b in zip(SEQ, out):
        assert chr(b) in cr.MUT[chr(a & 0xDF)]            # one of the three bases of MUT: never the residue itself
        assert b != (a & 0xDF)


def test_mutate_seq_substitutions_and_kept_bytes():
    out = api.mutate_seq(SEQ, 0.3, seed=5)
    changed = 0
    for a, b in zip(SEQ, out):
        if a == b:
            continue
        changed += 1
        assert chr(b) in cr.MUT[chr(a & 0xDF)]
    assert 0 < changed < len(SEQ)
    # unsubstituted residues keep their byte, lower case included
    assert any(a == b and chr(a).islower() for a, b in zip(SEQ, out))


def test_mutate_seq_rate_statistics():
    """100 000 residues at rate 0.25: the substituted count is Binomial(n, p), sigma = sqrt(n p (1 - p)) = 136.9; 6 sigma = 822."""
    s = random_dna(np.random.default_rng(12), 100_000)
    out = api.mutate_seq(s, 0.25)                              # the default seed, 42
    changed = sum(1 for a, b in zip(s, out) if a != b)
    print("substituted:", changed)
    assert abs(changed - 25_000) <= 822
    # the three alternatives are drawn about equally: each within 6 sigma of a third of the substitutions
    picks = {}
    for a, b in zip(s, out):
        if a != b:
            i = cr.MUT[chr(a)].index(chr(b))
            picks[i] = picks.get(i, 0) + 1
    for i in range(3):
        assert abs(picks[i] - changed / 3) <= 6 * math.sqrt(changed * (1 / 3) * (2 / 3))


def test_mutate_seq_streams_differ():
    outs = {api.mutate_seq(SEQ, 0.5, stream=st) for st in [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]}
    assert len(outs) == 5
    assert api.mutate_seq(SEQ, 0.5, seed=1) != api.mutate_seq(SEQ, 0.5, seed=2)


def test_mutate_seq_refuses_other_residues():
    with pytest.raises(KeyError):
        api.mutate_seq(b"ACGTNACGT", 0.0)
    with pytest.raises(ValueError):
        api.mutate_seq(b"ACGT", 1.5)


# ---- sample_window_starts ---------------------------------------------------------------------------------------------------

def test_sample_all_windows():
    c, s = api.sample_window_starts([10, 3, 8, 5], 5, 100, 1)
    assert list(zip(c.tolist(), s.tolist())) == [(0, p) for p in range(1, 7)] + [(2, p) for p in range(1, 5)] + [(3, 1)]
    assert c.dtype == np.int32 and s.dtype == np.int64
    # exactly n_samples valid windows: still every one of them once
    c2, s2 = api.sample_window_starts([10, 3, 8, 5], 5, 11, 1)
    assert c2.tolist() == c.tolist() and s2.tolist() == s.tolist()
    c3, s3 = api.sample_window_starts([3, 4], 5, 10, 1)
    assert c3.size == 0 and s3.size == 0
    c4, s4 = api.sample_window_starts([], 5, 10, 1)
    assert c4.size == 0 and s4.size == 0


def test_sample_draws():
    lens = [1000, 20, 289, 288, 5000, 290]
    W = 289
    c, s = api.sample_window_starts(lens, W, 700, 42)
    assert c.size == s.size == 700
    assert set(c.tolist()) <= {0, 2, 4, 5}                                   # records shorter than W are skipped
    for ci, si in zip(c.tolist(), s.tolist()):
        assert 1 <= si <= lens[ci] - W + 1                                   # every draw is a valid window
    pairs = list(zip(c.tolist(), s.tolist()))
    assert pairs == sorted(pairs)
    c2, s2 = api.sample_window_starts(lens, W, 700, 42)
    assert c2.tolist() == c.tolist() and s2.tolist() == s.tolist()           # the same seed, the same draws
    c3, s3 = api.sample_window_starts(lens, W, 700, 43)
    assert list(zip(c3.tolist(), s3.tolist())) != pairs
    # the draws are those of the documented generator, mapped through the cumulative counts
    counts = [max(L - W + 1, 0) for L in lens]
    want = []
    for d in sorted(np.random.default_rng(42).integers(0, sum(counts), 700).tolist()):
        r = 0
        while d >= counts[r]:
            d -= counts[r]
            r += 1
        want.append((r, d + 1))
    assert pairs == want


# ---- the off-lattice rule -------------------------------------------------------------------------------------------------------

def test_off_lattice_threshold_has_no_band(alp_ref):
    scale = 2.0 * 6 * alp_ref["N"] * alp_ref["N"]
    assert scale == 2 * 6 * alp_ref["N"] ** 2
    iscale = int(scale)
    rng = np.random.default_rng(5)
    ests = [20.0, 33.5, 41.7123, 1.0 / 3, 7 / iscale, 12345 / iscale] + (rng.random(200) * 60).tolist()
    band = Fraction(1, 2 ** 30)
    for est in ests:
        thr = api.off_lattice_threshold(est, scale)
        m = math.floor(est * scale)
        T = math.ceil(Fraction(thr) * iscale * (1 - band))
        T_hi = math.floor(Fraction(thr) * iscale * (1 + band))
        assert T == m + 1, est
        assert T_hi == m, est                                               # T_hi < T: the band is empty
