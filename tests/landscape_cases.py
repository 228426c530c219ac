"""Cases of the distance landscape (kgma_dist_bins / kgma_dist_sweep), shared by test_landscape_host.py (CPU: the model on exact
distances) and test_gpu_landscape.py (device against model).  Nothing here calls the library under test.

The kernels' geometry, restated from DESIGN.md section 5i (the tests do not read it from the library): the bin kernel takes 2 values
per lane, 128 per wave stretch, 512 per wave and 2048 per workgroup; the sweep kernel 128 per wave stretch, 2048 per wave and 8192
per workgroup and round.  Value i of a record is window start i + 2.

One reference (k = 6, windows of 65 residues, 5 mutated copies of a random base) and four genomes of a few kilobases each:
  edges   records without a window (L < W), with one window (no value), with 2, 3, 64 and 65 windows, then a record of 2500 values
          with two planted genes;
  tiny    300 records of 1 .. 3 values in a row (many record boundaries inside one wave stretch), then a record of 700 values;
  homo    a homopolymer record (every window at one distance: every bin's argmin is its first window) between two random records;
  long    one record of 19 000 values.  The exact base stands at value indices EQUAL_AT: twice inside one wave stretch, in another
          wave of the same workgroup, in the next workgroup and beyond the sweep's workgroup stretch -- the same smallest distance
          in different lanes, waves and workgroups.  A mutated copy stands 20 values behind every multiple of 2048, so the
          distances fall all through a wave's, a workgroup's and a round's edge: from them boundary_thresholds() makes runs that
          begin exactly on the last value before such an edge and on the first after it.
Each property a case is there for is asserted by the function that builds it, on the distances it is given (the host test passes
exact ones, the GPU test the device's)."""
import functools

import numpy as np

from tests import filter_cases as fc
from tests.helpers import mutate, random_dna

SEED = 9300
K, N_REFS, NK = 6, 5, 60
W = NK + K - 1
STRETCH, BINS_WAVE, BINS_WG, SWEEP_WAVE, SWEEP_WG = 128, 512, 2048, 2048, 8192
LONG_VALUES = 19_000
EQUAL_AT = (130, 195, 700, 2048 + 500, 8192 + 2048 + 300)
BINS = (1, 2, 63, 64, 65, 127, 128, 129, BINS_WG - 1, BINS_WG, BINS_WG + 1, 10 ** 7)
GENOMES = ("edges", "tiny", "homo", "long")
MAX_THRESHOLDS = 4096


@functools.lru_cache(maxsize=None)
def ref():
    return fc.family(K, N_REFS, NK, seed=SEED)


def _plant(a, value_index, seq):
    """seq becomes the window of value `value_index` (window start value_index + 2: residue offset value_index + 1)."""
    a[value_index + 1:value_index + 1 + len(seq)] = seq


@functools.lru_cache(maxsize=None)
def genome(name):
    base = ref()["base"]
    rng = np.random.default_rng([SEED, GENOMES.index(name)])
    if name == "edges":
        recs = [random_dna(rng, L) for L in (W - 1, W, W + 1, W + 2, W + 63, W + 64)]
        a = bytearray(random_dna(rng, W + 2500))
        _plant(a, 400, mutate(rng, base, 0.03))
        _plant(a, 1900, mutate(rng, base, 0.08))
        return recs + [bytes(a)]
    if name == "tiny":
        return [random_dna(rng, W + int(n)) for n in rng.integers(1, 4, size=300)] + [random_dna(rng, W + 700)]
    if name == "homo":
        return [random_dna(rng, W + 300), b"A" * (W + 700), random_dna(rng, W + 900)]
    a = bytearray(random_dna(rng, W + LONG_VALUES))
    for i, edge in enumerate(range(SWEEP_WAVE, LONG_VALUES - 200, SWEEP_WAVE)):
        _plant(a, edge + 20, mutate(rng, base, 0.06 + 0.03 * (i % 6)))       # the distances fall all through the edge
    for at in EQUAL_AT:
        _plant(a, at, base)
    return [bytes(a)]


@functools.lru_cache(maxsize=None)
def exact(name):
    """(d, offset): the exact distances D / (2 k N^2) of a genome (what an integer KFV's scan writes) and their layout."""
    r = ref()
    contigs = genome(name)
    D = fc.exact_D(contigs, r["S"], r["N"], K, W)
    d = np.concatenate([x[1:] for x in D]) / (2.0 * K * r["N"] * r["N"])
    offset = np.concatenate([[0], np.cumsum([max(len(c) - W, 0) for c in contigs])]).astype(np.int64)
    assert d.size == offset[-1]
    return d, offset


def check_genome(name, d, offset):
    """What the genome is there for, on the distances given."""
    n = np.diff(offset)
    if name == "edges":
        assert n[:6].tolist() == [0, 0, 1, 2, 63, 64]
    elif name == "tiny":
        assert set(n[:300].tolist()) == {1, 2, 3} and offset[300] > 4 * STRETCH          # boundaries all through several wave stretches
    elif name == "homo":
        x = d[offset[1]:offset[2]]
        assert x.size == 700 and np.all(x == x[0])
    else:
        assert n.tolist() == [LONG_VALUES]
        at = np.asarray(EQUAL_AT)
        assert np.all(d[at] == d.min()) and np.count_nonzero(d == d.min()) == at.size    # the smallest distance, and nowhere else
        assert at[0] // STRETCH == at[1] // STRETCH and at[0] // 2 != at[1] // 2           # two lanes of one wave stretch
        assert at[2] // BINS_WG == at[0] // BINS_WG and at[2] // BINS_WAVE != at[0] // BINS_WAVE
        assert at[3] // BINS_WG != at[0] // BINS_WG and at[4] // SWEEP_WG != at[0] // SWEEP_WG


def boundary_thresholds(d, offset):
    """Thresholds t = d[B - 1] for values B on either side of a wave's, a workgroup's and a round's boundary where d[B] < d[B - 1]:
    a run of values below t begins exactly at B (d[B - 1] itself is not below).  Returns (thresholds, the Bs they were made for)."""
    edges = sorted({e + s for unit in (STRETCH, SWEEP_WAVE, SWEEP_WG) for e in range(unit, d.size, unit) for s in (-1, 0)})
    starts = set(offset[:-1].tolist())
    at = [B for B in edges if B not in starts and d[B] < d[B - 1]]
    thr = np.unique(d[np.asarray(at, dtype=np.int64) - 1])
    assert any(B % SWEEP_WG == 0 for B in at) and any(B % SWEEP_WG == SWEEP_WG - 1 for B in at), "no run on a round's edge"
    assert any(B % SWEEP_WAVE == 0 for B in at) and any(B % SWEEP_WAVE == SWEEP_WAVE - 1 for B in at), "no run on a wave's edge"
    return thr[:MAX_THRESHOLDS], at


def sweep_cases(d, offset):
    """name -> thresholds, for one genome's distances: 1, 2 and 4096 thresholds; all below every value, all above, on values."""
    lo, hi = float(d.min()), float(d.max())
    values = np.unique(d)
    out = {
        "1-under": np.array([np.nextafter(lo, -np.inf)]),
        "1-at-min": np.array([lo]),                                     # the smallest value lies ON the threshold: not below
        "2-under": np.array([lo - 1.0, np.nextafter(lo, -np.inf)]),
        "1-over": np.array([np.nextafter(hi, np.inf)]),
        "1-at-max": np.array([hi]),
        "2-over": np.array([np.nextafter(hi, np.inf), hi + 1.0]),
        "2-split": np.array([float(np.median(d)), np.nextafter(hi, np.inf)]),
        "on-values": values[np.unique(np.linspace(0, values.size - 1, min(values.size, 700)).astype(np.int64))],
    }
    if hi > lo:
        out["4096-even"] = np.linspace(np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf), MAX_THRESHOLDS)
        fill = np.linspace(lo - 1.0, hi + 1.0, MAX_THRESHOLDS)
        out["4096-with-values"] = np.unique(np.concatenate([values[:MAX_THRESHOLDS // 2], fill]))[:MAX_THRESHOLDS]   # values among the rest
    for t in out.values():
        assert 1 <= t.size <= MAX_THRESHOLDS and np.all(np.isfinite(t)) and np.all(np.diff(t) > 0)
    return out
