"""The shape matrix of the prefilter tests (kmergma.jl_amd/csrc/kgma_filter.hip), shared by test_filter_bound.py (CPU) and
test_gpu_filter.py: for k in KS, N in NS and nk in NKS a reference family, a genome and a threshold, W = nk + k - 1.

k and the entry width select the kernel's instantiation: N = 7 keeps every S below 256 (one byte per entry), N = 300 does not (two
bytes); k = 6 with two bytes is the single-copy table.  nk selects nblk = (nk + 14) // 16 + 1, the distance in lanes between the two
prefix values of a granule's sum: 2, 2, 2, 3, 4, 8, 19, 25 for NKS.
Nothing here calls the library under test: distances come from the integer oracle."""
import functools

import numpy as np

from oracle import oracle as orc
from tests import filter_ref
from tests.helpers import kmer_values, mutate, random_dna

KS = (5, 6)
NS = (7, 300)
NKS = (2, 16, 17, 18, 34, 100, 284, 383)
MATRIX = [(k, N, nk) for k in KS for N in NS for nk in NKS]
CHAIN_NK = 100                          # the chain replay runs too at every nk up to this one
BUFF = 50
LONG, PLANT_EVERY, TANDEM_AT, TANDEM_WINDOWS = 200_000, 20_000, 110_000, 2_400
SEED = 6200


def cell_id(cell):
    return "k%d-N%d-nk%d" % cell


def nblk_of(nk):
    return (nk + 14) // 16 + 1


def form_of(k, Smax):
    """kgma_filter_stats.form of the instantiation launch_filter picks: S entry bytes | table copies << 8."""
    es = 1 if Smax < 256 else 2
    return es | ((1 if (k == 6 and es == 2) else 32) << 8)


def ref_from_S(S, N, k, W, base):
    S = np.asarray(S, dtype=np.int64)
    return dict(S=S, N=N, RV=S * (1.0 / N), ws=W, k=k, base=base)       # (RV: refprep's form)


def family(k, N, nk, seed=SEED):
    """A random base of W residues and N copies mutated at 3 %: S their k-mer counts."""
    W = nk + k - 1
    rng = np.random.default_rng([seed, k, N, nk])
    base = random_dna(rng, W)
    S = np.zeros(4 ** k, dtype=np.int64)
    for _ in range(N):
        S += np.bincount(kmer_values(mutate(rng, base, 0.03), k), minlength=4 ** k)
    return ref_from_S(S, N, k, W, base)


def plant_of(rng, base, nk):
    """Exact copies for nk < 34, copies mutated at 4 % otherwise."""
    return base if nk < 34 else mutate(rng, base, 0.04)


def genome(k, nk, base, seed=SEED, plant_rate=None):
    """(contigs, plants): one long record with the base planted every PLANT_EVERY residues and one tandem run of it, and short
    records of W - 1 ... 500 residues, each ending in a planted base where it has a window.  plants: (record, 0-based window).
    plant_rate: mutate every plant at that rate instead of plant_of's rule (the tandem run stays exact)."""
    W = nk + k - 1
    rng = np.random.default_rng([seed + 1, k, nk])
    plant = (lambda: mutate(rng, base, plant_rate)) if plant_rate is not None else (lambda: plant_of(rng, base, nk))
    a = bytearray(random_dna(rng, LONG))
    plants = []
    for pos in range(5_000, LONG, PLANT_EVERY):
        a[pos:pos + W] = plant()
        plants.append((0, pos))
    run = base * (-(-(TANDEM_WINDOWS + W) // W))
    a[TANDEM_AT:TANDEM_AT + len(run)] = run
    assert len(a) == LONG and len(run) < 10_000                        # (the next plant is 15 000 residues on)
    contigs = [bytes(a)]
    for L in (W, W + 15, W + 16, W - 1, W + 17, W + 63, W + 64, W + 65, 500):
        if L < W:
            contigs.append(random_dna(rng, L))                            # no window: it sits between the others
            continue
        contigs.append(random_dna(rng, L - W) + plant())                  # the record's last window is a plant
        plants.append((len(contigs) - 1, L - W))
    return contigs, plants


def exact_D(contigs, S, N, k, W):
    """Exact D of every window of every record (the integer oracle: the first window's D apart, then one value per later window)."""
    _, D, D1 = orc.single_scan_int(contigs, S, N, k, W, 1, BUFF, return_D=True)
    out, at = [], 0
    for c, seq in enumerate(contigs):
        nwin = len(seq) - W + 1
        if nwin <= 0:
            out.append(np.zeros(0, dtype=np.int64))
            continue
        out.append(np.concatenate([[D1[c]], D[at:at + nwin - 1]]))
        at += nwin - 1
    assert at == D.size
    return out


def planted_max(D, plants, k, N):
    """The largest exact distance of a planted window, in the scans' Float64 units (D / 2kN^2)."""
    return max(int(D[c][s]) for c, s in plants) / (2.0 * k * N * N)


def threshold(D, plants, k, N):
    return round(1.25 * planted_max(D, plants, k, N) + 0.05, 2)


def longest_run(cand, record=0):
    """Length of the longest run of consecutive candidate granules of one record."""
    g = cand[cand[:, 0] == record, 1]
    if g.size == 0:
        return 0
    cuts = np.nonzero(np.diff(g) != 1)[0]
    edges = np.concatenate([[-1], cuts, [g.size - 1]])
    return int(np.max(np.diff(edges)))


@functools.lru_cache(maxsize=None)
def cell(k, N, nk):
    """Everything the tests of one matrix cell share, computed once and never modified: ref, contigs, plants, D (exact, per
    record), thr, T, T_hi, U, want (the numpy candidate set)."""
    ref = family(k, N, nk)
    W = ref["ws"]
    contigs, plants = genome(k, nk, ref["base"])
    D = exact_D(contigs, ref["S"], N, k, W)
    thr = threshold(D, plants, k, N)
    T, T_hi = filter_ref.threshold_band(thr, k, N)
    U = filter_ref.bound_U(ref["S"], N, k, W, T, T_hi)
    want = filter_ref.candidates(contigs, ref["S"], k, W, U)
    return dict(ref=ref, W=W, contigs=contigs, plants=plants, D=D, thr=thr, T=T, T_hi=T_hi, U=U, want=want)
