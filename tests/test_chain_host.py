"""The host-side Float64 chain replay (kgma_chain.cpp, what KGMA_F_CHAIN_REPLAY runs) against the oracle's
reference-order distances: the same values bit for bit, at any set of sampled windows.  No GPU needed."""
import numpy as np
import pytest

from kmergma_amd import _lib
from oracle import oracle as orc
from tests.helpers import random_dna


def test_chain_values_equal_oracle_distances(alp_ref):
    rng = np.random.default_rng(5)
    k, W, RV = 6, alp_ref["ws"], alp_ref["RV"]
    a = bytearray(random_dna(rng, 60_000))
    a[1000:1600] = b"A" * 600
    a[7000:7500] = b"n" * 500
    a[20000:20400] = b"ACGT" * 100
    seq = bytes(a)
    _, od = orc.single_scan([seq], RV, k, W, 30.0, 50, return_dists=True)      # windows 2 .. L-W+1
    nwin = len(seq) - W + 1
    assert len(od) == nwin - 1
    full = _lib.host_chain_values(seq, RV, k, W, [(1, nwin)])
    assert len(full) == nwin
    assert full[0] == orc.kmer_dist_kfv(seq[:W], RV, k)                         # first window: (1/2k) * sqeuclidean, left to right
    assert np.array_equal(full[1:], od)                                        # bit for bit, 59 711 windows
    iv = [(1, 1), (17, 40), (41, 41), (999, 2000), (nwin - 3, nwin)]
    part = _lib.host_chain_values(seq, RV, k, W, iv)
    want = np.concatenate([full[lo - 1:hi] for lo, hi in iv])
    assert np.array_equal(part, want)


def test_chain_values_cluster_kfvs_and_other_k(alp_clusters, data_dir):
    import os
    from kmergma_amd import refprep
    rng = np.random.default_rng(6)
    seq = random_dna(rng, 9000)
    c = alp_clusters
    thr = [37, 33, 38, 34, 28]
    _, od = orc.omn_scan([seq], c["KFVs"], 6, c["ws"], thr, 50, 0, return_dists=True)
    for j, (kfv, w) in enumerate(zip(c["KFVs"], c["ws"])):
        n = len(od[j])                                                         # iterations of the cluster engine's loop
        v = _lib.host_chain_values(seq, kfv, 6, w, [(2, n + 1)])
        assert np.array_equal(v, od[j])
    for k in (4, 8):
        RV, ws, cons, _ = refprep.gen_ref_ws_cons(os.path.join(data_dir, "Alp_V_ref.fasta"), k, return_int=True)
        _, od1 = orc.single_scan([seq], RV, k, ws, 30.0, 50, return_dists=True)
        assert np.array_equal(_lib.host_chain_values(seq, RV, k, ws, [(2, len(seq) - ws + 1)]), od1)


def _edge_record(rng, W):
    a = bytearray(random_dna(rng, 6000))
    a[500:800] = b"A" * 300
    a[1500:1700] = b"N" * 100 + b"n" * 100
    a[2500:2800] = b"AC" * 150
    return a


@pytest.mark.parametrize("k", [3, 5, 6, 7, 8])
@pytest.mark.parametrize("nk", [2, 3, 15, 16, 17, 33, 62, 63, 64, 65, 66])
def test_chain_values_short_windows(k, nk):
    """Windows of 2 ... 66 k-mers (the host chain walks n_pos = n_valid + nk - 1 positions): every window of a 6 kb record with a
    homopolymer, an N run, a dinucleotide repeat and a planted base, bit for bit; then sampled windows and the records of W and W + 1."""
    from tests import filter_cases as fc
    ref = fc.family(k, 7, nk)
    W, RV = ref["ws"], ref["RV"]
    rng = np.random.default_rng([77, k, nk])
    a = _edge_record(rng, W)
    a[4000:4000 + W] = ref["base"]
    seq = bytes(a)
    _, od = orc.single_scan([seq], RV, k, W, 30.0, 50, return_dists=True)
    nwin = len(seq) - W + 1
    assert len(od) == nwin - 1
    full = _lib.host_chain_values(seq, RV, k, W, [(1, nwin)])
    assert full[0] == orc.kmer_dist_kfv(seq[:W], RV, k)
    assert np.array_equal(full[1:], od), "first mismatch at window %d" % (int(np.argmax(full[1:] != od)) + 2)
    iv = [(1, 1), (2, 3), (63, 66), (67 + nk, 68 + nk), (4001, 4001), (nwin - 1, nwin)]
    assert np.array_equal(_lib.host_chain_values(seq, RV, k, W, iv), np.concatenate([full[lo - 1:hi] for lo, hi in iv]))
    for rec in (ref["base"], seq[3999:4000 + W]):                       # records of one and of two windows
        _, o = orc.single_scan([rec], RV, k, W, 30.0, 50, return_dists=True)
        want = np.concatenate([[orc.kmer_dist_kfv(rec[:W], RV, k)], o])
        assert want.size == len(rec) - W + 1
        assert np.array_equal(_lib.host_chain_values(rec, RV, k, W, [(1, want.size)]), want)


def test_chain_values_cluster_short_windows():
    """Cluster engine, ws = 20, 21, 68 at k = 6: the running value of every loop iteration of every KFV."""
    from tests import filter_cases as fc
    k, ws = 6, [20, 21, 68]
    fams = [fc.family(k, 4 + j, w - k + 1, seed=900 + j) for j, w in enumerate(ws)]
    rng = np.random.default_rng(78)
    a = _edge_record(rng, max(ws))
    for j, f in enumerate(fams):
        a[3500 + 500 * j:3500 + 500 * j + ws[j]] = f["base"]
    seq = bytes(a)
    thr = [float(orc.kmer_dist_kfv(random_dna(rng, w), f["RV"], k)) * 0.8 for f, w in zip(fams, ws)]
    _, od = orc.omn_scan([seq], [f["RV"] for f in fams], k, ws, thr, 20, 55, return_dists=True)
    for j, (f, w) in enumerate(zip(fams, ws)):
        n = len(od[j])
        assert n > 5000
        v = _lib.host_chain_values(seq, f["RV"], k, w, [(2, n + 1)])
        assert np.array_equal(v, od[j]), "KFV %d: first mismatch at iteration %d" % (j + 1, int(np.argmax(v != od[j])) + 1)


def test_chain_values_argument_checks(alp_ref):
    import pytest
    seq = b"ACGT" * 200
    with pytest.raises(_lib.KgmaError):
        _lib.host_chain_values(seq, alp_ref["RV"], 6, 289, [(5, 3)])
    with pytest.raises(_lib.KgmaError):
        _lib.host_chain_values(seq, alp_ref["RV"], 6, 289, [(1, 10 ** 6)])
    with pytest.raises(_lib.KgmaError):
        _lib.host_chain_values(b"ACGR" * 200, alp_ref["RV"], 6, 289, [(1, 5)])
