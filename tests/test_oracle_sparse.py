"""The sparse oracle entry points (no 4^k table: what checks k = 14, 15) against the dense ones, bit for bit, at k <= 12.

Every hit field (dist included), every distance, every integer D and first-window D1 must be identical: the sparse functions
restate the same reference lines in the same operation order, and their first-window sum over the sorted union of the KFV's keys
and the window's k-mers is the dense left-to-right sum without its +0.0 terms."""
import numpy as np
import pytest

from kmergma_amd import refprep
from kmergma_amd.fasta import Record
from oracle import oracle as orc
from tests.helpers import (kmer_values, make_genome, mutate, random_dna, sparse_family, sparse_int_D,
                           thr_for_sparse)


def _family(rng, L, k, n_refs=7, rate=0.03):
    base = random_dna(rng, L)
    refs = [Record(f"g{i}", mutate(rng, base, rate)) for i in range(n_refs)]
    RV, ws, _, (S, N) = refprep.gen_ref_ws_cons(refs, k, return_int=True)
    return base, dict(RV=RV, ws=ws, S=S, N=N, k=k)


def _float_kfv(rng, RV, kind):
    """General Float64 KFVs: not S/N."""
    if kind == "perturbed":
        return RV * (1.0 + rng.uniform(-1.0, 1.0, RV.size) * 10.0 ** rng.uniform(-7, -3, RV.size))
    if kind == "negative":                        # some entries below zero, some zero entries made non-zero
        out = RV - 0.37 * (rng.random(RV.size) < 0.3) * RV.max()
        out[rng.integers(0, RV.size, 16)] = -1.0 / np.pi
        return out
    if kind == "pseudocount":                     # every entry non-zero
        return (RV + 0.01 / np.pi) / (1.0 + 0.01 / np.pi)
    raise ValueError(kind)


def _genome(rng, W, bases, k):
    """A record with planted copies and long A / T / N runs and lower case, records of W - 1, W, W + 1 residues."""
    L = 6 * W + 3000
    a = bytearray(random_dna(rng, L))
    pos = 300
    for b in bases:
        for rate in (0.02, 0.10):
            g = mutate(rng, b, rate)
            if pos + len(g) < L - 1500:
                a[pos:pos + len(g)] = g
                pos += len(g) + 250
    q = L - 1400
    a[q:q + 300] = b"A" * 300
    a[q + 400:q + 700] = b"T" * 300
    a[q + 800:q + 1000] = b"N" * 200
    a[q + 1050:q + 1100] = bytes(a[q + 1050:q + 1100]).lower()
    a[q + 1150:q + 1250] = b"n" * 50 + b"a" * 50
    return [bytes(a), random_dna(rng, W - 1), random_dna(rng, W), mutate(rng, bases[0], 0.04) + b"A", b"N" * (W + 3)]


def _same(a, b):
    """Hit lists equal field by field, dist to the bit."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert {f: v for f, v in x.items() if f != "dist"} == {f: v for f, v in y.items() if f != "dist"}
        if "dist" in x:
            assert np.float64(x["dist"]).tobytes() == np.float64(y["dist"]).tobytes()


def _both(dense, sparse):
    """Run both oracles; when the dense one raises (k = 1, cluster engine: the reference reads seq[i + ws] one residue past a
    record's end, OmnGenomeMiner.jl:97), the sparse one must raise the same error at the same place."""
    try:
        a = dense()
    except orc.OracleError as e0:
        with pytest.raises(orc.OracleError) as e1:
            sparse()
        assert (e0.code, e0.record, e0.position) == (e1.value.code, e1.value.record, e1.value.position)
        return None, None
    return a, sparse()


def _bits(x):
    return np.ascontiguousarray(x).tobytes()


def _single_case(rng, k, W):
    base, ref = _family(rng, W, k)
    return base, ref, _genome(rng, W, [base], k)


def _thr(rng, RV, k, W, frac=0.5):
    return float(np.round(frac * orc.kmer_dist_kfv(random_dna(rng, W), RV, k), 1))


@pytest.mark.parametrize("k", [1, 2, 6, 8, 11, 12])
def test_single_int_and_sn(k):
    rng = np.random.default_rng(70 + k)
    W = 120 if k >= 11 else 90
    base, ref, contigs = _single_case(rng, k, W)
    thr = _thr(rng, ref["RV"], k, W)
    N = ref["N"]
    T = orc.int_threshold(thr, k, N)
    sS = orc.to_sparse(ref["S"])
    h0, D0, D10 = orc.single_scan_int(contigs, ref["S"], N, k, W, T, 50, return_D=True)
    h1, D1, D11 = orc.single_scan_int_sparse(contigs, sS, N, k, W, T, 50, return_D=True)
    _same(h0, h1)
    assert np.array_equal(D0, D1) and np.array_equal(D10, D11)
    f0, d0 = orc.single_scan(contigs, ref["RV"], k, W, thr, 50, return_dists=True)
    f1, d1 = orc.single_scan_sparse(contigs, orc.to_sparse(ref["RV"]), k, W, thr, 50, return_dists=True)
    _same(f0, f1)
    assert _bits(d0) == _bits(d1)
    assert len(h0) >= 1 and len(f0) >= 1
    assert orc.kmer_dist_kfv_sparse(contigs[0][:W], orc.to_sparse(ref["RV"]), k) == orc.kmer_dist_kfv(contigs[0][:W], ref["RV"], k)


@pytest.mark.parametrize("k,kind", [(k, kind) for k in (1, 2, 6, 8, 11) for kind in ("perturbed", "negative", "pseudocount")]
                         + [(12, "pseudocount")])
def test_single_float64_kfv(k, kind):
    rng = np.random.default_rng(170 + k + len(kind))
    W = 120 if k >= 11 else 90
    base, ref, contigs = _single_case(rng, k, W)
    RV = _float_kfv(rng, ref["RV"], kind)
    _, d = orc.single_scan(contigs, RV, k, W, 0.0, 50, return_dists=True)
    thr = float(np.quantile(d, 0.02))                     # about 2 % of the windows below: dips on noise and on the plants
    f0, d0 = orc.single_scan(contigs, RV, k, W, thr, 50, return_dists=True)
    f1, d1 = orc.single_scan_sparse(contigs, orc.to_sparse(RV), k, W, thr, 50, return_dists=True)
    _same(f0, f1)
    assert _bits(d0) == _bits(d1)
    assert len(f0) >= 1


def _fake_align(contig, kfv, lo, hi, L):
    return lo + 3 + kfv, hi - 5


@pytest.mark.parametrize("align", [None, _fake_align])
@pytest.mark.parametrize("k", [1, 2, 6, 8, 11, 12])
def test_cluster_engine(k, align):
    """Three KFVs of different windows (one general Float64), genome_pos = 1234, with and without the aligner's feedback."""
    rng = np.random.default_rng(270 + k)
    lens = (100, 120, 135)
    fams = [_family(rng, L, k, n_refs=5) for L in lens]
    ws = [f[1]["ws"] for f in fams]
    contigs, _ = make_genome(rng, [9000, 4000, max(ws) + k - 2, max(ws) + k, max(ws) - 1, 300], [f[0] for f in fams],
                             n_plants_per_mb=900)
    Ns = [f[1]["N"] for f in fams]
    RVs = [f[1]["RV"] for f in fams]
    thr = [_thr(rng, r, k, w, 0.6) for r, w in zip(RVs, ws)]
    T = [orc.int_threshold(t, k, n) for t, n in zip(thr, Ns)]
    if k == 1:
        contigs.append(random_dna(rng, max(ws) + 40))     # the last record: the dense engine raises there, the sparse one must too
    I0, I1 = _both(lambda: orc.omn_scan_int(contigs, [f[1]["S"] for f in fams], Ns, k, ws, T, 100, 1234, return_D=True, align=align),
                   lambda: orc.omn_scan_int_sparse(contigs, [orc.to_sparse(f[1]["S"]) for f in fams], Ns, k, ws, T, 100, 1234,
                                                   return_D=True, align=align))
    RVs[1] = _float_kfv(rng, RVs[1], "perturbed")
    F0, F1 = _both(lambda: orc.omn_scan(contigs, RVs, k, ws, thr, 100, 1234, return_dists=True, align=align),
                   lambda: orc.omn_scan_sparse(contigs, [orc.to_sparse(r) for r in RVs], k, ws, thr, 100, 1234, return_dists=True,
                                               align=align))
    if k == 1:
        assert I0 is None and F0 is None
        contigs = contigs[:-1] + [random_dna(rng, 3)]     # (a record shorter than every window: the engines read nothing of it)
        I0, I1 = _both(lambda: orc.omn_scan_int(contigs, [f[1]["S"] for f in fams], Ns, k, ws, T, 100, 1234, return_D=True, align=align),
                       lambda: orc.omn_scan_int_sparse(contigs, [orc.to_sparse(f[1]["S"]) for f in fams], Ns, k, ws, T, 100, 1234,
                                                       return_D=True, align=align))
        F0, F1 = _both(lambda: orc.omn_scan(contigs, RVs, k, ws, thr, 100, 1234, return_dists=True, align=align),
                       lambda: orc.omn_scan_sparse(contigs, [orc.to_sparse(r) for r in RVs], k, ws, thr, 100, 1234,
                                                   return_dists=True, align=align))
    (h0, D0), (h1, D1) = I0, I1
    _same(h0, h1)
    assert all(np.array_equal(a, b) for a, b in zip(D0, D1))
    (f0, d0), (f1, d1) = F0, F1
    _same(f0, f1)
    assert all(_bits(a) == _bits(b) for a, b in zip(d0, d1))
    assert len(h0) >= 2 and len(f0) >= 2 and all(h["genome_pos"] >= 1234 for h in f0)


@pytest.mark.parametrize("k", [2, 6, 11, 12])
def test_key_range_ends(k):
    """KFV entries at key 0 (poly-A) and 4^k - 1 (poly-T, and what a run of N reads as)."""
    rng = np.random.default_rng(370 + k)
    W = 110
    base, ref = _family(rng, W, k)
    S = ref["S"].copy()
    S[0] += 3
    S[-1] += 5
    N = ref["N"]
    RV = S * (1.0 / N)
    a = bytearray(random_dna(rng, 4000))
    a[500:500 + len(base)] = mutate(rng, base, 0.02)
    a[1000:1400] = b"A" * 400
    a[1600:2000] = b"T" * 400
    a[2200:2500] = b"N" * 300
    a[2600:2700] = b"a" * 50 + b"tn" * 25
    a[3000:3000 + len(base)] = mutate(rng, base, 0.05)
    contigs = [bytes(a), b"A" * (W - 1), b"T" * W, b"N" * (W + 1), b"n" * 3 + random_dna(rng, W)]
    sS = orc.to_sparse(S)
    assert sS[0][0] == 0 and sS[0][-1] == 4 ** k - 1
    thr = _thr(rng, RV, k, W)
    T = orc.int_threshold(thr, k, N)
    h0, D0, D10 = orc.single_scan_int(contigs, S, N, k, W, T, 50, return_D=True)
    h1, D1, D11 = orc.single_scan_int_sparse(contigs, sS, N, k, W, T, 50, return_D=True)
    _same(h0, h1)
    assert np.array_equal(D0, D1) and np.array_equal(D10, D11)
    for R in (RV, _float_kfv(rng, RV, "negative")):
        f0, d0 = orc.single_scan(contigs, R, k, W, thr, 50, return_dists=True)
        f1, d1 = orc.single_scan_sparse(contigs, orc.to_sparse(R), k, W, thr, 50, return_dists=True)
        _same(f0, f1)
        assert _bits(d0) == _bits(d1)
    g0, e0 = orc.omn_scan(contigs, [RV], k, [W], [thr], 50, 7, return_dists=True)
    g1, e1 = orc.omn_scan_sparse(contigs, [orc.to_sparse(RV)], k, [W], [thr], 50, 7, return_dists=True)
    _same(g0, g1)
    assert _bits(e0[0]) == _bits(e1[0])
    assert len(h0) >= 1


def test_golden_scan_through_the_sparse_path(golden, alp_ref, alp_clusters, loci, alp_locus):
    from kmergma_amd import headers
    sref = orc.to_sparse(alp_ref["RV"])
    seqs = [r.sequence for r in loci]
    g = golden["scan"]["single_no_align"]
    hits, _ = orc.single_scan_sparse(seqs, sref, 6, alp_ref["ws"], g["thr"], g["buff"])
    assert len(hits) == g["n_hits"]
    for idx, expected in g["headers"].items():
        h = hits[int(idx) - 1]
        assert headers.single_header(loci[h["contig"]].identifier, h["dist"], h["lo"], h["hi"], h["genome_pos"]) == expected
    g = golden["scan"]["single_dists"]
    hits, d = orc.single_scan_sparse(seqs, sref, 6, alp_ref["ws"], g["thr"], g["buff"], return_dists=True)
    assert len(d) == g["n_dists"] and round(float(d.mean())) == g["round_mean"] and len(hits) == g["n_hits"]
    g = golden["scan"]["omn_buff200"]
    hits, _ = orc.omn_scan_sparse([r.sequence for r in alp_locus], [orc.to_sparse(r) for r in alp_clusters["KFVs"]], 6,
                                  alp_clusters["ws"], g["thr_vec"], g["buff"])
    assert [[headers.julia_round2(h["dist"]), h["kfv"]] for h in hits] == g["dist_kfv"]
    assert [h["cmi"] for h in hits] == [6851, 23690, 33843]


@pytest.mark.parametrize("k", [6, 11])
def test_sparse_family_is_gen_ref_ws_cons(k):
    """tests.helpers.sparse_family draws what test_gpu_wide._family draws and returns its non-zero entries."""
    _, dense = _family(np.random.default_rng(5), 150, k)
    _, sp = sparse_family(np.random.default_rng(5), 150, k)
    keys, S = orc.to_sparse(dense["S"])
    assert np.array_equal(sp["keys"], keys) and np.array_equal(sp["S"], S) and sp["N"] == dense["N"] and sp["ws"] == dense["ws"]
    assert _bits(sp["vals"]) == _bits(dense["RV"][keys])
    rng0, rng1 = np.random.default_rng(9), np.random.default_rng(9)
    assert thr_for_sparse(rng1, sp) == float(np.round(0.5 * orc.kmer_dist_kfv(random_dna(rng0, 150), dense["RV"], k), 1))


def test_numpy_restatement_k14():
    """A third, independent check at k = 14 (no dense oracle exists there): the numpy per-window restatement."""
    rng = np.random.default_rng(1414)
    k, W = 14, 80
    base, ref = sparse_family(rng, W, k, n_refs=6)
    seq = random_dna(rng, 300) + mutate(rng, base, 0.02) + b"A" * 120 + b"N" * 30 + random_dna(rng, 200) + b"T" * 90
    want = sparse_int_D(seq, ref["keys"], ref["S"], ref["N"], k, W)
    _, D, D1 = orc.single_scan_int_sparse([seq], (ref["keys"], ref["S"]), ref["N"], k, W, 1, 50, return_D=True)
    assert D1[0] == want[0] and np.array_equal(D, want[1:])
    kk = kmer_values(seq, k)
    assert kk.min() == 0 and kk.max() == 4 ** k - 1


def test_errors_match_dense():
    rng = np.random.default_rng(3)
    base, ref = _family(rng, 60, 6)
    contigs = [random_dna(rng, 500), random_dna(rng, 100) + b"R" + random_dna(rng, 100)]
    with pytest.raises(orc.OracleError) as e0:
        orc.single_scan(contigs, ref["RV"], 6, 60, 10.0)
    with pytest.raises(orc.OracleError) as e1:
        orc.single_scan_sparse(contigs, orc.to_sparse(ref["RV"]), 6, 60, 10.0)
    assert (e0.value.code, e0.value.record, e0.value.position) == (e1.value.code, e1.value.record, e1.value.position)
    keys, vals = orc.to_sparse(ref["RV"])
    with pytest.raises(orc.OracleError):
        orc.single_scan_sparse(contigs[:1], (keys[::-1], vals[::-1]), 6, 60, 10.0)
