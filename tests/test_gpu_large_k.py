"""k = 1 and 11 <= k <= 15 on the device: the generic kernels' 32-bit counter form (k = 1) and wide hash form (k >= 11: 30-bit
keys, 32-bit counts, the KFV's value cached per entry, the KFV itself an open-addressed table of its non-zero entries), in LDS
up to KGMA_WIDE_LDS_MAX_NK = 2048 k-mers per window and in global memory beyond, scan and Float64 chain.  Against the oracles
(dense 4^k tables: k <= 13), and at k = 14, 15 (kgma_set_refs_sparse) against a sparse integer restatement in numpy."""
import os

import numpy as np
import pytest

from kmergma_amd import _lib, api, fasta, headers, refprep
from kmergma_amd.fasta import Record
from oracle import oracle as orc
from tests.helpers import hit_key, make_genome, mutate, random_dna
from tests.test_gpu_parity import REL_TOL, _assert_chain_single, _assert_omn_chain_parity, _assert_single_parity, _scan_single
from tests.test_gpu_wide import _family, _thr_for, _wide_genome

pytestmark = pytest.mark.gpu

LDS_MAX_NK = 2048


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def genes(data_dir):
    return [r.sequence.upper() for r in fasta.read_fasta(os.path.join(data_dir, "Alp_V_ref.fasta"))]


def _parity(ctx, contigs, ref, thr, buff=50):
    """_assert_single_parity, except that at k = 1 the default mode is held to the record-level form of the flag contract
    (_assert_default_flag_contract below): per record, the hits equal the Float64 oracle's up to the first one
    that stems from a dip flagged rounding-ambiguous.  At k = 1 the distance lattice is so coarse that a dip's minimum is a
    plateau of many windows of the same exact distance, and the library leaves every such tie flagged (the local replay does
    not decide ties at k = 1); which window the reference's rounding picks moves the hit and the hits that follow it in the
    record, so a record's hit COUNT may differ too -- always behind a flagged dip.  Steps (1) and (3) are the same at every k."""
    if ref["k"] != 1:
        return _assert_single_parity(ctx, contigs, ref, thr, buff)
    k, W, N, S = ref["k"], ref["ws"], ref["N"], ref["S"]
    hits, d, D1, _, _ = _scan_single(ctx, contigs, ref, thr, buff, dists=True, no_tie_resolve=True)
    ohi, oD, oD1 = orc.single_scan_int(contigs, S, N, k, W, orc.int_threshold(thr, k, N), buff, return_D=True)
    assert np.array_equal(D1, oD1)
    assert np.array_equal(d, oD / (2.0 * k * N * N))
    assert [hit_key(h) for h in hits] == [hit_key(h) for h in ohi]
    hits_f, _, _, stats, dips = _scan_single(ctx, contigs, ref, thr, buff)
    ohits, od = orc.single_scan(contigs, ref["RV"], k, W, thr, buff, return_dists=True)
    assert len(od) == len(d) and (len(d) == 0 or np.max(np.abs(d - od) / np.maximum(od, 1e-300)) < REL_TOL)
    _assert_default_flag_contract(hits_f, dips, ohits, stats["n_at_threshold"])
    _assert_chain_single(ctx, contigs, ref, thr, buff, None, ohits)
    return hits, None


def _assert_default_flag_contract(hits_f, dips, ohits, n_at_threshold):
    """Single engine, record-level form of the flag contract: a record whose hits differ from the Float64 oracle's has a flagged
    dip, and the first differing hit (ours or the oracle's) carries a flag or lies in a flagged dip (cmi: the hit's window - 1)."""
    kf, ko = [hit_key(h) for h in hits_f], [hit_key(h) for h in ohits]
    if kf == ko:
        return
    AMB = _lib.HIT_TIE | _lib.HIT_AT_THRESHOLD
    flagged = [x for x in dips if x["flags"] & AMB]
    for rec in sorted({k_[0] for k_ in set(kf) ^ set(ko)}):
        mine = [h for h in hits_f if h["contig"] == rec]
        theirs = [h for h in ohits if h["contig"] == rec]
        first = next(i for i, (a, b) in enumerate(zip([hit_key(h) for h in mine] + [None], [hit_key(h) for h in theirs] + [None])) if a != b)
        in_rec = [x for x in flagged if x["contig"] == rec]
        assert in_rec, f"record {rec}: hits differ although none of its dips is flagged"
        if n_at_threshold:
            continue
        cands = ([mine[first]] if first < len(mine) else []) + ([theirs[first]] if first < len(theirs) else [])

        def explained(h):
            return bool(h.get("flags", 0) & AMB) or any(x["start"] - 1 <= h["cmi"] <= x["end"] for x in in_rec)
        assert any(explained(h) for h in cands), (f"record {rec}: the first differing hit does not stem from a flagged dip: {cands}; "
                                                  f"flagged dips {[(x['start'], x['end'], x['flags']) for x in in_rec][:20]}")


def _genome(rng, W, base):
    contigs = _wide_genome(rng, W, [base])
    contigs[0] = contigs[0][:40_000] + b"C" * 5000 + b"GT" * 1200 + b"N" * 800 + contigs[0][40_000:]
    return contigs


@pytest.mark.parametrize("k", [1, 11, 12, 13])
def test_single_engine_large_k(ctx, k):
    """All three modes: integer distances bit-exact, Float64 within 1e-6, chain-mode hits identical to the Float64 oracle."""
    rng = np.random.default_rng(500 + k)
    base, ref = _family(rng, 289, k)
    contigs = _genome(rng, 289, base)
    thr = _thr_for(rng, ref)
    hits, _ = _parity(ctx, contigs, ref, thr)
    assert ctx.kernel_name().startswith("gen_kernel"), ctx.kernel_name()
    assert len(hits) >= 1


@pytest.mark.parametrize("k,W", [(11, 12), (1, 2), (11, 11 + LDS_MAX_NK - 1), (11, 11 + LDS_MAX_NK), (12, 3000)])
def test_window_boundaries(ctx, k, W):
    """W = k + 1 (two k-mers per window: a leaving k-mer entered by a lower lane of the same step), both sides of the LDS /
    global-memory boundary of the wide tables, and a window in global memory."""
    rng = np.random.default_rng(7 * W + k)
    if W < 40:
        base = random_dna(rng, 40)
        refs = [Record(f"g{i}", mutate(rng, base[:W], 0.2)) for i in range(5)]
        RV, ws, cons, (S, N) = refprep.gen_ref_ws_cons(refs, k, return_int=True)
        ref = dict(RV=RV, ws=ws, S=S, N=N, k=k)
        contigs = [random_dna(rng, 5000) + b"A" * 300 + b"AC" * 100 + b"N" * 90 + random_dna(rng, 700), random_dna(rng, W),
                   random_dna(rng, W + 1), b"acgtNNacgt" * 20]
    else:
        base, ref = _family(rng, W, k)
        contigs = _genome(rng, W, base)
    assert ref["ws"] == W
    thr = _thr_for(rng, ref)
    _parity(ctx, contigs, ref, thr)


@pytest.mark.parametrize("k", [1, 11])
def test_longest_window(ctx, k):
    """n = 65535 k-mers: at k = 1 a homopolymer longer than the window (every count n + 64 in flight in 32-bit counters), at
    k = 11 the wide table in global memory (2^17 entries per wave slot)."""
    W = 65_535 + k - 1
    rng = np.random.default_rng(65 + k)
    base, ref = _family(rng, W, k, n_refs=3)
    L = 3 * W
    a = bytearray(random_dna(rng, L))
    a[W // 2:W // 2 + W + 5000] = b"A" * (W + 5000)
    a[2 * W:2 * W + len(base)] = mutate(rng, base, 0.02)
    contigs = [bytes(a), random_dna(rng, W), random_dna(rng, W + 7)]
    thr = _thr_for(rng, ref)
    _parity(ctx, contigs, ref, thr)


@pytest.mark.parametrize("k", [11, 13])
def test_chain_values_every_window(ctx, k):
    rng = np.random.default_rng(31 + k)
    base, ref = _family(rng, 289, k)
    contigs = _genome(rng, 289, base)
    seq = contigs[0][:30_000] + contigs[0][-9000:]
    W = ref["ws"]
    nwin = len(seq) - W + 1
    ctx.set_refs(k, [ref["RV"]], [W], [30.0], [ref["N"]])
    g = ctx.genome_from_host([seq])
    try:
        got = g.chain_values(0, 1, [(1, nwin)])
        assert ctx.stats()["chain_device_pairs"] == 1
        _, od = orc.single_scan([seq], ref["RV"], k, W, 30.0, 50, return_dists=True)
        want = np.concatenate([[orc.kmer_dist_kfv(seq[:W], ref["RV"], k)], od])
        assert np.array_equal(got, want), f"first mismatch at window {int(np.argmax(got != want)) + 1}"
    finally:
        g.free()


@pytest.mark.parametrize("k", [11, 12])
def test_cluster_engine_large_k(ctx, k):
    """Three KFVs of different window sizes, one of them a general Float64 KFV, with the cluster engine's alignment feedback."""
    rng = np.random.default_rng(900 + k)
    fams = [_family(rng, L, k, n_refs=5) for L in (250, 289, 330)]
    RVs = [f[1]["RV"] for f in fams]
    RVs[1] = RVs[1] * (1.0 + 1e-3 * rng.random(RVs[1].size))        # not S/N: the Float64 form
    ws = [f[1]["ws"] for f in fams]
    Ns = [f[1]["N"] for f in fams]
    contigs, _ = make_genome(rng, [90_011, 40_000, max(ws) + k - 2, max(ws) + k], [f[0] for f in fams], n_plants_per_mb=150)
    thr = [float(np.round(0.6 * orc.kmer_dist_kfv(random_dna(rng, w), r, k), 1)) for r, w in zip(RVs, ws)]
    ctx.set_refs(k, RVs, ws, thr, Ns)
    gen = ctx.genome_from_host(contigs)
    try:
        fo, od = orc.omn_scan(contigs, RVs, k, ws, thr, 100, 1234, return_dists=True)
        ctx.scan(gen, _lib.MODE_OMN, 100, 1234, _lib.F_RETURN_DISTS, None)
        assert ctx.kernel_name().startswith("gen_kernel")
        for j in range(3):
            d = ctx.dists(j + 1)
            assert d.size == od[j].size
            assert float(np.max(np.abs(d - od[j]) / np.maximum(od[j], 1e-300))) < 1e-6
        ctx.scan(gen, _lib.MODE_OMN, 100, 1234, _lib.F_CHAIN_REPLAY, None)
        _assert_omn_chain_parity(ctx.hits(), ctx.dips(), ctx.stats(), fo)
        assert len(fo) >= 1
    finally:
        gen.free()


def _sparse_of(RV):
    keys = np.flatnonzero(RV).astype(np.uint32)
    return keys, RV[keys]


def _dips_dists(ctx, contigs):
    g = ctx.genome_from_host(contigs)
    try:
        ctx.scan(g, _lib.MODE_SINGLE, 50, 0, _lib.F_RETURN_DISTS | _lib.F_NO_TIE_RESOLVE, None)
        return [tuple(sorted(d.items())) for d in ctx.dips()], ctx.dists(1).tobytes()
    finally:
        g.free()


@pytest.mark.parametrize("k", [6, 12])
def test_sparse_entry_equals_dense(ctx, k):
    rng = np.random.default_rng(60 + k)
    base, ref = _family(rng, 289, k)
    contigs = _genome(rng, 289, base)
    thr = _thr_for(rng, ref)
    ctx.set_refs(k, [ref["RV"]], [ref["ws"]], [thr], None)
    dense = _dips_dists(ctx, contigs)
    keys, vals = _sparse_of(ref["RV"])
    ctx.set_refs_sparse(k, [keys], [vals], [ref["ws"]], [thr], None)
    assert _dips_dists(ctx, contigs) == dense
    with pytest.raises(_lib.KgmaError):
        ctx.set_refs_sparse(k, [keys[::-1]], [vals[::-1]], [ref["ws"]], [thr], None)
    with pytest.raises(_lib.KgmaError) as e:
        ctx.set_refs_sparse(16, [keys], [vals], [ref["ws"]], [thr], None)
    assert e.value.status == _lib.KGMA_E_UNSUPPORTED


def _codes(seq: bytes):
    t = np.full(256, 3, dtype=np.int64)
    for c, v in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
        t[c] = v
    return t[np.frombuffer(seq, dtype=np.uint8)]


def _kmers(seq: bytes, k: int):
    c = _codes(seq)
    n = len(c) - k + 1
    v = np.zeros(n, dtype=np.int64)
    for j in range(k):
        v = (v << 2) | c[j:j + n]
    return v


def _sparse_int_D(seq, skeys, sS, N, k, W):
    """D = sum_x (S[x] - N c[x])^2 of every window, from the window's distinct k-mers and the KFV's non-zero keys."""
    km = _kmers(seq, k)
    nk = W - k + 1
    Smap = dict(zip(skeys.tolist(), sS.tolist()))
    base = int(np.sum(sS.astype(object) ** 2))
    out = []
    for s in range(len(seq) - W + 1):
        u, c = np.unique(km[s:s + nk], return_counts=True)
        D = base
        for x, cx in zip(u.tolist(), c.tolist()):
            Sx = Smap.get(x, 0)
            D += (Sx - N * cx) ** 2 - Sx * Sx
        out.append(D)
    return np.asarray(out, dtype=np.int64)


@pytest.mark.parametrize("k", [14, 15])
def test_sparse_kfv_k14_k15(ctx, k):
    rng = np.random.default_rng(1400 + k)
    W, Nref = 240, 6
    base = random_dna(rng, W)
    refs = [mutate(rng, base, 0.03) for _ in range(Nref)]
    from collections import Counter
    cnt = Counter()
    for r in refs:
        cnt.update(_kmers(r, k).tolist())
    skeys = np.asarray(sorted(cnt), dtype=np.uint32)
    sS = np.asarray([cnt[x] for x in sorted(cnt)], dtype=np.int64)
    vals = sS / Nref
    contigs = [random_dna(rng, 3000) + mutate(rng, base, 0.02) + random_dna(rng, 2500) + b"A" * 400 + mutate(rng, base, 0.05)
               + random_dna(rng, 900), random_dna(rng, W), b"ACGTN" * 100]
    want = [_sparse_int_D(c, skeys.astype(np.int64), sS, Nref, k, W) for c in contigs]
    # threshold between a planted copy and random sequence
    scale = 2.0 * k * Nref * Nref
    thr = float(np.round(0.5 * (want[0][3000] + np.median(want[0][:2000])) / scale, 1))
    ctx.set_refs_sparse(k, [skeys], [vals], [W], [thr], [Nref])
    g = ctx.genome_from_host(contigs)
    try:
        ctx.scan(g, _lib.MODE_SINGLE, 50, 0, _lib.F_RETURN_DISTS | _lib.F_NO_TIE_RESOLVE, None)
        assert ctx.kernel_name().startswith("gen_kernel")
        d = ctx.dists(1)
        exp = np.concatenate([w[1:] for w in want]) / scale
        assert np.array_equal(d, exp)
        hits = ctx.hits()
        assert any(h["contig"] == 0 and h["lo"] <= 3000 + W // 2 <= h["hi"] for h in hits), hits
        ctx.scan(g, _lib.MODE_SINGLE, 50, 0, _lib.F_CHAIN_REPLAY, None)
        assert len(ctx.hits()) == len(hits)
    finally:
        g.free()


# kernel_name() of the configurations of test_generic_kernel_forced (Alp_V_ref.fasta, single engine) without KGMA_KERNEL, as the
# code chose them before k = 1 and k >= 11 were served: nothing changes for 2 <= k <= 10
KERNEL_BY_K = {2: "scan_kernel<2>", 3: "scan_kernel<3>", 4: "scan_kernel<4>", 5: "stream8_kernel<5>", 6: "stream8_kernel<6>",
               7: "stream8_kernel<7>", 8: "scan_kernel<8>", 9: "scan_kernel<9>", 10: "scan_kernel<10>"}


@pytest.mark.parametrize("k", sorted(KERNEL_BY_K))
def test_kernel_choice_unchanged(ctx, data_dir, genes, k, monkeypatch):
    monkeypatch.delenv("KGMA_KERNEL", raising=False)
    rng = np.random.default_rng(100 + k)
    contigs, _ = make_genome(rng, [40_000, 33_100, 500, 289, 288], genes, n_plants_per_mb=200)
    thr = {2: 300.0, 3: 200.0, 4: 120.0, 5: 60.0, 6: 30.0, 7: 25.0, 8: 22.0, 9: 20.0, 10: 18.0}[k]
    RV, ws, cons, (S, N) = refprep.gen_ref_ws_cons(os.path.join(data_dir, "Alp_V_ref.fasta"), k, return_int=True)
    ctx.set_refs(k, [RV], [ws], [thr], [N])
    g = ctx.genome_from_host(contigs)
    try:
        ctx.scan(g, _lib.MODE_SINGLE, 50, 0, 0, None)
        assert ctx.kernel_name() == KERNEL_BY_K[k]
    finally:
        g.free()


def test_find_genes_k11(ctx, data_dir):
    gp, rp = os.path.join(data_dir, "Loci.fasta"), os.path.join(data_dir, "Alp_V_ref.fasta")
    k = 11
    out = api.findGenes(genome_path=gp, ref_path=rp, k=k, do_align=False, verbose=False, ctx=ctx)
    RV, W, _, _ = refprep.gen_ref_ws_cons(rp, k, return_int=True)
    thr = refprep.estimate_optimal_threshold(RV, W, buffer=8.0)
    recs = fasta.read_fasta(gp)
    ohits, _ = orc.single_scan([r.sequence for r in recs], RV, k, W, thr, 50)
    assert len(out[0]) == len(ohits) and len(ohits) >= 1
    for rec, h in zip(out[0], ohits):
        assert f"MatchPos = {h['lo']}:{h['hi']}" in rec.description, rec.description


def test_find_genes_cluster_mode_k11(ctx, data_dir):
    gp, rp = os.path.join(data_dir, "Loci.fasta"), os.path.join(data_dir, "Alp_V_ref.fasta")
    k = 11
    out = api.findGenes_cluster_mode(genome_path=gp, ref_path=rp, k=k, do_align=False, verbose=False, ctx=ctx)
    RVs, ws, cons, invalids, ints = refprep.cluster_ref_API(rp, k, cutoffs=[7, 12, 20, 25], return_int=True)
    RVs, ws, cons, ints = refprep.eliminate_null_params(RVs, ws, cons, invalids, ints)
    thr = refprep.estimate_optimal_threshold(RVs, ws, buffer=7)
    recs = fasta.read_fasta(gp)
    ohits, _ = orc.omn_scan([r.sequence for r in recs], RVs, k, ws, thr, 100)
    assert len(out[0]) == len(ohits) and len(ohits) >= 1
    for rec, h in zip(out[0], ohits):
        assert f"MatchPos = {h['lo']}:{h['hi']}" in rec.description, rec.description
