"""k = 1 and 11 <= k <= 15 on the device: the generic kernels' 32-bit counter form (k = 1) and wide hash form (k >= 11: 30-bit
keys, 32-bit counts, the KFV's value cached per entry, the KFV itself an open-addressed table of its non-zero entries), in LDS
up to KGMA_WIDE_LDS_MAX_NK = 2048 k-mers per window and in global memory beyond, scan and Float64 chain.  Against the oracles
(dense 4^k tables: k <= 13), and at k = 14, 15 (kgma_set_refs_sparse) against the oracle's sparse entry points (no 4^k table) and
a sparse integer restatement in numpy.  Each wide-table case shows the count mode it reached: the generic path's KGMA_GEOM_DEBUG
line (k, cmode, log2m, rebuild period) and, at the LDS / global-memory boundary, a second run with KGMA_WIDE_LDS_NK=0."""
import os
import re

import numpy as np
import pytest

from kmergma_amd import _lib, api, fasta, headers, refprep
from kmergma_amd.fasta import Record
from oracle import oracle as orc
from tests.helpers import (hit_key, kmer_values, make_genome, mutate, random_dna, sparse_family, sparse_int_D,
                           thr_for_sparse)
from tests.test_gpu_parity import (REL_TOL, _assert_chain_single, _assert_omn_chain_parity, _assert_omn_default_parity,
                                   _assert_single_parity, _scan_single)
from tests.test_gpu_wide import _assert_float_single, _family, _float_kfvs, _thr_for, _wide_genome

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


@pytest.mark.parametrize("k,form", [(12, "float64"), (13, "sn"), (13, "float64")])
def test_sparse_entry_equals_dense_k13_and_float64(ctx, k, form):
    """test_sparse_entry_equals_dense at k = 13 and with a general Float64 KFV.  (k = 13: the family from its non-zero entries, one
    dense KFV of 4^13 entries made from them for the dense entry point.)"""
    rng = np.random.default_rng(160 + k + len(form))
    base, sp = sparse_family(rng, 289, k)
    keys, vals = sp["keys"], sp["vals"]
    if form == "float64":
        vals = _float_kfvs(rng, vals, "perturbed")
    RV = np.zeros(4 ** k, dtype=np.float64)
    RV[keys] = vals
    contigs = _genome(rng, 289, base)
    thr = thr_for_sparse(rng, dict(sp, vals=vals))
    n_refs = [sp["N"]] if form == "sn" else None
    ctx.set_refs(k, [RV], [289], [thr], n_refs)
    del RV
    dense = _dips_dists(ctx, contigs)
    ctx.set_refs_sparse(k, [keys], [vals], [289], [thr], n_refs)
    assert _dips_dists(ctx, contigs) == dense
    assert len(dense[0]) >= 1


@pytest.mark.parametrize("k", [14, 15])
def test_sparse_kfv_k14_k15(ctx, k):
    rng = np.random.default_rng(1400 + k)
    W, Nref = 240, 6
    base = random_dna(rng, W)
    refs = [mutate(rng, base, 0.03) for _ in range(Nref)]
    from collections import Counter
    cnt = Counter()
    for r in refs:
        cnt.update(kmer_values(r, k).tolist())
    skeys = np.asarray(sorted(cnt), dtype=np.uint32)
    sS = np.asarray([cnt[x] for x in sorted(cnt)], dtype=np.int64)
    vals = sS / Nref
    contigs = [random_dna(rng, 3000) + mutate(rng, base, 0.02) + random_dna(rng, 2500) + b"A" * 400 + mutate(rng, base, 0.05)
               + random_dna(rng, 900), random_dna(rng, W), b"ACGTN" * 100]
    want = [sparse_int_D(c, skeys.astype(np.int64), sS, Nref, k, W) for c in contigs]
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
        hits_c, dips_c, st_c = ctx.hits(), ctx.dips(), ctx.stats()
    finally:
        g.free()
    # chain mode against the sparse Float64 oracle: identical hits, nothing flagged, chain-decided hits carry its dist bit for bit
    ohits, od = orc.single_scan_sparse(contigs, (skeys, vals), k, W, thr, 50, return_dists=True)
    assert np.max(np.abs(d - od) / od) < REL_TOL
    _assert_omn_chain_parity(hits_c, dips_c, st_c, ohits)
    assert len(ohits) >= 1


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


# ---- k = 14, 15 against the sparse oracle; the wide tables' forms and edges --------------------------------------------------------
_GEOM = re.compile(r"generic (scan|chain) geometry: k (\d+), cmode (\d+), log2m (\d+), rebuild (\d+)")


@pytest.fixture
def geom(monkeypatch, capfd):
    """The generic path's count modes, from its KGMA_GEOM_DEBUG lines: geom() -> {(kind, k, cmode, log2m, rebuild)} since the last
    call."""
    monkeypatch.setenv("KGMA_GEOM_DEBUG", "1")
    capfd.readouterr()

    def read():
        return {(m[0], int(m[1]), int(m[2]), int(m[3]), int(m[4])) for m in _GEOM.findall(capfd.readouterr().err)}
    return read


def _modes(lines, kind="scan"):
    return {c for kd, _, c, _, _ in lines if kd == kind}


def _sparse_with_ends(ref):
    """ref with entries at key 0 (poly-A) and 4^k - 1 (poly-T, and a run of N) added to S."""
    k, N = ref["k"], ref["N"]
    d = dict(zip(ref["keys"].tolist(), ref["S"].tolist()))
    d[0] = d.get(0, 0) + 3
    d[4 ** k - 1] = d.get(4 ** k - 1, 0) + 5
    keys = np.asarray(sorted(d), dtype=np.uint32)
    S = np.asarray([d[x] for x in sorted(d)], dtype=np.int64)
    return dict(ref, keys=keys, S=S, vals=S * (1.0 / N))


def _run_all_modes(ctx, contigs, ref, thr):
    """Hits, distances and dips of the exact and the default mode, and the chain-mode hits, of a sparse ref."""
    ctx.set_refs_sparse(ref["k"], [ref["keys"]], [ref["vals"]], [ref["ws"]], [thr], [ref["N"]])
    g = ctx.genome_from_host(contigs)
    try:
        out = []
        for fl in (_lib.F_RETURN_DISTS | _lib.F_NO_TIE_RESOLVE, _lib.F_RETURN_DISTS, _lib.F_CHAIN_REPLAY):
            ctx.scan(g, _lib.MODE_SINGLE, 50, 0, fl, None)
            out.append(([tuple(sorted(h.items())) for h in ctx.hits()], ctx.dists(1).tobytes() if fl & _lib.F_RETURN_DISTS else None,
                        [tuple(sorted(x.items())) for x in ctx.dips()]))
        return out
    finally:
        g.free()


@pytest.mark.parametrize("k", [14, 15])
def test_sparse_single_engine_k14_k15(ctx, geom, k):
    """W = 289, S/N: the LDS table (cmode 3) at the widest keys; all three modes against the sparse oracles."""
    rng = np.random.default_rng(1500 + k)
    base, ref = sparse_family(rng, 289, k)
    contigs = _genome(rng, 289, base)
    thr = thr_for_sparse(rng, ref)
    hits, _ = _parity(ctx, contigs, ref, thr)
    assert ctx.kernel_name().startswith("gen_kernel")
    g = geom()
    assert _modes(g) == {3} and {x[1] for x in g} == {k}
    assert _modes(g, "chain") <= {3}
    assert len(hits) >= 1


@pytest.mark.parametrize("nk", [LDS_MAX_NK, LDS_MAX_NK + 1])
def test_sparse_k15_lds_global_boundary(ctx, geom, monkeypatch, nk):
    """k = 15, W = 15 + 2047 and 15 + 2048 (2048 / 2049 k-mers): both sides of KGMA_WIDE_LDS_MAX_NK.  Full parity, the count mode
    from the debug line, and the same results once more with every table forced into global memory."""
    k = 15
    W = nk + k - 1
    rng = np.random.default_rng(2048 + nk)
    base, ref = sparse_family(rng, W, k, n_refs=5)
    contigs = _genome(rng, W, base)
    thr = thr_for_sparse(rng, ref)
    _parity(ctx, contigs, ref, thr)
    assert _modes(geom()) == ({3} if nk <= LDS_MAX_NK else {4})
    first = _run_all_modes(ctx, contigs, ref, thr)
    monkeypatch.setenv("KGMA_WIDE_LDS_NK", "0")
    geom()
    forced = _run_all_modes(ctx, contigs, ref, thr)
    assert _modes(geom()) == {4}
    assert forced == first
    assert len(first[2][0]) >= 1


@pytest.mark.parametrize("form", ["sn", "float64"])
def test_sparse_k15_longest_window(ctx, geom, form):
    """n = 65535 k-mers at k = 15: the global-memory table of 2^17 entries, S/N and a general Float64 KFV (its distance lattice at
    the coarsest: the largest window)."""
    k = 15
    W = 65_535 + k - 1
    rng = np.random.default_rng(65_549 + len(form))
    base, ref = sparse_family(rng, W, k, n_refs=3)
    a = bytearray(random_dna(rng, 3 * W))
    a[W // 2:W // 2 + 9000] = b"A" * 9000
    a[W + 9000:2 * W + 9000] = mutate(rng, base, 0.02)          # (the dip ends inside the record: a hit)
    contigs = [bytes(a), random_dna(rng, W), random_dna(rng, W + 7)]
    thr = thr_for_sparse(rng, ref)
    if form == "sn":
        hits, _ = _parity(ctx, contigs, ref, thr)
    else:
        vals = _float_kfvs(rng, ref["vals"], "perturbed")
        thr = float(np.round(0.5 * orc.kmer_dist_kfv_sparse(random_dna(rng, W), (ref["keys"], vals), k), 1))
        hits, _ = _assert_float_single(ctx, contigs, (ref["keys"], vals), k, W, thr)
    assert len(hits) >= 1
    assert {(c, lg) for kd, _, c, lg, _ in geom() if kd == "scan"} == {(4, 17)}


@pytest.mark.parametrize("k", [14, 15])
def test_sparse_chain_values_every_window(ctx, geom, k):
    """gen_chain_kernel's wide form: the reference's running value of every window of a 40 kb record, bit for bit."""
    rng = np.random.default_rng(1440 + k)
    base, ref = sparse_family(rng, 289, k)
    contigs = _genome(rng, 289, base)
    seq = contigs[0][:30_000] + contigs[0][-10_000:]
    W = ref["ws"]
    nwin = len(seq) - W + 1
    sref = (ref["keys"], ref["vals"])
    ctx.set_refs_sparse(k, [ref["keys"]], [ref["vals"]], [W], [30.0], [ref["N"]])
    g = ctx.genome_from_host([seq])
    try:
        got = g.chain_values(0, 1, [(1, nwin)])
        assert ctx.stats()["chain_device_pairs"] == 1
    finally:
        g.free()
    _, od = orc.single_scan_sparse([seq], sref, k, W, 30.0, 50, return_dists=True)
    want = np.concatenate([[orc.kmer_dist_kfv_sparse(seq[:W], sref, k)], od])
    assert np.array_equal(got, want), f"first mismatch at window {int(np.argmax(got != want)) + 1}"
    assert _modes(geom(), "chain") == {3}


def test_sparse_k15_host_chain(ctx, monkeypatch):
    """KGMA_CHAIN=host: the sparse host walk decides every chain pair; chain-mode hits identical to the sparse oracle's."""
    k = 15
    rng = np.random.default_rng(1515)
    base, ref = sparse_family(rng, 289, k)
    contigs = _genome(rng, 289, base)
    thr = thr_for_sparse(rng, ref)
    ohits, _ = orc.single_scan_sparse(contigs, (ref["keys"], ref["vals"]), k, 289, thr, 50)
    monkeypatch.setenv("KGMA_CHAIN", "host")
    st = _assert_chain_single(ctx, contigs, ref, thr, 50, None, ohits)
    assert st["chain_device_pairs"] == 0
    assert len(ohits) >= 1


def _sparse_omn_oracles(contigs, fams, vals, ws, thr, align):
    k = fams[0]["k"]
    return orc.omn_scan_sparse(contigs, [(f["keys"], v) for f, v in zip(fams, vals)], k, ws, thr, 100, 1234, return_dists=True,
                               align=align)


@pytest.mark.parametrize("with_float", [False, True])
def test_sparse_cluster_engine_k14(ctx, geom, with_float):
    """Cluster engine at k = 14, KFVs of W = 250, 289 and 2100 + k (windows on both sides of the LDS bound: the scan runs in
    global memory, the chain pairs of the short windows in LDS), with and without the aligner's feedback.  All S/N: integer D,
    hits and distances bit-exact against the sparse integer oracle; with a general Float64 KFV among them: distances within
    REL_TOL.  Both: default-mode contract and chain-mode hits against the sparse Float64 oracle."""
    k = 14
    rng = np.random.default_rng(1414 + with_float)
    fams = [sparse_family(rng, L, k, n_refs=5) for L in (250, 289, 2100 + k)]
    bases = [f[0] for f in fams]
    fams = [f[1] for f in fams]
    ws = [f["ws"] for f in fams]
    Ns = [f["N"] for f in fams]
    vals = [f["vals"] for f in fams]
    if with_float:
        vals[1] = _float_kfvs(rng, vals[1], "perturbed")
    contigs, _ = make_genome(rng, [90_011, 40_000, max(ws) + k - 2, max(ws) + k], bases, n_plants_per_mb=150)
    thr = [float(np.round(0.6 * orc.kmer_dist_kfv_sparse(random_dna(rng, w), (f["keys"], v), k), 1)) for f, v, w in zip(fams, vals, ws)]

    def fake_align(contig, kfv, lo, hi, L):
        return lo + 3 + kfv, hi - 5

    n_hits = 0
    for align in (None, fake_align):
        ctx.set_refs_sparse(k, [f["keys"] for f in fams], vals, ws, thr, None if with_float else Ns)
        gen = ctx.genome_from_host(contigs)
        try:
            ctx.scan(gen, _lib.MODE_OMN, 100, 1234, _lib.F_RETURN_DISTS | _lib.F_NO_TIE_RESOLVE, align)
            hits, dists = ctx.hits(), [ctx.dists(j + 1) for j in range(3)]
            ctx.scan(gen, _lib.MODE_OMN, 100, 1234, _lib.F_RETURN_DISTS, align)
            hits_f, dips, st_f = ctx.hits(), ctx.dips(), ctx.stats()
            ctx.scan(gen, _lib.MODE_OMN, 100, 1234, _lib.F_CHAIN_REPLAY, align)
            hits_c, dips_c, st_c = ctx.hits(), ctx.dips(), ctx.stats()
        finally:
            gen.free()
        if not with_float:
            T = [orc.int_threshold(t, k, n) for t, n in zip(thr, Ns)]
            ohi, oD = orc.omn_scan_int_sparse(contigs, [(f["keys"], f["S"]) for f in fams], Ns, k, ws, T, 100, 1234, return_D=True,
                                              align=align)
            assert [hit_key(h) for h in hits] == [hit_key(h) for h in ohi]
            assert [h["D"] for h in hits] == [h["D"] for h in ohi]
            for j in range(3):
                assert np.array_equal(dists[j], oD[j] / (2.0 * k * Ns[j] ** 2))
        ohits, od = _sparse_omn_oracles(contigs, fams, vals, ws, thr, align)
        for j in range(3):
            assert dists[j].size == od[j].size
            assert float(np.max(np.abs(dists[j] - od[j]) / np.maximum(od[j], 1e-300))) < REL_TOL
        _assert_omn_default_parity(hits_f, dips, ohits, st_f["n_at_threshold"])
        _assert_omn_chain_parity(hits_c, dips_c, st_c, ohits)
        n_hits += len(ohits)
    g = geom()
    assert _modes(g) == {4} and _modes(g, "chain") <= {3, 4}
    assert n_hits >= 2


def test_float64_kfv_k12_global_table(ctx, geom):
    """A general Float64 KFV at k = 12, W = 3000: the Float64 form in cmode 4, under the dense oracle."""
    k, W = 12, 3000
    rng = np.random.default_rng(1203)
    base, ref = _family(rng, W, k, n_refs=5)
    RV = _float_kfvs(rng, ref["RV"], "perturbed")
    contigs = _genome(rng, W, base)
    thr = float(np.round(0.5 * orc.kmer_dist_kfv(random_dna(rng, W), RV, k), 1))
    hits, _ = _assert_float_single(ctx, contigs, RV, k, W, thr)
    assert _modes(geom()) == {4}
    assert len(hits) >= 1


@pytest.mark.parametrize("kind", ["perturbed", "pseudocount"])
def test_float64_kfv_k1(ctx, geom, kind):
    """A general Float64 KFV at k = 1: cmode 5 (four 32-bit counters) in its Float64 form."""
    rng = np.random.default_rng(101 + len(kind))
    base, ref = _family(rng, 289, 1)
    RV = _float_kfvs(rng, ref["RV"], kind)
    contigs = _genome(rng, 289, base)
    _, od = orc.single_scan(contigs, RV, 1, 289, 0.0, 50, return_dists=True)
    thr = float(np.quantile(od, 0.01))
    hits, _ = _assert_float_single(ctx, contigs, RV, 1, 289, thr)
    assert _modes(geom()) == {5}
    assert len(hits) >= 1


def test_sparse_k15_key_range_ends(ctx, geom):
    """k = 15, a KFV with entries at key 0 and 4^15 - 1 (all 30 key bits set, next to W_LIVE), a genome with long A / T / N runs."""
    k, W = 15, 289
    rng = np.random.default_rng(4 ** 3)
    base, ref = sparse_family(rng, W, k)
    ref = _sparse_with_ends(ref)
    assert ref["keys"][0] == 0 and ref["keys"][-1] == 4 ** k - 1
    a = bytearray(random_dna(rng, 30_000))
    a[2000:2000 + W] = mutate(rng, base, 0.02)
    a[5000:6000] = b"A" * 1000
    a[8000:9000] = b"T" * 1000
    a[11000:12000] = b"N" * 1000
    a[13000:13600] = b"a" * 300 + b"n" * 300
    a[20000:20000 + W] = mutate(rng, base, 0.05)
    contigs = [bytes(a), b"A" * (W - 1), b"T" * W, b"N" * (W + 1), b"n" * 400 + random_dna(rng, 300)]
    thr = thr_for_sparse(rng, ref)
    hits, _ = _parity(ctx, contigs, ref, thr)
    assert _modes(geom()) == {3}
    assert len(hits) >= 1


def test_float64_pseudocount_k11_full_table(ctx, geom):
    """k = 11, a pseudocount KFV: all 4^11 entries non-zero, so the device's sparse table has 2^23 slots and every first window
    merges over 4M keys.  Dense and sparse entry points, a few records."""
    k, W = 11, 289
    rng = np.random.default_rng(1111)
    base, ref = _family(rng, W, k)
    RV = _float_kfvs(rng, ref["RV"], "pseudocount")
    assert np.count_nonzero(RV) == 4 ** k
    contigs, _ = make_genome(rng, [12_000, 5000, W, W + 1], [base], n_plants_per_mb=300)
    thr = float(np.round(0.5 * orc.kmer_dist_kfv(random_dna(rng, W), RV, k), 1))
    h0, _ = _assert_float_single(ctx, contigs, RV, k, W, thr)
    h1, _ = _assert_float_single(ctx, contigs, orc.to_sparse(RV), k, W, thr)
    assert [hit_key(h) for h in h0] == [hit_key(h) for h in h1]
    assert _modes(geom()) == {3}


def test_int64_bound_k12_longest_window(ctx):
    """S/N at k = 12 with 65535 k-mers per window and N just below the generic kernel's int64 bound (dmax = sum S^2 + N^2 nk^2 <
    2^61): accepted and exact; N one larger: KGMA_E_UNSUPPORTED."""
    k = 12
    nk = 65_535
    W = nk + k - 1
    rng = np.random.default_rng(2 ** 61 % 1000)
    base = random_dna(rng, W)
    keys, c = np.unique(kmer_values(base, k), return_counts=True)
    c2 = int(np.sum(c.astype(object) ** 2))
    Nmax = int(np.floor(np.sqrt(((1 << 61) - 1) / (c2 + nk * nk))))
    while Nmax * Nmax * (c2 + nk * nk) >= 1 << 61:
        Nmax -= 1
    while (Nmax + 1) ** 2 * (c2 + nk * nk) < 1 << 61:
        Nmax += 1
    assert 20_000 < Nmax < 25_000
    S = c.astype(np.int64) * Nmax
    ref = dict(keys=keys.astype(np.uint32), S=S, N=Nmax, vals=c.astype(np.float64), ws=W, k=k)
    a = bytearray(random_dna(rng, 3 * W))
    a[W:W + W] = mutate(rng, base, 0.01)
    a[2 * W + 5000:2 * W + 8000] = b"N" * 3000
    a += b"A" * (W + 4000) + random_dna(rng, 2000)          # homopolymer windows: D = N^2 (sum c^2 + nk^2 - 2 c[A..A] nk), the bound's own form
    contigs = [bytes(a), random_dna(rng, W + 3)]
    thr = thr_for_sparse(rng, ref)
    T = orc.int_threshold(thr, k, Nmax)
    _, oD, oD1 = orc.single_scan_int_sparse(contigs, (ref["keys"], S), Nmax, k, W, T, 50, return_D=True)
    assert int(oD.max()) > 1 << 60                      # the bound is what is exercised
    hits, _ = _assert_single_parity(ctx, contigs, ref, thr)
    assert len(hits) >= 1
    for n in (Nmax + 1, Nmax + 50):
        with pytest.raises(_lib.KgmaError) as e:
            ctx.set_refs_sparse(k, [ref["keys"]], [ref["vals"]], [W], [thr], [n])
        assert e.value.status == _lib.KGMA_E_UNSUPPORTED
