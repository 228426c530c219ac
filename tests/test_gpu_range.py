"""The integer scan paths at the ends of their range (tests/range_cases.py), through the C ABI against the oracles.

kgma_set_refs decides from magnitude predicates (fits32, big_ok, N < 2^22, dmax < 2^61) which kernel a KFV may take, and each
kernel keeps part of its arithmetic in the 32 bits its predicate promises.  Here every predicate is visited with the largest N for
which it holds (edge-) and that N + 1 (edge+), on genomes whose windows run from D = 0 to D = dmax and back: the prefix of a record
reaches the whole of what the predicate allows, and with the `all` threshold every tested window is under threshold.  A predicate one
bit too generous, a clamp that bites or an int32 product that wraps shows as a distance that differs from the integer oracle's.

kernel_name() is asserted in every case.  The 8-bit and the 16-bit counter form of stream8_kernel report the same name, and
KGMA_GEOM_DEBUG's line does not tell them apart either: at k = 5, 6 (and k = 7 with S in int16) the fits32 edge at 280-odd k-mers
has the 8-bit form on one side and the 16-bit form with 64-bit carries on the other, and what holds them is the parity on both.
"""
import numpy as np
import pytest

from kmergma_amd import _lib
from oracle import oracle as orc
from tests import range_cases as rc
from tests.helpers import hit_key
from tests.test_gpu_parity import _assert_omn_chain_parity, _assert_omn_default_parity, _assert_single_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _single(ctx, x, kernel=None):
    """All three modes against both oracles at the three thresholds, and the kernel.  (`all`: no window ever leaves the threshold,
    so no dip closes and neither oracle reports a hit -- what is compared there is every distance and every record's first window.
    `low`: record F, which starts at dmax and dips to 0.27 dmax, gives no hit.)"""
    n = []
    for thr in x["thr"]:
        hits, _ = _assert_single_parity(ctx, x["contigs"], x["ref"], thr, rc.BUFF)
        assert ctx.kernel_name().startswith(kernel or x["kernel"]), ctx.kernel_name()
        n.append(len(hits))
    assert n[0] >= 2 and n[2] >= 1, n
    return n


@pytest.mark.parametrize("c", rc.SINGLE_CELLS, ids=rc.cell_id)
def test_single_engine_at_the_edges(ctx, c):
    _single(ctx, rc.cell(*c))


@pytest.mark.parametrize("var,value,name", [("KGMA_KERNEL", "bitslice", "scan_kernel"), ("KGMA_KERNEL", "stream", "stream8_kernel"),
                                            ("KGMA_KERNEL", "generic", "gen_kernel"), ("KGMA_STREAM8", "0", "stream_kernel")])
def test_forced_kernels_at_the_fits32_edge(ctx, var, value, name, monkeypatch):
    """KGMA_KERNEL (read at every scan) at the fits32 edge- cell of k = 6: each int32 kernel, and the int64 one, with the largest
    prefix the int32 kernels are promised.  (KGMA_KERNEL=stream keeps the 8-bit counter kernel where it applies; the 16-bit counter
    stream_kernel is what KGMA_STREAM8=0 leaves.)"""
    monkeypatch.setenv(var, value)
    _single(ctx, rc.cell(*rc.FORCED_CELL), name)


@pytest.mark.parametrize("c", rc.REFUSED_CELLS, ids=rc.cell_id)
def test_beyond_int64_is_refused(ctx, c):
    """dmax >= 2^61: an argument error of kgma_set_refs, returned before any launch -- and the context serves the next set_refs."""
    pred, k, nk, family, side = c
    W = nk + k - 1
    lo, hi = rc.edge_N(pred, k, W, family)
    bad = rc.ref_of(family, k, W, hi)
    assert rc.dmax(bad["S"], hi, nk) >= 2 ** 61 > rc.dmax(rc.table(family, k, W, lo), lo, nk)
    with pytest.raises(_lib.KgmaError) as e:
        ctx.set_refs(k, [bad["RV"]], [W], [10.0], [hi])
    assert e.value.status == _lib.KGMA_E_UNSUPPORTED
    _single(ctx, rc.cell(pred, k, nk, family, "-"))                     # edge-: served, D and distances exact


# ---- cluster engine -------------------------------------------------------------------------------------------------------------------

def _cluster(ctx, x):
    k, ws, S, N, KFVs, contigs = x["k"], x["ws"], x["S"], x["N"], x["KFVs"], x["contigs"]
    gen = ctx.genome_from_host(contigs)
    try:
        for name in ("mid", "all", "low"):
            thr = x["thr"][name]
            T = [orc.int_threshold(t, k, n) for t, n in zip(thr, N)]
            ohi, oD = orc.omn_scan_int(contigs, S, N, k, ws, T, rc.OMN_BUFF, rc.OMN_GENOME_POS, return_D=True)
            assert len(ohi) >= {"mid": 2 * len(ws), "all": 0, "low": 2}[name]
            ctx.set_refs(k, KFVs, ws, thr, N)
            ctx.scan(gen, _lib.MODE_OMN, rc.OMN_BUFF, rc.OMN_GENOME_POS, _lib.F_RETURN_DISTS | _lib.F_NO_TIE_RESOLVE, None)
            assert ctx.kernel_name().startswith(x["kernel"]), ctx.kernel_name()
            hits = ctx.hits()
            assert [hit_key(h) for h in hits] == [hit_key(h) for h in ohi]
            assert [h["D"] for h in hits] == [h["D"] for h in ohi]
            for j in range(len(ws)):
                assert np.array_equal(ctx.dists(j + 1), oD[j] / (2.0 * k * N[j] ** 2)), j
            fo, _ = orc.omn_scan(contigs, KFVs, k, ws, thr, rc.OMN_BUFF, rc.OMN_GENOME_POS)
            ctx.scan(gen, _lib.MODE_OMN, rc.OMN_BUFF, rc.OMN_GENOME_POS, 0, None)
            _assert_omn_default_parity(ctx.hits(), ctx.dips(), fo, ctx.stats()["n_at_threshold"])
            ctx.scan(gen, _lib.MODE_OMN, rc.OMN_BUFF, rc.OMN_GENOME_POS, _lib.F_CHAIN_REPLAY, None)
            _assert_omn_chain_parity(ctx.hits(), ctx.dips(), ctx.stats(), fo)
    finally:
        gen.free()


@pytest.mark.parametrize("name", ["k6-84-fits32lo-fits32hi", "k6-84-beyond-big_ok"])
def test_cluster_engine_mixed_magnitudes(ctx, name):
    """KFVs of one window size whose N differ by orders of magnitude in ONE scan: a small family beside KFVs on either side of
    fits32, and beside one beyond big_ok.  Hits, D and every distance of every KFV against the integer oracle; default and chain
    mode against the Float64 oracle."""
    _cluster(ctx, rc.cluster_cell(name))


@pytest.mark.parametrize("two", ["1", "0"])
def test_cluster_engine_int32_s_at_the_fits32_edge(ctx, two, monkeypatch):
    """k = 7, two KFVs at fits32 edge- whose S exceeds int16: scan_kernel's per-window differences + pos_kernel (KGMA_TWOKERNEL,
    read at every scan: on and off)."""
    monkeypatch.setenv("KGMA_TWOKERNEL", two)
    _cluster(ctx, rc.cluster_cell("k7-fits32lo-x2-int32-S"))


# ---- chain ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", rc.CHAIN_CELLS, ids=rc.cell_id)
def test_chain_values_at_the_edges(ctx, c):
    """kgma_chain_values at EVERY window of record B (it starts at dmax, falls to the base and rises again, twice) against the
    reference-order oracle, bit for bit."""
    x = rc.cell(*c)
    ref, k, W = x["ref"], x["k"], x["W"]
    seq = x["contigs"][1]
    assert x["names"][1] == "B"
    ctx.set_refs(k, [ref["RV"]], [W], [x["thr"][0]], [ref["N"]])
    g = ctx.genome_from_host([seq])
    try:
        _, od = orc.single_scan([seq], ref["RV"], k, W, x["thr"][0], rc.BUFF, return_dists=True)
        chain = np.concatenate([[orc.kmer_dist_kfv(seq[:W], ref["RV"], k)], od])
        nwin = len(seq) - W + 1
        v = g.chain_values(0, 1, [(1, nwin)])
        assert np.array_equal(v, chain), f"first mismatch at window {int(np.argmax(v != chain)) + 1}"
        assert ctx.stats()["chain_device_pairs"] == 1
    finally:
        g.free()
