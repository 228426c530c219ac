"""The generic kernel's hash tables (Counts<2> at k = 8 ... 10, WCounts at k >= 11, the sparse KFV table) on k-mers computed to
collide: tests/hash_cases.py builds the inputs, tests/hash_model.py shows on the CPU what each of them reaches (probe paths of
dozens to hundreds of buckets across the table's end, claimed tombstones, live k-mers behind tombstones, dozens of lanes on one
free entry, rebuilds before every step, chains in the sparse KFV table -- tests/test_hash_cases.py).  Here every case runs on the
device: the geometry and the stream length the library reports equal the model's, and the results are held to the oracles by the
rules the other parity tests use -- nothing new is tolerated."""
import re

import numpy as np
import pytest

from kmergma_amd import _lib
from oracle import oracle as orc
from tests import hash_cases as hc
from tests import hash_model as hm
from tests.helpers import hit_key
from tests.test_gpu_parity import _assert_omn_chain_parity, _assert_single_parity
from tests.test_gpu_wide import _assert_float_single, ctx_dips_of

pytestmark = pytest.mark.gpu

_GEOM = re.compile(r"generic (scan|chain) geometry: k (\d+), cmode (\d+), log2m (\d+), rebuild (\d+)")
_STREAMS = re.compile(r"scan geometry: stream, .* -> streams of (\d+)")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture
def geom(monkeypatch, capfd):
    """geom() -> ({(kind, k, cmode, log2m, rebuild)}, {stream lengths}) of the library's KGMA_GEOM_DEBUG lines since the last call."""
    monkeypatch.setenv("KGMA_GEOM_DEBUG", "1")
    capfd.readouterr()

    def read():
        err = capfd.readouterr().err
        return ({(m[0], int(m[1]), int(m[2]), int(m[3]), int(m[4])) for m in _GEOM.findall(err)}, {int(x) for x in _STREAMS.findall(err)})
    return read


def _setenv(monkeypatch, c):
    monkeypatch.setenv("KGMA_KERNEL", "generic")
    monkeypatch.setenv("KGMA_CHAIN_GENERIC", "1")
    for key, v in c["env"].items():
        monkeypatch.setenv(key, v)


@pytest.mark.parametrize("name", hc.NAMES)
def test_colliding_case(ctx, geom, monkeypatch, name):
    """S/N KFV: exact mode bit for bit against the integer oracle (hits, dips' first-window D, every distance), default mode under
    _assert_single_parity's rule, chain replay identical with nothing flagged.  The geometry lines equal the model's.  At
    k = 8, 9, 10 the same scan with the 4^k counters in global memory (KGMA_GENERIC_HASH=0) gives identical dips and distances."""
    c = hc.case(name)
    k, nk = c["k"], c["nk"]
    _setenv(monkeypatch, c)
    geom()
    hits, _ = _assert_single_parity(ctx, c["records"], c["ref"], c["thr"])
    assert ctx.kernel_name().startswith("gen_kernel"), ctx.kernel_name()
    lines, streams = geom()
    want = (k,) + hm.geometry(k, nk, c["env"])
    assert {x[1:] for x in lines if x[0] == "scan"} == {want}
    assert {x[1:] for x in lines if x[0] == "chain"} <= {want}
    assert streams == {hm.stream_windows(nk)}
    assert len(hits) >= 1
    if k < hm.WIDE_MIN_K:
        first = ctx_dips_of(ctx, c["records"], c["ref"], c["thr"])
        monkeypatch.setenv("KGMA_GENERIC_HASH", "0")
        assert ctx_dips_of(ctx, c["records"], c["ref"], c["thr"]) == first
        assert {x[2] for x in geom()[0] if x[0] == "scan"} == ({2, 1} if want[1] == 2 else {1})


@pytest.mark.parametrize("name", [c["name"] for c in hc.cases() if c["fref"] is not None])
def test_colliding_case_float64(ctx, geom, monkeypatch, name):
    """A general Float64 KFV (the case's entries perturbed) per family: the Float64 form of the kernel over the same tables."""
    c = hc.case(name)
    _setenv(monkeypatch, c)
    geom()
    _assert_float_single(ctx, c["records"], c["fref"], c["k"], c["ws"], c["thr"])
    lines, _ = geom()
    assert {x[1:] for x in lines if x[0] == "scan"} == {(c["k"],) + hm.geometry(c["k"], c["nk"], c["env"])}


CHAIN_CASES = [c["name"] for c in hc.cases() if c["family"] in ("long", "tomb", "limit")]


@pytest.mark.parametrize("name", CHAIN_CASES)
def test_chain_values_every_window(ctx, geom, monkeypatch, name):
    """gen_chain_kernel over the same tables: the reference's running Float64 value at every window of the long-path, tombstone and
    limit records, bit for bit, for the S/N KFV and (where the case has one) the Float64 KFV."""
    c = hc.case(name)
    k, W = c["k"], c["ws"]
    _setenv(monkeypatch, c)
    seq = c["records"][0]
    nwin = len(seq) - W + 1
    ref = c["ref"]
    kfvs = [(ref["keys"], ref["vals"]) if "keys" in ref else ref["RV"]] + ([c["fref"]] if c["fref"] is not None else [])
    for kfv, n_refs in zip(kfvs, ([ref["N"]], None)):
        if isinstance(kfv, tuple):
            ctx.set_refs_sparse(k, [kfv[0]], [kfv[1]], [W], [c["thr"]], n_refs)
            _, od = orc.single_scan_sparse([seq], kfv, k, W, c["thr"], 50, return_dists=True)
            d1 = orc.kmer_dist_kfv_sparse(seq[:W], kfv, k)
        else:
            ctx.set_refs(k, [kfv], [W], [c["thr"]], n_refs)
            _, od = orc.single_scan([seq], kfv, k, W, c["thr"], 50, return_dists=True)
            d1 = orc.kmer_dist_kfv(seq[:W], kfv, k)
        g = ctx.genome_from_host([seq])
        try:
            geom()
            got = g.chain_values(0, 1, [(1, nwin)])
            assert ctx.stats()["chain_device_pairs"] == 1
        finally:
            g.free()
        want = np.concatenate([[d1], od])
        assert np.array_equal(got, want), f"first mismatch at window {int(np.argmax(got != want)) + 1}"
        assert {x[1:] for x in geom()[0] if x[0] == "chain"} == {(k,) + hm.geometry(k, c["nk"], c["env"])}


def test_cluster_engine_on_a_long_path_record(ctx, geom, monkeypatch):
    """Three KFVs of n, n and n + 1 = 449 k-mers per window at k = 8 over a long-path record: every launch takes the longest
    window's table (4096 entries), bit for bit against the integer oracle, chain mode against the Float64 oracle."""
    k = 8
    a, b, c3 = hc.case("long-k8-n448"), hc.case("contention-k8-n448"), hc.case("long-k8-n449")
    refs = [a["ref"], b["ref"], c3["ref"]]
    records = [a["records"][0], b["records"][0] + c3["records"][0][:1500]]
    RVs, ws, Ns, S = [r["RV"] for r in refs], [r["ws"] for r in refs], [r["N"] for r in refs], [r["S"] for r in refs]
    thr = [a["thr"], b["thr"], c3["thr"]]
    monkeypatch.setenv("KGMA_KERNEL", "generic")
    T = [orc.int_threshold(t, k, n) for t, n in zip(thr, Ns)]
    ohi, oD = orc.omn_scan_int(records, S, Ns, k, ws, T, 100, 55, return_D=True)
    assert len(ohi) >= 2
    ctx.set_refs(k, RVs, ws, thr, Ns)
    gen = ctx.genome_from_host(records)
    try:
        geom()
        ctx.scan(gen, _lib.MODE_OMN, 100, 55, _lib.F_RETURN_DISTS | _lib.F_NO_TIE_RESOLVE, None)
        assert ctx.kernel_name().startswith("gen_kernel")
        hits = ctx.hits()
        assert [hit_key(h) for h in hits] == [hit_key(h) for h in ohi]
        assert [h["D"] for h in hits] == [h["D"] for h in ohi]
        for j in range(3):
            assert np.array_equal(ctx.dists(j + 1), oD[j] / (2.0 * k * Ns[j] ** 2)), j
        lines, streams = geom()
        assert {x[1:] for x in lines if x[0] == "scan"} == {(k,) + hm.geometry(k, 449)}
        assert streams == {hm.stream_windows(449)}
        fo, _ = orc.omn_scan(records, RVs, k, ws, thr, 100, 55)
        ctx.scan(gen, _lib.MODE_OMN, 100, 55, _lib.F_CHAIN_REPLAY, None)
        _assert_omn_chain_parity(ctx.hits(), ctx.dips(), ctx.stats(), fo)
    finally:
        gen.free()
