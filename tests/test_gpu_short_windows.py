"""Windows of fewer k-mers than a 64-window step (tests/short_cases.py: nk = 2 ... 66) through every scan kernel form, against both
oracles.  With nk < 64 a lane's leaving k-mer entered in the same step, the stream kernels' warm-up steps and clamped leaving index
are all there is of a short record, the generic kernels take their `all` branch, and the position pass and the chains count
n_pos = n_valid + nk - 1 positions.  Each case names the kernel it must have run.

Single mode, at a sparse and a dense threshold: exact mode bit-equal to the integer oracle (first windows, every distance, hits, D),
default mode against the Float64 oracle under the record-level tie rule (_parity below), chain replay identical to it.
Cluster mode: test_stream8_derived_windows' assertions.  Then the three chains and the step path with the prefilter."""
import json
import os
import re

import numpy as np
import pytest

from kmergma_amd import _lib
from oracle import oracle as orc
from tests import filter_ref
from tests import short_cases as sc
from tests.helpers import hit_key
from tests import filter_cases as fc
from tests.test_gpu_fused_sums import _collect
from tests.test_gpu_fused_sums import _same as _same_step
from tests.test_gpu_parity import (REL_TOL, _assert_chain_single, _assert_omn_chain_parity, _assert_single_parity, _oracle_f64, _oracle_int,
                                   _scan_single)
from tests.test_gpu_wide import _assert_float_single

pytestmark = pytest.mark.gpu

SWITCHES = ("KGMA_KERNEL", "KGMA_STREAM8", "KGMA_STREAM8_DERIVE", "KGMA_STREAM8_WIDE", "KGMA_STREAM8_C16", "KGMA_TWOKERNEL", "KGMA_CHAIN",
            "KGMA_CHAIN_GENERIC", "KGMA_FILTER", "KGMA_FILTER_MIN_WINDOWS", "KGMA_FUSE_SUMS", "KGMA_OVERLAP", "KGMA_S8_MAXGROUP")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _no_inherited_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


# ---- single mode ------------------------------------------------------------------------------------------------------------------

FORM_ENV = {"stream8": {}, "stream": {"KGMA_STREAM8": "0"}, "bitslice": {"KGMA_KERNEL": "bitslice"}, "scan": {},
            "generic": {"KGMA_KERNEL": "generic"}, "gen": {}}
FORM_KERNEL = {"stream8": "stream8_kernel<%d>", "stream": "stream_kernel<%d>", "bitslice": "scan_kernel<%d>", "scan": "scan_kernel<%d>",
               "generic": "gen_kernel<%d>", "gen": "gen_kernel<%d>"}


def _assert_default_flag_contract(hits_f, dips, ohits, n_at_threshold, k):
    """The single engine's default mode, record by record (test_gpu_large_k's form of it, at any k): a record whose hits differ from
    the Float64 oracle's has a flagged dip, and the first differing hit (ours or the oracle's) carries a flag or lies in a flagged
    dip.  A hit's window is cmi - k + 1 (the reference reports the minimum's left index + 1); one window of slack as at k = 1."""
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
            return bool(h.get("flags", 0) & AMB) or any(x["start"] - 1 <= h["cmi"] - k + 1 <= x["end"] for x in in_rec)
        assert any(explained(h) for h in cands), (f"record {rec}: the first differing hit does not stem from a flagged dip: {cands}; "
                                                  f"flagged dips {[(x['start'], x['end'], x['flags']) for x in in_rec][:20]}")


def _parity(ctx, contigs, ref, thr, buff):
    """For the cells of RECORD_LEVEL: test_gpu_parity._assert_single_parity with its default-mode step in the record-level form (test_gpu_large_k): on the coarse
    distance lattice of a short window a dip's minimum is a plateau or recurs a few windows on, a flagged tie moves the hit and with
    it the range that suppresses the next dips, so a record's hits may differ in NUMBER from the Float64 oracle's -- always from a
    flagged dip on (EXPERIMENTS.md: every difference is downstream of a flagged dip).  Steps (1) and (3) are the helper's."""
    k, W, N = ref["k"], ref["ws"], ref["N"]
    # (1) exact arithmetic: first windows, every distance, hits and their D bit-identical to the integer oracle
    hits, d, D1, _, _ = _scan_single(ctx, contigs, ref, thr, buff, dists=True, no_tie_resolve=True)
    ohi, oD, oD1 = _oracle_int(contigs, ref, orc.int_threshold(thr, k, N), buff)
    assert np.array_equal(D1, oD1)
    want = oD / (2.0 * k * N * N)
    assert d.size == want.size
    assert np.array_equal(d, want), "first wrong distance: window entry %d" % int(np.argmax(d != want))
    assert [hit_key(h) for h in hits] == [hit_key(h) for h in ohi]
    assert [h["D"] for h in hits] == [h["D"] for h in ohi]
    # (2) default mode against the Float64 oracle: distances within tolerance, hits equal up to the first flagged dip of a record
    hits_f, _, _, stats, dips = _scan_single(ctx, contigs, ref, thr, buff)
    ohits, od = _oracle_f64(contigs, ref, thr, buff, None)
    assert len(od) == len(d) and np.max(np.abs(d - od) / np.maximum(od, 1e-300)) < REL_TOL
    _assert_default_flag_contract(hits_f, dips, ohits, stats["n_at_threshold"], k)
    for a, b in zip(hits_f, ohits):
        if hit_key(a) == hit_key(b):
            assert abs(a["dist"] - b["dist"]) <= REL_TOL * max(b["dist"], 1e-300)
    # (3) chain replay: identical to the Float64 oracle, nothing flagged, chain-decided hits with its distance bit for bit
    _assert_chain_single(ctx, contigs, ref, thr, buff, None, ohits)
    return hits


# The (k, N, nk, threshold) cells whose default-mode hits miss _assert_single_parity's rule (same number of hits as the Float64 oracle,
# every differing hit flagged itself), with what was seen at each: hits of ours and of the oracle, the first record that differs, its
# first differing hit of either side and the flagged dip that hit lies in.  The default mode is decided on the host, so a cell
# behaves the same in every kernel form.  These cells, and no others, are held to the record-level rule of _parity.
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "short_default_mode.json")) as _fh:
    RECORD_LEVEL = {(e["k"], e["N"], e["nk"], e["thr"]): e for e in json.load(_fh)}


@pytest.mark.parametrize("form,k,N,nk", sc.single_cells(), ids=lambda v: str(v))
def test_single_mode(ctx, monkeypatch, form, k, N, nk):
    for name, val in FORM_ENV[form].items():
        monkeypatch.setenv(name, val)
    c = sc.cell(k, N, nk)
    for which in ("sparse", "dense"):
        thr = c["thr"][which]
        if (k, N, nk, which) in RECORD_LEVEL:
            with pytest.raises(AssertionError):                         # (a cell that meets the helper's rule leaves the list)
                _assert_single_parity(ctx, c["contigs"], c["ref"], thr, sc.BUFF)
            _parity(ctx, c["contigs"], c["ref"], thr, sc.BUFF)
        else:
            _assert_single_parity(ctx, c["contigs"], c["ref"], thr, sc.BUFF)
        assert ctx.kernel_name() == FORM_KERNEL[form] % k, (which, ctx.kernel_name())


@pytest.mark.parametrize("nk", sc.NKS_MANDATORY)
def test_single_mode_float64_kfv(ctx, nk):
    """A general Float64 KFV at k = 6: the Float64 form of the generic kernel."""
    c = sc.float_cell(6, nk)
    for which in ("sparse", "dense"):
        hits, _ = _assert_float_single(ctx, c["contigs"], c["RV"], 6, c["W"], c["thr"][which], sc.BUFF)
        assert ctx.kernel_name() == "gen_kernel<f64,6>", (which, ctx.kernel_name())
        assert len(hits) > 0


# ---- cluster mode -----------------------------------------------------------------------------------------------------------------

def _cluster_scan(ctx, c, kernel, plain_too=False):
    """One exact scan with every distance, held to the integer oracle; returns (hits, dips, launches)."""
    k, ws, N = c["k"], c["ws"], c["N"]
    ctx.set_refs(k, c["KFVs"], ws, c["thr"], N)
    gen = ctx.genome_from_host(c["contigs"])
    try:
        ctx.scan(gen, _lib.MODE_OMN, sc.OMN_BUFF, sc.OMN_GENOME_POS, _lib.F_RETURN_DISTS | _lib.F_NO_TIE_RESOLVE, None)
        assert ctx.kernel_name() == kernel % k, ctx.kernel_name()
        hits, dips, st = ctx.hits(), ctx.dips(), ctx.stats()
        dists = [ctx.dists(j + 1) for j in range(len(ws))]
        if plain_too:                                                   # ... and without the distance arrays (the scan's usual form)
            ctx.scan(gen, _lib.MODE_OMN, sc.OMN_BUFF, sc.OMN_GENOME_POS, _lib.F_NO_TIE_RESOLVE, None)
            assert ctx.hits() == hits and ctx.dips() == dips
    finally:
        gen.free()
    assert [hit_key(h) for h in hits] == [hit_key(h) for h in c["ohi"]]
    assert [h["D"] for h in hits] == [h["D"] for h in c["ohi"]]
    for j in range(len(ws)):
        want = c["oD"][j] / (2.0 * k * N[j] ** 2)
        assert dists[j].size == want.size, j
        assert np.array_equal(dists[j], want), (j, int(np.argmax(dists[j] != want)))
    return hits, dips, st["n_launches"]


def _cluster_chain(ctx, c, kernel):
    k = c["k"]
    ctx.set_refs(k, c["KFVs"], c["ws"], c["thr"], c["N"])
    gen = ctx.genome_from_host(c["contigs"])
    try:
        ctx.scan(gen, _lib.MODE_OMN, sc.OMN_BUFF, sc.OMN_GENOME_POS, _lib.F_CHAIN_REPLAY, None)
        assert ctx.kernel_name() == kernel % k, ctx.kernel_name()
        _assert_omn_chain_parity(ctx.hits(), ctx.dips(), ctx.stats(), c["ohits"])
    finally:
        gen.free()


def _ids(v):
    return str(v).replace(" ", "")


@pytest.mark.parametrize("k,ws", sc.CLUSTER_ONE_SIZE, ids=_ids)
def test_cluster_stream8_one_size(ctx, k, ws):
    c = sc.cluster_cell(k, ws)
    _, _, launches = _cluster_scan(ctx, c, "stream8_kernel<%d>", plain_too=True)
    assert launches == 1
    _cluster_chain(ctx, c, "stream8_kernel<%d>")


@pytest.mark.parametrize("k,ws", sc.CLUSTER_DERIVED, ids=_ids)
def test_cluster_stream8_derived(ctx, monkeypatch, k, ws):
    """Windows of n and n + 1 k-mers off one count table, on both sides of a step's 64; the same with one size per launch."""
    c = sc.cluster_cell(k, ws)
    res = {}
    for derive in ("1", "0"):
        monkeypatch.setenv("KGMA_STREAM8_DERIVE", derive)
        res[derive] = _cluster_scan(ctx, c, "stream8_kernel<%d>", plain_too=True)
    assert res["1"][0] == res["0"][0] and res["1"][1] == res["0"][1]
    assert res["1"][2] == 1 and res["0"][2] == 2
    monkeypatch.delenv("KGMA_STREAM8_DERIVE")
    _cluster_chain(ctx, c, "stream8_kernel<%d>")


@pytest.mark.parametrize("k,ws,launches", sc.CLUSTER_WIDE, ids=_ids)
def test_cluster_stream8_five_and_eight_kfvs(ctx, monkeypatch, k, ws, launches):
    c = sc.cluster_cell(k, ws)
    res = {}
    for wide in ("1", "0"):
        monkeypatch.setenv("KGMA_STREAM8_WIDE", wide)
        res[wide] = _cluster_scan(ctx, c, "stream8_kernel<%d>", plain_too=True)
    assert res["1"][0] == res["0"][0] and res["1"][1] == res["0"][1]
    assert res["1"][2] == launches and res["0"][2] >= 2
    monkeypatch.delenv("KGMA_STREAM8_WIDE")
    _cluster_chain(ctx, c, "stream8_kernel<%d>")


@pytest.mark.parametrize("k,ws", sc.CLUSTER_TWO_KERNEL, ids=_ids)
def test_cluster_two_kernel_path(ctx, monkeypatch, k, ws):
    """scan_kernel<DIFFOUT> + pos_kernel, and the one-kernel form of the same bit-sliced group.  (kgma_scan_kernel_name says
    scan_kernel<k> for both: that the position pass ran rests on KGMA_TWOKERNEL alone, as in test_two_kernel_cluster_path.)"""
    c = sc.cluster_cell(k, ws)
    monkeypatch.setenv("KGMA_KERNEL", "bitslice")
    res = {}
    for two in ("1", "0"):
        monkeypatch.setenv("KGMA_TWOKERNEL", two)
        res[two] = _cluster_scan(ctx, c, "scan_kernel<%d>")
    assert res["1"][0] == res["0"][0] and res["1"][1] == res["0"][1]
    monkeypatch.setenv("KGMA_TWOKERNEL", "1")
    _cluster_chain(ctx, c, "scan_kernel<%d>")


@pytest.mark.parametrize("k,ws", sc.CLUSTER_BITSLICE_MIXED, ids=_ids)
def test_cluster_bitsliced_mixed_sizes(ctx, k, ws):
    c = sc.cluster_cell(k, ws)
    _cluster_scan(ctx, c, "scan_kernel<%d>", plain_too=True)
    _cluster_chain(ctx, c, "scan_kernel<%d>")


# ---- the chains -------------------------------------------------------------------------------------------------------------------

def _oracle_chain(seq, RV, k, W):
    _, od = orc.single_scan([seq], RV, k, W, 30.0, 50, return_dists=True)
    return np.concatenate([[orc.kmer_dist_kfv(seq[:W], RV, k)], od])


@pytest.mark.parametrize("k", sc.CHAIN_KS)
@pytest.mark.parametrize("nk", sc.CHAIN_NKS)
def test_chain_forms(ctx, monkeypatch, capfd, k, nk):
    """F_CHAIN_REPLAY with the chain in stream8_kernel<..., CHAIN>, in gen_chain_kernel and on the host, at the dense threshold and at
    a threshold that IS a window's distance (the largest below the dense one: every record with such a window is chained): the Float64
    oracle's hits each time, chain-decided hits with its distance bit for bit; the two device chains also at every window of the
    long record and of the records of W, W + 1 and W + 64 residues.  The scan's kernel name is stream8_kernel<k> in all three; which
    chain kernel ran is read from the generic path's KGMA_GEOM_DEBUG line, printed by gen_chain_kernel's launches only."""
    monkeypatch.setenv("KGMA_GEOM_DEBUG", "1")
    c = sc.cell(k, 7, nk)
    ref, W, contigs = c["ref"], c["W"], c["contigs"]
    Dall = np.concatenate(c["D"])
    on_a_window = int(Dall[Dall < orc.int_threshold(c["thr"]["dense"], k, 7)].max())
    thr_at = on_a_window / (2.0 * k * 7 * 7)
    T, T_hi = filter_ref.threshold_band(thr_at, k, 7)
    assert T <= on_a_window <= T_hi
    chains = {r: _oracle_chain(contigs[r], ref["RV"], k, W) for r in (0, 2, 3, 6)}
    for where, env in (("device", {}), ("generic", {"KGMA_CHAIN_GENERIC": "1"}), ("host", {"KGMA_CHAIN": "host"})):
        for name, val in env.items():
            monkeypatch.setenv(name, val)
        g = ctx.genome_from_host(contigs)
        capfd.readouterr()
        try:
            for thr in (c["thr"]["dense"], thr_at):
                ohits, _ = orc.single_scan(contigs, ref["RV"], k, W, thr, sc.BUFF)
                assert len(ohits) >= sc.MIN_DENSE_HITS // 2
                ctx.set_refs(k, [ref["RV"]], [W], [thr], [ref["N"]])
                ctx.scan(g, _lib.MODE_SINGLE, sc.BUFF, 0, _lib.F_CHAIN_REPLAY, None)
                hits, st, dips = ctx.hits(), ctx.stats(), ctx.dips()
                assert ctx.kernel_name() == "stream8_kernel<%d>" % k
                assert [hit_key(h) for h in hits] == [hit_key(h) for h in ohits], (where, thr)
                assert st["n_tie_flagged"] == 0 and not any(x["flags"] & (_lib.HIT_TIE | _lib.HIT_AT_THRESHOLD) for x in dips)
                if thr == thr_at:
                    assert st["n_chain_pairs"] >= 1, "no pair was chained although windows sit on the threshold"
                assert st["chain_device_pairs"] == (0 if where == "host" else st["n_chain_pairs"]), (where, st["chain_device_pairs"])
                for a, b in zip(hits, ohits):
                    if a["flags"] & _lib.HIT_CHAIN:
                        assert a["dist"] == b["dist"], where
                    else:
                        assert abs(a["dist"] - b["dist"]) <= REL_TOL * max(b["dist"], 1e-300)
            if where != "host":
                for r, want in chains.items():
                    got = g.chain_values(r, 1, [(1, want.size)])
                    assert ctx.stats()["chain_device_pairs"] == 1
                    assert np.array_equal(got, want), "%s chain, record %d: first mismatch at window %d" % (where, r, int(np.argmax(got != want)) + 1)
            generic_launches = re.findall(r"generic chain geometry: k (\d+)", capfd.readouterr().err)
            assert (set(generic_launches) == {str(k)}) if where == "generic" else not generic_launches, (where, generic_launches)
        finally:
            g.free()
            for name in env:
                monkeypatch.delenv(name)


# ---- the step path with the prefilter ---------------------------------------------------------------------------------------------

STEP_CELLS = [(k, N, nk) for k in sc.STEP_KS for N in sc.STEP_NS for nk in sc.STEP_NKS]


def _step(monkeypatch, contigs, ref, thr, fuse, k):
    """One fresh context, one kgma_repack_scan_hits under the chain replay: test_gpu_fused_sums._collect's fields and the kernel's name."""
    monkeypatch.setenv("KGMA_FUSE_SUMS", "1" if fuse else "0")
    ctx = _lib.Context(0)
    g = None
    try:
        ctx.set_refs(k, [ref["RV"]], [ref["ws"]], [thr], [ref["N"]])
        g = ctx.genome_from_host(contigs)
        ctx.step_hits(g, _lib.MODE_SINGLE, sc.BUFF, 0, _lib.F_CHAIN_REPLAY)
        out = _collect(ctx, g, False, len(contigs))
        out["kernel"] = ctx.kernel_name()
        return out
    finally:
        if g is not None:
            g.free()
        ctx.close()


@pytest.mark.parametrize("k,N,nk", STEP_CELLS, ids=["k%d-N%d-nk%d" % x for x in STEP_CELLS])
def test_step_path(monkeypatch, k, N, nk):
    """kgma_repack_scan_hits with the prefilter, the block sums fused into the pack and not: the same results, and the Float64
    oracle's hits under the chain replay.  The filter runs whenever its bound is positive (from 16 k-mers per window on; below it may
    decline, without a fallback) in the form of its S entries, PRESUMMED where the pack carried the sums.  On these genomes -- a
    tandem run, 8 kb of near copies and 48 short records -- the candidate regions with their warm-ups often pass half of the windows or
    make more streams than the scan has (FILTER_FRACTION, FILTER_STREAMS): the step then scans everything, and must say so."""
    monkeypatch.setenv("KGMA_FILTER", "1")
    monkeypatch.setenv("KGMA_FILTER_MIN_WINDOWS", "1")
    c = sc.cell(k, N, nk)
    ref, W, contigs = c["ref"], c["W"], c["contigs"]
    want_form = fc.form_of(k, int(ref["S"].max()))
    for which in ("sparse", "dense"):
        thr = c["thr"][which]
        ohits, _ = orc.single_scan(contigs, ref["RV"], k, W, thr, sc.BUFF)
        on = _step(monkeypatch, contigs, ref, thr, True, k)
        off = _step(monkeypatch, contigs, ref, thr, False, k)
        _same_step(on, off)
        T, T_hi = filter_ref.threshold_band(thr, k, ref["N"])
        U = filter_ref.bound_U(ref["S"], ref["N"], k, W, T, T_hi)
        for res, fused in ((on, N == 7), (off, False)):
            fs = res["fs"]
            assert res["kernel"] == "stream8_kernel<%d>" % k, (which, res["kernel"])
            if nk >= 16:
                assert fs["ran"] == (1 if U > 0 else 0), (which, U, fs)
            if fs["ran"] == 0:
                assert fs["fell_back"] == 0 and fs["form"] == 0, fs
            else:
                assert fs["bound"] == U
                assert fs["form"] == (want_form | _lib.FILTER_FORM_PRESUMMED if fused else want_form), (which, fs)
                if fs["fell_back"] == 0:
                    assert fs["reason"] == _lib.FILTER_OK and 0 < fs["windows"] <= fs["total_windows"], fs
                else:
                    assert fs["reason"] in (_lib.FILTER_FRACTION, _lib.FILTER_STREAMS), fs
                    assert fs["reason"] != _lib.FILTER_FRACTION or fs["positions"] > 0.5 * fs["total_windows"], fs
            assert [hit_key(h) for h in res["hits"]] == [hit_key(h) for h in ohits], which
        assert len(ohits) > 0
