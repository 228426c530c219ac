"""strobe_kernel<s> (kgma_strobe.hip) and its host half at the edges that tests/test_gpu_strobe.py does not reach, on the fixtures of
tests/strobe_cases.py (tests/test_strobe_cases.py shows, without a GPU, that none of them is vacuous).  Every expected value is the
oracle's (tests/strobe_oracle.py: Python integers and the reference's Float64 loop); nothing here has a tolerance.
  selection   strobe_bin<SS> at the ends of its parameters -- k = 16, w_min = 1, w_min = w_max, a score of 0 in each `zero` word, the
              largest sum of two s-mers -- under the discriminating table: first windows and every distance;
  short       windows of 1 .. 129 sliding items (the `all` correction rounds under 64, the D0 / TE hand-over where (nk - 1) >> 6
              changes), at a threshold between two distances and at one that IS a window's distance: kernel name, first windows, hits,
              distances, chain replay against the Float64 oracle, the flag contract;
  streams     a record cut into four streams at nk = 2 and 65, a dip across every boundary, a tie of the last window of one stream with
              the first of the next: hits, dips (first and last minimum, the tie flag) and distances;
  top         65 535 items per window, 65 535 of them in bin 0 while bin 1, the other half of its dword, is entered and left;
  range       the largest N and the largest table entry with sum S^2 + N^2 n^2 < 2^61 are scanned exactly, one more is refused.
Measured on one MI355X: 69 cases in 2.8 s, fixtures included; the slowest (four streams at nk = 2) 0.3 s."""
import re

import numpy as np
import pytest

from kmergma_amd import _lib
from tests import strobe_cases as sc
from tests.test_gpu_strobe import FLAGGED, _scan

pytestmark = pytest.mark.gpu

_STREAMS = re.compile(r"scan geometry: stream, .* windows -> streams of (\d+)")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _keys(hits):
    return [sc.hit_key(h) for h in hits]


def _as_dist(D, ref):
    return np.asarray([int(x) for x in D], dtype=np.int64).astype(np.float64) / float(sc.scale_of(ref))


def _assert_exact(ctx, seqs, ref, thr, o, genome=None):
    """Exact mode: kernel name, first windows, every distance and the hits against the integer oracle, bit for bit."""
    r = _scan(ctx, seqs, ref, thr, flags=_lib.F_RETURN_DISTS, buff=sc.BUFF, genome=genome)
    assert r["name"] == "strobe_kernel<%d>" % ref["cfg"][0]
    assert r["first"].tolist() == o["first_D"]
    want = _as_dist(o["dists_exact"], ref)
    assert r["dists"].size == want.size
    assert np.array_equal(r["dists"], want), "first wrong distance: step entry %d" % int(np.argmax(r["dists"] != want))
    assert _keys(r["hits"]) == _keys(o["exact"])
    scale = float(sc.scale_of(ref))
    assert all(h["kfv"] == 0 and h["dist"] == h["D"] / scale for h in r["hits"])
    return r


def _assert_chain_and_flags(ctx, seqs, ref, thr, o, r, genome):
    """Chain replay against the Float64 oracle, and test_gpu_strobe's flag contract on the unreplayed scan `r`."""
    rc = _scan(ctx, seqs, ref, thr, flags=_lib.F_CHAIN_REPLAY, buff=sc.BUFF, genome=genome)
    assert _keys(rc["hits"]) == _keys(o["float"])
    scale = float(sc.scale_of(ref))
    for a, b in zip(rc["hits"], o["float"]):
        if a["flags"] & _lib.HIT_CHAIN:
            assert a["dist"] == b["dist"]                                 # the reference's running value, bit for bit
        else:
            assert a["dist"] == a["D"] / scale
    flagged = {d["contig"] for d in r["dips"] if d["flags"] & FLAGGED} | {int(c) for c in r["att"][:, 0]}
    differ = [c for c, (e, f) in enumerate(o["per_record"]) if _keys(e) != _keys(f)]
    assert set(differ) <= flagged, (differ, sorted(flagged))
    assert r["stats"]["n_tie_flagged"] == sum(1 for d in r["dips"] if d["flags"] & _lib.HIT_TIE)


@pytest.mark.parametrize("cfg", [c for c, _, _ in sc.SELECT_SETS], ids=lambda v: str(v))
def test_selection_at_the_edges_of_its_parameters(ctx, cfg):
    c = sc.select_cell(cfg)
    o = dict(first_D=c["first_D"], dists_exact=c["D"], exact=[])
    r = _assert_exact(ctx, c["seqs"], c["ref"], 0.0, o)
    assert r["hits"] == [] and r["dips"] == []


@pytest.mark.parametrize("cfg,nk", sc.short_cells(), ids=lambda v: str(v))
def test_short_windows(ctx, cfg, nk):
    c = sc.short_cell(cfg, nk)
    g = ctx.genome_from_host(c["seqs"])
    try:
        for name in ("sparse", "dense"):
            o, thr = c["oracle"][name], c["thr"][name]
            r = _assert_exact(ctx, c["seqs"], c["ref"], thr, o, genome=g)
            if name == "dense":                                           # windows AT the threshold: reported, and not below it
                assert r["stats"]["n_at_threshold"] == c["at_threshold"] == r["att"].shape[0]
            _assert_chain_and_flags(ctx, c["seqs"], c["ref"], thr, o, r, g)
    finally:
        g.free()


@pytest.mark.parametrize("nk", sc.STREAMS_NKS)
def test_streams_beyond_a_records_first(ctx, monkeypatch, capfd, nk):
    monkeypatch.setenv("KGMA_GEOM_DEBUG", "1")

    def run(c):
        capfd.readouterr()
        r = _assert_exact(ctx, c["seqs"], c["ref"], c["thr"], c["oracle"])
        last_min = ctx.dip_last_min().tolist()
        return r, last_min, int(_STREAMS.findall(capfd.readouterr().err)[-1])

    c = sc.streams_cell(nk)
    r, last_min, P = run(c)
    if P != c["P"]:                                                       # the stream length is the library's to choose: plant at its boundaries
        c = sc.streams_cell(nk, P)
        r, last_min, P = run(c)
    assert P == c["P"]
    nwin = c["per"][0].size + 1
    assert nwin >= 6300 and r["stats"]["n_tiles"] == (nwin + P - 1) // P + 1 >= 3 + 1
    want = [(rec, d) for rec, dips in enumerate(c["dips"]) for d in dips]
    assert len(r["dips"]) == len(want) == len(last_min)
    for got, lm, (rec, d) in zip(r["dips"], last_min, want):
        assert (got["contig"], got["kfv"], got["start"], got["end"], got["argmin"], lm, got["D_min"], got["exit_pos"], got["D_exit"]) == \
            (rec, 1, d["start"], d["end"], d["argmin"], d["last_min"], d["D_min"], d["exit_pos"], d["D_exit"])
        assert bool(got["flags"] & _lib.HIT_TIE) == d["tie"] and not got["flags"] & _lib.HIT_AT_THRESHOLD
    assert r["att"].shape[0] == 0
    g = ctx.genome_from_host(c["seqs"])
    try:
        _assert_chain_and_flags(ctx, c["seqs"], c["ref"], c["thr"], c["oracle"], r, g)
    finally:
        g.free()


@pytest.mark.parametrize("cfg", sc.TOP_CFGS, ids=lambda v: str(v))
def test_top_of_the_16_bit_counters(ctx, cfg):
    c = sc.top_cell(cfg)
    r = _assert_exact(ctx, c["seqs"], c["ref"], c["thr"], c["oracle"])
    assert r["first"].tolist() == [c["dmax"]]
    assert any(abs(h["cmi"] - (c["at"] + 1)) <= 16 for h in r["hits"])


def _status(fn):
    with pytest.raises(_lib.KgmaError) as e:
        fn()
    return e.value.status


@pytest.mark.parametrize("cfg", sc.TOP_CFGS, ids=lambda v: str(v))
def test_largest_N(ctx, cfg):
    lo, hi = sc.top_edge_N(cfg)
    c = sc.top_cell(cfg, lo)
    r = _assert_exact(ctx, c["seqs"], c["ref"], c["thr"], c["oracle"])
    assert r["first"].tolist() == [c["dmax"]] and c["dmax"] > 0.999 * 2 ** 61
    shape = c["ref"]["S"] // lo
    for N in (hi, hi + 50):
        ref = sc.ref_of(shape * np.int64(N), N, cfg, c["W"])
        assert _status(lambda: ctx.set_strobe_ref(*cfg, ref["RV"], ref["W"], c["thr"], N)) == _lib.KGMA_E_UNSUPPORTED


def test_largest_entry(ctx):
    c = sc.entry_cell()
    _assert_exact(ctx, c["seqs"], c["ref"], c["thr"], c["oracle"])
    for S in (c["S_hi"], 2 ** 31):
        RV = np.zeros(c["ref"]["S"].size)
        RV[sc.ENTRY_BIN] = float(S)
        assert _status(lambda: ctx.set_strobe_ref(*c["cfg"], RV, c["W"], c["thr"], 1)) == _lib.KGMA_E_UNSUPPORTED
