"""The step's pack with the prefilter's block sums (kgma_filter.hip: pack_sums_kernel, filter_kernel<..., PRESUMMED>; switch
KGMA_FUSE_SUMS): a step with the sums fused into the pack gives what the step with the plain pack and the looking-up filter gives --
hits (every field), dips, first-window D, guard-band windows, counters, candidate granules, the filter's numbers -- and what the
oracle gives; the sums read back are the numpy restatement's (tests/sums_ref.py) for every record.  The records sit where the pack's
paths change: a pack block is 32768 residues, a wave takes 4096 at a time in chunks of 2048, and everything that is not a run of
full words of one record followed by k - 1 more of its residues goes word by word with a mask."""
import functools
import os

import numpy as np
import pytest

from kmergma_amd import _lib
from oracle import oracle as orc
from tests import filter_cases as fc
from tests import filter_ref, sums_ref
from tests.helpers import hit_key, mutate, random_dna

pytestmark = pytest.mark.gpu

BUFF = 50
PRESUMMED = _lib.FILTER_FORM_PRESUMMED
LONG = 200_000


@pytest.fixture(autouse=True)
def _small_genomes(monkeypatch):
    monkeypatch.setenv("KGMA_FILTER_MIN_WINDOWS", "1")
    monkeypatch.setenv("KGMA_FILTER", "1")
    monkeypatch.delenv("KGMA_OVERLAP", raising=False)


def records(rng, gene, W):
    """(contigs, plants): the records of the module docstring for a gene of at least W residues; plants are (record, 0-based window)
    of the clean copies (mutated at 4 %)."""
    g = lambda: mutate(rng, gene, 0.04)[:W]
    contigs, plants = [], []

    def rec(L, at=()):
        a = bytearray(random_dna(rng, L))
        for pos in at:
            a[pos:pos + W] = g()
            plants.append((len(contigs), pos))
        contigs.append(bytes(a))

    rec(3 * 32768, at=(5_000, 32768 - W // 2, 2 * 32768 - 3, 3 * 32768 - W))      # the record's end on a pack-block end
    rec(32768 + 5, at=(32768 + 5 - W,))                                          # k - 1 residues spill into the next block
    rec(32768 + 31, at=(20_000,))
    rec(65536 - 1, at=(65535 - W,))
    rec(W - 1)                                                                   # no window
    contigs.append(g()); plants.append((len(contigs) - 1, 0))                    # one window
    rec(3)                                                                       # shorter than k
    for L in (40, 70, 33, 100, 32, 64, 1, W + 20, 95):                           # several short records inside one chunk
        rec(L)
    # one long record: genes across a pack-block boundary, across a chunk boundary inside a run of full words, on the record's last
    # residue and on its first; an N run over a gene's edge; a lower-case stretch over another
    at = [0, 32768 - W // 3, 40 * 2048 - W // 2, 43 * 2048 - 7, 4 * 32768 - 11, LONG - W]
    a = bytearray(random_dna(rng, LONG))
    for pos in at:
        a[pos:pos + W] = g()
        plants.append((len(contigs), pos))
    a[120_000:120_000 + W] = g()
    a[120_000 - 50:120_000 + 20] = b"N" * 70
    a[150_100:150_100 + W] = g()
    a[150_000:150_300] = bytes(a[150_000:150_300]).lower()
    a[170_000:170_040] = b"n" * 40
    contigs.append(bytes(a))
    assert sum(len(c) for c in contigs) < 1_000_000
    return contigs, plants


@functools.lru_cache(maxsize=None)
def cell(k, N, nk):
    """What the tests of one (k, N, nk) share, computed once and never modified."""
    ref = fc.family(k, N, nk)
    W = ref["ws"]
    contigs, plants = records(np.random.default_rng([6501, k, N, nk]), ref["base"], W)
    D = fc.exact_D(contigs, ref["S"], N, k, W)
    thr = fc.threshold(D, plants, k, N)
    sums = [sums_ref.block_sums(c, ref["S"], k) for c in contigs]
    ohits, _ = orc.single_scan(contigs, ref["RV"], k, W, thr, BUFF)
    return dict(ref=ref, W=W, contigs=contigs, plants=plants, D=D, thr=thr, sums=sums, ohits=ohits)


def _collect(ctx, g, fused, n_records):
    st = ctx.stats()
    out = dict(hits=ctx.hits(), dips=ctx.dips(), D1=ctx.first_window(1), att=ctx.att(),
               counts=(st["n_dips"], st["n_tie_flagged"], st["n_at_threshold"]), windows=st["windows_scanned"],
               fs=ctx.filter_stats(), cand=ctx.filter_candidates(), sums=None)
    if fused:
        out["sums"] = [ctx.get_block_sums(g, c) for c in range(n_records)]
    return out


def _steps(monkeypatch, contigs, ref, thr, flags, fuse, k, pokes=(), read_sums=True):
    """One fresh context; one step, plus one per entry of `pokes` (None, or (record, 1-based position, bytes) planted before it).
    Returns every step's results, and the context's filter stats after one more plain scan when there were pokes."""
    monkeypatch.setenv("KGMA_FUSE_SUMS", "1" if fuse else "0")
    ctx = _lib.Context(0)
    g = None
    try:
        ctx.set_refs(k, [ref["RV"]], [ref["ws"]], [thr], [ref["N"]])
        g = ctx.genome_from_host(contigs)
        outs = []
        for poke in (None,) + tuple(pokes):
            if poke is not None:
                g.poke(*poke)
            ctx.step_hits(g, _lib.MODE_SINGLE, BUFF, 0, flags)
            outs.append(_collect(ctx, g, fuse and read_sums, len(contigs)))
        plain = None
        if pokes:
            ctx.scan(g, _lib.MODE_SINGLE, BUFF, 0, flags, None)
            plain = _collect(ctx, g, False, len(contigs))
        return outs, plain
    finally:
        if g is not None:
            g.free()
        ctx.close()


def _same(a, b):
    assert a["hits"] == b["hits"]
    assert a["dips"] == b["dips"]
    assert np.array_equal(a["D1"], b["D1"])
    assert np.array_equal(a["att"], b["att"])
    assert a["counts"] == b["counts"]
    assert a["windows"] == b["windows"]
    assert np.array_equal(a["cand"], b["cand"])
    for name in ("ran", "fell_back", "reason", "granules", "regions", "streams", "windows", "positions", "total_windows", "bound"):
        assert a["fs"][name] == b["fs"][name], name


def _check_sums(got, want):
    for c, (x, y) in enumerate(zip(got, want)):
        assert x.size == y.size, c
        bad = np.nonzero(x.astype(np.int64) != y)[0]
        assert bad.size == 0, "record %d (%d blocks): block %d is %d, not %d (%d wrong)" % (c, y.size, bad[0], x[bad[0]], y[bad[0]], bad.size)


def _on_off(monkeypatch, contigs, ref, thr, k, W, ohits, sums, all_flags=(0, _lib.F_CHAIN_REPLAY), fused_form=True):
    first = None
    for flags in all_flags:
        (on,), _ = _steps(monkeypatch, contigs, ref, thr, flags, True, k, read_sums=fused_form)
        (off,), _ = _steps(monkeypatch, contigs, ref, thr, flags, False, k)
        assert on["fs"]["ran"] == 1 and on["fs"]["fell_back"] == 0, on["fs"]
        want_form = fc.form_of(k, int(np.max(ref["S"])))
        assert off["fs"]["form"] == want_form
        assert on["fs"]["form"] == (want_form | PRESUMMED if fused_form else want_form)
        if fused_form:
            _check_sums(on["sums"], sums)                               # (first: a wrong sum names its block)
        _same(on, off)
        if flags & _lib.F_CHAIN_REPLAY:
            assert [hit_key(h) for h in on["hits"]] == [hit_key(h) for h in ohits]
        first = first or on
    return first


CELLS = [(k, nk) for k in (5, 6) for nk in (17, 284, 383)]


@pytest.mark.parametrize("k,nk", CELLS, ids=["k%d-nk%d" % c for c in CELLS])
def test_fused_on_off_oracle_and_sums(monkeypatch, k, nk):
    c = cell(k, 7, nk)
    assert int(c["ref"]["S"].max()) < 256
    on = _on_off(monkeypatch, c["contigs"], c["ref"], c["thr"], k, c["W"], c["ohits"], c["sums"])
    T, T_hi = filter_ref.threshold_band(c["thr"], k, 7)
    U = filter_ref.bound_U(c["ref"]["S"], 7, k, c["W"], T, T_hi)
    assert on["fs"]["bound"] == U
    assert np.array_equal(on["cand"], filter_ref.candidates(c["contigs"], c["ref"]["S"], k, c["W"], U))
    assert len(c["ohits"]) >= 8 and len(on["hits"]) > 0
    have = set(map(tuple, on["cand"].tolist()))
    assert all((r, s // 16) in have for r, s in c["plants"])


def test_alpaca_reference_thr_30(monkeypatch, alp_ref, data_dir):
    """The bench's reference (k = 6, W = 289) at thr = 30; the record of 289 residues is a gene's first 289, below the threshold."""
    from kmergma_amd import fasta
    genes = [r.sequence.upper() for r in fasta.read_fasta(os.path.join(data_dir, "Alp_V_ref.fasta"))]
    W = int(alp_ref["ws"])
    contigs, _ = records(np.random.default_rng(6502), next(x for x in genes if len(x) >= W), W)
    assert [len(c) for c in contigs[4:7]] == [288, 289, 3]
    ohits, _ = orc.single_scan(contigs, alp_ref["RV"], 6, W, 30.0, BUFF)
    sums = [sums_ref.block_sums(c, alp_ref["S"], 6) for c in contigs]
    on = _on_off(monkeypatch, contigs, alp_ref, 30.0, 6, W, ohits, sums)
    assert len(ohits) >= 8
    assert 0 <= on["D1"][5] < orc.int_threshold(30.0, 6, alp_ref["N"])


@pytest.mark.parametrize("k,nk", [(5, 17), (6, 284), (5, 383)])
def test_threshold_on_a_windows_distance(monkeypatch, k, nk):
    """thr exactly on a window's distance: guard-band windows are the same with the sums fused."""
    c = cell(k, 7, nk)
    D = c["D"][len(c["contigs"]) - 1]                                   # the long record
    scale = 2.0 * k * 7 * 7
    target = 1.15 * D[LONG - c["W"]]
    s = int(np.argmin(np.abs(D[1:] - target))) + 1
    thr = float(D[s]) / scale
    T, T_hi = filter_ref.threshold_band(thr, k, 7)
    assert T == D[s] <= T_hi
    ohits, _ = orc.single_scan(c["contigs"], c["ref"]["RV"], k, c["W"], thr, BUFF)
    on = _on_off(monkeypatch, c["contigs"], c["ref"], thr, k, c["W"], ohits, c["sums"])
    assert on["counts"][2] > 0 and [len(c["contigs"]) - 1, 1, s + 1] in on["att"].tolist()


@pytest.mark.parametrize("k", [5, 6])
def test_wide_entries_keep_the_two_kernels(monkeypatch, k):
    """A reference with an S entry of 256 or more: the plain pack and the looking-up filter run, whatever the switch says."""
    c = cell(k, 300, 17)
    assert int(c["ref"]["S"].max()) >= 256
    _on_off(monkeypatch, c["contigs"], c["ref"], c["thr"], k, c["W"], c["ohits"], None, fused_form=False)


def _status(monkeypatch, contigs, ref, thr, fuse, k):
    try:
        _steps(monkeypatch, contigs, ref, thr, 0, fuse, k, read_sums=False)
    except _lib.KgmaError as e:
        return e.status, e.message
    return 0, ""


@pytest.mark.parametrize("where", ["full_words", "last_partial_word"])
def test_bad_residue(monkeypatch, where):
    """An X inside a run of full words and in a record's last partial word: same status, record and position."""
    c = cell(6, 7, 284)
    contigs = list(c["contigs"])
    r, pos = (len(contigs) - 1, 40 * 2048 + 777) if where == "full_words" else (2, 32768 + 29)
    a = bytearray(contigs[r]); a[pos] = ord("X"); contigs[r] = bytes(a)
    on = _status(monkeypatch, contigs, c["ref"], c["thr"], True, 6)
    off = _status(monkeypatch, contigs, c["ref"], c["thr"], False, 6)
    assert on == off
    assert on[0] == _lib.KGMA_E_BADBASE and "record %d position %d" % (r, pos + 1) in on[1], on


def test_repeated_steps_and_a_plain_scan(monkeypatch):
    """Three steps on one context with a gene planted before the third: both paths agree after every step (no stale sums, no
    left-over counter); a plain scan afterwards runs the looking-up filter."""
    c = cell(6, 7, 284)
    k, W, ref = 6, c["W"], c["ref"]
    last = len(c["contigs"]) - 1
    gene = mutate(np.random.default_rng(6503), ref["base"], 0.03)
    pokes = (None, (last, 90_001, gene))
    flags = _lib.F_CHAIN_REPLAY
    on, on_plain = _steps(monkeypatch, c["contigs"], ref, c["thr"], flags, True, k, pokes=pokes)
    off, off_plain = _steps(monkeypatch, c["contigs"], ref, c["thr"], flags, False, k, pokes=pokes)
    want_form = fc.form_of(k, int(ref["S"].max()))
    for a, b in zip(on, off):
        _same(a, b)
        assert a["fs"]["form"] == want_form | PRESUMMED and b["fs"]["form"] == want_form
    _same(on[0], on[1])
    _check_sums(on[0]["sums"], c["sums"])
    poked = bytearray(c["contigs"][last]); poked[90_000:90_000 + W] = gene
    contigs2 = list(c["contigs"][:last]) + [bytes(poked)]
    _check_sums(on[2]["sums"], [sums_ref.block_sums(x, ref["S"], k) for x in contigs2])
    assert len(on[2]["hits"]) == len(on[1]["hits"]) + 1
    ohits, _ = orc.single_scan(contigs2, ref["RV"], k, W, c["thr"], BUFF)
    assert [hit_key(h) for h in on[2]["hits"]] == [hit_key(h) for h in ohits]
    _same(on_plain, off_plain)
    _same(on_plain, on[2])
    assert on_plain["fs"]["ran"] == 1 and on_plain["fs"]["form"] == want_form      # bit 16 clear: the sums are only good inside their step


def test_block_sums_need_a_fused_step(monkeypatch):
    c = cell(6, 7, 17)
    monkeypatch.setenv("KGMA_FUSE_SUMS", "0")
    ctx = _lib.Context(0)
    try:
        ctx.set_refs(6, [c["ref"]["RV"]], [c["W"]], [c["thr"]], [7])
        g = ctx.genome_from_host(c["contigs"])
        ctx.step_hits(g, _lib.MODE_SINGLE, BUFF, 0, 0)
        with pytest.raises(_lib.KgmaError) as ei:
            ctx.get_block_sums(g, 0)
        assert ei.value.status == _lib.KGMA_E_STATE
        g.free()
    finally:
        ctx.close()


def _planes_run(monkeypatch, c, fuse, gene, last):
    """A bit-sliced scan (it makes the genome's bit-plane copy), two steps with a gene planted between them, and a bit-sliced scan of
    the planes the last step's pack wrote."""
    monkeypatch.setenv("KGMA_FUSE_SUMS", "1" if fuse else "0")
    ctx = _lib.Context(0)
    g = None
    try:
        ctx.set_refs(6, [c["ref"]["RV"]], [c["W"]], [c["thr"]], [7])
        g = ctx.genome_from_host(c["contigs"])
        monkeypatch.setenv("KGMA_KERNEL", "bitslice")
        ctx.scan(g, _lib.MODE_SINGLE, BUFF, 0, 0, None)
        assert ctx.kernel_name().startswith("scan_kernel")
        monkeypatch.delenv("KGMA_KERNEL")
        ctx.step_hits(g, _lib.MODE_SINGLE, BUFF, 0, 0)
        first = _collect(ctx, g, fuse, len(c["contigs"]))
        g.poke(last, 90_001, gene)
        ctx.step_hits(g, _lib.MODE_SINGLE, BUFF, 0, 0)
        second = _collect(ctx, g, fuse, len(c["contigs"]))
        monkeypatch.setenv("KGMA_KERNEL", "bitslice")
        ctx.scan(g, _lib.MODE_SINGLE, BUFF, 0, 0, None)
        planes = dict(hits=ctx.hits(), dips=ctx.dips(), D1=ctx.first_window(1))
        monkeypatch.delenv("KGMA_KERNEL")
        return first, second, planes
    finally:
        if g is not None:
            g.free()
        ctx.close()


def test_genome_with_bit_planes(monkeypatch):
    """A genome that keeps the bit-plane copy: the fused pack writes the planes too, through pack_word, and they are the plain pack's."""
    c = cell(6, 7, 284)
    last = len(c["contigs"]) - 1
    gene = mutate(np.random.default_rng(6504), c["ref"]["base"], 0.03)
    on = _planes_run(monkeypatch, c, True, gene, last)
    off = _planes_run(monkeypatch, c, False, gene, last)
    for a, b in zip(on[:2], off[:2]):
        _same(a, b)
        assert a["fs"]["form"] == b["fs"]["form"] | PRESUMMED
    _check_sums(on[0]["sums"], c["sums"])
    assert len(on[1]["hits"]) == len(on[0]["hits"]) + 1
    assert on[2]["hits"] == off[2]["hits"] and on[2]["dips"] == off[2]["dips"] and np.array_equal(on[2]["D1"], off[2]["D1"])
    assert len(on[2]["hits"]) == len(on[1]["hits"])
