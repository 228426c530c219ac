"""The edit-distance search without a GPU: the oracle's two statements against each other (tests/approx_oracle.py), its start
rule, the warm-up bound the device kernel relies on, what the case lists of tests/approx_cases.py are for, the argument checks
of api.approxMatch, the exported symbols and struct layouts, and tests/golden/approx.json."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from kmergma_amd import _lib, api
from tests import approx_cases as ac
from tests import approx_oracle as ao
from tests.conftest import DATA, GOLDEN, ROOT

TILE, WG_BASES = 256, 32768          # a geometry to build the seam cases with here (the GPU test passes the library's)
ALPHABET = np.frombuffer(b"ACGTN", dtype=np.uint8)


def rand_text(rng, n, with_n=True):
    p = [0.23, 0.23, 0.23, 0.23, 0.08] if with_n else [0.25, 0.25, 0.25, 0.25, 0.0]
    return ALPHABET[rng.choice(5, size=n, p=p)].tobytes()


def rand_query(rng, m):
    syms = np.frombuffer(ac.SYMS, dtype=np.uint8)
    q = syms[rng.choice(len(syms), size=m, p=[0.2] * 4 + [0.2 / 11] * 11)].tobytes()
    return q if any(ch != ord("N") for ch in q) else b"A" + q[1:]


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, 7, 16, 31, 32, 33, 48, 63, 64])
def test_the_two_statements_agree(m):
    rng = np.random.default_rng(100 + m)
    for trial in range(6):
        q = rand_query(rng, m)
        t = bytearray(rand_text(rng, 300))
        if trial % 2 == 0:
            occ = bytes(ALPHABET[[b"ACGT".index(bytes([ch])) if ch in b"ACGT" else 4 for ch in q.upper()]])
            t[100:100 + m] = occ.replace(b"N", b"A") if trial % 4 == 0 else occ
        a, b = ao.scores(q, bytes(t)), ao.bitvector_scores(q, bytes(t))
        assert np.array_equal(a, b), (q, int(np.flatnonzero(a != b)[0]))
        assert a.min() >= 0 and a.max() <= m


def test_scores_of_small_cases_by_hand():
    assert ao.scores(b"ACG", b"TTACGTT").tolist() == [3, 3, 2, 1, 0, 1, 2]
    assert ao.scores(b"ACG", b"AG").tolist() == [2, 1]                        # one symbol deleted
    assert ao.scores(b"ANG", b"ACGANG").tolist()[2] == 0 and ao.scores(b"ACG", b"ANG").tolist()[2] == 1   # a genome N matches only N
    assert ao.scores(b"AN", b"AN").tolist() == [1, 0]
    assert ao.ends(b"ACG", b"TTACGTT", 1) == [(4, 1), (5, 0), (6, 1)]
    assert ao.runs_best([(4, 1), (5, 0), (6, 1), (9, 1), (10, 1)]) == [(5, 0), (9, 1)]
    assert ao.find(b"ACG", b"TTACGTT", 1) == [(3, 5, 0)] and ao.find(b"ACG", b"TTACGTT", 1, False) == [(3, 4, 1), (3, 5, 0), (3, 6, 1)]
    assert ao.revcomp(b"ACGTRYN") == b"NRYACGT"


def brute_edit_distance(qs, rs) -> int:
    D = list(range(len(rs) + 1))
    for i in range(1, len(qs) + 1):
        prev, D[0] = D[0], i
        for j in range(1, len(rs) + 1):
            cur = min(prev + (0 if (rs[j - 1] & ~qs[i - 1] & 15) == 0 else 1), D[j] + 1, D[j - 1] + 1)
            prev, D[j] = D[j], cur
    return D[-1]


def test_start_is_the_largest_start_that_attains_the_score():
    rng = np.random.default_rng(7)
    for trial in range(40):
        m = int(rng.integers(1, 13))
        q, t = rand_query(rng, m), rand_text(rng, 40)
        sc = ao.scores(q, t)
        qs, rs = ao.query_sets(q).tolist(), ao.residue_sets(t).tolist()
        for j in (1, 2, m, 17, 40):
            by_start = [brute_edit_distance(qs, rs[s - 1:j]) for s in range(1, j + 2)]       # s = j + 1: the empty substring
            assert min(by_start) == sc[j - 1]
            want = max(s for s, d in zip(range(1, j + 2), by_start) if d == sc[j - 1])
            assert ao.start_of(q, t, j) == want, (q, t, j)


@pytest.mark.parametrize("m", [1, 2, 5, 20, 31, 32, 33, 63, 64])
def test_warm_up_bound(m):
    """A state made fresh m + e columns before a tile gives scores >= the true ones, equal wherever the true one is <= e."""
    rng = np.random.default_rng(200 + m)
    for e in sorted({0, min(2, m - 1), min(15, m - 1)}):
        q = ac.plain_query(rng, m)
        t = bytearray(rand_text(rng, 700, with_n=False))
        for at in range(40, 700 - m - 20, 97):                                   # occurrences all over the tiles' seams
            occ = q
            for _ in range(int(rng.integers(0, e + 1))):
                occ = ac.inserted(occ, int(rng.integers(1, len(occ) + 1))) if rng.integers(0, 2) else ac.substituted(occ, int(rng.integers(1, len(occ) + 1)))
            t[at:at + len(occ)] = occ
        full = ao.scores(q, bytes(t))
        for tile in (16, 100):
            cut = ao.restarted_scores(q, bytes(t), e, tile)
            assert (cut >= full).all()
            assert np.array_equal(cut <= e, full <= e) and np.array_equal(cut[full <= e], full[full <= e])


# ---- the case lists -------------------------------------------------------------------------------------------------------------
def all_cases():
    return (ac.word_seam_cases() + ac.tile_seam_cases(TILE, WG_BASES) + ac.record_cases() + ac.alphabet_cases() + [ac.batch_case()])


@pytest.fixture(scope="module")
def searched():
    return {c.name: (c, ao.search(c.queries, c.records, c.max_edits, c.best_only)) for c in all_cases()}


def test_case_names_are_unique():
    names = [c.name for c in all_cases()]
    assert len(names) == len(set(names))


def test_word_seam_cases_cover_the_lengths():
    cases = ac.word_seam_cases()
    assert {len(c.queries[0]) for c in cases} == set(ac.WORD_LENGTHS)
    assert {(len(c.queries[0]), c.max_edits[0]) for c in cases} >= {(m, e) for m in ac.WORD_LENGTHS for e in (0, 1, 15) if e < m}
    assert {c.name for c in cases} >= {f"m64_{k}_{p}" for k in ("sub", "ins", "del") for p in (1, 32, 33, 64)}


def test_every_case_hits_what_it_is_for(searched):
    for name, (c, found) in searched.items():
        aim = c.aim
        by_end = {(r, j): (s, k) for qi, r, s, j, k in found if qi == 0}
        if "end" in aim:
            assert by_end[(aim["record"], aim["end"])][1] == aim["edits"], name
        if aim.get("any_end"):
            assert any(r == aim["record"] and k <= aim["edits"] for (r, j), (s, k) in by_end.items()), name
        for r, j, k in aim.get("ends", []) if not aim.get("per_query") else []:
            assert (r, j) in by_end and by_end[(r, j)][1] == k, (name, r, j)
        if aim.get("per_query"):
            assert {(i, r, j, k) for i, (r, j, k) in enumerate(aim["ends"])} <= {(q, r, j, k) for q, r, s, j, k in found}, name
            assert any(k > 0 for q, r, s, j, k in found), name
        if aim.get("none"):
            assert found == [], name
        if aim.get("any"):
            assert len(found) > 20 and len({q for q, *_ in found}) == len(c.queries), name
        if "starts" in aim:
            assert [by_end[(r, j)][0] for r, j, _ in aim["ends"]] == aim["starts"], name
        if "lengths" in aim:
            assert [len(r) for r in c.records] == aim["lengths"], name


def test_seam_cases_lie_on_the_seams(searched):
    for kind, B in ac.seams(TILE, WG_BASES).items():
        assert B % TILE == 0
        c, found = searched[f"end_around_{kind}_seam"]
        assert [(r, j, k) for _, r, s, j, k in found] == [(0, B - 1, 0), (1, B, 0), (2, B + 1, 0)]
        c, found = searched[f"insertions_begin_before_{kind}_seam"]
        for r, j, k in c.aim["ends"]:
            s = next(s for _, r2, s, j2, k2 in found if (r2, j2, k2) == (r, j, k))
            assert j - s + 1 == c.aim["length"] and s <= B < j              # begins in the tile before the seam, ends behind it
        c, found = searched[f"run_across_{kind}_seam"]
        assert [(r, j, k) for _, r, s, j, k in found] == c.aim["ends"]
        r, j0, j1, k = c.aim["tie"]
        sc = ao.scores(c.queries[0], c.records[r])
        assert sc[j0 - 1] == sc[j1 - 1] == k and j0 == B and (sc[j0 - 2:j1 + 1] <= c.max_edits[0]).all()   # one run, the tie across the seam
        for r, (j, side) in enumerate(((B - 1, "before"), (B + 2, "behind"))):
            run = ao.ends(c.queries[0], c.records[r], c.max_edits[0])
            assert run[0][0] <= B < run[-1][0] and (j <= B) == (side == "before")
    assert ac.seams(TILE, WG_BASES)["wave"] == 64 * TILE and ac.seams(TILE, WG_BASES)["wg"] == WG_BASES


# ---- api.approxMatch: the checks come before any device call -----------------------------------------------------------------
class NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before the argument checks")


@pytest.mark.parametrize("query, kw, exc, text", [
    (b"", {}, ValueError, "0 symbols"),
    (b"A" * 65, {}, ValueError, "65 symbols"),
    (b"ACXG", {}, ValueError, "symbol 3"),
    (b"AC-G", {}, ValueError, "symbol 3"),
    (b"ACGT", {"max_edits": 4}, ValueError, "max_edits 4 is not smaller"),
    (b"ACGT", {"max_edits": -1}, ValueError, "max_edits -1"),
    (b"A" * 20, {"max_edits": 16}, ValueError, "max_edits 16"),
    (b"ANNT", {"max_edits": 2}, ValueError, "2 informative"),
    (b"NNNN", {"max_edits": 0}, ValueError, "0 informative"),
    (b"ACGT", {"strand": "x"}, ValueError, ""),
    (12, {}, TypeError, "Invalid"),
])
def test_argument_checks_come_first(query, kw, exc, text):
    for subject in (b"ACGTACGT", "no_such_file.fasta"):
        with pytest.raises(exc) as ei:
            api.approxMatch(query, subject, ctx=NoDevice(), **kw)
        assert text in str(ei.value)
    with pytest.raises(exc):
        api.approxMatch_batch([b"ACGTA", query], "no_such_file.fasta", ctx=NoDevice(), **kw)


def test_batch_needs_one_max_edits_per_query_and_a_subject():
    with pytest.raises(ValueError):
        api.approxMatch_batch([b"ACGT", b"ACGT"], "x.fasta", max_edits=[1], ctx=NoDevice())
    with pytest.raises(TypeError):
        api.approxMatch_batch([b"ACGT"], 17, ctx=NoDevice())
    with pytest.raises(ValueError) as ei:
        api.findRSS_edits("x.fasta", max_edits=16, ctx=NoDevice())
    assert "max_edits 16" in str(ei.value)


# ---- the library's surface --------------------------------------------------------------------------------------------------
def header_struct(name: str) -> str:
    with open(os.path.join(ROOT, "include", "kgma.h")) as f:
        text = f.read()
    return re.search(r"typedef struct \{([^}]*)\} " + name + ";", text).group(1)


def header_fields(name: str) -> list:
    """[(c type, field)] of a struct of include/kgma.h, comments removed, `a, b` declarations split."""
    body = re.sub(r"/\*.*?\*/", "", header_struct(name), flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            out += [(ctype, n.strip()) for n in names.split(",")]
    return out


@pytest.mark.parametrize("name, mirror, size", [("kgma_approx_hit", _lib.KgmaApproxHit, 32), ("kgma_approx_stats", _lib.KgmaApproxStats, 48)])
def test_struct_mirrors_follow_the_header(name, mirror, size):
    ctypes_of = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    fields = header_fields(name)
    assert [(n, t) for n, t in mirror._fields_] == [(n, ctypes_of[t]) for t, n in fields]
    assert C.sizeof(mirror) == size
    off = 0
    for n, t in mirror._fields_:                                             # (natural alignment, no holes)
        assert getattr(mirror, n).offset == off
        off += C.sizeof(t)
    if name == "kgma_approx_hit":
        assert _lib.APPROX_HIT_DTYPE.itemsize == size and list(_lib.APPROX_HIT_DTYPE.names) == [n for n, _ in mirror._fields_]
        assert [_lib.APPROX_HIT_DTYPE.fields[n][1] for n, _ in mirror._fields_] == [getattr(mirror, n).offset for n, _ in mirror._fields_]


def test_symbols_are_exported():
    lib = C.CDLL(_lib.LIB_PATH)                                              # (loading needs no device)
    for name in ("kgma_approx_match", "kgma_get_approx_matches", "kgma_get_approx_stats"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    for name in ("approxMatch", "approxMatch_batch", "findRSS_edits"):
        assert callable(getattr(api, name))
    for name in ("approx_match", "approx_matches", "approx_stats"):
        assert callable(getattr(_lib.Context, name))


# ---- the golden file --------------------------------------------------------------------------------------------------------
ISSUE_COUNTS = {("HumanRSSD", 1, "+"): (13, 7), ("HumanRSSD", 1, "-"): (0, 0), ("HumanRSSD", 2, "+"): (27, 7), ("HumanRSSD", 2, "-"): (9, 9),
                ("HumanRSSV", 1, "+"): (6, 4), ("HumanRSSV", 1, "-"): (0, 0), ("HumanRSSV", 2, "+"): (20, 8), ("HumanRSSV", 2, "-"): (2, 2)}
RSSD_E1_BEST = [(0, 8877, 0), (0, 20759, 1), (2, 1019, 0), (2, 13125, 1), (3, 7186, 1), (3, 24244, 1), (3, 34176, 0)]


@pytest.fixture(scope="module")
def golden_approx():
    with open(os.path.join(GOLDEN, "approx.json")) as f:
        return json.load(f)


def test_golden_file_holds_what_was_recorded(golden_approx):
    assert golden_approx["made_by"] == ao.MADE_BY
    ent = golden_approx["entries"]
    assert set(ent) == {f"{n}|{e}|{s}" for n in ("HumanRSSD", "HumanRSSV") for e in (0, 1, 2) for s in "+-"}
    for (name, e, strand), (n_ends, n_runs) in ISSUE_COUNTS.items():
        v = ent[f"{name}|{e}|{strand}"]
        assert (len(v["all"]), len(v["best"])) == (n_ends, n_runs), (name, e, strand)
    assert [(c, j, k) for c, s, j, k in ent["HumanRSSD|1|+"]["best"]] == RSSD_E1_BEST
    assert ao.HumanRSSD == api.HumanRSSD and ao.HumanRSSV == api.HumanRSSV
    for v in ent.values():                                                   # best is a subset of all; both sorted by (record, end)
        assert all(h in v["all"] for h in v["best"])
        assert v["all"] == sorted(v["all"], key=lambda h: (h[0], h[2])) and all(1 <= s <= j for _, s, j, _ in v["all"])


def test_golden_file_is_rederived_for_record_3(golden_approx):
    rec = ao.read_fasta_sequences(os.path.join(DATA, "Loci.fasta"))[3]
    assert len(rec) == 41260
    for name, motif in ao.GOLDEN_MOTIFS.items():
        for strand, q in (("+", motif), ("-", ao.revcomp(motif))):
            sc = ao.scores(q, rec)                                           # one pass serves e = 0, 1, 2
            for e in ao.GOLDEN_EDITS:
                idx = np.flatnonzero(sc <= e)
                found = list(zip((idx + 1).tolist(), sc[idx].tolist()))
                v = golden_approx["entries"][f"{name}|{e}|{strand}"]
                assert [[3, ao.start_of(q, rec, j), j, k] for j, k in found] == [h for h in v["all"] if h[0] == 3]
                assert [[3, ao.start_of(q, rec, j), j, k] for j, k in ao.runs_best(found)] == [h for h in v["best"] if h[0] == 3]
