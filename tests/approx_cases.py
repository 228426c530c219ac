"""Case builders of the edit-distance search tests (tests/test_approx_host.py checks that every list hits what it is for;
tests/test_gpu_approx.py runs them on the device with the library's real geometry).

A case is a Case(name, queries, max_edits, records, best_only, aim): `aim` says what the case is for in a form the host test
checks -- {"end": j, "record": c, "edits": k, ...} names a matching end the oracle must report there."""
from typing import NamedTuple

import numpy as np

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
WORD_LENGTHS = (1, 2, 31, 32, 33, 63, 64)
SYMS = b"ACGTRYSWKMBDHVN"


class Case(NamedTuple):
    name: str
    queries: list
    max_edits: list
    records: list
    best_only: bool
    aim: dict


def rand_dna(rng, n) -> bytes:
    return BASES[rng.integers(0, 4, size=n)].tobytes()


def other_base(ch: int, step: int = 1) -> bytes:
    return b"ACGT"[(b"ACGT".index(ch) + step) % 4:][:1]


def substituted(q: bytes, pos: int) -> bytes:
    """q with symbol `pos` (1-based) changed to a base that differs from it and from both neighbours."""
    near = set(q[max(0, pos - 2):pos + 1])
    return q[:pos - 1] + next(bytes([b]) for b in b"ACGT" if b not in near) + q[pos:]


def deleted(q: bytes, pos: int) -> bytes:
    return q[:pos - 1] + q[pos:]


def inserted(q: bytes, pos: int) -> bytes:
    """q with a base inserted before symbol `pos` that differs from both neighbours."""
    near = {q[pos - 1]} | ({q[pos - 2]} if pos >= 2 else set())
    extra = next(bytes([b]) for b in b"ACGT" if b not in near)
    return q[:pos - 1] + extra + q[pos - 1:]


def plain_query(rng, m: int) -> bytes:
    """A/C/G/T, no two neighbours equal (an inserted or deleted base cannot be explained as a shift in a homopolymer)."""
    out = [int(rng.integers(0, 4))]
    while len(out) < m:
        out.append((out[-1] + int(rng.integers(1, 4))) % 4)
    return BASES[np.array(out)].tobytes()


def place(background: bytearray, end: int, occ: bytes) -> None:
    """Lay `occ` so that its last residue is position `end` (1-based)."""
    assert end - len(occ) >= 0 and end <= len(background), (end, len(occ), len(background))
    background[end - len(occ):end] = occ


# ---- word seams -----------------------------------------------------------------------------------------------------------------
def word_seam_cases(seed: int = 11) -> list:
    rng = np.random.default_rng(seed)
    out = []
    for m in WORD_LENGTHS:
        q = plain_query(rng, m)
        text = bytearray(rand_dna(rng, 400))
        place(text, 100, q)
        if m >= 2:
            place(text, 200, substituted(q, (m + 1) // 2))
            place(text, 300, deleted(q, m // 2 + 1))
        for e in (0, 1, 15):
            if e < m:
                out.append(Case(f"m{m}_e{e}", [q], [e], [bytes(text)], False, {"record": 0, "end": 100, "edits": 0}))
    q = plain_query(rng, 64)
    base = rand_dna(rng, 150)
    out.append(Case("carry_through_bit31", [q], [0], [base + q + base], False, {"record": 0, "end": 214, "edits": 0}))
    for pos in (1, 32, 33, 64):
        for kind, occ in (("sub", substituted(q, pos)), ("ins", inserted(q, pos)), ("del", deleted(q, pos))):
            # (a deleted first / last symbol is also a shorter match one column away: the case holds whatever the oracle says)
            out.append(Case(f"m64_{kind}_{pos}", [q], [1], [base + occ + base], False, {"record": 0, "edits": 1, "any_end": True}))
    return out


# ---- tile seams -----------------------------------------------------------------------------------------------------------------
def seams(tile: int, wg_bases: int) -> dict:
    """The last end position (1-based) of a lane's tile, of a wave's ends and of a workgroup's ends."""
    return {"tile": 3 * tile, "wave": 64 * tile, "wg": wg_bases}


def tile_seam_cases(tile: int, wg_bases: int, seed: int = 12) -> list:
    rng = np.random.default_rng(seed)
    out = []
    m, e = 20, 2
    q = plain_query(rng, m)
    for kind, B in seams(tile, wg_bases).items():
        L = B + 200
        # an occurrence ending at B - 1, B, B + 1: three records
        recs = []
        for dlt in (-1, 0, 1):
            t = bytearray(rand_dna(rng, L))
            place(t, B + dlt, q)
            recs.append(bytes(t))
        out.append(Case(f"end_around_{kind}_seam", [q], [e], recs, True, {"ends": [(c, B + c - 1, 0) for c in range(3)]}))
        # m + e residues, every edit an insertion, beginning before the seam: its end is owned by the lane behind the seam and
        # the warm-up has to reach its first residue
        occ = inserted(inserted(q, 15), 6)
        assert len(occ) == m + e
        recs = []
        for first in (B, B - 1):                              # begins on the seam's last position / one before it
            t = bytearray(rand_dna(rng, L))
            place(t, first + m + e - 1, occ)
            recs.append(bytes(t))
        out.append(Case(f"insertions_begin_before_{kind}_seam", [q], [e], recs, False,
                        {"ends": [(0, B + m + e - 1, e), (1, B + m + e - 2, e)], "length": m + e, "begins_at_or_before": B}))
        # a run of matching ends across the seam under best_only: the minimum before it, behind it, and a tie on both sides
        recs, want = [], []
        for j in (B - 1, B + 2):                              # runs j - 2 .. j + 2
            t = bytearray(rand_dna(rng, L))
            place(t, j, q)
            recs.append(bytes(t))
            want.append((len(recs) - 1, j, 0))
        t = bytearray(rand_dna(rng, L))
        tie = q[:-1] + other_base(q[-1])                      # ends B (last symbol deleted) and B + 1 (substituted): 1 edit each
        place(t, B + 1, tie)
        recs.append(bytes(t))
        want.append((2, B, 1))
        out.append(Case(f"run_across_{kind}_seam", [q], [e], recs, True, {"ends": want, "tie": (2, B, B + 1, 1)}))
    return out


# ---- records --------------------------------------------------------------------------------------------------------------------
def record_cases(seed: int = 13) -> list:
    rng = np.random.default_rng(seed)
    m, e = 24, 2
    q = plain_query(rng, m)
    out = []
    shorter = deleted(deleted(q, 17), 5)                      # m - e residues: e deletions
    longer = inserted(inserted(q, 17), 5)                     # m + e residues: e insertions
    recs = [b"", q[:1], shorter[:-1], shorter, q, longer]
    out.append(Case("record_lengths", [q], [e], recs, False, {"lengths": [0, 1, m - e - 1, m - e, m, m + e], "ends": [(3, m - e, e), (4, m, 0), (5, m + e, e)]}))
    out.append(Case("record_lengths_best", [q], [e], recs, True, {"ends": [(3, m - e, e), (4, m, 0), (5, m + e, e)]}))
    a, b = rand_dna(rng, 60), rand_dna(rng, 60)
    out.append(Case("query_cut_by_a_record_boundary", [q], [e], [a + q[:12], q[12:] + b], False, {"none": True}))
    tiny = [rand_dna(rng, int(n)) for n in rng.integers(1, 4, size=300)]
    out.append(Case("300_tiny_records_first", [q], [e], tiny + [a + q + b], True, {"ends": [(300, 60 + m, 0)]}))
    out.append(Case("hit_ends_on_the_last_residue", [q], [e], [a + b + q], True, {"ends": [(0, 120 + m, 0)]}))
    out.append(Case("hit_starts_on_the_first_residue", [q], [e], [q + a, substituted(q, 2) + b], True, {"ends": [(0, m, 0), (1, m, 1)], "starts": [1, 1]}))
    return out


# ---- alphabet -------------------------------------------------------------------------------------------------------------------
def alphabet_cases(seed: int = 14) -> list:
    rng = np.random.default_rng(seed)
    a, b = rand_dna(rng, 50), rand_dna(rng, 50)
    out = []
    out.append(Case("genome_n_under_query_n", [b"ACGTNNACGTCA"], [0], [a + b"ACGTNNACGTCA" + b + b"ACGTNAACGTCA" + a], False,
                    {"ends": [(0, 62, 0), (0, 124, 0)]}))
    out.append(Case("genome_n_under_query_t", [b"ACGTTTACGTCA"], [1], [a + b"ACGTNTACGTCA" + b + b"ACGTNNACGTCA" + a], False,
                    {"ends": [(0, 62, 1)]}))
    q = b"GATTACAGATTACA"
    out.append(Case("lower_case_genome", [q, q.lower()], [1, 1], [(a + q + b).lower(), a + substituted(q, 7).lower() + b], False,
                    {"ends": [(0, 64, 0), (1, 64, 1)]}))
    # every symbol of the alphabet (set sizes 1 ... 4) against a text that goes through every base and N under each of them
    text = b"".join(bytes([x]) * 15 for x in b"ACGTN") + a
    cyc = b"".join(text[i::15][:5] for i in range(15))
    out.append(Case("iupac_symbols_of_every_set_size", [SYMS, SYMS[::-1], b"RYSWKM", b"BDHV", b"NNANN"], [3, 3, 1, 1, 0],
                    [text, cyc + b + cyc.lower()], False, {"any": True}))
    return out


# ---- batch ----------------------------------------------------------------------------------------------------------------------
def batch_case(seed: int = 15) -> Case:
    rng = np.random.default_rng(seed)
    lens, eds = (5, 12, 20, 31, 32, 33, 47, 64), (0, 1, 2, 3, 2, 1, 4, 5)
    qs = [plain_query(rng, m) for m in lens]
    text = bytearray(rand_dna(rng, 3000))
    for i, q in enumerate(qs):
        place(text, 200 + 300 * i, q)
        if len(q) > 5:
            place(text, 330 + 300 * i, deleted(substituted(q, 3), len(q) // 2))
    return Case("eight_queries", qs, list(eds), [bytes(text), rand_dna(rng, 500)], True, {"ends": [(0, 200 + 300 * i, 0) for i in range(8)], "per_query": True})


def random_case(seed: int = 16) -> Case:
    rng = np.random.default_rng(seed)
    return Case("random_100kb", [plain_query(rng, 8)], [2], [rand_dna(rng, 100_000)], False, {"many": 1000})
