"""align_kernel (kgma_align.hip, through kgma_align_hits_device) against the aligner's model stated on its own (tests/align_ref.py).

For every job of every batch, two assertions:
  * the device score equals align_ref.optimum -- the independent check;
  * the device (first, last) equals cigar_to_UnitRange of the host aligner's CIGAR -- the choice among co-optimal alignments follows
    the host restatement, whose score and CIGAR tests/test_align_host.py checks against the same model.
Shapes: consensus and segment lengths around the 64-row strips and the 64-lane wavefront, five gap models (one with free gap opening,
where nearly every cell is a tie), low-complexity and off-alphabet input, segments at the edges of several records, the 8191-residue
segment limit inside a batch of short jobs, a call cut into two launches, the 65535-residue consensus limit, and calls of different
geometry on one context."""
import functools

import numpy as np
import pytest

from kmergma_amd import _lib, align
from tests import align_cases as ac
from tests import align_ref as ar

pytestmark = pytest.mark.gpu

GAPS = [(-69, -1), (-200, -1), (-5, -3), (-69, -5), (0, -1)]
MAX_SEGMENT = 8191       # KGMA_ALIGN_MAX_SEGMENT
MAX_CONSENSUS = 65535    # KGMA_ALIGN_MAX_CONSENSUS


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)          # no references are set on this context: the aligner needs none
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def expected(cons, seg, go, ge):
    """(the model's optimum, cigar_to_UnitRange of the host CIGAR): computed once per distinct job."""
    cigar, _ = align.semiglobal_cigar(cons, seg, go, ge)
    return ar.optimum(cons, seg, go, ge), align.cigar_to_UnitRange(cigar)


def device(ctx, g, cons, go, ge, jobs):
    first, last, score = ctx.align_hits_device(g, cons, go, ge, [j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs])
    return [(int(s), (int(a), int(b))) for s, a, b in zip(score, first, last)]


def check_jobs(ctx, records, cons, go, ge, jobs, g=None):
    """jobs: (record, lo, hi), 1-based inclusive.  Every job's score and range are asserted."""
    own = g is None
    if own:
        g = ctx.genome_from_host(records)
    try:
        got = device(ctx, g, cons, go, ge, jobs)
    finally:
        if own:
            g.free()
    assert len(got) == len(jobs)
    for k, (r, lo, hi) in enumerate(jobs):
        want = expected(bytes(cons), bytes(records[r][lo - 1:hi]), go, ge)
        assert got[k][0] == want[0], ("score", k, len(cons), hi - lo + 1, go, ge, got[k], want)
        assert got[k][1] == want[1], ("range", k, len(cons), hi - lo + 1, go, ge, got[k], want)
    return got


def pack(segs, lead=b"", tail=b""):
    """One record holding the segments back to back, and their jobs on record 0."""
    rec = lead + b"".join(segs) + tail
    pos = len(lead) + np.cumsum([0] + [len(s) for s in segs])
    return rec, [(0, int(pos[k]) + 1, int(pos[k + 1])) for k in range(len(segs))]


def segment_of_length(rng, cons, n):
    """A mutated copy of the consensus cut or padded to n residues where n >= m/2, random sequence otherwise."""
    if 2 * n < len(cons):
        return ac.rand_seq(rng, n)
    s = ac.mutated(rng, cons, flank=0)
    if len(s) < n:
        left = int(rng.integers(0, n - len(s) + 1))
        return ac.rand_seq(rng, left) + s + ac.rand_seq(rng, n - len(s) - left)
    off = int(rng.integers(0, len(s) - n + 1))
    return s[off:off + n]


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 127, 128, 129, 192, 193])
def test_strip_and_wave_boundaries(ctx, m):
    """One batch per consensus length and gap model; the segment lengths sit around the wavefront's 64 lanes and around m."""
    rng = np.random.default_rng(300 + m)
    cons = ac.rand_seq(rng, m)
    ns = sorted({n for n in (1, 2, 62, 63, 64, 65, 66, 127, 128, 129, m - 1, m, m + 1) if n >= 1})
    segs = [segment_of_length(rng, cons, n) for n in ns]
    assert [len(s) for s in segs] == ns
    rec, jobs = pack(segs)
    g = ctx.genome_from_host([rec])
    try:
        for go, ge in GAPS:
            check_jobs(ctx, [rec], cons, go, ge, jobs, g)
    finally:
        g.free()


def test_low_complexity_and_alphabet_cases(ctx):
    """Homopolymers, (AC)^r, N, lower case and bytes outside ACGTN, read from a resident genome (stored, never scanned)."""
    cases = ac.low_complexity_cases()
    rec, jobs = pack([b for _, b in cases], lead=b"-r", tail=b"N")
    g = ctx.genome_from_host([rec])
    try:
        for (a, _), job in zip(cases, jobs):
            for go, ge in ac.LOW_COMPLEXITY_GAPS:
                check_jobs(ctx, [rec], a, go, ge, [job], g)
        # and the segments of all cases in one batch against one tie-rich consensus
        for go, ge in GAPS:
            check_jobs(ctx, [rec], b"AC" * 32, go, ge, jobs, g)
    finally:
        g.free()


def test_record_geometry(ctx):
    """Segments in records other than the first, at a record's first and last residue, at odd offsets, a whole record, a one-residue
    record, and the same range twice in one batch."""
    rng = np.random.default_rng(77)
    cons = ac.rand_seq(rng, 150)
    recs = [ac.rand_seq(rng, 333), ac.rand_seq(rng, 41) + ac.mutated(rng, cons, 0) + ac.rand_seq(rng, 501), b"G",
            ac.mutated(rng, cons, 0) + ac.rand_seq(rng, 97) + ac.mutated(rng, cons, 0), ac.mutated(rng, cons, 30)]
    L = [len(r) for r in recs]
    jobs = [(1, 1, L[1]), (1, 1, 200), (1, 42, 42 + 170), (1, L[1] - 256, L[1]), (0, 1, 1), (0, L[0], L[0]), (0, 7, 333), (2, 1, 1),
            (3, 1, 163), (3, L[3] - 162, L[3]), (3, 1, L[3]), (3, 13, L[3] - 17), (4, 1, L[4]), (1, 42, 42 + 170), (3, 1, L[3]),
            (4, 3, L[4] - 1), (0, 1, 1)]
    for go, ge in ((-69, -1), (-5, -3)):
        got = check_jobs(ctx, recs, cons, go, ge, jobs)
        assert got[2] == got[13] and got[10] == got[14] and got[4] == got[16]


def long_segment(rng, cons, n=MAX_SEGMENT):
    """n random residues with the consensus planted in two pieces, far apart."""
    s = bytearray(ac.rand_seq(rng, n))
    h = len(cons) // 2
    s[1000:1000 + h] = cons[:h]
    s[6000:6000 + len(cons) - h] = cons[h:]
    assert len(s) == n
    return bytes(s)


@pytest.fixture(scope="module")
def limit_batch():
    rng = np.random.default_rng(8191)
    cons = ac.rand_seq(rng, 300)
    short = [segment_of_length(rng, cons, n) for n in [1, 2, 3, 64, 150, 299, 300] + rng.integers(1, 301, size=23).tolist()]
    rec0, jobs0 = pack(short[:15], lead=b"ACG")
    rec1, jobs1 = pack(short[15:] + [long_segment(rng, cons)], lead=b"T" * 9)        # the long job ends with its record
    jobs = jobs0 + [(1, lo, hi) for _, lo, hi in jobs1]
    jobs.insert(11, jobs.pop())                                                      # ... and sits in the middle of the batch
    assert sum(hi - lo + 1 == MAX_SEGMENT for _, lo, hi in jobs) == 1 and len(jobs) == 31 and jobs[11][2] == len(rec1)
    return cons, [rec0, rec1], jobs


def test_the_segment_limit_sets_the_layout_for_short_jobs(ctx, limit_batch):
    """One job of exactly 8191 residues sets max_n -- the LDS layout and the trace stride -- for thirty jobs of 1 to 300."""
    cons, recs, jobs = limit_batch
    check_jobs(ctx, recs, cons, -69, -1, jobs)
    check_jobs(ctx, recs, cons, -5, -3, jobs[:12])


def test_a_segment_past_the_limit_is_refused(ctx):
    rec = b"ACGT" * 2100
    g = ctx.genome_from_host([rec])
    try:
        with pytest.raises(_lib.KgmaError) as ei:
            ctx.align_hits_device(g, b"ACGTTGCA", -69, -1, [0, 0, 0, 0], [1, 5, 9, 2], [10, 50, 99, MAX_SEGMENT + 2])
        assert ei.value.status == _lib.KGMA_E_UNSUPPORTED and "hit 3" in ei.value.message and "8192" in ei.value.message
        check_jobs(ctx, [rec], b"ACGTTGCA", -69, -1, [(0, 2, MAX_SEGMENT + 1), (0, 1, 10)], g)     # 8191 is served, and after an error
    finally:
        g.free()


def test_a_call_cut_into_two_launches(ctx):
    """m = 700 is 11 strips; with one 8191-residue job the trace stride is 11 * (8191 + 63) * 64 bytes, so 184 jobs fill the 1 GiB
    the call may allocate and 200 jobs take two launches.  One long job in each launch; every job of both is checked."""
    rng = np.random.default_rng(184)
    cons = ac.rand_seq(rng, 700)
    stride = (11 * (MAX_SEGMENT + 63) * 64 + 255) & ~255      # per job, rounded up to 256 bytes
    assert (1 << 30) // stride == 184
    pieces = [cons[int(o):int(o) + int(n)] for o, n in zip(rng.integers(0, 640, size=40), rng.integers(1, 61, size=40))]
    segs = [pieces[k % 40] if k % 5 else ac.rand_seq(rng, 1 + k % 60) for k in range(200)]
    segs[100] = long_segment(rng, cons)
    segs[190] = long_segment(rng, cons)
    rec, jobs = pack(segs)
    check_jobs(ctx, [rec], cons, -69, -1, jobs)


def test_the_longest_consensus(ctx):
    """m = 65535 (1024 strips) against segments of 1, 50 and 300 residues; |gap_open| + m * |gap_extend| = 327744 < 2^28."""
    rng = np.random.default_rng(65535)
    cons = ac.rand_seq(rng, MAX_CONSENSUS)
    segs = [b"C", ac.rand_seq(rng, 50), ac.mutated(rng, cons[40000:40290], flank=0)[:300].ljust(300, b"A")]
    assert [len(s) for s in segs] == [1, 50, 300] and 69 + 5 * MAX_CONSENSUS < 1 << 28
    rec, jobs = pack(segs, lead=b"N")
    g = ctx.genome_from_host([rec])
    try:
        check_jobs(ctx, [rec], cons, -69, -5, jobs, g)
        with pytest.raises(_lib.KgmaError) as ei:
            ctx.align_hits_device(g, cons + b"A", -69, -5, [0], [1], [10])
        assert ei.value.status == _lib.KGMA_E_UNSUPPORTED and "65536" in ei.value.message
    finally:
        g.free()


def test_state_between_calls(ctx, limit_batch):
    """A call with a large consensus and max_n, then m = 1 against n = 1, then the first call again: the dynamic-LDS size is set per
    call, and nothing of one call's geometry survives into the next."""
    cons, recs, jobs = limit_batch
    g = ctx.genome_from_host(recs)
    try:
        one = check_jobs(ctx, recs, cons, -69, -1, jobs, g)
        check_jobs(ctx, recs, b"A", -69, -1, [(0, 1, 1)], g)
        check_jobs(ctx, recs, b"C", -69, -1, [(0, 2, 2)], g)
        assert check_jobs(ctx, recs, cons, -69, -1, jobs, g) == one
    finally:
        g.free()
