"""Case builders of the k-mer counting tests (tests/test_spectrum_host.py checks that they hit what they are for;
tests/test_gpu_spectrum.py runs them on the device with the geometry the library reports in kgma_get_spectrum_stats).

A case is a Case(name, records, k, ranges, flags, bad): ranges are (record 0-based, lo, hi 1-based inclusive) triples, `bad` the
(record, position) KGMA_E_BADBASE must name, or None.  `span` is the number of considered starts of a unit of work of the form
under test: the seams of the kernel lie at its multiples, counted from a range's lo."""
from typing import NamedTuple, Optional

import numpy as np

from tests import spectrum_ref as model

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
FORM_WG, FORM_WAVE, FORM_GLOBAL = 0, 1, 2
FORM_NAMES = ("wg", "wave", "global")
FORM_KS = {FORM_WG: range(1, 8), FORM_WAVE: range(1, 5), FORM_GLOBAL: range(1, 11)}     # the k every form serves
HOST_SPANS = {FORM_WG: 8192, FORM_WAVE: 1024, FORM_GLOBAL: 8192}                        # what the host test builds the cases with
FLAG_SETS = (0, model.SKIP_N, model.SKIP_MASKED, model.SKIP_N | model.SKIP_MASKED, model.BY_START,
             model.BY_START | model.SKIP_N | model.SKIP_MASKED)


class Case(NamedTuple):
    name: str
    records: list
    k: int
    ranges: list
    flags: int
    bad: Optional[tuple]


def rand_dna(rng, n) -> bytes:
    return BASES[rng.integers(0, 4, size=n)].tobytes()


def auto_form(k, n_starts_total, n_ranges, wg_span=HOST_SPANS[FORM_WG]) -> int:
    """The form the library chooses unforced."""
    if k > 7:
        return FORM_GLOBAL
    return FORM_WAVE if k <= 4 and n_starts_total < n_ranges * wg_span else FORM_WG


def max_ranges(k) -> int:
    return 4 if k >= 9 else 12 if k == 8 else 1000


def seam_record(rng, k, span) -> bytes:
    """5 spans and a little of random A/C/G/T with, counted from residue 5 (the lo of the seam ranges): single Ns on either
    side of the first seam, a run of N across the second, a lower-case stretch across the third and a lower-case n."""
    t = bytearray(rand_dna(rng, 5 * span + k + 60))
    lo0 = 4                                                   # 0-based residue of lo = 5
    t[lo0 + span - 1] = ord("N")                              # the last residue in front of the seam
    t[lo0 + span + k] = ord("N")
    t[lo0 + 2 * span - 3:lo0 + 2 * span + 6] = b"N" * 9
    t[lo0 + 3 * span - 20:lo0 + 3 * span + 20] = bytes(t[lo0 + 3 * span - 20:lo0 + 3 * span + 20]).lower()
    t[lo0 + 3 * span + 100] = ord("n")
    t[40:44] = b"acgt"
    return bytes(t)


def core_case(k, span, flags, *, mean_at_least=None, seed=0) -> Case:
    """The ranges every form must get right at one k: a whole record; lengths 0, k - 1, k, k + 1 at a record's first and last
    residue; lo at each of 16 consecutive residues; ranges whose considered starts end 1 before, at and 1 behind a unit seam; a
    range of 3 spans + 1 starts; a second record; duplicates, overlaps, no order.  mean_at_least: whole-record duplicates are
    added until the mean number of considered starts per range reaches it (the unforced choice is then `wg` at k <= 7)."""
    rng = np.random.default_rng(1000 * k + span + seed)
    rec0, rec1 = seam_record(rng, k, span), rand_dna(rng, 1500 + k)[:-3] + b"NnN"
    L0, L1 = len(rec0), len(rec1)
    by_start = bool(flags & model.BY_START)

    def with_starts(lo, n):                                   # the range from lo with n considered starts
        return (0, lo, lo + n - 1) if by_start else (0, lo, lo + n + k - 2)

    long_ranges = [(0, 1, L0), with_starts(5, 3 * span + 1), with_starts(5, span - 1), with_starts(5, span), with_starts(5, span + 1)]
    edge = [(0, 1, 0), (0, 1, k - 1), (0, 1, k), (0, 1, k + 1), (0, L0 + 1, L0), (0, L0 - k + 2, L0), (0, L0 - k + 1, L0), (0, L0 - k, L0)]
    offsets = [(0, 17 + o, 17 + o + span + span // 2 + 3 * o) for o in range(16)]
    other = [(1, 1, L1), (1, 1, L1), (1, 7, L1 - 9), (1, L1, L1), (0, 3 * span, 3 * span + 50)]
    cap = max_ranges(k)
    if cap <= 4:
        ranges = [long_ranges[1], long_ranges[3], edge[6], other[0]]
    elif cap <= 12:
        ranges = long_ranges[1:] + edge[1:4] + offsets[:2] + other[:3]
    else:
        ranges = long_ranges + edge + offsets + other
    order = rng.permutation(len(ranges))
    ranges = [ranges[i] for i in order]
    if mean_at_least is not None:
        while model.n_considered([rec0, rec1], k, ranges, flags).mean() < mean_at_least and len(ranges) < cap:
            ranges.append((0, 1, L0))
    return Case(f"k{k}_span{span}_flags{flags}", [rec0, rec1], k, ranges, flags, None)


def tiling_case(k, span, bin_width, flags=model.BY_START, length=None) -> Case:
    """BY_START bins of `bin_width` starts over both records of the core case (cut to `length` residues), and the two whole
    records last: the bins' rows sum to the whole rows."""
    base = core_case(k, span, flags)
    base = base._replace(records=[r[:length] for r in base.records])
    ranges = []
    for c, rec in enumerate(base.records):
        L = len(rec)
        ranges += [(c, lo, min(lo + bin_width - 1, L)) for lo in range(1, L + 1, bin_width)]
    ranges += [(c, 1, len(rec)) for c, rec in enumerate(base.records)]
    return Case(f"tiling_k{k}_bin{bin_width}", base.records, k, ranges, flags | model.BY_START, None)


def contention_cases(k=6):
    """Counts above 65,535 on one k-mer (a 16-bit table, a lost wave-aggregated add), and two alternating k-mers (the
    wave-uniform path must not fire)."""
    n = 70_000
    recs = [b"A" * n, b"N" * n, b"AC" * (n // 2), b"ACGT" * 50 + b"T" * n + b"ACGT" * 50]
    whole = [(c, 1, len(r)) for c, r in enumerate(recs)]
    return [Case(f"contention_k{k}_flags{f}", recs, k, whole + [(0, 3, 66_000), (1, 2, 2)], f, None) for f in (0, model.SKIP_N)]


def iupac_cases(k, span):
    """An R inside a range, at flags == 0 (KGMA_E_BADBASE with its record and position) and with SKIP_N (skipped); the same
    byte outside every range (no error); two bad bytes in two ranges given in descending order (the smallest is named); a bad
    byte only the k - 1 residues behind hi cover (an error with BY_START alone)."""
    rng = np.random.default_rng(77 + k)
    r0, r1 = bytearray(rand_dna(rng, span + 500)), bytearray(rand_dna(rng, 900))
    r0[span + 10] = ord("R")                                  # position span + 11
    r1[99], r1[399] = ord("y"), ord("*")                      # positions 100 and 400
    recs = [bytes(r0), bytes(r1)]
    inside = [(1, 350, 450), (0, 1, len(r0)), (1, 50, 150)]
    out = [Case("r_inside", recs, k, inside, 0, (0, span + 11)),
           Case("r_inside_by_start", recs, k, inside, model.BY_START, (0, span + 11)),
           Case("r_skipped", recs, k, inside, model.SKIP_N, None),
           Case("r_masked_only", recs, k, inside, model.SKIP_MASKED, (0, span + 11)),
           Case("second_record_descending", recs, k, [(1, 350, 450), (1, 50, 150)], 0, (1, 100)),
           Case("r_outside", recs, k, [(0, 1, span + 10), (0, span + 12, len(r0)), (1, 101, 399), (1, 401, 900), (1, 100, 99)], 0, None),
           Case("short_range_is_looked_up", recs, k, [(1, 400, 400)], 0, (1, 400))]
    if k > 1:
        out.append(Case("behind_hi_by_start", recs, k, [(1, 398, 399)], model.BY_START, (1, 400)))
        out.append(Case("behind_hi_default", recs, k, [(1, 398, 399)], 0, None))
    return out


def masked_record(rng, n=6000):
    """Random DNA with lower-case blocks and N runs, as a soft-masked assembly has them."""
    t = bytearray(rand_dna(rng, n))
    for lo, hi in ((0, 37), (100, 101), (1000, 1999), (2500, 2516), (n - 33, n)):
        t[lo:hi] = bytes(t[lo:hi]).lower()
    t[1500:1520] = b"n" * 20
    t[3000:3040] = b"N" * 40
    return bytes(t)


def expected(case):
    """(counts, skipped) of the model, or the BadBase it raises."""
    try:
        return model.kmer_count(case.records, case.k, case.ranges, case.flags)
    except model.BadBase as e:
        return e
