"""The hit-buffer protocol the four sequence searches share (csrc/kgma_search.h), pinned at its boundary: a result of exactly the
buffer's first capacity (65,536 records) takes one launch and no memory, one record more takes a second launch and a buffer of
exactly the counted size, and the regrown buffer is kept -- neither regrown again nor shrunk -- by the calls that follow.

One record of L times A, searched for a pattern that matches at every position (and, as the warm-up, for one that matches nowhere),
through kgma_exact_match, kgma_motif_match, kgma_approx_match and kgma_pwm_match, each on a context of its own.

The context publishes its account of device memory in kgma_stats.device_bytes when it scans, so the account is read by a small scan
of a genome of its own (as tests/test_gpu_genome_module.py reads it); the first such scan, which allocates the scan's buffers, is
part of the warm-up."""
import numpy as np
import pytest

from kmergma_amd import _lib

pytestmark = pytest.mark.gpu
FIRST_CAP = 1 << 16


class Search:
    def __init__(self, name, record_bytes, extra_launches, run, fetch, fields):
        self.name, self.record_bytes, self.extra_launches = name, record_bytes, extra_launches
        self.run, self.fetch, self.fields = run, fetch, fields

    def rows(self, ctx):
        m = getattr(ctx, self.fetch)()
        return list(zip(*(m[f].tolist() for f in ("contig",) + self.fields)))


SEARCHES = [
    Search("exact", 16, 0, lambda c, g, base: c.exact_match(g, [base]), "matches", ("start",)),
    Search("motif", 24, 0, lambda c, g, base: c.motif_match(g, [base], [0]), "motif_matches", ("start", "mismatches")),
    # (every end is reported, and each is given its start by a launch of the start kernel: one launch more when there are hits)
    Search("approx", 32, 1, lambda c, g, base: c.approx_match(g, [base], [0], False), "approx_matches", ("start", "end", "edits")),
    Search("pwm", 24, 0, lambda c, g, base: c.pwm_match(g, [[[5 if b == base else 0 for b in (b"A", b"C", b"G", b"T")]]], [5]),
           "pwm_matches", ("start", "score")),
]
WANT = {"exact": lambda p: (0, p), "motif": lambda p: (0, p, 0), "approx": lambda p: (0, p, p, 0), "pwm": lambda p: (0, p, 5)}


@pytest.mark.parametrize("L", [65_536, 65_537, 70_000])
@pytest.mark.parametrize("search", SEARCHES, ids=lambda s: s.name)
def test_regrow_at_the_first_capacity(search, L, alp_ref):
    ctx = _lib.Context(0)
    try:
        ctx.set_refs(6, [alp_ref["RV"]], [alp_ref["ws"]], [30.0], [alp_ref["N"]])
        text = np.random.default_rng(3).integers(0, 4, size=2000, dtype=np.uint8)
        small = np.frombuffer(b"ACGT", dtype=np.uint8)[text].tobytes()

        def device_bytes():
            s = ctx.genome_from_host([small])
            try:
                ctx.scan(s, _lib.MODE_SINGLE, 50, 0, 0, None)
                return ctx.stats()["device_bytes"]
            finally:
                s.free()

        def call(base):
            search.run(ctx, g, base)
            return search.rows(ctx), ctx.stats()["n_launches"]

        g = ctx.genome_from_host([b"A" * L])
        want = [WANT[search.name](p) for p in range(1, L + 1)]
        regrown = L > FIRST_CAP
        device_bytes()
        assert call(b"C") == ([], 1)                                    # the warm-up: every kept buffer of the search exists
        b0 = device_bytes()
        got, n_launches = call(b"A")
        assert got == want
        assert n_launches == (2 if regrown else 1) + search.extra_launches
        b1 = device_bytes()
        assert b1 - b0 == (L - FIRST_CAP) * search.record_bytes        # exactly the counted size; nothing at the first capacity
        assert call(b"A") == (want, 1 + search.extra_launches)          # one launch fewer: the buffer is kept ...
        assert device_bytes() == b1
        assert call(b"C") == ([], 1)
        assert device_bytes() == b1                                     # ... and not shrunk
        g.free()
    finally:
        ctx.close()
