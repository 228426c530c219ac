"""Gene assignment's model, stated on its own: what kgma_assign_seqs / kgma_assign_ranges must return.

  * the score matrix: align_ref.optimum(reference, query) per pair -- the aligner's model, written from its definition;
  * the choice: per query the first `top` references of a STABLE sort on (-score, index);
  * the column counts of a chosen pair: those of the host aligner's CIGAR (align.semiglobal_cigar) read with align_ref.runs, the
    leading and the trailing 'D' run (the query's free overhang) taken off.  align_ref.rescore(cigar) == optimum is asserted for
    every pair used, so the counts rest on an alignment that is well formed and optimal under the model.
Nothing here looks at the device or at kgma_assign.*.
"""
import functools
from typing import NamedTuple

import numpy as np

from kmergma_amd import align
from tests import align_ref as ar


class Want(NamedTuple):
    ref: int
    score: int
    n_eq: int
    n_x: int
    n_ins: int
    n_del: int
    q_lo: int
    q_hi: int


@functools.lru_cache(maxsize=None)
def optimum(ref: bytes, query: bytes, go: int, ge: int) -> int:
    return ar.optimum(ref, query, go, ge)


def score_matrix(refs, queries, go, ge) -> np.ndarray:
    return np.array([[optimum(bytes(r), bytes(q), go, ge) for r in refs] for q in queries], dtype=np.int64).reshape(len(queries), len(refs))


def choose(row, top):
    """The first `top` reference indices: higher score first, lower index among equal scores."""
    return sorted(range(len(row)), key=lambda r: (-int(row[r]), r))[:top]


def count_columns(cigar: str, n: int):
    """(n_eq, n_x, n_ins, n_del, q_lo, q_hi) of a CIGAR over a query of n residues."""
    rr = ar.runs(cigar)
    lead = rr[0][0] if rr and rr[0][1] == "D" else 0
    trail = rr[-1][0] if len(rr) > 1 and rr[-1][1] == "D" else 0
    tot = {o: sum(L for L, x in rr if x == o) for o in "=XID"}
    return tot["="], tot["X"], tot["I"], tot["D"] - lead - trail, lead + 1, n - trail


@functools.lru_cache(maxsize=None)
def pair(ref: bytes, query: bytes, go: int, ge: int):
    """(score, n_eq, n_x, n_ins, n_del, q_lo, q_hi) of one pair, the CIGAR checked against the model."""
    cigar, host_score = align.semiglobal_cigar(ref, query, go, ge)
    best = optimum(ref, query, go, ge)
    assert ar.rescore(cigar, ref, query, go, ge) == best == host_score, (cigar, best, host_score)
    return (best,) + count_columns(cigar, len(query))


def assign(refs, queries, go, ge, top, scores=None):
    """[[Want] * top] per query."""
    S = score_matrix(refs, queries, go, ge) if scores is None else scores
    return [[Want(r, *pair(bytes(refs[r]), bytes(q), go, ge)) for r in choose(S[k], top)] for k, q in enumerate(queries)]


def uses(cigar: str, op: str) -> bool:
    """The CIGAR has an `op` run that is not a leading or trailing D run."""
    rr = ar.runs(cigar)
    inner = rr[1:-1] if op == "D" else rr
    return any(x == op for _, x in inner)
