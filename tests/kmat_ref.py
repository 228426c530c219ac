"""The all-pairs k-mer distance's model, stated on its own: what kgma_kmer_dist_matrix, kgma_kmer_nearest and the screened
assignment must return.  Python / numpy integers only; nothing here looks at the device or at kgma_kmat.*.

  * counts: refprep.kmer_indices (every residue through A0 C1 G2 T3 N3, a KeyError outside it, nothing counted below k residues)
    + np.unique, kept SPARSE (k = 10 needs no 4^k x n array);
  * D(a, b) = sum_x (c_a[x] - c_b[x])^2 from the definition, over the union of the two supports;
  * dist = (1.0 / (2 * k)) * D, one Float64 multiply;
  * the nearest: np.lexsort((index, D)) -- D ascending, then index ascending;
  * the screened assignment: tests/assign_ref.assign restricted to the model's candidates.
"""
import numpy as np

from kmergma_amd import refprep
from tests import assign_ref


def counts(seq: bytes, k: int):
    """(sorted k-mer values, their counts) of one sequence."""
    x, c = np.unique(refprep.kmer_indices(bytes(seq), k), return_counts=True)
    return x.astype(np.int64), c.astype(np.int64)


def sq_dist(ca, cb) -> int:
    """sum_x (c_a[x] - c_b[x])^2 of two sparse count vectors, a Python int."""
    x = np.union1d(ca[0], cb[0])
    va = np.zeros(x.size, dtype=np.int64)
    vb = np.zeros(x.size, dtype=np.int64)
    va[np.searchsorted(x, ca[0])] = ca[1]
    vb[np.searchsorted(x, cb[0])] = cb[1]
    d = va - vb
    return int(np.dot(d, d))


def D_matrix(seqs_a, seqs_b, k: int) -> np.ndarray:
    """int64 [n_a, n_b]; seqs_b None: A against A."""
    ca = [counts(s, k) for s in seqs_a]
    cb = ca if seqs_b is None else [counts(s, k) for s in seqs_b]
    return np.array([[sq_dist(x, y) for y in cb] for x in ca], dtype=np.int64).reshape(len(ca), len(cb))


def dist_matrix(D: np.ndarray, k: int) -> np.ndarray:
    return (1.0 / (2 * k)) * D.astype(np.float64)


def nearest(D: np.ndarray, n_near: int):
    """(index, D_near), each int64 [n_a, n_near]: per row the first n_near columns in the order (D, index)."""
    idx = np.array([np.lexsort((np.arange(row.size), row))[:n_near] for row in D], dtype=np.int64).reshape(D.shape[0], n_near)
    return idx, np.take_along_axis(D, idx, axis=1) if D.shape[0] else idx.copy()


def screened_assign(refs, queries, go, ge, top, screen_k, n_near):
    """(out, cand, scores): cand the model's candidates per query (int64 [n_q, n_near]), scores their model scores in candidate
    order, out per query [Want] * top -- assign_ref.assign over the candidates only, the reference named by its index in `refs`
    (higher score first, lower REFERENCE index among equal scores)."""
    cand, _ = nearest(D_matrix(queries, refs, screen_k), n_near)
    out, scores = [], []
    for q, row in zip(queries, cand):
        sub = [refs[int(r)] for r in row]
        S = assign_ref.score_matrix(sub, [q], go, ge)
        scores.append(S[0].tolist())
        order = sorted(range(n_near), key=lambda c: (-int(S[0][c]), int(row[c])))[:top]
        out.append([assign_ref.Want(int(row[c]), *assign_ref.pair(bytes(sub[c]), bytes(q), go, ge)) for c in order])
    return out, cand, np.array(scores, dtype=np.int64).reshape(len(queries), n_near)
