"""k = 1 and 11 <= k <= 15 on the host side (no GPU): the reference's running Float64 distance from kgma_host_chain_values
(the sparse walk at k >= 11: the first window merged over the KFV's non-zero keys and the window's k-mers) bit for bit against
the oracle, and the sparse reference entry point in the library's exports with the header's prototype."""
import os
import re

import numpy as np
import pytest

from kmergma_amd import _lib, refprep
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("k", [1, 11, 12])
def test_host_chain_values_large_k(alp_locus, data_dir, k):
    RV, W, _, _ = refprep.gen_ref_ws_cons(os.path.join(data_dir, "Alp_V_ref.fasta"), k, return_int=True)
    seq = alp_locus[0].sequence[:60_000]
    a = bytearray(seq)
    a[5000:5700] = b"A" * 700                                                  # all of a step's lanes on one k-mer
    a[9000:9400] = b"ACGT" * 100
    seq = bytes(a)
    _, od = orc.single_scan([seq], RV, k, W, 30.0, 50, return_dists=True)      # windows 2 .. L-W+1
    nwin = len(seq) - W + 1
    full = _lib.host_chain_values(seq, RV, k, W, [(1, nwin)])
    assert len(full) == nwin
    assert full[0] == orc.kmer_dist_kfv(seq[:W], RV, k)
    assert np.array_equal(full[1:], od)
    iv = [(1, 1), (17, 40), (999, 2000), (nwin - 3, nwin)]
    assert np.array_equal(_lib.host_chain_values(seq, RV, k, W, iv), np.concatenate([full[lo - 1:hi] for lo, hi in iv]))


def test_host_chain_values_k_bounds():
    seq = b"ACGT" * 200
    ref = np.zeros(4, dtype=np.float64)
    ref[1] = 0.5
    assert _lib.host_chain_values(seq, ref, 1, 20, [(1, 3)]).size == 3
    with pytest.raises(_lib.KgmaError):
        _lib.host_chain_values(seq, ref, 0, 20, [(1, 3)])


def test_set_refs_sparse_exported_with_header_prototype():
    assert "kgma_set_refs_sparse" in _lib.EXPORTS
    assert hasattr(_lib.load(), "kgma_set_refs_sparse")
    hdr = open(os.path.join(ROOT, "include", "kgma.h")).read()
    m = re.search(r"int kgma_set_refs_sparse\(([^)]*)\);", hdr)
    assert m, "kgma_set_refs_sparse is not declared in kgma.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["kgma_ctx *ctx", "int32_t k", "int32_t m", "const int64_t *nnz", "const uint32_t *keys", "const double *vals",
                      "const int64_t *windowsizes", "const double *thr", "const int64_t *n_refs"]
    import ctypes as C
    at = _lib.load().kgma_set_refs_sparse.argtypes
    assert [t for t in at[1:3]] == [C.c_int32, C.c_int32]
    assert at[3]._type_ is C.c_int64 and at[4]._type_ is C.c_uint32 and at[5]._type_ is C.c_double
