"""ctypes binding of libkgma.so (the C ABI of include/kgma.h).

This is what the Julia shim's `ccall`s mirror one to one.  The library is
the product: if it is missing or no MI355X is present the calls fail loudly -- there is no CPU
fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, List, Optional, Sequence

import numpy as np

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("KGMA_LIB") or os.path.join(_PKG_DIR, "libkgma.so")

KGMA_OK = 0
KGMA_E_ARG, KGMA_E_NODEVICE, KGMA_E_HIP, KGMA_E_BADBASE, KGMA_E_BOUNDS = 1, 2, 3, 4, 5
KGMA_E_UNSUPPORTED, KGMA_E_OVERFLOW, KGMA_E_NOMEM, KGMA_E_STATE = 6, 7, 8, 9
MODE_SINGLE, MODE_OMN, MODE_STROBE = 0, 1, 2
F_RETURN_DISTS, F_NO_TIE_RESOLVE, F_CHAIN_REPLAY = 1, 2, 4
HIT_TIE, HIT_AT_THRESHOLD, HIT_TIE_RESOLVED, HIT_CHAIN = 1, 2, 4, 8

EXPORTS = [
    "kgma_version", "kgma_status_string", "kgma_last_error", "kgma_create", "kgma_destroy",
    "kgma_set_refs", "kgma_set_refs_sparse", "kgma_set_thresholds", "kgma_genome_from_host", "kgma_genome_synthetic",
    "kgma_genome_fetch", "kgma_genome_fetch_batch", "kgma_genome_num_contigs", "kgma_genome_contig_len", "kgma_genome_total_bases",
    "kgma_genome_free", "kgma_genome_repack", "kgma_genome_poke", "kgma_scan", "kgma_scan_device", "kgma_get_hits",
    "kgma_get_dips", "kgma_get_first_window", "kgma_get_dists", "kgma_get_stats", "kgma_stream",
    "kgma_host_semiglobal_cigar", "kgma_genome_from_fasta", "kgma_genome_from_fasta_file", "kgma_genome_header", "kgma_scan_kernel_name",
    "kgma_resolve_ties_local", "kgma_get_dip_last_min", "kgma_replay_dips", "kgma_align_hits_device", "kgma_repack_scan_hits",
    "kgma_kmer_count_batch", "kgma_kmer_dist_batch", "kgma_step_begin", "kgma_step_end", "kgma_set_reserved_cus",
    "kgma_scan_aligned", "kgma_get_alignments", "kgma_set_residue_source", "kgma_host_chain_values",
    "kgma_chain_values", "kgma_host_chain_walk", "kgma_chain_chunk_steps", "kgma_set_chain_source", "kgma_get_att", "kgma_set_att",
    "kgma_chain_export", "kgma_chain_export_copy", "kgma_kfv_scale", "kgma_kfv_is_float",
    "kgma_set_strobe_ref", "kgma_strobe_scan", "kgma_exact_match", "kgma_get_matches",
    "kgma_motif_match", "kgma_get_motif_matches",
    "kgma_approx_match", "kgma_get_approx_matches", "kgma_get_approx_stats",
    "kgma_pwm_match", "kgma_get_pwm_matches", "kgma_get_pwm_stats",
    "kgma_codon_match", "kgma_get_codon_matches", "kgma_get_codon_stats", "kgma_codon_fold",
    "kgma_get_filter_stats", "kgma_get_filter_candidates", "kgma_genome_revcomp", "kgma_genome_revcomp_into",
    "kgma_get_block_sums", "kgma_genome_from_2bit_file", "kgma_get_2bit_unpack_ms", "kgma_twobit_inspect",
    "kgma_window_dists", "kgma_mutation_dists", "kgma_strobe_window_dists", "kgma_strobe_mutation_dists",
    "kgma_assign_seqs", "kgma_assign_ranges", "kgma_get_assign_stats",
    "kgma_kmer_dist_matrix", "kgma_kmer_dist_matrix_ranges", "kgma_kmer_nearest", "kgma_kmer_nearest_ranges", "kgma_get_kmat_stats",
    "kgma_assign_seqs_screened", "kgma_assign_ranges_screened",
    "kgma_dist_layout", "kgma_dist_bins", "kgma_dist_sweep", "kgma_get_landscape_stats",
    "kgma_genome_inter_state",
    "kgma_genome_kmer_count", "kgma_get_spectrum_stats",
    "kgma_get_pack_test_stats",
]
SWEEP_MAX_THRESHOLDS = 4096          # KGMA_SWEEP_MAX_THRESHOLDS
ASSIGN_MAX_LEN = 8191                # KGMA_ASSIGN_MAX_LEN
KMAT_MAX_LEN = 32767                 # KGMA_KMAT_MAX_LEN
KMAT_MAX_NEAR = 128                  # KGMA_KMAT_MAX_NEAR
KMAT_FORM_LDS, KMAT_FORM_GLOBAL = 0, 1   # kgma_kmat_stats.form
COUNT_SKIP_N, COUNT_SKIP_MASKED, COUNT_BY_START = 1, 2, 4   # kgma_genome_kmer_count flags
SPECTRUM_FORM_WG, SPECTRUM_FORM_WAVE, SPECTRUM_FORM_GLOBAL = 0, 1, 2   # kgma_spectrum_stats.form
SPECTRUM_MAX_COUNTS = 1 << 28        # n_ranges * 4^k of one kgma_genome_kmer_count at most
TWOBIT_NOMASK = 1                    # KGMA_2BIT_NOMASK
TWOBIT_SIGNATURE = b"\x43\x27\x41\x1a"  # the first four bytes of a .2bit file in this machine's byte order
FILTER_FORM_PRESUMMED = 1 << 16      # kgma_filter_stats.form: the filter read the block sums the step's pack wrote (KGMA_FUSE_SUMS)
INTER_FULL, INTER_PARTIAL = 0, 1     # kgma_genome_inter_state: the device's 2-bit copy of the genome (KGMA_SPARSE_PACK)
FILTER_OK, FILTER_OVERFLOW, FILTER_STREAMS, FILTER_FRACTION, FILTER_REMEMBERED = 0, 1, 2, 3, 4


class KgmaHit(C.Structure):
    _fields_ = [("contig", C.c_int32), ("kfv", C.c_int32), ("cmi", C.c_int64), ("lo", C.c_int64),
                ("hi", C.c_int64), ("genome_pos", C.c_int64), ("dist", C.c_double), ("D", C.c_int64),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class KgmaDip(C.Structure):
    _fields_ = [("contig", C.c_int32), ("kfv", C.c_int32), ("start", C.c_int64), ("end", C.c_int64),
                ("argmin", C.c_int64), ("D_min", C.c_int64), ("exit_pos", C.c_int64), ("D_exit", C.c_int64),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class KgmaAlignment(C.Structure):
    _fields_ = [("contig", C.c_int32), ("kfv", C.c_int32), ("lo", C.c_int64), ("hi", C.c_int64),
                ("first", C.c_int64), ("last", C.c_int64)]


class KgmaMatch(C.Structure):
    _fields_ = [("query", C.c_int32), ("contig", C.c_int32), ("start", C.c_int64)]


class KgmaMotifHit(C.Structure):
    _fields_ = [("motif", C.c_int32), ("contig", C.c_int32), ("start", C.c_int64), ("mismatches", C.c_int32),
                ("reserved", C.c_int32)]


class KgmaApproxHit(C.Structure):
    _fields_ = [("query", C.c_int32), ("contig", C.c_int32), ("start", C.c_int64), ("end", C.c_int64), ("edits", C.c_int32),
                ("reserved", C.c_int32)]


class KgmaApproxStats(C.Structure):
    _fields_ = [("tile", C.c_int32), ("wg_bases", C.c_int32), ("words", C.c_int32), ("n_launches", C.c_int32),
                ("n_ends", C.c_int64), ("n_hits", C.c_int64), ("search_ms", C.c_double), ("starts_ms", C.c_double)]


class KgmaPwmHit(C.Structure):
    _fields_ = [("matrix", C.c_int32), ("contig", C.c_int32), ("start", C.c_int64), ("score", C.c_int32), ("reserved", C.c_int32)]


class KgmaPwmStats(C.Structure):
    _fields_ = [("lane_starts", C.c_int32), ("wave_starts", C.c_int32), ("wg_starts", C.c_int32), ("n_launches", C.c_int32),
                ("n_candidates", C.c_int64), ("n_hits", C.c_int64), ("search_ms", C.c_double)]


class KgmaCodonHit(C.Structure):
    _fields_ = [("matrix", C.c_int32), ("contig", C.c_int32), ("start", C.c_int64), ("score", C.c_int32), ("reserved", C.c_int32)]


class KgmaCodonStats(C.Structure):
    _fields_ = [("lane_starts", C.c_int32), ("wave_starts", C.c_int32), ("wg_starts", C.c_int32), ("n_launches", C.c_int32),
                ("n_candidates", C.c_int64), ("n_hits", C.c_int64), ("search_ms", C.c_double)]


class KgmaTwobitInfo(C.Structure):
    _fields_ = [("version", C.c_int32), ("reserved", C.c_int32), ("n_records", C.c_int64), ("total_bases", C.c_int64),
                ("n_blocks", C.c_int64), ("mask_blocks", C.c_int64), ("packed_bytes", C.c_int64)]


class KgmaStats(C.Structure):
    _fields_ = [("bases_scanned", C.c_int64), ("windows_scanned", C.c_int64), ("n_dips", C.c_int64),
                ("n_hits", C.c_int64), ("n_tie_flagged", C.c_int64), ("n_at_threshold", C.c_int64),
                ("pack_ms", C.c_double), ("scan_ms", C.c_double), ("replay_ms", C.c_double),
                ("device_bytes", C.c_int64), ("n_tiles", C.c_int32), ("n_launches", C.c_int32),
                ("chain_ms", C.c_double), ("n_chain_pairs", C.c_int64), ("chain_windows", C.c_int64),
                ("chain_device_pairs", C.c_int64), ("chain_device_ms", C.c_double), ("chain_raw_steps", C.c_int64),
                ("chain_max_drift", C.c_double), ("chain_band_log2", C.c_int32), ("chain_rescans", C.c_int32),
                ("overlap_ms", C.c_double)]


class KgmaFilterStats(C.Structure):
    _fields_ = [("ran", C.c_int32), ("fell_back", C.c_int32), ("reason", C.c_int32), ("form", C.c_int32),
                ("granules", C.c_int64), ("regions", C.c_int64), ("streams", C.c_int64), ("windows", C.c_int64),
                ("positions", C.c_int64), ("total_windows", C.c_int64), ("bound", C.c_int64), ("filter_ms", C.c_double)]


class KgmaPackTestStats(C.Structure):
    _fields_ = [("tested", C.c_int32), ("run", C.c_int32), ("units", C.c_int64), ("slow_units", C.c_int64),
                ("primed_chunks", C.c_int64)]


class KgmaAssignStats(C.Structure):
    _fields_ = [("score_ms", C.c_double), ("trace_ms", C.c_double), ("n_pairs", C.c_int64), ("n_cells", C.c_int64),
                ("n_traced", C.c_int64), ("n_score_launches", C.c_int32), ("n_trace_launches", C.c_int32)]


class KgmaKmatStats(C.Structure):
    _fields_ = [("kmat_ms", C.c_double), ("select_ms", C.c_double), ("n_pairs", C.c_int64), ("n_launches", C.c_int32),
                ("form", C.c_int32), ("tile", C.c_int32), ("chunks", C.c_int32)]


class KgmaSpectrumStats(C.Structure):
    _fields_ = [("count_ms", C.c_double), ("n_ranges", C.c_int64), ("n_positions", C.c_int64), ("form", C.c_int32),
                ("span", C.c_int32), ("n_workgroups", C.c_int32), ("n_launches", C.c_int32)]


class KgmaLandscapeStats(C.Structure):
    _fields_ = [("bins_ms", C.c_double), ("combine_ms", C.c_double), ("sweep_ms", C.c_double), ("n_values", C.c_int64),
                ("n_bins", C.c_int64), ("n_launches", C.c_int32), ("sweep_slots", C.c_int32)]


HIT_DTYPE = np.dtype([("contig", "<i4"), ("kfv", "<i4"), ("cmi", "<i8"), ("lo", "<i8"), ("hi", "<i8"),
                      ("genome_pos", "<i8"), ("dist", "<f8"), ("D", "<i8"), ("flags", "<u4"), ("reserved", "<u4")])

DIP_DTYPE = np.dtype([("contig", "<i4"), ("kfv", "<i4"), ("start", "<i8"), ("end", "<i8"), ("argmin", "<i8"),
                      ("D_min", "<i8"), ("exit_pos", "<i8"), ("D_exit", "<i8"), ("flags", "<u4"), ("reserved", "<u4")])

MATCH_DTYPE = np.dtype([("query", "<i4"), ("contig", "<i4"), ("start", "<i8")])

MOTIF_HIT_DTYPE = np.dtype([("motif", "<i4"), ("contig", "<i4"), ("start", "<i8"), ("mismatches", "<i4"), ("reserved", "<i4")])

APPROX_HIT_DTYPE = np.dtype([("query", "<i4"), ("contig", "<i4"), ("start", "<i8"), ("end", "<i8"), ("edits", "<i4"), ("reserved", "<i4")])

PWM_HIT_DTYPE = np.dtype([("matrix", "<i4"), ("contig", "<i4"), ("start", "<i8"), ("score", "<i4"), ("reserved", "<i4")])

CODON_HIT_DTYPE = np.dtype([("matrix", "<i4"), ("contig", "<i4"), ("start", "<i8"), ("score", "<i4"), ("reserved", "<i4")])
CODON_ENTRIES, CODON_MAX_ROWS, CODON_AA_COLUMNS = 65, 64, 21   # KGMA_CODON_ENTRIES, KGMA_CODON_MAX_ROWS, KGMA_CODON_AA_COLUMNS

ASSIGNMENT_DTYPE = np.dtype([("ref", "<i4"), ("score", "<i4"), ("n_eq", "<i4"), ("n_x", "<i4"), ("n_ins", "<i4"), ("n_del", "<i4"),
                             ("q_lo", "<i4"), ("q_hi", "<i4")])   # kgma_assignment

ALIGN_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                       C.POINTER(C.c_int64), C.POINTER(C.c_int64))
FETCH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.POINTER(C.c_uint8))
CHAIN_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                       C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double))


class KgmaError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libkgma status {status}: {message}")
        self.status = status
        self.message = message


class BadBaseError(KgmaError, KeyError):
    """KGMA_E_BADBASE: the reference raises KeyError from NUCLEOTIDE_BITS (src/Consts.jl:22-28)."""


class RecordBoundsError(KgmaError, IndexError):
    """KGMA_E_BOUNDS: BoundsError in the reference (src/OmnGenomeMiner.jl:84-86)."""


_lib = None


def load():
    """Load libkgma.so; raises (never falls back) when the extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: build it with `make -C kmergma.jl_amd/csrc` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, u32, u64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_double
    P = C.POINTER
    L.kgma_version.restype = C.c_int
    L.kgma_status_string.restype = C.c_char_p
    L.kgma_status_string.argtypes = [C.c_int]
    L.kgma_last_error.restype = C.c_char_p
    L.kgma_last_error.argtypes = [vp]
    L.kgma_create.argtypes = [C.c_int, P(vp)]
    L.kgma_destroy.argtypes = [vp]
    L.kgma_destroy.restype = None
    L.kgma_set_refs.argtypes = [vp, i32, i32, P(dbl), P(i64), P(dbl), P(i64)]
    L.kgma_set_refs_sparse.argtypes = [vp, i32, i32, P(i64), P(C.c_uint32), P(dbl), P(i64), P(dbl), P(i64)]
    L.kgma_set_thresholds.argtypes = [vp, P(dbl)]
    L.kgma_set_strobe_ref.argtypes = [vp, i32, i32, i32, i64, P(dbl), i64, dbl, i64]
    L.kgma_strobe_scan.argtypes = [vp, vp, i64, u32, C.c_char_p, i64, i32, i32, i64]
    L.kgma_exact_match.argtypes = [vp, vp, C.c_char_p, P(i64), i32, i32]
    L.kgma_get_matches.argtypes = [vp, P(KgmaMatch), i64, P(i64)]
    L.kgma_motif_match.argtypes = [vp, vp, C.c_char_p, P(i64), i32, P(i32)]
    L.kgma_get_motif_matches.argtypes = [vp, P(KgmaMotifHit), i64, P(i64)]
    L.kgma_approx_match.argtypes = [vp, vp, C.c_char_p, P(i64), i32, P(i32), i32]
    L.kgma_get_approx_matches.argtypes = [vp, P(KgmaApproxHit), i64, P(i64)]
    L.kgma_get_approx_stats.argtypes = [vp, P(KgmaApproxStats)]
    L.kgma_pwm_match.argtypes = [vp, vp, P(C.c_int16), P(i64), i32, P(i32)]
    L.kgma_get_pwm_matches.argtypes = [vp, P(KgmaPwmHit), i64, P(i64)]
    L.kgma_get_pwm_stats.argtypes = [vp, P(KgmaPwmStats)]
    L.kgma_codon_match.argtypes = [vp, vp, P(C.c_int16), P(i64), i32, P(i32)]
    L.kgma_get_codon_matches.argtypes = [vp, P(KgmaCodonHit), i64, P(i64)]
    L.kgma_get_codon_stats.argtypes = [vp, P(KgmaCodonStats)]
    L.kgma_codon_fold.argtypes = [P(C.c_int16), i32, P(C.c_uint8), P(C.c_int16), i32, P(C.c_int16)]
    L.kgma_genome_from_host.argtypes = [vp, P(C.c_char_p), P(i64), i64, P(vp)]
    L.kgma_genome_from_fasta.argtypes = [vp, vp, i64, P(vp)]
    L.kgma_genome_from_fasta_file.argtypes = [vp, C.c_char_p, P(vp)]
    L.kgma_genome_header.argtypes = [vp, i64, P(C.c_char_p), P(i64)]
    L.kgma_genome_from_2bit_file.argtypes = [vp, C.c_char_p, u32, P(vp)]
    L.kgma_get_2bit_unpack_ms.argtypes = [vp, P(dbl)]
    L.kgma_twobit_inspect.argtypes = [C.c_char_p, P(KgmaTwobitInfo), C.c_char_p, i64]
    L.kgma_genome_synthetic.argtypes = [vp, P(i64), i64, u64, C.c_char_p, i64, P(i64), P(i64), i64, P(vp)]
    L.kgma_genome_fetch.argtypes = [vp, vp, i64, i64, i64, C.c_char_p]
    L.kgma_genome_fetch_batch.argtypes = [vp, vp, i64, P(i64), P(i64), P(i64), C.c_char_p, i64]
    L.kgma_genome_num_contigs.argtypes = [vp]
    L.kgma_genome_num_contigs.restype = i64
    L.kgma_genome_contig_len.argtypes = [vp, i64]
    L.kgma_genome_contig_len.restype = i64
    L.kgma_genome_total_bases.argtypes = [vp]
    L.kgma_genome_total_bases.restype = i64
    L.kgma_genome_free.argtypes = [vp, vp]
    L.kgma_genome_free.restype = None
    L.kgma_genome_repack.argtypes = [vp, vp]
    L.kgma_genome_poke.argtypes = [vp, vp, i64, i64, i64, C.c_char_p]
    L.kgma_genome_revcomp.argtypes = [vp, vp, P(vp)]
    L.kgma_genome_revcomp_into.argtypes = [vp, vp, vp]
    L.kgma_scan.argtypes = [vp, vp, i32, i64, i64, u32, ALIGN_FN, vp]
    L.kgma_scan_device.argtypes = [vp, vp, i32, u32]
    L.kgma_get_hits.argtypes = [vp, P(KgmaHit), i64, P(i64)]
    L.kgma_get_dips.argtypes = [vp, P(KgmaDip), i64, P(i64)]
    L.kgma_get_first_window.argtypes = [vp, i32, P(i64), i64, P(i64)]
    L.kgma_get_dists.argtypes = [vp, i32, P(dbl), i64, P(i64)]
    L.kgma_get_stats.argtypes = [vp, P(KgmaStats)]
    L.kgma_get_filter_stats.argtypes = [vp, P(KgmaFilterStats)]
    L.kgma_get_pack_test_stats.argtypes = [vp, P(KgmaPackTestStats)]
    L.kgma_get_filter_candidates.argtypes = [vp, P(i32), P(i64), i64, P(i64)]
    L.kgma_get_block_sums.argtypes = [vp, vp, i64, i64, i64, P(C.c_uint32)]
    L.kgma_genome_inter_state.argtypes = [vp, P(i32), P(i64)]
    L.kgma_resolve_ties_local.argtypes = [vp, vp]
    L.kgma_repack_scan_hits.argtypes = [vp, vp, i32, i64, i64, C.c_uint32, P(KgmaHit), i64, P(i64)]
    L.kgma_align_hits_device.argtypes = [vp, vp, C.c_char_p, i64, i32, i32, i64, P(i32), P(i64), P(i64), P(i64), P(i64), P(i64)]
    L.kgma_get_dip_last_min.argtypes = [vp, P(i64), i64, P(i64)]
    L.kgma_replay_dips.argtypes = [vp, i32, i64, i64, C.c_uint32, i64, P(i64), P(i64), P(KgmaDip), P(i64), i64, ALIGN_FN, vp]
    L.kgma_host_semiglobal_cigar.argtypes = [C.c_char_p, i64, C.c_char_p, i64, i32, i32, C.c_char_p, i64, P(i64)]
    L.kgma_set_reserved_cus.argtypes = [vp, i32]
    L.kgma_step_begin.argtypes = [vp, vp, i32, i64, i64, C.c_uint32]
    L.kgma_step_end.argtypes = [vp, P(KgmaHit), i64, P(i64)]
    L.kgma_kmer_count_batch.argtypes = [vp, i32, C.c_char_p, P(i64), i64, P(dbl)]
    L.kgma_kmer_dist_batch.argtypes = [vp, i32, P(dbl), C.c_char_p, P(i64), i64, P(dbl)]
    L.kgma_scan_aligned.argtypes = [vp, vp, i32, i64, i64, C.c_uint32, P(C.c_char_p), P(i64), i32, i32]
    L.kgma_get_alignments.argtypes = [vp, P(KgmaAlignment), i64, P(i64), P(i64), P(i64)]
    L.kgma_set_residue_source.argtypes = [vp, FETCH_FN, vp]
    L.kgma_set_chain_source.argtypes = [vp, CHAIN_FN, vp]
    L.kgma_kfv_scale.argtypes = [vp, i32, P(dbl), P(i64)]
    L.kgma_kfv_is_float.argtypes = [vp, i32, P(i32)]
    L.kgma_get_att.argtypes = [vp, P(i32), P(i32), P(i64), i64, P(i64)]
    L.kgma_set_att.argtypes = [vp, P(i32), P(i32), P(i64), i64]
    L.kgma_chain_export.argtypes = [vp, vp, i64, i32, i64, P(i64), P(i64), i64, P(i64), P(i64), P(i64), P(dbl)]
    L.kgma_chain_export_copy.argtypes = [vp, P(i64), P(i32), P(i64), P(i64), vp, vp]
    L.kgma_host_chain_values.argtypes = [C.c_char_p, i64, P(dbl), i32, i64, P(i64), P(i64), i64, P(dbl), i64, P(i64)]
    L.kgma_chain_values.argtypes = [vp, vp, i64, i32, P(i64), P(i64), i64, P(dbl), i64, P(i64)]
    L.kgma_host_chain_walk.argtypes = [dbl, dbl, i32, i64, P(i64), P(i32), P(i64), P(i64), vp, i64, vp, i64, P(i64), P(i64), i64,
                                       P(dbl), i64, P(i64), P(dbl)]
    L.kgma_window_dists.argtypes = [vp, vp, i32, i64, P(i32), P(i64), P(i64), P(dbl)]
    L.kgma_mutation_dists.argtypes = [vp, i32, C.c_char_p, P(i64), i64, P(dbl), i32, i32, u64, P(i64), P(dbl)]
    L.kgma_strobe_window_dists.argtypes = [vp, vp, i64, P(i32), P(i64), P(i64), P(dbl)]
    L.kgma_strobe_mutation_dists.argtypes = [vp, C.c_char_p, P(i64), i64, P(dbl), i32, i32, u64, P(i64), P(dbl)]
    L.kgma_assign_seqs.argtypes = [vp, C.c_char_p, P(i64), i32, C.c_char_p, P(i64), i64, i32, i32, i32, vp, P(i32)]
    L.kgma_assign_ranges.argtypes = [vp, vp, C.c_char_p, P(i64), i32, i64, P(i32), P(i64), P(i64), i32, i32, i32, vp, P(i32)]
    L.kgma_get_assign_stats.argtypes = [vp, P(KgmaAssignStats)]
    L.kgma_kmer_dist_matrix.argtypes = [vp, i32, C.c_char_p, P(i64), i64, C.c_char_p, P(i64), i32, P(i32), P(dbl)]
    L.kgma_kmer_dist_matrix_ranges.argtypes = [vp, vp, i32, i64, P(i32), P(i64), P(i64), C.c_char_p, P(i64), i32, P(i32), P(dbl)]
    L.kgma_kmer_nearest.argtypes = [vp, i32, C.c_char_p, P(i64), i64, C.c_char_p, P(i64), i32, i32, P(i32), P(i32)]
    L.kgma_kmer_nearest_ranges.argtypes = [vp, vp, i32, i64, P(i32), P(i64), P(i64), C.c_char_p, P(i64), i32, i32, P(i32), P(i32)]
    L.kgma_get_kmat_stats.argtypes = [vp, P(KgmaKmatStats)]
    L.kgma_assign_seqs_screened.argtypes = [vp, C.c_char_p, P(i64), i32, C.c_char_p, P(i64), i64, i32, i32, i32, i32, i32, vp, P(i32), P(i32)]
    L.kgma_assign_ranges_screened.argtypes = [vp, vp, C.c_char_p, P(i64), i32, i64, P(i32), P(i64), P(i64), i32, i32, i32, i32, i32, vp,
                                              P(i32), P(i32)]
    L.kgma_dist_layout.argtypes = [vp, P(i64), i64, P(i64)]
    L.kgma_dist_bins.argtypes = [vp, i32, i64, P(dbl), P(i64), P(i64), i64, P(i64)]
    L.kgma_dist_sweep.argtypes = [vp, i32, P(dbl), i64, P(i64), P(i64)]
    L.kgma_get_landscape_stats.argtypes = [vp, P(KgmaLandscapeStats)]
    L.kgma_genome_kmer_count.argtypes = [vp, vp, i32, C.c_uint32, i64, P(i32), P(i64), P(i64), P(i64), P(i64)]
    L.kgma_get_spectrum_stats.argtypes = [vp, P(KgmaSpectrumStats)]
    L.kgma_stream.argtypes = [vp]
    L.kgma_stream.restype = vp
    L.kgma_scan_kernel_name.argtypes = [vp]
    L.kgma_scan_kernel_name.restype = C.c_char_p
    _lib = L
    return L


def host_chain_values(seq: bytes, ref, k: int, windowsize: int, intervals) -> np.ndarray:
    """kgma_host_chain_values: the reference's running Float64 distance of `seq` at the windows of `intervals`
    (list of (lo, hi), 1-based window starts).  Host only: needs no GPU."""
    r = np.ascontiguousarray(ref, dtype=np.float64)
    lo = np.asarray([a for a, _ in intervals], dtype=np.int64)
    hi = np.asarray([b for _, b in intervals], dtype=np.int64)
    n = int((hi - lo + 1).sum())
    out = np.zeros(max(n, 1), dtype=np.float64)
    nn = C.c_int64(0)
    st = load().kgma_host_chain_values(bytes(seq), len(seq), r.ctypes.data_as(C.POINTER(C.c_double)), int(k), int(windowsize),
                                       lo.ctypes.data_as(C.POINTER(C.c_int64)), hi.ctypes.data_as(C.POINTER(C.c_int64)), lo.size,
                                       out.ctypes.data_as(C.POINTER(C.c_double)), out.size, C.byref(nn))
    if st != KGMA_OK:
        raise KgmaError(st, "kgma_host_chain_values failed")
    return out[:nn.value]


def twobit_inspect(path) -> dict:
    """kgma_twobit_inspect: what the host parser of genome_from_2bit makes of a .2bit file -- dict(version, n_records,
    total_bases, n_blocks, mask_blocks, packed_bytes), block counts after normalisation.  Host only: needs no GPU.  A file the
    parser refuses raises KgmaError with its status and message."""
    info = KgmaTwobitInfo()
    err = C.create_string_buffer(512)
    st = load().kgma_twobit_inspect(os.fsencode(path), C.byref(info), err, len(err))
    if st != KGMA_OK:
        raise KgmaError(st, err.value.decode("utf-8", "replace"))
    return {f: int(getattr(info, f)) for f, _ in KgmaTwobitInfo._fields_ if f != "reserved"}


def codon_fold(aa_weights, code, x_weight, minus: bool = False) -> np.ndarray:
    """kgma_codon_fold: the (m, 65) codon matrix of one strand from an amino-acid profile -- `aa_weights` (m, 21) integers, the
    columns in the order ACDEFGHIKLMNPQRSTVWY*; `code` 64 column numbers (0 ... 20) indexed by the codon 16 b0 + 4 b1 + b2
    (A 0, C 1, G 2, T 3); `x_weight` (m,) the weight of a codon with an N.  minus: the rows reversed and each codon read as
    its reverse complement.  Host only: needs no GPU."""
    aa = np.asarray(aa_weights)
    cd = np.asarray(code)
    xw = np.asarray(x_weight)
    if aa.ndim != 2 or aa.shape[1] != CODON_AA_COLUMNS or not np.issubdtype(aa.dtype, np.integer):
        raise ValueError(f"aa_weights: need an (m, {CODON_AA_COLUMNS}) array of integers")
    if xw.shape != (aa.shape[0],) or not np.issubdtype(xw.dtype, np.integer):
        raise ValueError("x_weight: need one integer per row")
    if cd.shape != (64,) or not np.issubdtype(cd.dtype, np.integer) or (cd < 0).any() or (cd > 255).any():
        raise ValueError("code: need 64 column numbers")
    for a in (aa, xw):
        if a.size and (int(a.min()) < -32768 or int(a.max()) > 32767):
            raise ValueError("a weight is outside -32768 ... 32767")
    aa16, x16, cd8 = np.ascontiguousarray(aa, dtype=np.int16), np.ascontiguousarray(xw, dtype=np.int16), np.ascontiguousarray(cd, dtype=np.uint8)
    out = np.zeros((max(aa.shape[0], 1), CODON_ENTRIES), dtype=np.int16)
    st = load().kgma_codon_fold(_np_ptr(aa16, C.c_int16), aa.shape[0], _np_ptr(cd8, C.c_uint8), _np_ptr(x16, C.c_int16), int(bool(minus)),
                                _np_ptr(out, C.c_int16))
    if st != KGMA_OK:
        raise KgmaError(st, f"kgma_codon_fold: 1 ... {CODON_MAX_ROWS} rows and code entries 0 ... {CODON_AA_COLUMNS - 1}")
    return out[:aa.shape[0]].astype(np.int64)


def is_twobit(path) -> bool:
    """True when the file begins with the .2bit signature, in either byte order (a byte-swapped file is then refused by the
    parser, with its own message, instead of being read as FASTA)."""
    with open(path, "rb") as fh:
        head = fh.read(4)
    return head in (TWOBIT_SIGNATURE, TWOBIT_SIGNATURE[::-1])


def chain_steps() -> int:
    """kgma_device.h: KGMA_CHAIN_STEPS (64-position steps per chunk of the device chain)."""
    return int(load().kgma_chain_chunk_steps())


CHAIN_CHUNK_DTYPE = np.dtype([("A0", "<i8"), ("info", "<u4"), ("raw", "<u4")])   # kgma_device.h: ChainChunk


CHAIN_RAW, CHAIN_DETAIL = 1 << 10, 1 << 11      # kgma_device.h: KGMA_CHAIN_RAW / KGMA_CHAIN_DETAIL


def host_chain_walk(first: float, scale: float, nk: int, win0, n_valid, chunk_base, D0, chunks, pool, intervals):
    """kgma_host_chain_walk: the host half of the device chain on caller-supplied chunk records (tests).  `pool`: the
    entries of detailed chunks and the raw increments, as an array of CHAIN_CHUNK_DTYPE units (16 bytes each; a raw step's
    64 doubles take 32 units).  Returns (values at the windows of `intervals`, largest drift seen at a stream start)."""
    win0 = np.ascontiguousarray(win0, dtype=np.int64)
    n_valid = np.ascontiguousarray(n_valid, dtype=np.int32)
    chunk_base = np.ascontiguousarray(chunk_base, dtype=np.int64)
    D0 = np.ascontiguousarray(D0, dtype=np.int64)
    chunks = np.ascontiguousarray(chunks, dtype=CHAIN_CHUNK_DTYPE)
    pool = np.ascontiguousarray(pool, dtype=CHAIN_CHUNK_DTYPE).reshape(-1)
    lo = np.asarray([a for a, _ in intervals], dtype=np.int64)
    hi = np.asarray([b for _, b in intervals], dtype=np.int64)
    n = int((hi - lo + 1).sum())
    out = np.zeros(max(n, 1), dtype=np.float64)
    nn = C.c_int64(0)
    drift = C.c_double(0)
    st = load().kgma_host_chain_walk(float(first), float(scale), int(nk), win0.size, _np_ptr(win0, C.c_int64), _np_ptr(n_valid, C.c_int32),
                                     _np_ptr(chunk_base, C.c_int64), _np_ptr(D0, C.c_int64), chunks.ctypes.data_as(C.c_void_p), chunks.size,
                                     pool.ctypes.data_as(C.c_void_p) if pool.size else None, pool.size, _np_ptr(lo, C.c_int64),
                                     _np_ptr(hi, C.c_int64), lo.size, _np_ptr(out, C.c_double), out.size, C.byref(nn), C.byref(drift))
    if st != KGMA_OK:
        raise KgmaError(st, "kgma_host_chain_walk failed")
    return out[:nn.value], drift.value


def _np_ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Genome:
    """Device-resident genome (two bit-planes + the ASCII residues)."""

    def __init__(self, ctx: "Context", handle):
        self._ctx = ctx
        self._h = handle

    @property
    def n_contigs(self) -> int:
        return int(load().kgma_genome_num_contigs(self._h))

    def contig_len(self, c: int) -> int:
        return int(load().kgma_genome_contig_len(self._h, c))

    @property
    def total_bases(self) -> int:
        return int(load().kgma_genome_total_bases(self._h))

    def header(self, contig: int) -> str:
        txt = C.c_char_p()
        n = C.c_int64(0)
        st = load().kgma_genome_header(self._h, contig, C.byref(txt), C.byref(n))
        if st != KGMA_OK:
            raise KgmaError(st, "genome has no FASTA headers (it was not built from FASTA text)")
        return C.string_at(txt, n.value).decode("utf-8", "replace")

    def chain_values(self, contig: int, kfv: int, intervals) -> np.ndarray:
        """kgma_chain_values: the reference's running Float64 distance of record `contig` for KFV `kfv` (1-based) at the
        windows of `intervals` ((lo, hi) pairs, 1-based window starts), computed by the chain kernel on the device."""
        lo = np.asarray([a for a, _ in intervals], dtype=np.int64)
        hi = np.asarray([b for _, b in intervals], dtype=np.int64)
        n = int((hi - lo + 1).sum())
        out = np.zeros(max(n, 1), dtype=np.float64)
        nn = C.c_int64(0)
        self._ctx._check(load().kgma_chain_values(self._ctx._h, self._h, int(contig), int(kfv), _np_ptr(lo, C.c_int64), _np_ptr(hi, C.c_int64),
                                                  lo.size, _np_ptr(out, C.c_double), out.size, C.byref(nn)))
        return out[:nn.value]

    def fetch(self, contig: int, pos: int, length: int) -> bytes:
        buf = C.create_string_buffer(max(length, 1))
        self._ctx._check(load().kgma_genome_fetch(self._ctx._h, self._h, contig, pos, length, buf))
        return buf.raw[:length]

    def fetch_batch(self, ranges) -> list:
        """`ranges`: (contig, pos, length) triples; one device gather + one download for all of them."""
        ranges = list(ranges)
        if not ranges:
            return []
        c = np.asarray([r[0] for r in ranges], dtype=np.int64)
        p = np.asarray([r[1] for r in ranges], dtype=np.int64)
        ln = np.asarray([r[2] for r in ranges], dtype=np.int64)
        total = int(ln.sum())
        buf = C.create_string_buffer(max(total, 1))
        self._ctx._check(load().kgma_genome_fetch_batch(self._ctx._h, self._h, len(ranges), _np_ptr(c, C.c_int64), _np_ptr(p, C.c_int64),
                                                        _np_ptr(ln, C.c_int64), buf, total))
        raw = buf.raw
        offs = np.concatenate(([0], np.cumsum(ln)))
        return [raw[int(offs[i]):int(offs[i + 1])] for i in range(len(ranges))]

    def poke(self, contig: int, pos: int, data: bytes) -> None:
        self._ctx._check(load().kgma_genome_poke(self._ctx._h, self._h, contig, pos, len(data), bytes(data)))

    def repack(self) -> None:
        self._ctx._check(load().kgma_genome_repack(self._ctx._h, self._h))

    def inter_state(self) -> tuple:
        """kgma_genome_inter_state: (INTER_FULL / INTER_PARTIAL, pack blocks the last step packed on demand)."""
        st, nb = C.c_int32(0), C.c_int64(0)
        self._ctx._check(load().kgma_genome_inter_state(self._h, C.byref(st), C.byref(nb)))
        return int(st.value), int(nb.value)

    def revcomp(self) -> "Genome":
        """kgma_genome_revcomp: a new device genome whose record c is the reverse complement of this genome's record c
        (same lengths and headers), made on the device.  Results on it are in the reversed records' coordinates: position
        p there is L - p + 1 here.  This genome is left as it is; free the new one like any other."""
        h = C.c_void_p()
        self._ctx._check(load().kgma_genome_revcomp(self._ctx._h, self._h, C.byref(h)))
        return Genome(self._ctx, h)

    def revcomp_into(self, rc: "Genome") -> None:
        """kgma_genome_revcomp_into: the kernel alone, into a genome of the same record lengths (repack() it afterwards)."""
        self._ctx._check(load().kgma_genome_revcomp_into(self._ctx._h, self._h, rc._h))

    def free(self) -> None:
        if self._h is not None:
            load().kgma_genome_free(self._ctx._h, self._h)
            self._h = None

    def __del__(self):
        try:
            if self._ctx._h is not None:
                self.free()
        except Exception:
            pass


class Context:
    """One libkgma context = one GPU."""

    def __init__(self, device: int = 0):
        L = load()
        h = C.c_void_p()
        st = L.kgma_create(device, C.byref(h))
        if st != KGMA_OK:
            raise KgmaError(st, L.kgma_status_string(st).decode())
        self._h = h
        self.k = 0
        self.m = 0

    def close(self) -> None:
        if self._h is not None:
            load().kgma_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int) -> None:
        if st == KGMA_OK:
            return
        msg = load().kgma_last_error(self._h).decode()
        if st == KGMA_E_BADBASE:
            raise BadBaseError(st, msg)
        if st == KGMA_E_BOUNDS:
            raise RecordBoundsError(st, msg)
        raise KgmaError(st, msg)

    def set_refs(self, k: int, refs: Sequence[np.ndarray], windowsizes: Sequence[int], thr: Sequence[float],
                 n_refs: Optional[Sequence[int]] = None) -> None:
        m = len(windowsizes)
        R = np.ascontiguousarray(np.stack([np.asarray(r, dtype=np.float64) for r in refs[:m]]))
        if R.shape[1] != 4 ** k:
            raise ValueError(f"KFV length {R.shape[1]} != 4^{k}")
        ws = np.asarray(windowsizes, dtype=np.int64)
        th = np.asarray(list(thr)[:m], dtype=np.float64)
        if th.size != m:
            raise ValueError("need one threshold per KFV")
        nr = None if n_refs is None else np.asarray(n_refs, dtype=np.int64)
        self._check(load().kgma_set_refs(self._h, k, m, _np_ptr(R, C.c_double), _np_ptr(ws, C.c_int64),
                                         _np_ptr(th, C.c_double), None if nr is None else _np_ptr(nr, C.c_int64)))
        self.k, self.m = k, m
        self.ws = [int(w) for w in ws]

    def set_refs_sparse(self, k: int, keys: Sequence[np.ndarray], vals: Sequence[np.ndarray], windowsizes: Sequence[int],
                        thr: Sequence[float], n_refs: Optional[Sequence[int]] = None) -> None:
        """kgma_set_refs_sparse: KFV j given by its non-zero entries -- keys[j] natural k-mer values (0-based, first base most
        significant: the reference's index - 1), strictly increasing, vals[j] their values.  Same semantics as set_refs on the
        dense vectors, 1 <= k <= 15 (a dense KFV at k = 15 is 8 GiB)."""
        m = len(windowsizes)
        ks = [np.asarray(x, dtype=np.uint32).ravel() for x in keys[:m]]
        vs = [np.asarray(x, dtype=np.float64).ravel() for x in vals[:m]]
        if len(ks) != m or len(vs) != m or any(a.size != b.size for a, b in zip(ks, vs)):
            raise ValueError("need one (keys, vals) pair of equal lengths per KFV")
        nnz = np.asarray([a.size for a in ks], dtype=np.int64)
        K = np.ascontiguousarray(np.concatenate(ks + [np.zeros(1, np.uint32)]))
        V = np.ascontiguousarray(np.concatenate(vs + [np.zeros(1, np.float64)]))
        ws = np.asarray(windowsizes, dtype=np.int64)
        th = np.asarray(list(thr)[:m], dtype=np.float64)
        if th.size != m:
            raise ValueError("need one threshold per KFV")
        nr = None if n_refs is None else np.asarray(n_refs, dtype=np.int64)
        self._check(load().kgma_set_refs_sparse(self._h, k, m, _np_ptr(nnz, C.c_int64), _np_ptr(K, C.c_uint32), _np_ptr(V, C.c_double),
                                                _np_ptr(ws, C.c_int64), _np_ptr(th, C.c_double),
                                                None if nr is None else _np_ptr(nr, C.c_int64)))
        self.k, self.m = k, m
        self.ws = [int(w) for w in ws]

    def set_strobe_ref(self, s: int, w_min: int, w_max: int, q: int, ref: np.ndarray, windowsize: int, thr: float,
                       n_refs: Optional[int] = None) -> None:
        """kgma_set_strobe_ref: the strobemer method's reference (4^(2s) bins, natural bin order); replaces the context's
        references.  n_refs=None: N is inferred from the entries."""
        R = np.ascontiguousarray(np.asarray(ref, dtype=np.float64).ravel())
        if not 1 <= int(s) <= 7 or R.size != 4 ** (2 * int(s)):
            raise ValueError(f"KFV length {R.size} != 4^(2*{s})")
        self._check(load().kgma_set_strobe_ref(self._h, int(s), int(w_min), int(w_max), int(q), _np_ptr(R, C.c_double),
                                               int(windowsize), float(thr), 0 if n_refs is None else int(n_refs)))
        self.k, self.m = int(w_max) + int(s) - 1, 1
        self.ws = [int(windowsize)]

    def strobe_scan(self, genome: Genome, buff: int = 50, flags: int = 0, consensus: Optional[bytes] = None,
                    gap_open: int = -69, gap_extend: int = -5, score_threshold: int = 0) -> None:
        """kgma_strobe_scan: StrobeGMA! over every record; consensus=None is do_align = false, otherwise the candidates are
        aligned on the device and those scoring below score_threshold dropped (process_hit!)."""
        cons = None if consensus is None else bytes(consensus)
        self._check(load().kgma_strobe_scan(self._h, genome._h, int(buff), int(flags), cons, 0 if cons is None else len(cons),
                                            int(gap_open), int(gap_extend), int(score_threshold)))

    def exact_match(self, genome: Genome, queries: Sequence[bytes], overlap: bool = True) -> None:
        """kgma_exact_match: every occurrence of every query (DNA symbols, either case) in every record of `genome`, one
        pass over the genome for the whole batch; overlap=False keeps FindAll's non-overlapping leftmost matches.
        Needs no references.  matches() afterwards."""
        text, off = self._concat(queries)
        self._check(load().kgma_exact_match(self._h, genome._h, text, _np_ptr(off, C.c_int64), off.size - 1, 1 if overlap else 0))

    def matches(self) -> np.ndarray:
        """Matches of the last exact_match as a structured array (MATCH_DTYPE: 0-based query and contig, 1-based start),
        sorted by (query, contig, start)."""
        n = C.c_int64(0)
        self._check(load().kgma_get_matches(self._h, None, 0, C.byref(n)))
        arr = np.zeros(max(n.value, 1), dtype=MATCH_DTYPE)
        self._check(load().kgma_get_matches(self._h, arr.ctypes.data_as(C.POINTER(KgmaMatch)), n.value, C.byref(n)))
        return arr[:n.value]

    def motif_match(self, genome: Genome, motifs: Sequence[bytes], max_mismatch: Sequence[int]) -> None:
        """kgma_motif_match: every start in every record of `genome` at which motif i (1 ... 64 IUPAC symbols, either case)
        lies with at most max_mismatch[i] non-matching positions; one pass over the genome for the whole batch.  Needs no
        references.  motif_matches() afterwards."""
        text, off = self._concat(motifs)
        mm = np.ascontiguousarray(np.asarray(list(max_mismatch), dtype=np.int32).ravel())
        if mm.size != off.size - 1:
            raise ValueError("need one max_mismatch per motif")
        mm = np.concatenate([mm, np.zeros(1, np.int32)])          # (never empty: a pointer to take)
        self._check(load().kgma_motif_match(self._h, genome._h, text, _np_ptr(off, C.c_int64), off.size - 1, _np_ptr(mm, C.c_int32)))

    def motif_matches(self) -> np.ndarray:
        """Hits of the last motif_match as a structured array (MOTIF_HIT_DTYPE: 0-based motif and contig, 1-based start,
        mismatches), sorted by (motif, contig, start)."""
        n = C.c_int64(0)
        self._check(load().kgma_get_motif_matches(self._h, None, 0, C.byref(n)))
        arr = np.zeros(max(n.value, 1), dtype=MOTIF_HIT_DTYPE)
        self._check(load().kgma_get_motif_matches(self._h, arr.ctypes.data_as(C.POINTER(KgmaMotifHit)), n.value, C.byref(n)))
        return arr[:n.value]

    def approx_match(self, genome: Genome, queries: Sequence[bytes], max_edits: Sequence[int], best_only: bool = True) -> None:
        """kgma_approx_match: every end in every record of `genome` at which query i (1 ... 64 IUPAC symbols, either case) lies
        within max_edits[i] edits (substitutions, insertions, deletions) of a substring ending there; best_only keeps the best
        end of every run of consecutive ends.  One pass over the genome for the whole batch.  Needs no references.
        approx_matches() afterwards."""
        text, off = self._concat(queries)
        ed = np.ascontiguousarray(np.asarray(list(max_edits), dtype=np.int32).ravel())
        if ed.size != off.size - 1:
            raise ValueError("need one max_edits per query")
        ed = np.concatenate([ed, np.zeros(1, np.int32)])          # (never empty: a pointer to take)
        self._check(load().kgma_approx_match(self._h, genome._h, text, _np_ptr(off, C.c_int64), off.size - 1, _np_ptr(ed, C.c_int32),
                                             1 if best_only else 0))

    def approx_matches(self) -> np.ndarray:
        """Hits of the last approx_match as a structured array (APPROX_HIT_DTYPE: 0-based query and contig, the 1-based
        inclusive range start:end, edits), sorted by (query, contig, end)."""
        n = C.c_int64(0)
        self._check(load().kgma_get_approx_matches(self._h, None, 0, C.byref(n)))
        arr = np.zeros(max(n.value, 1), dtype=APPROX_HIT_DTYPE)
        self._check(load().kgma_get_approx_matches(self._h, arr.ctypes.data_as(C.POINTER(KgmaApproxHit)), n.value, C.byref(n)))
        return arr[:n.value]

    def approx_stats(self) -> dict:
        """kgma_get_approx_stats: the search kernel's geometry and form, ends, hits, launches and device times of the last
        approx_match."""
        s = KgmaApproxStats()
        self._check(load().kgma_get_approx_stats(self._h, C.byref(s)))
        return {name: getattr(s, name) for name, _ in KgmaApproxStats._fields_}

    def pwm_match(self, genome: Genome, matrices: Sequence, thresholds: Sequence[int]) -> None:
        """kgma_pwm_match: every start in every record of `genome` at which matrix i -- (m, 4) integer weights in the order
        A, C, G, T, 1 <= m <= 64, each in -32768 ... 32767 -- scores at least thresholds[i]; a genome N scores its row's minimum.
        One pass over the genome for the whole batch.  Needs no references.  pwm_matches() afterwards."""
        mats = [np.asarray(m) for m in matrices]
        for i, m in enumerate(mats):
            if m.ndim != 2 or m.shape[1] != 4 or not np.issubdtype(m.dtype, np.integer):
                raise ValueError(f"matrix {i}: need an (m, 4) array of integers")
            bad = np.argwhere((m < -32768) | (m > 32767))
            if bad.size:
                raise ValueError(f"matrix {i}, row {int(bad[0][0]) + 1}: weight {int(m[tuple(bad[0])])} is outside -32768 ... 32767")
        thr = [int(t) for t in thresholds]
        if len(thr) != len(mats):
            raise ValueError("need one threshold per matrix")
        for i, t in enumerate(thr):
            if not -2 ** 31 <= t < 2 ** 31:
                raise ValueError(f"matrix {i}: threshold {t} does not fit an int32")
        w = np.ascontiguousarray(np.concatenate([m.reshape(-1, 4) for m in mats] + [np.zeros((1, 4), np.int64)]).astype(np.int16))
        off = np.zeros(len(mats) + 1, dtype=np.int64)
        off[1:] = np.cumsum([m.shape[0] for m in mats])
        th = np.asarray(thr + [0], dtype=np.int32)                  # (never empty: a pointer to take)
        self._check(load().kgma_pwm_match(self._h, genome._h, _np_ptr(w, C.c_int16), _np_ptr(off, C.c_int64), len(mats),
                                          _np_ptr(th, C.c_int32)))

    def pwm_matches(self) -> np.ndarray:
        """Hits of the last pwm_match as a structured array (PWM_HIT_DTYPE: 0-based matrix and contig, 1-based start, score),
        sorted by (matrix, contig, start)."""
        n = C.c_int64(0)
        self._check(load().kgma_get_pwm_matches(self._h, None, 0, C.byref(n)))
        arr = np.zeros(max(n.value, 1), dtype=PWM_HIT_DTYPE)
        self._check(load().kgma_get_pwm_matches(self._h, arr.ctypes.data_as(C.POINTER(KgmaPwmHit)), n.value, C.byref(n)))
        return arr[:n.value]

    def pwm_stats(self) -> dict:
        """kgma_get_pwm_stats: the kernel's geometry, candidates, hits, launches and device time of the last pwm_match."""
        s = KgmaPwmStats()
        self._check(load().kgma_get_pwm_stats(self._h, C.byref(s)))
        return {name: getattr(s, name) for name, _ in KgmaPwmStats._fields_}

    def codon_match(self, genome: Genome, matrices: Sequence, thresholds: Sequence[int]) -> None:
        """kgma_codon_match: every nucleotide start in every record of `genome` at which codon matrix i -- (m, 65) integer
        weights, 1 <= m <= 64, each in -32768 ... 32767; entry 16 b0 + 4 b1 + b2 (A 0, C 1, G 2, T 3) the codon b0 b1 b2,
        entry 64 a codon with an N -- scores at least thresholds[i], all three frames.  One pass over the genome for the whole
        batch.  Needs no references.  codon_matches() afterwards."""
        mats = [np.asarray(m) for m in matrices]
        for i, m in enumerate(mats):
            if m.ndim != 2 or m.shape[1] != CODON_ENTRIES or not np.issubdtype(m.dtype, np.integer):
                raise ValueError(f"matrix {i}: need an (m, {CODON_ENTRIES}) array of integers")
            bad = np.argwhere((m < -32768) | (m > 32767))
            if bad.size:
                raise ValueError(f"matrix {i}, row {int(bad[0][0]) + 1}: weight {int(m[tuple(bad[0])])} is outside -32768 ... 32767")
        thr = [int(t) for t in thresholds]
        if len(thr) != len(mats):
            raise ValueError("need one threshold per matrix")
        for i, t in enumerate(thr):
            if not -2 ** 31 <= t < 2 ** 31:
                raise ValueError(f"matrix {i}: threshold {t} does not fit an int32")
        w = np.ascontiguousarray(np.concatenate([m.reshape(-1, CODON_ENTRIES) for m in mats]
                                                + [np.zeros((1, CODON_ENTRIES), np.int64)]).astype(np.int16))
        off = np.zeros(len(mats) + 1, dtype=np.int64)
        off[1:] = np.cumsum([m.shape[0] for m in mats])
        th = np.asarray(thr + [0], dtype=np.int32)                  # (never empty: a pointer to take)
        self._check(load().kgma_codon_match(self._h, genome._h, _np_ptr(w, C.c_int16), _np_ptr(off, C.c_int64), len(mats),
                                            _np_ptr(th, C.c_int32)))

    def codon_matches(self) -> np.ndarray:
        """Hits of the last codon_match as a structured array (CODON_HIT_DTYPE: 0-based matrix and contig, 1-based nucleotide
        start, score), sorted by (matrix, contig, start)."""
        n = C.c_int64(0)
        self._check(load().kgma_get_codon_matches(self._h, None, 0, C.byref(n)))
        arr = np.zeros(max(n.value, 1), dtype=CODON_HIT_DTYPE)
        self._check(load().kgma_get_codon_matches(self._h, arr.ctypes.data_as(C.POINTER(KgmaCodonHit)), n.value, C.byref(n)))
        return arr[:n.value]

    def codon_stats(self) -> dict:
        """kgma_get_codon_stats: the kernel's geometry, candidates, hits, launches and device time of the last codon_match."""
        s = KgmaCodonStats()
        self._check(load().kgma_get_codon_stats(self._h, C.byref(s)))
        return {name: getattr(s, name) for name, _ in KgmaCodonStats._fields_}

    def set_thresholds(self, thr: Sequence[float]) -> None:
        th = np.asarray(list(thr)[:self.m], dtype=np.float64)
        self._check(load().kgma_set_thresholds(self._h, _np_ptr(th, C.c_double)))

    def genome_from_host(self, contigs: Sequence[bytes]) -> Genome:
        n = len(contigs)
        arr = (C.c_char_p * max(n, 1))(*[bytes(c) for c in contigs])
        lens = np.asarray([len(c) for c in contigs], dtype=np.int64)
        h = C.c_void_p()
        self._check(load().kgma_genome_from_host(self._h, arr, _np_ptr(lens, C.c_int64) if n else None, n, C.byref(h)))
        return Genome(self, h)

    def genome_from_fasta(self, source) -> Genome:
        """Device-side FASTA ingest. `source` is a path (kgma_genome_from_fasta_file: read straight into the pinned staging
        buffers) or a bytes object."""
        h = C.c_void_p()
        if not isinstance(source, (bytes, bytearray)):
            self._check(load().kgma_genome_from_fasta_file(self._h, os.fsencode(source), C.byref(h)))
            return Genome(self, h)
        buf = np.frombuffer(bytes(source), dtype=np.uint8)
        ptr = buf.ctypes.data_as(C.c_void_p) if buf.size else None
        self._check(load().kgma_genome_from_fasta(self._h, ptr, int(buf.size), C.byref(h)))
        return Genome(self, h)

    def genome_from_2bit(self, path, mask: bool = True) -> Genome:
        """kgma_genome_from_2bit_file: a UCSC .2bit file, shipped packed (0.25 byte per base) and expanded to the resident
        text on the device; header(c) is record c's name.  mask=False ignores the soft-mask blocks (all upper case)."""
        h = C.c_void_p()
        self._check(load().kgma_genome_from_2bit_file(self._h, os.fsencode(path), 0 if mask else TWOBIT_NOMASK, C.byref(h)))
        return Genome(self, h)

    def twobit_unpack_ms(self) -> float:
        """kgma_get_2bit_unpack_ms: device time of the unpack kernel in the last genome_from_2bit."""
        ms = C.c_double(0)
        self._check(load().kgma_get_2bit_unpack_ms(self._h, C.byref(ms)))
        return ms.value

    def genome_from_path(self, path) -> Genome:
        """A genome file by its content: the .2bit signature in the first four bytes -> genome_from_2bit, anything else ->
        genome_from_fasta (the file extension is not looked at)."""
        return self.genome_from_2bit(path) if is_twobit(path) else self.genome_from_fasta(path)

    def genome_synthetic(self, contig_lens: Sequence[int], seed: int, plant: bytes = b"",
                         plants: Sequence = ()) -> Genome:
        lens = np.asarray(contig_lens, dtype=np.int64)
        pc = np.asarray([p[0] for p in plants], dtype=np.int64)
        pp = np.asarray([p[1] for p in plants], dtype=np.int64)
        h = C.c_void_p()
        self._check(load().kgma_genome_synthetic(
            self._h, _np_ptr(lens, C.c_int64), lens.size, C.c_uint64(seed & (2 ** 64 - 1)), plant if plants else None,
            len(plant), _np_ptr(pc, C.c_int64) if len(plants) else None, _np_ptr(pp, C.c_int64) if len(plants) else None,
            len(plants), C.byref(h)))
        return Genome(self, h)

    def scan(self, genome: Genome, mode: int, buff: int = 50, genome_pos: int = 0, flags: int = 0,
             align: Optional[Callable] = None) -> None:
        if align is None:
            cb = C.cast(None, ALIGN_FN)
        else:
            def tramp(_u, contig, kfv, lo, hi, L, plo, phi):
                nlo, nhi = align(int(contig), int(kfv), int(lo), int(hi), int(L))
                plo[0], phi[0] = int(nlo), int(nhi)
            cb = ALIGN_FN(tramp)
        self._check(load().kgma_scan(self._h, genome._h, mode, buff, genome_pos, flags, cb, None))

    def scan_aligned(self, genome: Genome, mode: int, buff: int, genome_pos: int, flags: int, consensus: Sequence[bytes],
                     gap_open: int, gap_extend: int) -> None:
        """kgma_scan_aligned: the scan with the hits re-aligned on the device in batches (cluster engine: every dip's
        candidate range is aligned speculatively and looked up by the hit state machine)."""
        cons = [bytes(c) for c in consensus]
        arr = (C.c_char_p * max(len(cons), 1))(*cons)
        lens = np.asarray([len(c) for c in cons], dtype=np.int64)
        self._check(load().kgma_scan_aligned(self._h, genome._h, mode, buff, genome_pos, flags, arr, _np_ptr(lens, C.c_int64),
                                             int(gap_open), int(gap_extend)))

    def alignments(self):
        """(list of dict(contig, kfv, lo, hi, first, last) consumed by the last scan_aligned, n on the device, n on the host)."""
        n, nd, nh = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._check(load().kgma_get_alignments(self._h, None, 0, C.byref(n), C.byref(nd), C.byref(nh)))
        arr = (KgmaAlignment * max(n.value, 1))()
        self._check(load().kgma_get_alignments(self._h, arr, n.value, C.byref(n), C.byref(nd), C.byref(nh)))
        return ([dict(contig=x.contig, kfv=x.kfv, lo=x.lo, hi=x.hi, first=x.first, last=x.last) for x in arr[:n.value]],
                int(nd.value), int(nh.value))

    def scan_device(self, genome: Genome, mode: int, flags: int = 0) -> None:
        self._check(load().kgma_scan_device(self._h, genome._h, mode, flags))

    def hits(self) -> List[dict]:
        n = C.c_int64(0)
        self._check(load().kgma_get_hits(self._h, None, 0, C.byref(n)))
        arr = (KgmaHit * max(n.value, 1))()
        self._check(load().kgma_get_hits(self._h, arr, n.value, C.byref(n)))
        return [dict(contig=h.contig, kfv=h.kfv, cmi=h.cmi, lo=h.lo, hi=h.hi, genome_pos=h.genome_pos,
                     dist=h.dist, D=h.D, flags=h.flags) for h in arr[:n.value]]

    def hits_array(self) -> np.ndarray:
        """Hits of the last scan as a numpy structured array (no per-hit Python objects)."""
        n = C.c_int64(0)
        self._check(load().kgma_get_hits(self._h, None, 0, C.byref(n)))
        arr = np.zeros(max(n.value, 1), dtype=HIT_DTYPE)
        self._check(load().kgma_get_hits(self._h, arr.ctypes.data_as(C.POINTER(KgmaHit)), n.value, C.byref(n)))
        return arr[:n.value]

    def dips(self) -> List[dict]:
        n = C.c_int64(0)
        self._check(load().kgma_get_dips(self._h, None, 0, C.byref(n)))
        arr = (KgmaDip * max(n.value, 1))()
        self._check(load().kgma_get_dips(self._h, arr, n.value, C.byref(n)))
        return [dict(contig=d.contig, kfv=d.kfv, start=d.start, end=d.end, argmin=d.argmin, D_min=d.D_min,
                     exit_pos=d.exit_pos, D_exit=d.D_exit, flags=d.flags) for d in arr[:n.value]]

    def first_window(self, kfv: int = 1) -> np.ndarray:
        n = C.c_int64(0)
        self._check(load().kgma_get_first_window(self._h, kfv, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.int64)
        self._check(load().kgma_get_first_window(self._h, kfv, _np_ptr(out, C.c_int64), out.size, C.byref(n)))
        return out[:n.value]

    def dists(self, kfv: int = 1) -> np.ndarray:
        n = C.c_int64(0)
        self._check(load().kgma_get_dists(self._h, kfv, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.float64)
        self._check(load().kgma_get_dists(self._h, kfv, _np_ptr(out, C.c_double), out.size, C.byref(n)))
        return out[:n.value]

    def dist_layout(self) -> np.ndarray:
        """kgma_dist_layout: record c's values are offset[c] .. offset[c + 1] of dists(); value i of a record is window start i + 2."""
        n = C.c_int64(0)
        self._check(load().kgma_dist_layout(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.int64)
        self._check(load().kgma_dist_layout(self._h, _np_ptr(out, C.c_int64), out.size, C.byref(n)))
        return out[:n.value]

    def dist_bins(self, kfv: int = 1, bin: int = 1):
        """kgma_dist_bins over the distances the last scan kept on the device: (bin_min, bin_argmin, bin_offset).  Record c's bins
        are bin_offset[c] .. bin_offset[c + 1]; bin_argmin is the window start (1-based, within the record) of the first value
        attaining bin_min."""
        n_rec = self.dist_layout().size - 1
        n = C.c_int64(0)
        off = np.zeros(n_rec + 1, dtype=np.int64)
        self._check(load().kgma_dist_bins(self._h, int(kfv), int(bin), None, None, _np_ptr(off, C.c_int64), 0, C.byref(n)))
        bmin = np.zeros(max(n.value, 1), dtype=np.float64)
        barg = np.zeros(max(n.value, 1), dtype=np.int64)
        self._check(load().kgma_dist_bins(self._h, int(kfv), int(bin), _np_ptr(bmin, C.c_double), _np_ptr(barg, C.c_int64),
                                          _np_ptr(off, C.c_int64), bmin.size, C.byref(n)))
        return bmin[:n.value], barg[:n.value], off

    def dist_sweep(self, thresholds, kfv: int = 1):
        """kgma_dist_sweep: (windows_below, dips_below) per threshold (finite, strictly increasing, at most SWEEP_MAX_THRESHOLDS)."""
        thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        below = np.zeros(max(thr.size, 1), dtype=np.int64)
        dips = np.zeros(max(thr.size, 1), dtype=np.int64)
        self._check(load().kgma_dist_sweep(self._h, int(kfv), _np_ptr(thr, C.c_double) if thr.size else None, thr.size,
                                           _np_ptr(below, C.c_int64), _np_ptr(dips, C.c_int64)))
        return below[:thr.size], dips[:thr.size]

    def landscape_stats(self) -> dict:
        """kgma_get_landscape_stats: device times, values read and launches of the last dist_bins / dist_sweep."""
        s = KgmaLandscapeStats()
        self._check(load().kgma_get_landscape_stats(self._h, C.byref(s)))
        return {name: getattr(s, name) for name, _ in KgmaLandscapeStats._fields_}

    def dips_array(self) -> np.ndarray:
        """Dips of the last scan as a numpy structured array (DIP_DTYPE)."""
        n = C.c_int64(0)
        self._check(load().kgma_get_dips(self._h, None, 0, C.byref(n)))
        arr = np.zeros(max(n.value, 1), dtype=DIP_DTYPE)
        self._check(load().kgma_get_dips(self._h, arr.ctypes.data_as(C.POINTER(KgmaDip)), n.value, C.byref(n)))
        return arr[:n.value]

    def dip_last_min(self) -> np.ndarray:
        """Last window attaining the minimum of every dip (parallel to dips_array())."""
        n = C.c_int64(0)
        self._check(load().kgma_get_dip_last_min(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.int64)
        self._check(load().kgma_get_dip_last_min(self._h, _np_ptr(out, C.c_int64), out.size, C.byref(n)))
        return out[:n.value]

    def set_residue_source(self, fetch: Optional[Callable]) -> None:
        """kgma_set_residue_source: `fetch(record, pos, length) -> bytes` serves residues to kgma_replay_dips (ties between a
        dip found on another GPU and the stale running minimum); None removes it."""
        if fetch is None:
            self._fetch_cb = None
            self._check(load().kgma_set_residue_source(self._h, C.cast(None, FETCH_FN), None))
            return

        def tramp(_u, contig, pos, length, out):
            try:
                data = fetch(int(contig), int(pos), int(length))
                if len(data) != length:
                    return 1
                C.memmove(out, bytes(data), length)
                return 0
            except Exception:
                return 1
        self._fetch_cb = FETCH_FN(tramp)                 # kept alive with the context
        self._check(load().kgma_set_residue_source(self._h, self._fetch_cb, None))

    def set_chain_source(self, source: Optional[Callable]) -> None:
        """kgma_set_chain_source: `source(pairs) -> list of arrays`, pairs = [(record, kfv (1-based), [(lo, hi), ...]), ...],
        must return for every pair the reference's running Float64 value at its wanted windows, in order; None removes it."""
        if source is None:
            self._chain_cb = None
            self._check(load().kgma_set_chain_source(self._h, C.cast(None, CHAIN_FN), None))
            return

        def tramp(_u, n_pairs, contig, kfv, ivb, lo, hi, values):
            try:
                pairs = []
                for p in range(int(n_pairs)):
                    pairs.append((int(contig[p]), int(kfv[p]), [(int(lo[i]), int(hi[i])) for i in range(int(ivb[p]), int(ivb[p + 1]))]))
                out = source(pairs)
                off = 0
                for (c, j, iv), v in zip(pairs, out):
                    n = sum(b - a + 1 for a, b in iv)
                    v = np.ascontiguousarray(v, dtype=np.float64)
                    if v.size != n:
                        return 2
                    C.memmove(C.addressof(values.contents) + 8 * off, v.ctypes.data, 8 * n)
                    off += n
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return 1
        self._chain_cb = CHAIN_FN(tramp)                 # kept alive with the context
        self._check(load().kgma_set_chain_source(self._h, self._chain_cb, None))

    def kfv_scale(self, kfv: int) -> float:
        """2 k N^2 of KFV `kfv` (1-based)."""
        sc = C.c_double(0)
        self._check(load().kgma_kfv_scale(self._h, int(kfv), C.byref(sc), None))
        return sc.value

    def kfv_is_float(self, kfv: int) -> bool:
        """True if KFV `kfv` (1-based) is scanned as a general Float64 vector (not S/N)."""
        v = C.c_int32(0)
        self._check(load().kgma_kfv_is_float(self._h, int(kfv), C.byref(v)))
        return bool(v.value)

    def att(self) -> np.ndarray:
        """kgma_get_att: tested windows inside the threshold guard band, as an (n, 3) int64 array (record, 1-based KFV, window)."""
        n = C.c_int64(0)
        self._check(load().kgma_get_att(self._h, None, None, None, 0, C.byref(n)))
        c = np.zeros(max(n.value, 1), dtype=np.int32); j = np.zeros(max(n.value, 1), dtype=np.int32); p = np.zeros(max(n.value, 1), dtype=np.int64)
        if n.value:
            self._check(load().kgma_get_att(self._h, _np_ptr(c, C.c_int32), _np_ptr(j, C.c_int32), _np_ptr(p, C.c_int64), n.value, C.byref(n)))
        return np.stack([c[:n.value].astype(np.int64), j[:n.value].astype(np.int64), p[:n.value]], axis=1) if n.value else np.zeros((0, 3), dtype=np.int64)

    def set_att(self, att) -> None:
        """kgma_set_att: guard-band windows ((n, 3): record, 1-based KFV, window) for the next replay_dips."""
        a = np.asarray(att, dtype=np.int64).reshape(-1, 3)
        c = np.ascontiguousarray(a[:, 0], dtype=np.int32); j = np.ascontiguousarray(a[:, 1], dtype=np.int32); p = np.ascontiguousarray(a[:, 2], dtype=np.int64)
        n = a.shape[0]
        self._check(load().kgma_set_att(self._h, _np_ptr(c, C.c_int32) if n else None, _np_ptr(j, C.c_int32) if n else None,
                                        _np_ptr(p, C.c_int64) if n else None, n))

    def chain_export(self, genome: "Genome", contig: int, kfv: int, last_window: int, intervals) -> dict:
        """kgma_chain_export: the chain kernel's output for windows 1 .. last_window of (record, KFV), as host_chain_walk takes
        it: dict(first, win0, n_valid, chunk_base, D0, chunks, pool)."""
        lo = np.asarray([a for a, _ in intervals], dtype=np.int64)
        hi = np.asarray([b for _, b in intervals], dtype=np.int64)
        ns, nc, npool, first = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_double(0)
        self._check(load().kgma_chain_export(self._h, genome._h, int(contig), int(kfv), int(last_window), _np_ptr(lo, C.c_int64) if lo.size else None,
                                             _np_ptr(hi, C.c_int64) if hi.size else None, lo.size, C.byref(ns), C.byref(nc), C.byref(npool),
                                             C.byref(first)))
        win0 = np.zeros(max(ns.value, 1), dtype=np.int64); nv = np.zeros(max(ns.value, 1), dtype=np.int32)
        cb = np.zeros(max(ns.value, 1), dtype=np.int64); D0 = np.zeros(max(ns.value, 1), dtype=np.int64)
        chunks = np.zeros(max(nc.value, 1), dtype=CHAIN_CHUNK_DTYPE); pool = np.zeros(max(npool.value, 1), dtype=CHAIN_CHUNK_DTYPE)
        self._check(load().kgma_chain_export_copy(self._h, _np_ptr(win0, C.c_int64), _np_ptr(nv, C.c_int32), _np_ptr(cb, C.c_int64), _np_ptr(D0, C.c_int64),
                                                  chunks.ctypes.data_as(C.c_void_p), pool.ctypes.data_as(C.c_void_p)))
        return dict(first=first.value, win0=win0[:ns.value], n_valid=nv[:ns.value], chunk_base=cb[:ns.value], D0=D0[:ns.value],
                    chunks=chunks[:nc.value], pool=pool[:npool.value])

    def resolve_ties_local(self, genome: "Genome") -> None:
        self._check(load().kgma_resolve_ties_local(self._h, genome._h))

    def replay_dips(self, mode: int, buff: int, genome_pos: int, flags: int, record_len, first_D, dips: np.ndarray,
                    last_min: np.ndarray, align: Optional[Callable] = None) -> None:
        """Hit state machine over dips gathered from a sharded scan (kgma_replay_dips); hits() afterwards."""
        rl = np.ascontiguousarray(record_len, dtype=np.int64)
        fd = np.ascontiguousarray(first_D, dtype=np.int64).reshape(-1)
        dd = np.ascontiguousarray(dips, dtype=DIP_DTYPE)
        lm = np.ascontiguousarray(last_min, dtype=np.int64)
        if align is None:
            cb = C.cast(None, ALIGN_FN)
        else:
            def tramp(_u, contig, kfv, lo, hi, L, plo, phi):
                nlo, nhi = align(int(contig), int(kfv), int(lo), int(hi), int(L))
                plo[0], phi[0] = int(nlo), int(nhi)
            cb = ALIGN_FN(tramp)
        self._check(load().kgma_replay_dips(self._h, mode, buff, genome_pos, flags, rl.size, _np_ptr(rl, C.c_int64),
                                            _np_ptr(fd, C.c_int64), dd.ctypes.data_as(C.POINTER(KgmaDip)),
                                            _np_ptr(lm, C.c_int64), dd.size, cb, None))

    def align_hits_device(self, genome: "Genome", consensus: bytes, gap_open: int, gap_extend: int, contig, lo, hi):
        """Batched semi-global affine re-alignment of hit ranges on the device (kgma_align_hits_device).
        Returns (first, last, score) arrays: cigar_to_UnitRange's range of every alignment."""
        c = np.ascontiguousarray(contig, dtype=np.int32)
        a = np.ascontiguousarray(lo, dtype=np.int64)
        b = np.ascontiguousarray(hi, dtype=np.int64)
        n = c.size
        first = np.zeros(max(n, 1), dtype=np.int64)
        last = np.zeros(max(n, 1), dtype=np.int64)
        score = np.zeros(max(n, 1), dtype=np.int64)
        self._check(load().kgma_align_hits_device(self._h, genome._h, bytes(consensus), len(consensus), int(gap_open), int(gap_extend),
                                                  n, _np_ptr(c, C.c_int32) if n else None, _np_ptr(a, C.c_int64) if n else None,
                                                  _np_ptr(b, C.c_int64) if n else None, _np_ptr(first, C.c_int64),
                                                  _np_ptr(last, C.c_int64), _np_ptr(score, C.c_int64)))
        return first[:n], last[:n], score[:n]

    @staticmethod
    def _concat(seqs):
        seqs = [bytes(x) for x in seqs]
        off = np.zeros(len(seqs) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in seqs], out=off[1:])
        return b"".join(seqs), off

    def kmer_count_batch(self, seqs, k: int) -> np.ndarray:
        """kmer_count (src/Kmers.jl:14-28) of every sequence on the device: Float64 array [n, 4^k]."""
        text, off = self._concat(seqs)
        n = off.size - 1
        bins = np.zeros((max(n, 1), 4 ** k), dtype=np.float64)
        self._check(load().kgma_kmer_count_batch(self._h, int(k), text, _np_ptr(off, C.c_int64), n, _np_ptr(bins, C.c_double)))
        return bins[:n]

    def kmer_dist_batch(self, seqs, kfv, k: int) -> np.ndarray:
        """kmer_dist(seq, KFV, k) (src/Kmers.jl:58-60) of every sequence against one KFV on the device."""
        ref = np.ascontiguousarray(kfv, dtype=np.float64)
        if ref.size != 4 ** k:
            raise ValueError("the KFV must have 4^k entries")
        text, off = self._concat(seqs)
        n = off.size - 1
        out = np.zeros(max(n, 1), dtype=np.float64)
        self._check(load().kgma_kmer_dist_batch(self._h, int(k), _np_ptr(ref, C.c_double), text, _np_ptr(off, C.c_int64), n,
                                                _np_ptr(out, C.c_double)))
        return out[:n]

    def window_dists(self, genome: "Genome", kfv: int, contig, start):
        """kgma_window_dists: (D, dist) of the windows of W residues that begin at `start[i]` (1-based) of record `contig[i]`
        (0-based) against KFV `kfv` (1-based; W is that KFV's window size).  D: int64, the exact integer distance of an S/N
        KFV (llround(dist * scale) for a Float64 KFV); dist: float64.  Any list: unsorted, with duplicates, empty."""
        c = np.ascontiguousarray(np.asarray(contig, dtype=np.int32).ravel())
        s = np.ascontiguousarray(np.asarray(start, dtype=np.int64).ravel())
        if c.size != s.size:
            raise ValueError("need one start per contig")
        n = int(c.size)
        D = np.zeros(max(n, 1), dtype=np.int64)
        dist = np.zeros(max(n, 1), dtype=np.float64)
        self._check(load().kgma_window_dists(self._h, genome._h, int(kfv), n, _np_ptr(c, C.c_int32) if n else None,
                                             _np_ptr(s, C.c_int64) if n else None, _np_ptr(D, C.c_int64), _np_ptr(dist, C.c_double)))
        return D[:n], dist[:n]

    def mutation_dists(self, seqs, kfv: int, rates, n_trials: int, seed: int):
        """kgma_mutation_dists: (D, dist), each [n_seqs, n_rates, n_trials]: the distance to KFV `kfv` (1-based) of sequence i
        (A/C/G/T, either case) mutated at rates[r] in trial t -- api.mutate_seq(seq_i, rates[r], seed=seed, stream=(i, r, t)),
        never materialised on the device.  The index r is part of the trial key: reordering `rates` redraws the substitutions
        (a rate of 0 excepted, which never substitutes); nothing depends on the sequences, rates or trials that follow."""
        text, off = self._concat(seqs)
        ns = off.size - 1
        rt = np.ascontiguousarray(np.asarray(rates, dtype=np.float64).ravel())
        nr, nt = int(rt.size), int(n_trials)
        shape = (ns, max(nr, 0), max(nt, 0))
        D = np.zeros(max(int(np.prod(shape)), 1), dtype=np.int64)
        dist = np.zeros(D.size, dtype=np.float64)
        rt_arg = rt if nr else np.zeros(1, dtype=np.float64)
        self._check(load().kgma_mutation_dists(self._h, int(kfv), text, _np_ptr(off, C.c_int64), ns, _np_ptr(rt_arg, C.c_double), nr, nt,
                                               C.c_uint64(int(seed) & (2 ** 64 - 1)), _np_ptr(D, C.c_int64), _np_ptr(dist, C.c_double)))
        n = int(np.prod(shape))
        return D[:n].reshape(shape), dist[:n].reshape(shape)

    def strobe_window_dists(self, genome: "Genome", contig, start):
        """kgma_strobe_window_dists: (D, dist) of the strobemer scan's windows with start `start[i]` (1-based, 1 ... max(1, L - W))
        of record `contig[i]` (0-based) against the reference of set_strobe_ref: the W - k + 1 randstrobes the scan's count
        vector holds there, the record's permanent one (position W - k + 1) included for start >= 2.  D: int64, exactly what
        hits()["D"] and first_window() report; dist = D / kfv_scale(1).  Any list: unsorted, with duplicates, empty."""
        c = np.ascontiguousarray(np.asarray(contig, dtype=np.int32).ravel())
        s = np.ascontiguousarray(np.asarray(start, dtype=np.int64).ravel())
        if c.size != s.size:
            raise ValueError("need one start per contig")
        n = int(c.size)
        D = np.zeros(max(n, 1), dtype=np.int64)
        dist = np.zeros(max(n, 1), dtype=np.float64)
        self._check(load().kgma_strobe_window_dists(self._h, genome._h, n, _np_ptr(c, C.c_int32) if n else None,
                                                    _np_ptr(s, C.c_int64) if n else None, _np_ptr(D, C.c_int64), _np_ptr(dist, C.c_double)))
        return D[:n], dist[:n]

    def strobe_mutation_dists(self, seqs, rates, n_trials: int, seed: int):
        """kgma_strobe_mutation_dists: (D, dist), each [n_seqs, n_rates, n_trials]: the distance of the reference of set_strobe_ref
        to the randstrobe counts of api.mutate_seq(seq_i, rates[r], seed=seed, stream=(i, r, t)) -- all len - k + 1 of them, no
        permanent item --, never materialised on the device.  Keys, layout and errors as mutation_dists."""
        text, off = self._concat(seqs)
        ns = off.size - 1
        rt = np.ascontiguousarray(np.asarray(rates, dtype=np.float64).ravel())
        nr, nt = int(rt.size), int(n_trials)
        shape = (ns, max(nr, 0), max(nt, 0))
        n = int(np.prod(shape))
        D = np.zeros(max(n, 1), dtype=np.int64)
        dist = np.zeros(D.size, dtype=np.float64)
        rt_arg = rt if nr else np.zeros(1, dtype=np.float64)
        self._check(load().kgma_strobe_mutation_dists(self._h, text, _np_ptr(off, C.c_int64), ns, _np_ptr(rt_arg, C.c_double), nr, nt,
                                                      C.c_uint64(int(seed) & (2 ** 64 - 1)), _np_ptr(D, C.c_int64), _np_ptr(dist, C.c_double)))
        return D[:n].reshape(shape), dist[:n].reshape(shape)

    def assign_seqs(self, refs, queries, gap_open: int = -69, gap_extend: int = -1, top: int = 1):
        """kgma_assign_seqs: every query (bytes) against every reference (bytes) under the hit aligner's model.  Returns
        (out, scores): out is an ASSIGNMENT_DTYPE array [n_queries, top] -- per query its `top` best references, higher score
        first, lower index among equal scores, with the column counts of that alignment --, scores the int32 matrix
        [n_queries, n_refs]."""
        rtext, roff = self._concat(refs)
        qtext, qoff = self._concat(queries)
        nr, nq, top = roff.size - 1, qoff.size - 1, int(top)
        out = np.zeros((nq, max(top, 0)), dtype=ASSIGNMENT_DTYPE)
        scores = np.zeros((nq, max(nr, 0)), dtype=np.int32)
        self._check(load().kgma_assign_seqs(self._h, rtext, _np_ptr(roff, C.c_int64), nr, qtext, _np_ptr(qoff, C.c_int64), nq,
                                            int(gap_open), int(gap_extend), top, out.ctypes.data if out.size else None,
                                            _np_ptr(scores, C.c_int32) if scores.size else None))
        return out, scores

    def assign_ranges(self, genome: "Genome", refs, contig, lo, hi, gap_open: int = -69, gap_extend: int = -1, top: int = 1):
        """kgma_assign_ranges: as assign_seqs, the queries being residues lo[i] .. hi[i] (1-based inclusive) of record contig[i]
        (0-based) of the resident genome."""
        rtext, roff = self._concat(refs)
        c = np.ascontiguousarray(np.asarray(contig, dtype=np.int32).ravel())
        a = np.ascontiguousarray(np.asarray(lo, dtype=np.int64).ravel())
        b = np.ascontiguousarray(np.asarray(hi, dtype=np.int64).ravel())
        if not (c.size == a.size == b.size):
            raise ValueError("need one lo and one hi per contig")
        nr, nq, top = roff.size - 1, int(c.size), int(top)
        out = np.zeros((nq, max(top, 0)), dtype=ASSIGNMENT_DTYPE)
        scores = np.zeros((nq, max(nr, 0)), dtype=np.int32)
        self._check(load().kgma_assign_ranges(self._h, genome._h, rtext, _np_ptr(roff, C.c_int64), nr, nq,
                                              _np_ptr(c, C.c_int32) if nq else None, _np_ptr(a, C.c_int64) if nq else None,
                                              _np_ptr(b, C.c_int64) if nq else None, int(gap_open), int(gap_extend), top,
                                              out.ctypes.data if out.size else None, _np_ptr(scores, C.c_int32) if scores.size else None))
        return out, scores

    def assign_stats(self) -> dict:
        """kgma_get_assign_stats: device times and counts of the last assign_seqs / assign_ranges."""
        s = KgmaAssignStats()
        self._check(load().kgma_get_assign_stats(self._h, C.byref(s)))
        return {name: getattr(s, name) for name, _ in KgmaAssignStats._fields_}

    @staticmethod
    def _ranges(contig, lo, hi):
        c = np.ascontiguousarray(np.asarray(contig, dtype=np.int32).ravel())
        a = np.ascontiguousarray(np.asarray(lo, dtype=np.int64).ravel())
        b = np.ascontiguousarray(np.asarray(hi, dtype=np.int64).ravel())
        if not (c.size == a.size == b.size):
            raise ValueError("need one lo and one hi per contig")
        n = int(c.size)
        return n, (_np_ptr(c, C.c_int32) if n else None, _np_ptr(a, C.c_int64) if n else None, _np_ptr(b, C.c_int64) if n else None), (c, a, b)

    def kmer_dist_matrix(self, seqs_a, seqs_b=None, k: int = 6):
        """kgma_kmer_dist_matrix: (D, dist), each [n_a, n_b]: D[i, j] = sum_x (c_i[x] - c_j[x])^2 over the k-mer counts of
        sequence i of `seqs_a` and sequence j of `seqs_b` (int32, exact), dist = (1 / 2k) * D = kmer_dist(a_i, b_j, k) bit for
        bit (float64).  seqs_b=None: B = A, the symmetric matrix."""
        atext, aoff = self._concat(seqs_a)
        na = aoff.size - 1
        if seqs_b is None:
            btext, boff, nb = None, None, na
        else:
            btext, boff = self._concat(seqs_b)
            nb = boff.size - 1
        D = np.zeros((na, max(nb, 0)), dtype=np.int32)
        dist = np.zeros(D.shape, dtype=np.float64)
        self._check(load().kgma_kmer_dist_matrix(self._h, int(k), atext, _np_ptr(aoff, C.c_int64), na, btext,
                                                 _np_ptr(boff, C.c_int64) if boff is not None else None, 0 if seqs_b is None else nb,
                                                 _np_ptr(D, C.c_int32) if D.size else None, _np_ptr(dist, C.c_double) if D.size else None))
        return D, dist

    def kmer_dist_matrix_ranges(self, genome: "Genome", contig, lo, hi, seqs_b, k: int = 6):
        """kgma_kmer_dist_matrix_ranges: as kmer_dist_matrix, A being residues lo[i] .. hi[i] (1-based inclusive; hi = lo - 1:
        empty) of record contig[i] (0-based) of the resident genome."""
        btext, boff = self._concat(seqs_b)
        nb = boff.size - 1
        na, ptrs, _keep = self._ranges(contig, lo, hi)
        D = np.zeros((na, max(nb, 0)), dtype=np.int32)
        dist = np.zeros(D.shape, dtype=np.float64)
        self._check(load().kgma_kmer_dist_matrix_ranges(self._h, genome._h, int(k), na, *ptrs, btext, _np_ptr(boff, C.c_int64), nb,
                                                        _np_ptr(D, C.c_int32) if D.size else None,
                                                        _np_ptr(dist, C.c_double) if D.size else None))
        return D, dist

    def kmer_nearest(self, seqs_a, seqs_b, k: int = 6, n_near: int = 1):
        """kgma_kmer_nearest: (index, D_near), each int32 [n_a, n_near]: per sequence of A its n_near nearest of B in the order
        (D ascending, index ascending).  The matrix stays on the device.  seqs_b=None: B = A."""
        atext, aoff = self._concat(seqs_a)
        na = aoff.size - 1
        if seqs_b is None:
            btext, boff, nb = None, None, 0
        else:
            btext, boff = self._concat(seqs_b)
            nb = boff.size - 1
        index = np.zeros((na, max(int(n_near), 0)), dtype=np.int32)
        Dn = np.zeros(index.shape, dtype=np.int32)
        self._check(load().kgma_kmer_nearest(self._h, int(k), atext, _np_ptr(aoff, C.c_int64), na, btext,
                                             _np_ptr(boff, C.c_int64) if boff is not None else None, nb, int(n_near),
                                             _np_ptr(index, C.c_int32) if index.size else None, _np_ptr(Dn, C.c_int32) if Dn.size else None))
        return index, Dn

    def kmer_nearest_ranges(self, genome: "Genome", contig, lo, hi, seqs_b, k: int = 6, n_near: int = 1):
        """kgma_kmer_nearest_ranges: kmer_nearest for ranges of the resident genome."""
        btext, boff = self._concat(seqs_b)
        nb = boff.size - 1
        na, ptrs, _keep = self._ranges(contig, lo, hi)
        index = np.zeros((na, max(int(n_near), 0)), dtype=np.int32)
        Dn = np.zeros(index.shape, dtype=np.int32)
        self._check(load().kgma_kmer_nearest_ranges(self._h, genome._h, int(k), na, *ptrs, btext, _np_ptr(boff, C.c_int64), nb, int(n_near),
                                                    _np_ptr(index, C.c_int32) if index.size else None,
                                                    _np_ptr(Dn, C.c_int32) if Dn.size else None))
        return index, Dn

    def kmat_stats(self) -> dict:
        """kgma_get_kmat_stats: device times, pairs, launches and kernel form of the last distance-matrix / nearest call."""
        s = KgmaKmatStats()
        self._check(load().kgma_get_kmat_stats(self._h, C.byref(s)))
        return {name: getattr(s, name) for name, _ in KgmaKmatStats._fields_}

    def genome_kmer_count(self, genome: "Genome", k: int, contig, lo, hi, flags: int = 0):
        """kgma_genome_kmer_count: (counts, skipped): counts int64 [n, 4^k], row r the k-mer counts (natural k-mer value, first
        base most significant) of residues lo[r] .. hi[r] (1-based inclusive; hi = lo - 1: empty) of record contig[r] (0-based)
        of the resident genome; skipped int64 [n]: the considered starts the flags (COUNT_SKIP_N, COUNT_SKIP_MASKED) left out.
        COUNT_BY_START: a k-mer belongs to the range it starts in."""
        n, ptrs, _keep = self._ranges(contig, lo, hi)
        k = int(k)
        served = 1 <= k <= 10 and (n << (2 * k)) <= SPECTRUM_MAX_COUNTS          # (else the call is refused: no rows needed)
        counts = np.zeros((n, 4 ** k if served else 1), dtype=np.int64)
        skipped = np.zeros(n, dtype=np.int64)
        self._check(load().kgma_genome_kmer_count(self._h, genome._h, k, int(flags), n, *ptrs,
                                                  _np_ptr(counts, C.c_int64) if n else None, _np_ptr(skipped, C.c_int64) if n else None))
        return counts, skipped

    def spectrum_stats(self) -> dict:
        """kgma_get_spectrum_stats: device time, ranges, considered starts, form, span, workgroups and launches of the last
        genome_kmer_count."""
        s = KgmaSpectrumStats()
        self._check(load().kgma_get_spectrum_stats(self._h, C.byref(s)))
        return {name: getattr(s, name) for name, _ in KgmaSpectrumStats._fields_}

    def assign_seqs_screened(self, refs, queries, gap_open: int = -69, gap_extend: int = -1, top: int = 1, screen_k: int = 6,
                             n_near: int = 8):
        """kgma_assign_seqs_screened: assign_seqs over every query's n_near nearest references by k-mer distance (screen_k) only.
        Returns (out, cand, scores): out as assign_seqs -- the best AMONG THE CANDIDATES --, cand the int32 [n_queries, n_near]
        candidate reference indices in (D, index) order, scores their int32 scores in the same order.  Unlike assign_seqs a byte
        outside A/C/G/T/N is a BadBaseError (the k-mer pass follows kmer_count)."""
        rtext, roff = self._concat(refs)
        qtext, qoff = self._concat(queries)
        nr, nq, top, nn = roff.size - 1, qoff.size - 1, int(top), int(n_near)
        out = np.zeros((nq, max(top, 0)), dtype=ASSIGNMENT_DTYPE)
        cand = np.zeros((nq, max(nn, 0)), dtype=np.int32)
        scores = np.zeros(cand.shape, dtype=np.int32)
        self._check(load().kgma_assign_seqs_screened(self._h, rtext, _np_ptr(roff, C.c_int64), nr, qtext, _np_ptr(qoff, C.c_int64), nq,
                                                     int(gap_open), int(gap_extend), top, int(screen_k), nn,
                                                     out.ctypes.data if out.size else None, _np_ptr(cand, C.c_int32) if cand.size else None,
                                                     _np_ptr(scores, C.c_int32) if scores.size else None))
        return out, cand, scores

    def assign_ranges_screened(self, genome: "Genome", refs, contig, lo, hi, gap_open: int = -69, gap_extend: int = -1, top: int = 1,
                               screen_k: int = 6, n_near: int = 8):
        """kgma_assign_ranges_screened: as assign_seqs_screened, the queries being ranges of the resident genome."""
        rtext, roff = self._concat(refs)
        nq, ptrs, _keep = self._ranges(contig, lo, hi)
        nr, top, nn = roff.size - 1, int(top), int(n_near)
        out = np.zeros((nq, max(top, 0)), dtype=ASSIGNMENT_DTYPE)
        cand = np.zeros((nq, max(nn, 0)), dtype=np.int32)
        scores = np.zeros(cand.shape, dtype=np.int32)
        self._check(load().kgma_assign_ranges_screened(self._h, genome._h, rtext, _np_ptr(roff, C.c_int64), nr, nq, *ptrs,
                                                       int(gap_open), int(gap_extend), top, int(screen_k), nn,
                                                       out.ctypes.data if out.size else None, _np_ptr(cand, C.c_int32) if cand.size else None,
                                                       _np_ptr(scores, C.c_int32) if scores.size else None))
        return out, cand, scores

    def step_hits(self, genome: "Genome", mode: int, buff: int = 50, genome_pos: int = 0, flags: int = 0) -> np.ndarray:
        """repack + scan + hits in ONE library call (kgma_repack_scan_hits); returns the hits as a structured
        array (a view of a buffer owned by this context and reused by the next call)."""
        buf = getattr(self, "_step_buf", None)
        if buf is None:
            buf = self._step_buf = np.zeros(4096, dtype=HIT_DTYPE)
            self._step_ptr = buf.ctypes.data_as(C.POINTER(KgmaHit))
            self._step_n = C.c_int64(0)
        st = load().kgma_repack_scan_hits(self._h, genome._h, mode, buff, genome_pos, flags, self._step_ptr, buf.size,
                                          C.byref(self._step_n))
        if st != 0 and self._step_n.value > buf.size:          # more hits than the buffer holds: grow and fetch
            buf = self._step_buf = np.zeros(int(self._step_n.value) * 2, dtype=HIT_DTYPE)
            self._step_ptr = buf.ctypes.data_as(C.POINTER(KgmaHit))
            st = load().kgma_get_hits(self._h, self._step_ptr, buf.size, C.byref(self._step_n))
        self._check(st)
        return buf[:self._step_n.value]

    def set_reserved_cus(self, n: int) -> None:
        """Leave `n` CUs free of scan workgroups (kgma_set_reserved_cus): for callers that run a collective beside the scan."""
        self._check(load().kgma_set_reserved_cus(self._h, int(n)))

    def step_begin(self, genome: "Genome", mode: int, buff: int = 50, genome_pos: int = 0, flags: int = 0) -> None:
        """First half of step_hits (kgma_step_begin): the step runs on the context's helper thread while the
        caller queues other work; nothing else may use the context or the genome until step_end()."""
        self._check(load().kgma_step_begin(self._h, genome._h, mode, buff, genome_pos, flags))

    def step_end(self) -> np.ndarray:
        """Second half (kgma_step_end): waits for the step and returns its hits like step_hits."""
        buf = getattr(self, "_step_buf", None)
        if buf is None:
            buf = self._step_buf = np.zeros(4096, dtype=HIT_DTYPE)
            self._step_ptr = buf.ctypes.data_as(C.POINTER(KgmaHit))
            self._step_n = C.c_int64(0)
        st = load().kgma_step_end(self._h, self._step_ptr, buf.size, C.byref(self._step_n))
        if st != 0 and self._step_n.value > buf.size:
            buf = self._step_buf = np.zeros(int(self._step_n.value) * 2, dtype=HIT_DTYPE)
            self._step_ptr = buf.ctypes.data_as(C.POINTER(KgmaHit))
            st = load().kgma_get_hits(self._h, self._step_ptr, buf.size, C.byref(self._step_n))
        self._check(st)
        return buf[:self._step_n.value]

    def stats(self) -> dict:
        s = KgmaStats()
        self._check(load().kgma_get_stats(self._h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in KgmaStats._fields_}

    def filter_stats(self) -> dict:
        """kgma_get_filter_stats: what the distance-bound prefilter did in the last scan."""
        s = KgmaFilterStats()
        self._check(load().kgma_get_filter_stats(self._h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in KgmaFilterStats._fields_}

    def pack_test_stats(self) -> dict:
        """kgma_get_pack_test_stats: whether the last step's pack made the prefilter's granule test itself, and on how many units."""
        s = KgmaPackTestStats()
        self._check(load().kgma_get_pack_test_stats(self._h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in KgmaPackTestStats._fields_}

    def get_block_sums(self, genome: "Genome", contig: int, first_block: int = 0, n: int = -1) -> np.ndarray:
        """kgma_get_block_sums: record `contig`'s block sums (one per 16 positions) of the last step whose pack computed them."""
        if n < 0:
            n = 2 * ((genome.contig_len(contig) + 31) // 32) - first_block
        out = np.zeros(max(n, 1), dtype=np.uint32)
        self._check(load().kgma_get_block_sums(self._h, genome._h, contig, first_block, n, _np_ptr(out, C.c_uint32)))
        return out[:n]

    def filter_candidates(self) -> np.ndarray:
        """kgma_get_filter_candidates: the last scan's candidate granules as an (n, 2) int64 array (record, granule), sorted."""
        n = C.c_int64(0)
        self._check(load().kgma_get_filter_candidates(self._h, None, None, 0, C.byref(n)))
        c = np.zeros(max(n.value, 1), dtype=np.int32); g = np.zeros(max(n.value, 1), dtype=np.int64)
        if n.value:
            self._check(load().kgma_get_filter_candidates(self._h, _np_ptr(c, C.c_int32), _np_ptr(g, C.c_int64), n.value, C.byref(n)))
        return np.stack([c[:n.value].astype(np.int64), g[:n.value]], axis=1) if n.value else np.zeros((0, 2), dtype=np.int64)

    @property
    def stream(self) -> int:
        return int(load().kgma_stream(self._h) or 0)

    def kernel_name(self) -> str:
        """Device kernel launched by the last scan."""
        return (load().kgma_scan_kernel_name(self._h) or b"").decode()

