"""The scan plan, pinned: one small configuration per branch of the host's decisions in kgma_scan_device (which kernel, how the
KFVs are grouped into launches, streams per CU, stream length, prefilter, deferred pack), shared by tools/record_scan_plan.py (which
records what the library does with them into tests/golden/scan_plan.json) and tests/test_gpu_scan_plan.py (which holds the library
to that record).  Results are the parity tests' business; what is recorded here is the plan's footprint: the kernel's name, the
number of launches and streams, the windows and bases scanned, the dip / hit counts and what the prefilter did.  The rows with
KGMA_F_CHAIN_REPLAY pin the host control of the Float64 chain replay the same way (chain_decide, chain_on_device): the pairs selected,
the pairs and windows chained on the device, the raw steps, the guard band, and a digest of the hit list; the chain_export rows the
stream layout kgma_chain_export hands out for one pair.

Every row scans ONE genome (a few records, 2.4 Mb, planted fixture genes, one record shorter than every window), except the row whose
point is a genome without a single window.  Each row takes its references and environment from the test that already reaches that
branch (named in the row's `like`).  A row runs in a fresh context with exactly its own environment switches set."""
import functools
import hashlib
import os
import struct

import numpy as np

from kmergma_amd import _lib, refprep
from kmergma_amd.fasta import Record
from tests.conftest import DATA
from tests.helpers import hit_key, make_genome, mutate, random_dna, sparse_family

REF_FASTA = os.path.join(DATA, "Alp_V_ref.fasta")
GENOME_SEED = 20240
GENOME_LENGTHS = [1_100_000, 800_000, 12, 400_000, 70_001, 30_000]      # (12 residues: shorter than every window, longer than k - 1)
BUFF = 50

# every switch a row may set; the runner clears all of them before it sets the row's own
SWITCHES = ("KGMA_KERNEL", "KGMA_STREAM8", "KGMA_STREAM8_DERIVE", "KGMA_STREAM8_WIDE", "KGMA_STREAM8_C16", "KGMA_TWOKERNEL", "KGMA_FILTER",
            "KGMA_FILTER_MIN_WINDOWS", "KGMA_FUSE_SUMS", "KGMA_OVERLAP", "KGMA_OVERLAP_MIN_BASES", "KGMA_STREAM_MINSLOTS", "KGMA_STREAM_ROUNDS",
            "KGMA_STREAM_ROUND_WINDOWS", "KGMA_DEBUG_SKIP", "KGMA_GENERIC_HASH", "KGMA_S8_MAXGROUP", "KGMA_CHAIN", "KGMA_CHAIN_GENERIC",
            "KGMA_CHAIN_GROUP", "KGMA_CHAIN_STREAM", "KGMA_CHAIN_POOL_UNITS", "KGMA_CHAIN_BATCH_WINDOWS", "KGMA_CHAIN_BATCH_MB", "KGMA_CHAIN_THREADS")

STATS_FIELDS = ("n_launches", "n_tiles", "n_dips", "n_hits", "n_at_threshold", "bases_scanned", "windows_scanned")
FILTER_FIELDS = ("ran", "fell_back", "reason", "regions", "streams", "windows")
CU_FIELDS = {"stats": ("n_tiles",), "filter": ("streams",)}              # compared only on a device with the recorded CU count
# the chain replay's footprint (rows with F_CHAIN_REPLAY): what chain_decide selected and where the chains ran.  The stream length of
# a chain launch follows from the CU count unless KGMA_CHAIN_STREAM is set or its floor max(1024, 4 nk) binds, so every chain row
# sets it -- but for the one row of DEFAULT_STREAM_ROW, whose chain_raw_steps joins the fields compared on the recorded CU count only
CHAIN_FIELDS = ("n_chain_pairs", "chain_windows", "chain_device_pairs", "chain_raw_steps", "chain_band_log2", "chain_rescans", "n_tie_flagged")
DEFAULT_STREAM_ROW = "k6_chain_default_stream"
# what kgma_chain_export hands out of a pair's stream layout (rows with entry "chain_export"); pool_units is recorded only where two
# recordings agreed on it
EXPORT_FIELDS = ("n_streams", "n_chunks", "win0", "n_valid", "chunk_base", "first")


def cu_fields(name, part):
    """The fields of `part` that row `name` compares only on a device with the recorded CU count."""
    return CU_FIELDS.get(part, ()) + (("chain_raw_steps",) if part == "chain" and name == DEFAULT_STREAM_ROW else ())


@functools.lru_cache(maxsize=None)
def genes():
    from kmergma_amd import fasta
    return tuple(r.sequence.upper() for r in fasta.read_fasta(REF_FASTA))


@functools.lru_cache(maxsize=None)
def genome():
    contigs, _ = make_genome(np.random.default_rng(GENOME_SEED), GENOME_LENGTHS, list(genes()), n_plants_per_mb=40.0)
    return tuple(contigs)


def short_genome():
    rng = np.random.default_rng(GENOME_SEED + 1)
    return (random_dna(rng, 100), random_dna(rng, 12), random_dna(rng, 288))


# ---- references ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fixture_single(k):
    """gen_ref_ws_cons of the fixture at k (conftest.alp_ref)."""
    RV, ws, cons, (S, N) = refprep.gen_ref_ws_cons(REF_FASTA, k, return_int=True)
    return dict(k=k, KFVs=[RV], ws=[ws], N=[N])


@functools.lru_cache(maxsize=None)
def fixture_clusters(k):
    """The fixture clustered into 5 KFVs, W = 288, 288, 288, 289, 290 (conftest.alp_clusters, workloads.fixture_clusters)."""
    from kmergma_amd import workloads
    c = workloads.fixture_clusters(DATA, k)
    return dict(k=k, KFVs=list(c["KFVs"]), ws=[int(w) for w in c["ws"]], N=list(c["N"]))


@functools.lru_cache(maxsize=None)
def families(k, lens, seed):
    """One reference family per window length, as test_stream8_derived_windows builds them (3 + i references mutated at 3 %); the
    base of family i begins with fixture gene i, which the genome holds mutated copies of."""
    rng = np.random.default_rng([seed, k, sum(lens)])
    KFVs, ws, N = [], [], []
    for i, L in enumerate(lens):
        base = (genes()[i % len(genes())] + random_dna(rng, L))[:L]
        refs = [Record(f"g{i}_{u}", mutate(rng, base, 0.03)) for u in range(3 + i)]
        RV, w, cons, (s, n) = refprep.gen_ref_ws_cons(refs, k, return_int=True)
        assert w == L
        KFVs.append(RV); ws.append(w); N.append(n)
    return dict(k=k, KFVs=KFVs, ws=ws, N=N)


def subset(ref, idx):
    return dict(k=ref["k"], KFVs=[ref["KFVs"][i] for i in idx], ws=[ref["ws"][i] for i in idx], N=[ref["N"][i] for i in idx])


def float_kfv(RV, seed):
    """test_gpu_wide._float_kfvs, "perturbed": entries moved by a relative 1e-7 ... 1e-3 -- no S / N any more."""
    rng = np.random.default_rng(seed)
    RV = np.asarray(RV, dtype=np.float64)
    return RV * (1.0 + rng.uniform(-1.0, 1.0, RV.size) * 10.0 ** rng.uniform(-7, -3, RV.size))


def _int64_prefix():
    from tests import range_cases as rc
    ref = rc.ref_of("near_copies", 6, 330, 12_000)                         # test_gpu_wide.test_prefix_beyond_int32
    return dict(k=6, KFVs=[ref["RV"]], ws=[330], N=[12_000])


def _float_single():
    r = fixture_single(6)
    return dict(k=6, KFVs=[float_kfv(r["KFVs"][0], 1)], ws=r["ws"], N=None)


def _float_mixed():
    c = fixture_clusters(6)                                                # test_gpu_wide.test_float64_kfvs_cluster: KFV 3 stays S/N
    return dict(k=6, KFVs=[c["KFVs"][j] if j == 2 else float_kfv(c["KFVs"][j], 10 + j) for j in range(5)], ws=c["ws"], N=None)


def _two_residencies():
    """Four KFVs of 288 / 289 residues (one launch) and one of 340 (a launch of its own): two residencies in one scan."""
    c, f = subset(fixture_clusters(6), (0, 1, 2, 3)), families(6, (340,), 5)
    return dict(k=6, KFVs=c["KFVs"] + f["KFVs"], ws=c["ws"] + f["ws"], N=c["N"] + f["N"])


def _sparse_k11():
    base, sp = sparse_family(np.random.default_rng(1100), 289, 11)
    return dict(k=11, sparse=True, keys=[sp["keys"]], vals=[sp["vals"]], ws=[289], N=[sp["N"]])


def _strobe():
    cfg = (2, 3, 5, 5)                                                     # tests/test_gpu_strobe.py: CONFIGS[0]
    RV, W, cons, (S, N) = refprep.gen_ref_ws_cons_strobe(REF_FASTA, *cfg, return_int=True)
    return dict(strobe=cfg, RV=RV, W=W, N=N)


S, O = _lib.MODE_SINGLE, _lib.MODE_OMN
SMALL, OVL = {"KGMA_FILTER": "1", "KGMA_FILTER_MIN_WINDOWS": "1"}, {"KGMA_OVERLAP_MIN_BASES": "1000000"}
CL5_THR = [37.0, 33.0, 38.0, 34.0, 28.0]

# name -> dict(ref: a function returning the references, mode, thr, flags, env, entry: "scan" | "step" | "strobe" | "chain_export",
#              genome, like; buff: where BUFF does not serve; chain replay rows: min_pairs (1), device_pairs (all of them);
#              chain_export rows: last_window)
CASES = {
    "k6_one_kfv_stream8": dict(ref=lambda: fixture_single(6), mode=S, thr=[30.0], like="test_gpu_parity::test_both_kernels_single"),
    "k6_one_kfv_bitslice": dict(ref=lambda: fixture_single(6), mode=S, thr=[30.0], env={"KGMA_KERNEL": "bitslice"},
                                like="test_gpu_parity::test_both_kernels_single"),
    "k6_one_kfv_stream16": dict(ref=lambda: fixture_single(6), mode=S, thr=[30.0], env={"KGMA_STREAM8": "0"},
                                like="test_gpu_parity::test_stream_kernel_16bit_counters_single"),
    "k6_515_kmers_c16": dict(ref=lambda: families(6, (520,), 1), mode=S, thr=[25.0], like="test_gpu_parity::test_large_windows"),
    "k6_prefix_beyond_int32": dict(ref=_int64_prefix, mode=S, thr=[20.0], like="test_gpu_wide::test_prefix_beyond_int32"),
    "k6_derive_288_288_289": dict(ref=lambda: subset(fixture_clusters(6), (1, 2, 3)), mode=O, thr=CL5_THR[1:4],
                                  like="test_gpu_parity::test_stream8_derived_windows"),
    "k6_derive_off": dict(ref=lambda: subset(fixture_clusters(6), (1, 2, 3)), mode=O, thr=CL5_THR[1:4], env={"KGMA_STREAM8_DERIVE": "0"},
                          like="test_gpu_parity::test_stream8_derived_windows"),
    "k6_five_kfvs_wide": dict(ref=lambda: fixture_clusters(6), mode=O, thr=CL5_THR, like="test_gpu_parity::test_stream8_five_kfv_launch"),
    "k6_five_kfvs_wide_off": dict(ref=lambda: fixture_clusters(6), mode=O, thr=CL5_THR, env={"KGMA_STREAM8_WIDE": "0"},
                                  like="test_gpu_parity::test_stream8_five_kfv_launch"),
    "k7_eight_kfvs": dict(ref=lambda: families(7, (288, 288, 288, 288, 289, 289, 289, 290), 2), mode=O, thr=[22.0] * 8,
                          like="test_gpu_parity::test_stream8_five_kfv_launch"),
    "k7_bitslice_two_kernels": dict(ref=lambda: fixture_clusters(7), mode=O, thr=CL5_THR, env={"KGMA_KERNEL": "bitslice", "KGMA_TWOKERNEL": "1"},
                                    like="test_gpu_parity::test_two_kernel_cluster_path"),
    "k7_bitslice_one_kernel": dict(ref=lambda: fixture_clusters(7), mode=O, thr=CL5_THR, env={"KGMA_KERNEL": "bitslice", "KGMA_TWOKERNEL": "0"},
                                   like="test_gpu_parity::test_two_kernel_cluster_path"),
    "k6_two_residencies": dict(ref=_two_residencies, mode=O, thr=CL5_THR[:4] + [25.0], like="BASELINE configs[3]: the natural-slots search"),
    "k6_two_residencies_minslots": dict(ref=_two_residencies, mode=O, thr=CL5_THR[:4] + [25.0], env={"KGMA_STREAM_MINSLOTS": "1"},
                                        like="BASELINE configs[3]: the natural-slots search"),
    "k4_generic": dict(ref=lambda: fixture_single(4), mode=S, thr=[120.0], like="test_gpu_parity::test_other_k_values"),
    "k8_default": dict(ref=lambda: fixture_single(8), mode=S, thr=[22.0], like="test_gpu_parity::test_other_k_values"),
    "k8_generic_hash": dict(ref=lambda: fixture_single(8), mode=S, thr=[22.0], env={"KGMA_KERNEL": "generic"},
                            like="test_gpu_wide::test_generic_kernel_hash_counts"),
    "k8_generic_global_counts": dict(ref=lambda: fixture_single(8), mode=S, thr=[22.0], env={"KGMA_KERNEL": "generic", "KGMA_GENERIC_HASH": "0"},
                                     like="test_gpu_wide::test_generic_kernel_hash_counts"),
    "k11_sparse": dict(ref=_sparse_k11, mode=S, thr=[15.0], like="test_gpu_large_k::test_single_engine_large_k"),
    "k6_float64": dict(ref=_float_single, mode=S, thr=[30.0], like="test_gpu_wide::test_float64_kfv_single"),
    "k6_float64_and_sn": dict(ref=_float_mixed, mode=O, thr=CL5_THR, like="test_gpu_wide::test_float64_kfvs_cluster"),
    "k6_2595_kmers": dict(ref=lambda: families(6, (2600,), 3), mode=S, thr=[25.0], like="test_gpu_wide::test_wide_windows_stream8"),
    "k4_2997_kmers": dict(ref=lambda: families(4, (3000,), 4), mode=S, thr=[60.0], like="test_gpu_wide::test_wide_windows_generic_kernel"),
    "strobemers": dict(ref=_strobe, mode=_lib.MODE_STROBE, thr=[30.0], entry="strobe", like="test_gpu_strobe::test_exact_parity"),
    "k6_filter_runs": dict(ref=lambda: fixture_single(6), mode=S, thr=[30.0], env=SMALL, like="test_gpu_filter::test_filter_on_off_and_candidates"),
    "k6_filter_off": dict(ref=lambda: fixture_single(6), mode=S, thr=[30.0], env={"KGMA_FILTER": "0", "KGMA_FILTER_MIN_WINDOWS": "1"},
                          like="test_gpu_filter::test_filter_on_off_and_candidates"),
    "k6_step": dict(ref=lambda: fixture_single(6), mode=S, thr=[30.0], entry="step", like="test_gpu_parity::test_overlapped_step_equals_sequential_step"),
    "k6_step_pack_carries_sums": dict(ref=lambda: fixture_single(6), mode=S, thr=[30.0], entry="step", env=SMALL, like="tests/test_gpu_fused_sums.py"),
    "k6_step_sequential": dict(ref=lambda: fixture_single(6), mode=S, thr=[30.0], entry="step", env=dict(OVL, KGMA_OVERLAP="0"),
                               like="test_gpu_parity::test_overlapped_step_equals_sequential_step"),
    "k6_step_overlapped": dict(ref=lambda: fixture_single(6), mode=S, thr=[30.0], entry="step", env=dict(OVL, KGMA_OVERLAP="1"),
                               like="test_gpu_parity::test_overlapped_step_equals_sequential_step"),
    "k6_return_dists": dict(ref=lambda: fixture_single(6), mode=S, thr=[30.0], flags=_lib.F_RETURN_DISTS, like="test_gpu_parity::test_golden_single_dists"),
    "k6_omn_return_dists": dict(ref=lambda: fixture_clusters(6), mode=O, thr=CL5_THR, flags=_lib.F_RETURN_DISTS | _lib.F_NO_TIE_RESOLVE,
                                like="test_gpu_parity::test_random_genomes_omn"),
    "k6_no_window_at_all": dict(ref=lambda: fixture_single(6), mode=S, thr=[30.0], genome="short", like="test_gpu_parity::test_empty_and_tiny_inputs"),
}

# ---- the chain replay (kgma_api.cpp: chain_decide, chain_on_device): thresholds near the random-sequence distance, so that pairs
#      are selected (the recorder refuses a replay row that selects none) ----------------------------------------------------------
CH, ST = _lib.F_CHAIN_REPLAY, {"KGMA_CHAIN_STREAM": "1024"}
K7_THR = [36.0, 32.0, 39.5, 30.0, 40.5]                                   # (random windows: 37.4, 33.5, 41.0, 31.0, 42.0)


def _chain_single(env, like="test_gpu_chain::test_chain_replay_in_small_batches", **kw):
    return dict(ref=lambda: fixture_single(6), mode=S, thr=[37.0], flags=CH, env=env, like=like, **kw)


def _chain_clusters(ref, thr, env, like="test_gpu_chain::test_chain_replay_with_grouped_launches"):
    return dict(ref=ref, mode=O, thr=thr, flags=CH, buff=100, env=env, min_pairs=3, like=like)


CASES.update({
    "k6_chain": _chain_single(ST),
    "k6_chain_three_batches": _chain_single(dict(ST, KGMA_CHAIN_BATCH_WINDOWS="100000")),     # alternating buffer sets, the worker
    "k6_chain_pool_regrowth": _chain_single(dict(ST, KGMA_CHAIN_POOL_UNITS="100"), like="test_gpu_chain::test_chain_values_raw_pool_regrowth"),
    "k6_chain_on_the_host": _chain_single(dict(ST, KGMA_CHAIN="host"), device_pairs=0,
                                          like="test_gpu_chain::test_chain_replay_runs_on_the_device_and_agrees_with_the_host_chain"),
    "k6_chain_generic_kernel": _chain_single(dict(ST, KGMA_CHAIN_GENERIC="1"), like="test_gpu_chain::test_generic_chain_kernel_every_window"),
    DEFAULT_STREAM_ROW: _chain_single({}),
    "k6_chain_clusters": _chain_clusters(lambda: fixture_clusters(6), CL5_THR, ST),
    "k6_chain_clusters_group4": _chain_clusters(lambda: fixture_clusters(6), CL5_THR, dict(ST, KGMA_CHAIN_GROUP="4")),
    "k6_chain_float64_and_sn": _chain_clusters(_float_mixed, CL5_THR, ST, like="test_gpu_wide::test_float64_kfvs_cluster"),   # both passes
    "k7_chain_clusters": _chain_clusters(lambda: fixture_clusters(7), K7_THR, ST, like="test_gpu_chain::test_chain_values_cluster_kfvs_and_other_k"),
    "k8_chain": dict(ref=lambda: fixture_single(8), mode=S, thr=[25.6], flags=CH, env=ST, like="test_gpu_chain::test_generic_chain_kernel_every_window"),
    "k11_sparse_chain": dict(ref=_sparse_k11, mode=S, thr=[20.7], flags=CH, env=ST, like="test_gpu_large_k::test_single_engine_large_k"),
})

# ---- kgma_chain_export on the 70 001-residue record: a pair's stream layout.  At 284 k-mers per window the default stream length is
#      its floor, 4 x 284 rounded up to 64 = 1152, whatever the device; last_window = 2, T + 1, T + 2: one stream at its shortest, one
#      that is exactly full, a second stream of two windows ------------------------------------------------------------------------
EXPORT_RECORD = 4


def _export(ref, last, env, like="test_gpu_sharded: parallel.scan_sharded's chain source"):
    """(last = None: the record's last window)"""
    return dict(ref=ref, mode=S, thr=[30.0], entry="chain_export", last_window=last, env=env, like=like)


for _T, _env in ((1152, {}), (4096, {"KGMA_CHAIN_STREAM": "4096"})):
    for _last in (2, _T + 1, _T + 2):
        CASES[f"k6_export_T{_T}_last{_last}"] = _export(lambda: fixture_single(6), _last, _env)
CASES.update({
    "k6_export_c16": _export(lambda: families(6, (520,), 1), None, {"KGMA_CHAIN_STREAM": "4096"}),
    "k7_export": _export(lambda: fixture_single(7), None, {"KGMA_CHAIN_STREAM": "4096"}),
    "k6_export_generic_kernel": _export(lambda: fixture_single(6), None, {"KGMA_CHAIN_STREAM": "4096", "KGMA_CHAIN_GENERIC": "1"}),
})


def hits_digest(hits):
    """SHA-256 over the hit list: hit_key, the bit pattern of dist, flags."""
    h = hashlib.sha256()
    for x in hits:
        h.update(struct.pack("<6qdQ", *(int(v) for v in hit_key(x)), float(x["dist"]), int(x["flags"])))
    return h.hexdigest()


def run_case(name):
    """Run one row in a fresh context under its own environment; returns dict(kernel, stats, filter), for a chain replay row also
    chain and hits_sha256; for a chain_export row dict(export) alone."""
    case = CASES[name]
    saved = {s: os.environ.pop(s, None) for s in SWITCHES}
    os.environ.update(case.get("env", {}))
    ctx = _lib.Context(0)
    try:
        ref, thr, flags, buff = case["ref"](), case["thr"], case.get("flags", 0), case.get("buff", BUFF)
        if "strobe" in ref:
            ctx.set_strobe_ref(*ref["strobe"], ref["RV"], ref["W"], thr[0], ref["N"])
        elif ref.get("sparse"):
            ctx.set_refs_sparse(ref["k"], ref["keys"], ref["vals"], ref["ws"], thr, ref["N"])
        else:
            ctx.set_refs(ref["k"], ref["KFVs"], ref["ws"], thr, ref["N"])
        contigs = list(short_genome() if case.get("genome") == "short" else genome())
        g = ctx.genome_from_host(contigs)
        try:
            entry = case.get("entry", "scan")
            if entry == "chain_export":
                last = case["last_window"] or len(contigs[EXPORT_RECORD]) - ref["ws"][0] + 1
                ex = ctx.chain_export(g, EXPORT_RECORD, 1, last, [(1, 1), (last, last)])
                out = dict(n_streams=len(ex["win0"]), n_chunks=len(ex["chunks"]), pool_units=len(ex["pool"]),
                           first=struct.pack("<d", ex["first"]).hex())
                out.update({f: [int(v) for v in ex[f]] for f in ("win0", "n_valid", "chunk_base")})
                return dict(export=out)
            if entry == "strobe":
                ctx.strobe_scan(g, buff, flags)
            elif entry == "step":
                ctx.step_hits(g, case["mode"], buff, 0, flags)
            else:
                ctx.scan(g, case["mode"], buff, 0, flags, None)
            st, fs = ctx.stats(), ctx.filter_stats()
            out = dict(kernel=ctx.kernel_name(), stats={f: int(st[f]) for f in STATS_FIELDS}, filter={f: int(fs[f]) for f in FILTER_FIELDS})
            if flags & _lib.F_CHAIN_REPLAY:
                out["chain"] = {f: int(st[f]) for f in CHAIN_FIELDS}
                out["hits_sha256"] = hits_digest(ctx.hits())
            return out
        finally:
            g.free()
    finally:
        ctx.close()
        for s in SWITCHES:
            os.environ.pop(s, None)
            if saved[s] is not None:
                os.environ[s] = saved[s]


def chain_row_error(name, got):
    """A replay row that selects no pair pins nothing: what is wrong with the record `got` of row `name`, or None."""
    case = CASES[name]
    if "chain" not in got:
        return None
    ch, least = got["chain"], case.get("min_pairs", 1)
    if ch["n_chain_pairs"] < least:
        return f"{ch['n_chain_pairs']} chain pairs selected, at least {least} wanted: move the row's threshold"
    want = case.get("device_pairs", ch["n_chain_pairs"])
    if ch["chain_device_pairs"] != want:
        return f"{ch['chain_device_pairs']} pairs chained on the device, {want} wanted"
    return None
