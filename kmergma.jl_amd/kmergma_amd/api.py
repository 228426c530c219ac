"""Host-side mirror of the reference's operator interface for the scan path.

Same names, keyword arguments, mutation-of-caller-vectors behaviour and error behaviour as

    ac_gma_testing!        src/GenomeMiner.jl:4-109
    Omn_KmerGMA!           src/OmnGenomeMiner.jl:7-162
    record_KmerGMA!        src/MultiThread/GenomeMiner.jl:8-98
    findGenes              src/API.jl:60-104
    findGenes_cluster_mode src/API.jl:161-226
    write_results          src/API.jl:234-241
    StrobeGMA!             src/StrobemerGMA/StrobeGenomeMiner.jl:5-95
    Strobemer_findGenes    src/StrobemerGMA/StrobeGenomeMiner.jl:119-158
    exactMatch             src/ExactMatch.jl:89-121
    fasta_id_to_cumulative_len_dict  src/ExactMatch.jl:146-158
    HumanRSSV, HumanRSSD, RSS_dist   src/RSS.jl:11-28 (and motifMatch / findRSS: the search that file is after)

but the per-record scan runs on the MI355X through libkgma's C ABI (include/kgma.h).  The host
keeps what the reference keeps on the host: FASTA parsing, reference preparation, optional
re-alignment of hits and FASTA-record construction.  There is no CPU scan path in this package.

Differences a caller can observe (all documented in DESIGN.md):
  * a `refVec` that is an average of integer histograms (KFV = S/N: what gen_ref_ws_cons / cluster_ref_API produce) is
    scanned in exact integers: pass `n_refs=N` (the number of reference sequences) or let the library infer it.  Any
    other Float64 vector is scanned in Float64 (kgma.h, kgma_set_refs).
  * with KmerDistThr = 0 the threshold estimate uses numpy's RNG, not Julia's (explicit
    thresholds reproduce the reference bit for bit).
  * `do_align=True` needs an `aligner` callable (see `kmergma_amd.align`); the default is the
    package's restatement of BioAlignments' semi-global affine alignment.
  * `strand=` (no counterpart in the reference, which reads every record left to right only): "+" (default) is the
    reference's scan; "-" scans the reverse complement of every record, made on the device from the resident text
    (kgma_genome_revcomp), and reports the hits in FORWARD coordinates with ` | Strand = -` in the header and the gene in
    reference orientation as the body; "both" returns the plus results followed by the minus results (`strand_range`).
"""
from __future__ import annotations

import logging
import math
from typing import Callable, List, NamedTuple, Optional, Sequence

import numpy as np

from . import _lib, headers, refprep
from .fasta import Record, read_fasta, reverse_complement, write_fasta
from .twobit import twobit_names_and_lengths

log = logging.getLogger("KmerGMA")

_CTX = {}


def default_context(device: int = 0) -> "_lib.Context":
    """One lazily created libkgma context per device (raises if no MI355X / library)."""
    if device not in _CTX:
        _CTX[device] = _lib.Context(device)
    return _CTX[device]


class _GenomeView:
    """The records of a scan input: FASTA path -> parsed and packed on the device
    (kgma_genome_from_fasta, replaces FASTX + getSeq at src/GenomeMiner.jl:31-35); .2bit path (told by the file's first four
    bytes) -> unpacked on the device (kgma_genome_from_2bit_file), the record names are the descriptions; an open device
    genome (_lib.Genome) -> used as it is and NOT owned: free() leaves it open, so one resident genome serves many calls;
    list of Record -> uploaded from host memory.  Sequences of hits are read back on demand."""

    def __init__(self, ctx, genome_path):
        self._owned = True
        if isinstance(genome_path, _lib.Genome):
            self.genome = genome_path
            self._owned = False
            try:
                self.descriptions = [self.genome.header(c) for c in range(self.genome.n_contigs)]
            except _lib.KgmaError:                 # (a genome made from host records or synthetically carries no names)
                self.descriptions = [""] * self.genome.n_contigs
            self._recs = None
        elif isinstance(genome_path, str):
            self.genome = ctx.genome_from_path(genome_path)
            self.descriptions = [self.genome.header(c) for c in range(self.genome.n_contigs)]
            self._recs = None
        else:
            self._recs = list(genome_path)
            self.genome = ctx.genome_from_host([r.sequence for r in self._recs])
            self.descriptions = [r.description for r in self._recs]

    def identifier(self, c: int) -> str:
        parts = self.descriptions[c].split(None, 1)
        return parts[0] if parts else ""

    def subseq(self, c: int, lo: int, hi: int) -> bytes:
        """view(seq, lo:hi), 1-based inclusive."""
        if hi < lo:
            return b""
        if self._recs is not None:
            return self._recs[c].sequence[lo - 1:hi]
        return self.genome.fetch(c, lo, hi - lo + 1)

    def subseqs(self, ranges) -> list:
        """view(seq, lo:hi) for (record, lo, hi) triples: the bodies of all hit records of a scan in ONE device
        gather (kgma_genome_fetch_batch) instead of one download per hit."""
        ranges = list(ranges)
        if self._recs is not None:
            return [self._recs[c].sequence[lo - 1:hi] if hi >= lo else b"" for c, lo, hi in ranges]
        return self.genome.fetch_batch([(c, lo, max(hi - lo + 1, 0)) for c, lo, hi in ranges])

    def reversed(self) -> "_GenomeView":
        """The same records reverse-complemented ON THE DEVICE (kgma_genome_revcomp): same headers, same lengths.  Its
        subsequences -- bodies of minus-strand hits, segments for an aligner -- always come from the reversed device genome,
        also when this view was built from host records.  The caller frees it."""
        v = object.__new__(_GenomeView)
        v.genome = self.genome.revcomp()
        v.descriptions = self.descriptions
        v._recs = None
        v._owned = True
        return v

    def free(self):
        if self._owned:
            self.genome.free()


STRANDS = ("+", "-", "both")


def _check_strand(strand) -> None:
    if strand not in STRANDS:
        raise ValueError(f"strand must be one of '+', '-', 'both', not {strand!r}")


def strand_range(L: int, lo: int, hi: int):
    """lo:hi (1-based, inclusive) of a record of length L in the coordinates of its reverse complement: position p is
    L - p + 1 there, so the range is (L - hi + 1):(L - lo + 1).  The map is its own inverse."""
    return L - hi + 1, L - lo + 1


def _for_strands(view: _GenomeView, strand: str, run) -> None:
    """run(view, "+") and / or run(reversed view, "-").  With "both" the reversed genome is made after the forward scan's
    results have been taken, and freed before returning: two genomes on the device at the peak."""
    if strand != "-":
        run(view, "+")
    if strand != "+":
        rc = view.reversed()
        try:
            run(rc, "-")
        finally:
            rc.free()


def _emit_hits(view, strand, hits, header_of, resultVec, hit_loci_vec) -> None:
    """The FASTA records of a scan's hits.  Minus strand: `view` is the reversed genome and the hits are in its coordinates;
    the body is the reversed genome's lo:hi (the gene in reference orientation), header and locus use the forward range."""
    bodies = view.subseqs((h["contig"], h["lo"], h["hi"]) for h in hits)
    for h, body in zip(hits, bodies):
        lo, hi = h["lo"], h["hi"]
        if strand == "-":
            lo, hi = strand_range(view.genome.contig_len(h["contig"]), lo, hi)
        resultVec.append(Record(header_of(h, lo, hi), body))
        if hit_loci_vec is not None:
            hit_loci_vec.append(lo + h["genome_pos"])


def _emit_aligns(view, strand, aligns, out) -> None:
    """Alignment tuples (contig, kfv, lo, hi, first, last): lo:hi in forward coordinates; first / last stay relative to the
    aligned segment, which is gene-oriented on either strand."""
    for c, kfv, lo, hi, first, last in aligns:
        if strand == "-":
            lo, hi = strand_range(view.genome.contig_len(c), lo, hi)
        out.append((c, kfv, lo, hi, first, last))


def _check_derived(k: int, mask, ScaleFactor) -> None:
    # the engines take `mask` and `ScaleFactor` explicitly (GenomeMiner.jl:13-15); API.jl always
    # passes 4^k-1 and 1/k (API.jl:86,204).  The device derives both from k.
    if mask is not None and int(mask) != 4 ** k - 1:
        raise ValueError(f"mask = {mask} is not 4^k - 1 for k = {k}")
    if ScaleFactor is not None and abs(float(ScaleFactor) - 1.0 / k) > 1e-12:
        raise ValueError(f"ScaleFactor = {ScaleFactor} is not 1/k for k = {k}")


def _make_align_cb(aligner, view, consensus_of, windowsize_of, gap_open, gap_extend, store):
    """Adapts `aligner(consensus, segment, gap_open, gap_extend) -> (first, last)` (the role of
    pairalign + cigar_to_UnitRange, Alignment.jl:13-52) to the library's range callback."""

    def cb(contig, kfv, lo, hi, L):
        cons = consensus_of(kfv)
        ws = windowsize_of(kfv)
        a_first, a_last = aligner(cons[:ws] if ws is not None else cons, view.subseq(contig, lo, hi), gap_open, gap_extend)
        if store is not None:
            store.append((contig, kfv, lo, hi, a_first, a_last))
        return max(1, lo + a_first - 1), min(lo + a_last - 1, L)

    return cb


def ac_gma_testing(*, genome_path, refVec, consensus_refseq: bytes = b"", k: int = 6, windowsize: int = 289,
                   thr: float = 33.5, buff: int = 50, mask=None, Nt_bits=None, ScaleFactor=None,
                   do_align: bool = True, result_align_vec: Optional[list] = None, gap_open_score: int = -69,
                   gap_extend_score: int = -1, do_return_dists: bool = False, dist_vec: Optional[list] = None,
                   do_return_align: bool = False, get_hit_loci: bool = False,
                   hit_loci_vec: Optional[list] = None, resultVec: Optional[list] = None,
                   n_refs: Optional[int] = None, aligner: Optional[Callable] = None,
                   with_genome_pos: bool = True, ctx: Optional["_lib.Context"] = None, float_chain: bool = True,
                   strand: str = "+") -> None:
    """`ac_gma_testing!` (src/GenomeMiner.jl:4-109): mutates resultVec / hit_loci_vec / dist_vec.
    float_chain (default on): KGMA_F_CHAIN_REPLAY -- every decision that hangs on the rounding of the reference's
    running Float64 distance is taken from a host replay of that value (kgma.h).
    strand: "+" (default) is the reference's scan.  "-" is the same scan over the reverse complement of every record (same
    headers, same order; made on the device), each hit then rewritten to forward coordinates: lo:hi ->
    (L - hi + 1):(L - lo + 1), header from that range with ` | Strand = -` appended, locus = forward lo + GenomePos, body =
    the gene in reference orientation (the reverse complement of the forward range); alignment tuples get the same range
    map, their first / last stay relative to the gene-oriented segment.  "both": the plus results, then the minus results
    in the order the engine emitted them (distances: the plus vector, then the minus vector).  Hits are NOT de-duplicated
    between the strands: a palindromic region may be reported twice."""
    _check_strand(strand)
    _check_derived(k, mask, ScaleFactor)
    resultVec = resultVec if resultVec is not None else []
    ctx = ctx or default_context()
    ctx.set_refs(k, [np.asarray(refVec, dtype=np.float64)], [int(windowsize)], [float(thr)],
                 None if n_refs is None else [int(n_refs)])
    view = _GenomeView(ctx, genome_path)
    device_align = do_align and aligner is None and int(windowsize) + 2 * int(buff) <= 8191
    if do_align and not device_align and aligner is None:
        from .align import align_range as aligner  # noqa: N813
    flags = (_lib.F_RETURN_DISTS if do_return_dists else 0) | (_lib.F_CHAIN_REPLAY if float_chain else 0)

    def run(v, sd):
        aligns: list = []
        if device_align:
            # the single engine's alignment does not feed back into the hit state machine
            # (GenomeMiner.jl:96-99): all hits of the scan are re-aligned in one device batch
            ctx.scan_aligned(v.genome, _lib.MODE_SINGLE, int(buff), 0, flags, [consensus_refseq], gap_open_score, gap_extend_score)
            if do_return_align:
                aligns.extend((a["contig"], 0, a["lo"], a["hi"], a["first"], a["last"]) for a in ctx.alignments()[0])
        else:
            cb = None
            if do_align:
                cb = _make_align_cb(aligner, v, lambda kfv: consensus_refseq, lambda kfv: int(windowsize),
                                    gap_open_score, gap_extend_score, aligns if do_return_align else None)
            ctx.scan(v.genome, _lib.MODE_SINGLE, int(buff), 0, flags, cb)
        if result_align_vec is not None:
            _emit_aligns(v, sd, aligns, result_align_vec)
        _emit_hits(v, sd, ctx.hits(),
                   lambda h, lo, hi: headers.single_header(v.identifier(h["contig"]), h["dist"], lo, hi, h["genome_pos"],
                                                           with_genome_pos, strand=sd),
                   resultVec, hit_loci_vec if get_hit_loci else None)
        if do_return_dists and dist_vec is not None:
            dist_vec.extend(ctx.dists(1).tolist())

    try:
        _for_strands(view, strand, run)
    finally:
        view.free()


def record_KmerGMA(*, record: Record, refVec, consensus_refseq: bytes = b"", resultVec_vec: List[list],
                   k: int = 6, windowsize: int = 289, thr: float = 30, buff: int = 50, do_align: bool = True,
                   gap_open_score: int = -69, gap_extend_score: int = -1, n_refs: Optional[int] = None,
                   aligner: Optional[Callable] = None, ctx=None, strand: str = "+") -> None:
    """`record_KmerGMA!` (src/MultiThread/GenomeMiner.jl:8-98): one record, header without GenomePos.
    strand: as ac_gma_testing."""
    ac_gma_testing(genome_path=[record], refVec=refVec, consensus_refseq=consensus_refseq, k=k,
                   windowsize=windowsize, thr=thr, buff=buff, do_align=do_align, gap_open_score=gap_open_score,
                   gap_extend_score=gap_extend_score, resultVec=resultVec_vec[0], n_refs=n_refs, aligner=aligner,
                   with_genome_pos=False, ctx=ctx, strand=strand)


def Omn_KmerGMA(*, genome_path, refVecs: Sequence, windowsizes: Sequence[int], consensus_seqs: Sequence[bytes] = (),
                resultVec: list, k: int = 6, ScaleFactor=None, mask=None,
                thr_vec: Sequence[float] = (35, 31, 38, 34, 27, 27), buff: int = 50, Nt_bits=None,
                align_hits: bool = True, align_vec: Optional[list] = None, gap_open_score: int = -200,
                gap_extend_score: int = -1, genome_pos: int = 0, get_hit_loci: bool = False,
                hit_loci_vec: Optional[list] = None, get_aligns: bool = False, do_return_dists: bool = False,
                dist_vec_vec: Optional[List[list]] = None, n_refs: Optional[Sequence[int]] = None,
                aligner: Optional[Callable] = None, ctx=None, float_chain: bool = True, strand: str = "+") -> None:
    """`Omn_KmerGMA!` (src/OmnGenomeMiner.jl:7-162).  Without a caller-supplied `aligner` the hits are re-aligned on the
    device: every dip's candidate range in one batch per KFV, looked up by the hit state machine (kgma_scan_aligned).
    strand: "+", "-" or "both", as ac_gma_testing (with "both" every KFV's distances are its plus vector followed by its
    minus vector; hits are not de-duplicated between the strands)."""
    _check_strand(strand)
    _check_derived(k, mask, ScaleFactor)
    m = len(windowsizes)
    ctx = ctx or default_context()
    ctx.set_refs(k, [np.asarray(r, dtype=np.float64) for r in refVecs], [int(w) for w in windowsizes],
                 [float(t) for t in list(thr_vec)[:m]], None if n_refs is None else [int(n) for n in n_refs])
    view = _GenomeView(ctx, genome_path)
    flags = (_lib.F_RETURN_DISTS if do_return_dists else 0) | (_lib.F_CHAIN_REPLAY if float_chain else 0)
    device_align = (align_hits and aligner is None and len(consensus_seqs) >= m
                    and max(int(w) for w in windowsizes) + 2 * int(buff) <= 8191)
    if align_hits and not device_align and aligner is None:
        from .align import align_range as aligner  # noqa: N813

    def run(v, sd):
        aligns: list = []
        if device_align:
            # the cluster engine aligns against the whole consensus_seqs[ind] (OmnGenomeMiner.jl:131)
            ctx.scan_aligned(v.genome, _lib.MODE_OMN, int(buff), int(genome_pos), flags, list(consensus_seqs)[:m],
                             gap_open_score, gap_extend_score)
            if get_aligns:
                aligns.extend((a["contig"], a["kfv"], a["lo"], a["hi"], a["first"], a["last"]) for a in ctx.alignments()[0])
        else:
            cb = None
            if align_hits:
                cb = _make_align_cb(aligner, v, lambda kfv: consensus_seqs[kfv - 1], lambda kfv: None,
                                    gap_open_score, gap_extend_score, aligns if get_aligns else None)
            ctx.scan(v.genome, _lib.MODE_OMN, int(buff), int(genome_pos), flags, cb)
        if align_vec is not None:
            _emit_aligns(v, sd, aligns, align_vec)
        _emit_hits(v, sd, ctx.hits(),
                   lambda h, lo, hi: headers.omn_header(v.identifier(h["contig"]), h["dist"], h["kfv"], lo, hi, h["genome_pos"],
                                                        strand=sd),
                   resultVec, hit_loci_vec if get_hit_loci else None)
        if do_return_dists and dist_vec_vec is not None:
            for j in range(m):
                dist_vec_vec[j].extend(ctx.dists(j + 1).tolist())

    try:
        _for_strands(view, strand, run)
    finally:
        view.free()


def _prep_ctx(ctx, k: int):
    """The context for reference preparation: the device refprep entry points serve 1 <= k <= 10; beyond, the host restatement
    (ctx=None) prepares the references and the scan still runs on `ctx`."""
    return ctx if k <= 10 else None


def warn_helper(k: int, do_return_dists: bool) -> None:
    """src/API.jl:8-11 (exact strings are part of the reference's tested contract)."""
    if k < 5:
        log.warning(f"Such a low k value of {k} likely won't yield the most accurate results")
    if do_return_dists:
        log.warning("Setting do_return_dists to true may be very memory intensive")


def _julia_num(x) -> str:
    return headers.julia_float_str(float(x)) if isinstance(x, float) else str(x)


def findGenes(*, genome_path: str, ref_path: str, k: int = 6, KmerDistThr=0, buffer: int = 50,
              do_align: bool = True, gap_open_score: int = -69, gap_extend_score: int = -1,
              do_return_dists: bool = False, do_return_hit_loci: bool = False, do_return_align: bool = False,
              verbose: bool = True, KmerDist_threshold_buffer: float = 8.0, aligner: Optional[Callable] = None,
              ctx=None, strand: str = "+") -> list:
    """`findGenes` (src/API.jl:60-104). Returns [hits, (loci), (aligns), (dists)].

    genome_path: a FASTA path, a UCSC .2bit path (told by the file's first four bytes, not its name), or a device genome
    that is already open (ctx.genome_from_path / genome_from_2bit / genome_from_fasta): it is scanned where it lies and stays
    open, so several gene families are searched on one resident genome without paying the ingest again.  The same holds for
    findGenes_cluster_mode and Strobemer_findGenes.

    strand: "+" (default: the reference's scan), "-" (genes on the reverse strand, reported in forward coordinates with
    ` | Strand = -` in the header and the gene in reference orientation as the body) or "both" (the plus results followed by
    the minus results; not de-duplicated, a palindromic region may be reported twice): see ac_gma_testing.

    Every 1 <= k <= 15 is served.  Reference preparation runs its k-mer counting and kmer_dist batches on the device for
    k <= 10; for k >= 11 it uses the host restatement in refprep (the device refprep entry points stop at k = 10), and the scan
    itself runs on the device at every k."""
    _check_strand(strand)
    if verbose:
        log.info("pre-processing references and parameters...")
    warn_helper(k, do_return_dists)
    ctx = ctx if ctx is not None else default_context()
    prep_ctx = _prep_ctx(ctx, k)
    # reference preparation: the k-mer counting and kmer_dist batches run on the device
    RV, windowsize, consensus_refseq, (_S, N) = refprep.gen_ref_ws_cons(ref_path, k, return_int=True, ctx=prep_ctx)
    if k >= windowsize:
        raise ValueError(f"the average reference sequence length {windowsize} exceeds/is equal to the chosen "
                         f"kmer length {k}. please reduce k. ")
    est = refprep.estimate_optimal_threshold(RV, windowsize, buffer=KmerDist_threshold_buffer, ctx=prep_ctx)
    if KmerDistThr == 0:
        KmerDistThr = est
    elif KmerDistThr < est:   # (sic) API.jl:75-76
        log.warning(f"The kmer distance threshold {_julia_num(KmerDistThr)} for k = {k} is likely too high, "
                    "and can result in many false positives")
    hit_vector: list = []
    dist_vec: list = []
    hit_loci_vec: list = []
    alignment_vec: list = []
    if verbose:
        log.info("initializing iteration...")
    ac_gma_testing(genome_path=genome_path, refVec=RV, consensus_refseq=consensus_refseq, k=k,
                   windowsize=windowsize, thr=KmerDistThr, buff=buffer, mask=4 ** k - 1, ScaleFactor=1 / k,
                   do_align=do_align, gap_open_score=gap_open_score, gap_extend_score=gap_extend_score,
                   do_return_dists=do_return_dists, do_return_align=do_return_align,
                   get_hit_loci=do_return_hit_loci, dist_vec=dist_vec, result_align_vec=alignment_vec,
                   hit_loci_vec=hit_loci_vec, resultVec=hit_vector, n_refs=N, aligner=aligner, ctx=ctx, strand=strand)
    info = "genome mining completed successfully, returning vector of: vector of hits"
    out = [hit_vector]
    if do_return_hit_loci:
        out.append(hit_loci_vec); info += ", vector of hit locations"
    if do_return_align:
        out.append(alignment_vec); info += ", vector of alignments"
    if do_return_dists:
        out.append(dist_vec); info += ", vector of kmer distances along the genome"
    if verbose:
        log.info(info)
    return out


def findGenes_cluster_mode(*, genome_path: str, ref_path: str, cluster_cutoffs=(7, 12, 20, 25), k: int = 6,
                           KmerDistThrs: Sequence[float] = (0.0,), buffer: int = 100, do_align: bool = True,
                           gap_open_score: int = -200, gap_extend_score: int = -1, do_return_dists: bool = False,
                           do_return_hit_loci: bool = False, do_return_align: bool = False, verbose: bool = True,
                           kmerDist_threshold_buffer: float = 7, aligner: Optional[Callable] = None, ctx=None,
                           strand: str = "+") -> list:
    """`findGenes_cluster_mode` (src/API.jl:161-226).

    strand: "+", "-" or "both", as findGenes (with "both" every KFV's distance vector is its plus vector followed by its
    minus vector; hits are not de-duplicated between the strands).

    Every 1 <= k <= 15 is served; for k >= 11 reference preparation uses the host restatement in refprep (the device refprep
    entry points stop at k = 10), as in findGenes."""
    _check_strand(strand)
    if verbose:
        log.info("pre-processing references and parameters...")
    warn_helper(k, do_return_dists)
    ctx = ctx if ctx is not None else default_context()
    prep_ctx = _prep_ctx(ctx, k)
    RVs, windowsizes, cons, invalids, ints = refprep.cluster_ref_API(ref_path, k, cutoffs=list(cluster_cutoffs),
                                                                      return_int=True, ctx=prep_ctx)
    RVs, windowsizes, cons, ints = refprep.eliminate_null_params(RVs, windowsizes, cons, invalids, ints)
    if k >= min(windowsizes):
        raise ValueError("some/all of the average reference sequence lengths exceeds/is equal to the chosen "
                         f"kmer length {k}. please reduce k. ")
    KmerDistThrs = [float(x) for x in KmerDistThrs]
    est = refprep.estimate_optimal_threshold(RVs, windowsizes, buffer=kmerDist_threshold_buffer, ctx=prep_ctx)
    if KmerDistThrs[0] == 0:
        KmerDistThrs = est
    else:
        idx = [str(i + 1) for i, num in enumerate(KmerDistThrs) if i < len(est) and num > est[i]]
        if idx:
            thr_str = "[" + ", ".join(headers.julia_float_str(x) for x in KmerDistThrs) + "]"
            log.warning(f"The kmer distance thresholds {thr_str} at index/indicies {', '.join(idx)} for k = {k} "
                        "is potentially too high, and may result in more false positives.")
    hit_vector: list = []
    hit_loci_vec: list = []
    alignment_vec: list = []
    dist_vec_vec = [[] for _ in windowsizes]
    if verbose:
        log.info("initializing iteration...")
    Omn_KmerGMA(genome_path=genome_path, refVecs=RVs, windowsizes=windowsizes, consensus_seqs=cons,
                resultVec=hit_vector, k=k, ScaleFactor=1 / k, mask=4 ** k - 1, thr_vec=KmerDistThrs, buff=buffer,
                align_hits=do_align, gap_open_score=gap_open_score, gap_extend_score=gap_extend_score,
                get_aligns=do_return_align, get_hit_loci=do_return_hit_loci, hit_loci_vec=hit_loci_vec,
                align_vec=alignment_vec, do_return_dists=do_return_dists, dist_vec_vec=dist_vec_vec,
                n_refs=[n for _, n in ints], aligner=aligner, ctx=ctx, strand=strand)
    info = "genome mining completed successfully, returning vector of: vector of hits"
    out = [hit_vector]
    if do_return_hit_loci:
        out.append(hit_loci_vec); info += ", vector of hit locations"
    if do_return_align:
        out.append(alignment_vec); info += ", vector of alignments"
    if do_return_dists:
        out.append(dist_vec_vec); info += ", vector of vectors of kmer distances along the genome"
    if verbose:
        log.info(info)
        log.info("To write the results, use `KmerGMA.write_results`")
    return out


def StrobeGMA(*, genome_path, refVec, consensus_refseq: bytes = b"", s: int = 2, w_min: int = 3, w_max: int = 5, q: int = 5,
              windowsize: int = 289, thr: float = 33.5, ScaleFactor=None, buff: int = 50, do_align: bool = True,
              gap_open_score: int = -69, gap_extend_score: int = -5, score_threshold: int = 0,
              do_return_dists: bool = False, do_return_align: bool = False, get_hit_loci: bool = False,
              dist_vec: Optional[list] = None, result_align_vec: Optional[list] = None, hit_loci_vec: Optional[list] = None,
              resultVec: Optional[list] = None, n_refs: Optional[int] = None, ctx: Optional["_lib.Context"] = None,
              float_chain: bool = True, strand: str = "+") -> None:
    """`StrobeGMA!` (src/StrobemerGMA/StrobeGenomeMiner.jl:5-95): mutates resultVec / hit_loci_vec / dist_vec /
    result_align_vec.  The scan, the re-alignment of process_hit! (src/Alignment.jl:83-111; the reference's score model
    defaults to gap_open = -69, gap_extend = -5) and its score gate run on the device (kgma_strobe_scan).
    float_chain (default on): KGMA_F_CHAIN_REPLAY -- records whose decisions hang on the rounding of the reference's
    running Float64 distance are decided by a host replay of that loop (kgma.h).
    strand: "+", "-" or "both", as ac_gma_testing (hits are not de-duplicated between the strands)."""
    _check_strand(strand)
    k = int(w_max) + int(s) - 1
    if ScaleFactor is not None and abs(float(ScaleFactor) - 1.0 / k) > 1e-12:
        raise ValueError(f"ScaleFactor = {ScaleFactor} is not 1/(w_max + s - 1) = 1/{k}")
    resultVec = resultVec if resultVec is not None else []
    ctx = ctx or default_context()
    ctx.set_strobe_ref(s, w_min, w_max, q, np.asarray(refVec, dtype=np.float64), int(windowsize), float(thr), n_refs)
    view = _GenomeView(ctx, genome_path)
    flags = (_lib.F_RETURN_DISTS if do_return_dists else 0) | (_lib.F_CHAIN_REPLAY if float_chain else 0)

    def run(v, sd):
        ctx.strobe_scan(v.genome, int(buff), flags, bytes(consensus_refseq) if do_align else None,
                        gap_open_score, gap_extend_score, int(score_threshold))
        if do_align and do_return_align and result_align_vec is not None:
            _emit_aligns(v, sd, [(a["contig"], 0, a["lo"], a["hi"], a["first"], a["last"]) for a in ctx.alignments()[0]],
                         result_align_vec)
        _emit_hits(v, sd, ctx.hits(),
                   lambda h, lo, hi: headers.single_header(v.identifier(h["contig"]), h["dist"], lo, hi, h["genome_pos"], strand=sd),
                   resultVec, hit_loci_vec if get_hit_loci else None)
        if do_return_dists and dist_vec is not None:
            dist_vec.extend(ctx.dists(1).tolist())

    try:
        _for_strands(view, strand, run)
    finally:
        view.free()


def Strobemer_findGenes(*, genome_path: str, ref_path: str, s: int = 2, w_min: int = 3, w_max: int = 5, q: int = 5,
                        KmerDistThr=30, buffer: int = 50, do_align: bool = True, align_score_thr: int = 0,
                        do_return_dists: bool = False, do_return_hit_loci: bool = False, do_return_align: bool = False,
                        verbose: bool = True, ctx=None, float_chain: bool = True, strand: str = "+") -> list:
    """`Strobemer_findGenes` (src/StrobemerGMA/StrobeGenomeMiner.jl:119-158).  Returns [hits, (loci), (aligns), (dists)].
    strand: "+", "-" or "both", as findGenes (hits are not de-duplicated between the strands)."""
    _check_strand(strand)
    RV, windowsize, consensus_refseq, (_S, N) = refprep.gen_ref_ws_cons_strobe(ref_path, s, w_min, w_max, q, return_int=True)
    hit_vector: list = []
    dist_vec: list = []
    hit_loci_vec: list = []
    alignment_vec: list = []
    if verbose:
        log.info("initializing iteration...")
    StrobeGMA(genome_path=genome_path, refVec=RV, consensus_refseq=consensus_refseq, s=s, w_min=w_min, w_max=w_max, q=q,
              windowsize=windowsize, thr=KmerDistThr, ScaleFactor=1 / (w_max + s - 1), buff=buffer,
              score_threshold=align_score_thr, do_align=do_align, do_return_dists=do_return_dists,
              do_return_align=do_return_align, get_hit_loci=do_return_hit_loci, dist_vec=dist_vec,
              result_align_vec=alignment_vec, hit_loci_vec=hit_loci_vec, resultVec=hit_vector, n_refs=N, ctx=ctx,
              float_chain=float_chain, strand=strand)
    info = "genome mining completed successfully, returning vector of: vector of hits"
    out = [hit_vector]
    if do_return_hit_loci:
        out.append(hit_loci_vec); info += ", vector of hit locations"
    if do_return_align:
        out.append(alignment_vec); info += ", vector of alignments"
    if do_return_dists:
        out.append(dist_vec); info += ", vector of kmer distances along the genome"
    if verbose:
        log.info(info)
    return out


_DNA_SYMBOLS = frozenset(b"ACGTMRWSYKVHDBNacgtmrwsykvhdbn-")


def _query_bytes(query) -> bytes:
    """convert_to_search_query (src/ExactMatch.jl:46-58): a Record, a str or bytes of DNA symbols."""
    if isinstance(query, Record):
        q = bytes(query.sequence)
    elif isinstance(query, str):
        q = query.encode()
    elif isinstance(query, (bytes, bytearray, memoryview)):
        q = bytes(query)
    else:
        raise TypeError("Invalid query sequence type")
    if not q:
        raise ValueError("empty query")
    if not _DNA_SYMBOLS.issuperset(q):
        i = next(i for i, ch in enumerate(q) if ch not in _DNA_SYMBOLS)
        raise ValueError(f"query symbol {i + 1} ({q[i:i + 1]!r}) is outside the DNA alphabet")
    return q


def _open_subject(ctx, subject):
    """(device genome, per-record identifier lookup, owned) for a FASTA or .2bit path, an open device genome or a _GenomeView."""
    if isinstance(subject, str):
        g = ctx.genome_from_path(subject)
        return g, g, True
    if isinstance(subject, _GenomeView):
        return subject.genome, subject, False
    return subject, subject, False


def _identifier(src, c: int) -> str:
    if isinstance(src, _GenomeView):
        return src.identifier(c)
    parts = src.header(c).split(None, 1)       # FASTA.identifier: the header up to the first whitespace
    return parts[0] if parts else ""


def exactMatch_batch(queries, genome_or_path, *, overlap: bool = True, ctx=None) -> list:
    """exactMatch (src/ExactMatch.jl:100-121) for many queries in ONE pass over the genome (kgma_exact_match): per query
    the dict {identifier: [(lo, hi), ...]} over the records with at least one match, or the string "no match".
    `genome_or_path`: a FASTA or .2bit path, or a device genome that is already open (it stays open)."""
    qs = [_query_bytes(q) for q in queries]
    if not isinstance(genome_or_path, (str, _GenomeView, _lib.Genome)):
        raise TypeError("Invalid subject sequence type")
    ctx = ctx or default_context()
    g, src, owned = _open_subject(ctx, genome_or_path)
    try:
        ctx.exact_match(g, qs, overlap)
        mt = ctx.matches()
        ids = {int(c): _identifier(src, int(c)) for c in np.unique(mt["contig"])}
    finally:
        if owned:
            g.free()
    out = [dict() for _ in qs]
    # (sorted by query, record, start: one run per (query, record); a later record with the same identifier replaces the
    #  earlier one's entry, as the reference's Dict assignment does)
    bounds = np.flatnonzero(np.diff(mt["query"]) | np.diff(mt["contig"])) + 1
    for run in np.split(mt, bounds) if mt.size else []:
        qi, m = int(run["query"][0]), len(qs[int(run["query"][0])])
        out[qi][ids[int(run["contig"][0])]] = [(s, s + m - 1) for s in run["start"].tolist()]
    return [d if d else "no match" for d in out]


def exactMatch(query, subject_seq, *, overlap: bool = True, ctx=None):
    """exactMatch (src/ExactMatch.jl:89-121).  `query`: bytes / str / Record.  A `subject_seq` of residues (bytes, or a
    Record) returns the list of 1-based inclusive (lo, hi) matches, or None when there is none (:89-98); a str is a FASTA
    path, as in the reference (:100-107), and it or an open device genome returns {identifier: [(lo, hi), ...]} over the
    records with a match, or the string "no match".  overlap=False keeps FindAll's non-overlapping matches (:20-30).
    Symbols compare as BioSequences' isequal does: N only matches N, an IUPAC code only itself."""
    q = _query_bytes(query)
    if isinstance(subject_seq, (Record, bytes, bytearray, memoryview)):
        seq = bytes(subject_seq.sequence if isinstance(subject_seq, Record) else subject_seq)
        ctx = ctx or default_context()
        g = ctx.genome_from_host([seq])
        try:
            ctx.exact_match(g, [q], overlap)
            starts = ctx.matches()["start"].tolist()
        finally:
            g.free()
        return [(s, s + len(q) - 1) for s in starts] or None
    return exactMatch_batch([q], subject_seq, overlap=overlap, ctx=ctx)[0]


# ---- IUPAC motif search with mismatches (kgma_motif_match): the working form of src/RSS.jl ----------------------------------

# The recombination signal sequence heptamer - spacer - nonamer, as src/RSS.jl:11-15 defines it and under the reference's
# names: HumanRSSV has the 12-nt spacer, HumanRSSD the 23-nt one.  The names are the reference's; which gene segment carries
# which spacer depends on the locus, and IGHV genes carry the 23-nt form: on tests/data/Loci.fasta it is HumanRSSD that lies
# behind each of the seven V genes the scan finds.
HumanRSSV = b"CACAGTG" + b"N" * 12 + b"ACAAAAACC"
HumanRSSD = b"CACAGTG" + b"N" * 23 + b"ACAAAAACC"

_IUPAC_SYMBOLS = frozenset(b"ACGTRYSWKMBDHVNacgtryswkmbdhvn")
MOTIF_MAX_LEN, MOTIF_MAX_MISMATCH = 64, 15


def RSS_dist(RSS1, RSS2=HumanRSSV) -> int:
    """RSS_dist (src/RSS.jl:22-28), literally: the number of positions i of RSS1 at which RSS1[i] != RSS2[i], symbols
    compared for inequality after case folding.  The quirk is the reference's: an `N` of RSS2 is unequal to every base, so
    against HumanRSSV every sequence has a distance of at least 12 and `is_RSS(..., thr = 1)` can never hold.  Use motifMatch
    / findRSS for the search the file is after.  An RSS2 shorter than RSS1 raises IndexError (the reference: BoundsError)."""
    a, b = _query_bytes(RSS1).upper(), _query_bytes(RSS2).upper()
    if len(b) < len(a):
        raise IndexError(f"RSS2 has {len(b)} symbols, RSS1 {len(a)} (BoundsError, src/RSS.jl:25)")
    return sum(1 for i in range(len(a)) if a[i] != b[i])


def _motif_bytes(motif, max_mismatch, which: str = "motif", limit: str = "max_mismatch") -> bytes:
    """The checks of kgma_motif_match (and, with limit="max_edits", of kgma_approx_match), made before any device call."""
    if isinstance(motif, Record):
        m = bytes(motif.sequence)
    elif isinstance(motif, str):
        m = motif.encode()
    elif isinstance(motif, (bytes, bytearray, memoryview)):
        m = bytes(motif)
    else:
        raise TypeError("Invalid motif type")
    if not 1 <= len(m) <= MOTIF_MAX_LEN:
        raise ValueError(f"{which} has {len(m)} symbols (1 ... {MOTIF_MAX_LEN})")
    for i, ch in enumerate(m):
        if ch not in _IUPAC_SYMBOLS:
            raise ValueError(f"{which}, symbol {i + 1} ({m[i:i + 1]!r}) is not an IUPAC nucleotide code")
    d = int(max_mismatch)
    if not 0 <= d <= MOTIF_MAX_MISMATCH:
        raise ValueError(f"{which}: {limit} {d} (0 ... {MOTIF_MAX_MISMATCH})")
    informative = sum(1 for ch in m.upper() if ch != ord("N"))
    if d >= informative:
        raise ValueError(f"{which}: {limit} {d} is not smaller than its {informative} informative (non-N) positions: "
                         "every start would match")
    return m


def _motif_args(motifs, max_mismatch, strand, which: str = "motif", limit: str = "max_mismatch"):
    _check_strand(strand)
    motifs = list(motifs)
    if isinstance(max_mismatch, (int, np.integer)):
        ds = [int(max_mismatch)] * len(motifs)
    else:
        ds = [int(d) for d in max_mismatch]
        if len(ds) != len(motifs):
            raise ValueError(f"need one {limit} per {which}")
    ms = [_motif_bytes(m, d, f"{which} {i}", limit) for i, (m, d) in enumerate(zip(motifs, ds))]
    # the minus strand: the reverse-complemented motif on the SAME genome, in the same pass
    sent, tags = [], []
    for i, (m, d) in enumerate(zip(ms, ds)):
        if strand != "-":
            sent.append((m, d)); tags.append((i, "+"))
        if strand != "+":
            sent.append((reverse_complement(m), d)); tags.append((i, "-"))
    return ms, sent, tags


def _motif_run(ctx, g, ms, sent, tags) -> list:
    """Per motif the hits (record, lo, hi, strand, mismatches), sorted by (record, lo, strand)."""
    ctx.motif_match(g, [m for m, _ in sent], [d for _, d in sent])
    out = [[] for _ in ms]
    for h in ctx.motif_matches().tolist():
        i, st = tags[h[0]]
        out[i].append((h[1], h[2], h[2] + len(ms[i]) - 1, st, h[3]))
    for lst in out:
        lst.sort(key=lambda t: (t[0], t[1], t[3]))              # ("+" sorts before "-")
    return out


def motifMatch_batch(motifs, genome_or_path, *, max_mismatch=0, strand: str = "+", ctx=None) -> list:
    """Many IUPAC motifs in ONE pass over the genome (kgma_motif_match): per motif the list of
    (record_index, identifier, lo, hi, strand, mismatches) -- 0-based record, 1-based inclusive lo:hi in forward coordinates --
    sorted by (record, lo, strand).  `max_mismatch`: one number for all motifs or one per motif.  Semantics: motifMatch.
    `genome_or_path`: a FASTA or .2bit path, or a device genome that is already open (it stays open)."""
    ms, sent, tags = _motif_args(motifs, max_mismatch, strand)
    if not isinstance(genome_or_path, (str, _GenomeView, _lib.Genome)):
        raise TypeError("Invalid subject sequence type")
    ctx = ctx or default_context()
    g, src, owned = _open_subject(ctx, genome_or_path)
    try:
        res = _motif_run(ctx, g, ms, sent, tags)
        ids = {c: _identifier(src, c) for c in {t[0] for lst in res for t in lst}}
    finally:
        if owned:
            g.free()
    return [[(c, ids[c], lo, hi, st, mm) for c, lo, hi, st, mm in lst] for lst in res]


def motifMatch(motif, subject_seq, *, max_mismatch: int = 0, strand: str = "+", ctx=None):
    """Every place at which `motif` -- 1 ... 64 IUPAC symbols (ACGTRYSWKMBDHVN, either case; bytes / str / Record) -- lies on
    the subject with at most `max_mismatch` (0 ... 15) non-matching positions; overlapping places included, none spanning two
    records.  A genome base matches a symbol whose set contains it; a genome N matches only a motif N (assembly gaps never
    match informative positions).  `max_mismatch` must be smaller than the number of non-N symbols of the motif.  The subject
    may hold A/C/G/T/N only (KgmaError KGMA_E_BADBASE otherwise).
    strand: "+" the motif as given; "-" its reverse complement, searched on the same genome and reported at the forward
    lo:hi it covers; "both" the two together (a motif equal to its own reverse complement is reported on both strands).
    A `subject_seq` of residues (bytes, or a Record) returns [(lo, hi, strand, mismatches)] sorted by (lo, strand); a FASTA
    path or an open device genome returns motifMatch_batch(...)[0].  An empty list when there is no match."""
    if isinstance(subject_seq, (Record, bytes, bytearray, memoryview)):
        ms, sent, tags = _motif_args([motif], max_mismatch, strand)
        seq = bytes(subject_seq.sequence if isinstance(subject_seq, Record) else subject_seq)
        ctx = ctx or default_context()
        g = ctx.genome_from_host([seq])
        try:
            res = _motif_run(ctx, g, ms, sent, tags)[0]
        finally:
            g.free()
        return [(lo, hi, st, mm) for _, lo, hi, st, mm in res]
    return motifMatch_batch([motif], subject_seq, max_mismatch=max_mismatch, strand=strand, ctx=ctx)[0]


def findRSS(genome_or_path, rss=HumanRSSD, max_mismatch: int = 1, strand: str = "both", ctx=None):
    """Recombination signal sequences on a genome: motifMatch with the 23-nt-spacer RSS, one mismatch and both strands as the
    defaults.  (The reference's Align_RSS / is_RSS are not mirrored: DESIGN.md, section 8.)"""
    return motifMatch(rss, genome_or_path, max_mismatch=max_mismatch, strand=strand, ctx=ctx)


# ---- edit-distance search (kgma_approx_match): what motifMatch cannot express -- a base inserted or deleted -------------------

def _approx_run(ctx, g, qs, sent, tags, all_ends: bool) -> list:
    """Per query the hits (record, lo, hi, strand, edits), sorted by (record, lo, strand)."""
    ctx.approx_match(g, [q for q, _ in sent], [e for _, e in sent], best_only=not all_ends)
    out = [[] for _ in qs]
    for query, contig, start, end, edits, _ in ctx.approx_matches().tolist():
        i, st = tags[query]
        out[i].append((contig, start, end, st, edits))
    for lst in out:
        lst.sort(key=lambda t: (t[0], t[1], t[3], t[2]))        # ("+" sorts before "-"; all_ends: several ends may share a lo)
    return out


def approxMatch_batch(queries, genome_or_path, *, max_edits=1, strand: str = "+", all_ends: bool = False, ctx=None) -> list:
    """Many queries in ONE pass over the genome (kgma_approx_match): per query the list of
    (record_index, identifier, lo, hi, strand, edits) -- 0-based record, 1-based inclusive lo:hi in forward coordinates --
    sorted by (record, lo, strand).  `max_edits`: one number for all queries or one per query.  Semantics: approxMatch.
    `genome_or_path`: a FASTA or .2bit path, or a device genome that is already open (it stays open)."""
    qs, sent, tags = _motif_args(queries, max_edits, strand, "query", "max_edits")
    if not isinstance(genome_or_path, (str, _GenomeView, _lib.Genome)):
        raise TypeError("Invalid subject sequence type")
    ctx = ctx or default_context()
    g, src, owned = _open_subject(ctx, genome_or_path)
    try:
        res = _approx_run(ctx, g, qs, sent, tags, all_ends)
        ids = {c: _identifier(src, c) for c in {t[0] for lst in res for t in lst}}
    finally:
        if owned:
            g.free()
    return [[(c, ids[c], lo, hi, st, ed) for c, lo, hi, st, ed in lst] for lst in res]


def approxMatch(query, subject_seq, *, max_edits: int = 1, strand: str = "+", all_ends: bool = False, ctx=None):
    """Every place at which `query` -- 1 ... 64 IUPAC symbols (ACGTRYSWKMBDHVN, either case; bytes / str / Record) -- lies on the
    subject within `max_edits` (0 ... 15) edits: substitutions, inserted and deleted bases, one each (Sellers' semi-global edit
    distance: the whole query against any substring of one record).  Symbols match as in motifMatch: a genome base matches a
    symbol whose set contains it, a genome N only a query N.  `max_edits` must be smaller than the number of non-N symbols of
    the query.  The subject may hold A/C/G/T/N only (KgmaError KGMA_E_BADBASE otherwise).
    An end position whose best substring is within max_edits is a matching end; consecutive matching ends form a run, and per
    run the end with the fewest edits (the leftmost of them) is reported with lo:hi, the SHORTEST substring ending there that
    attains its edits.  all_ends=True reports every matching end instead.
    strand: "+" the query as given; "-" its reverse complement, searched on the same genome and reported at the forward lo:hi
    it covers; "both" the two together.
    A `subject_seq` of residues (bytes, or a Record) returns [(lo, hi, strand, edits)] sorted by (lo, strand); a FASTA path or
    an open device genome returns approxMatch_batch(...)[0].  An empty list when there is no match."""
    if isinstance(subject_seq, (Record, bytes, bytearray, memoryview)):
        qs, sent, tags = _motif_args([query], max_edits, strand, "query", "max_edits")
        seq = bytes(subject_seq.sequence if isinstance(subject_seq, Record) else subject_seq)
        ctx = ctx or default_context()
        g = ctx.genome_from_host([seq])
        try:
            res = _approx_run(ctx, g, qs, sent, tags, all_ends)[0]
        finally:
            g.free()
        return [(lo, hi, st, ed) for _, lo, hi, st, ed in res]
    return approxMatch_batch([query], subject_seq, max_edits=max_edits, strand=strand, all_ends=all_ends, ctx=ctx)[0]


def findRSS_edits(genome_or_path, rss=HumanRSSD, max_edits: int = 1, strand: str = "both", ctx=None):
    """Recombination signal sequences within `max_edits` edits: with the default, one substitution or a spacer one base longer
    or shorter than the 23 (12) nt findRSS lays rigidly.  approxMatch's best end per run."""
    return approxMatch(rss, genome_or_path, max_edits=max_edits, strand=strand, ctx=ctx)


# ---- position-weight-matrix search (kgma_pwm_match): positions weighted by how much they matter -----------------------------

PWM_MAX_ROWS, PWM_WEIGHT_MIN, PWM_WEIGHT_MAX = 64, -32768, 32767
_UNIFORM = (0.25, 0.25, 0.25, 0.25)
_IUPAC_SETS = {"A": 1, "C": 2, "G": 4, "T": 8, "R": 5, "Y": 10, "S": 6, "W": 9, "K": 12, "M": 3, "B": 14, "D": 13, "H": 11, "V": 7,
               "N": 15}          # bit 0 A, 1 C, 2 G, 3 T


def _background(background) -> np.ndarray:
    bg = np.asarray(background, dtype=np.float64)
    if bg.shape != (4,) or not np.isfinite(bg).all() or (bg <= 0).any() or not math.isclose(float(bg.sum()), 1.0, rel_tol=0, abs_tol=1e-9):
        raise ValueError("background: four positive probabilities (A, C, G, T) that sum to 1")
    return bg


def _pwm_matrix(matrix, which: str = "matrix") -> np.ndarray:
    """The checks of kgma_pwm_match on one matrix, made before any device call: an (m, 4) int64 array."""
    if isinstance(matrix, (str, bytes, bytearray, memoryview, Record)) or matrix is None:
        raise TypeError("Invalid matrix type")
    a = np.asarray(matrix)
    if a.dtype.kind not in "iu":
        raise TypeError(f"{which}: the weights must be integers (scale and round a log-odds matrix: pwm_from_sequences)")
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError(f"{which}: need rows of four weights (A, C, G, T), got shape {a.shape}")
    if not 1 <= a.shape[0] <= PWM_MAX_ROWS:
        raise ValueError(f"{which} has {a.shape[0]} rows (1 ... {PWM_MAX_ROWS})")
    a = a.astype(np.int64)
    bad = np.argwhere((a < PWM_WEIGHT_MIN) | (a > PWM_WEIGHT_MAX))
    if bad.size:
        raise ValueError(f"{which}, row {int(bad[0][0]) + 1}: weight {int(a[tuple(bad[0])])} is outside {PWM_WEIGHT_MIN} ... {PWM_WEIGHT_MAX}")
    return a


def pwm_from_sequences(seqs, *, pseudocount: float = 1.0, background=_UNIFORM, scale: float = 100) -> np.ndarray:
    """Log-odds position weight matrix of equal-length example sites (A/C/G/T, either case; bytes / str / Record): the (m, 4)
    int64 array np.rint(scale * log2(((count + pseudocount * bg) / (n + pseudocount)) / bg)), columns in the order A, C, G, T.
    With scale = 100 the weights are centibits.  ValueError when a weight leaves the int16 range of kgma_pwm_match (a count of 0
    without a pseudocount, a scale too large)."""
    rows = [_query_bytes(q).upper() for q in seqs]
    if not rows:
        raise ValueError("need at least one sequence")
    m = len(rows[0])
    if not 1 <= m <= PWM_MAX_ROWS:
        raise ValueError(f"the sequences have {m} symbols (1 ... {PWM_MAX_ROWS})")
    if any(len(r) != m for r in rows):
        raise ValueError("the sequences differ in length")
    bg = _background(background)
    if not (math.isfinite(pseudocount) and pseudocount >= 0 and math.isfinite(scale) and scale > 0):
        raise ValueError("pseudocount must be >= 0 and scale > 0")
    text = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), m)
    count = np.stack([(text == ch).sum(axis=0) for ch in b"ACGT"], axis=1).astype(np.float64)
    if (count.sum(axis=1) != len(rows)).any():
        raise ValueError("the sequences may hold A, C, G and T only")
    with np.errstate(divide="ignore"):
        w = np.rint(scale * np.log2(((count + pseudocount * bg) / (len(rows) + pseudocount)) / bg))
    if not np.isfinite(w).all() or (w < PWM_WEIGHT_MIN).any() or (w > PWM_WEIGHT_MAX).any():
        i = int(np.argwhere(~np.isfinite(w) | (w < PWM_WEIGHT_MIN) | (w > PWM_WEIGHT_MAX))[0][0])
        raise ValueError(f"row {i + 1}: a weight leaves {PWM_WEIGHT_MIN} ... {PWM_WEIGHT_MAX} (give a pseudocount or a smaller scale)")
    return w.astype(np.int64)


def pwm_from_motif(motif):
    """The 0/1 matrix of an IUPAC motif and its number of informative (non-N) symbols: weight 1 where the symbol's set holds
    the base, all four weights 0 for N.  With threshold = informative - d, pwmMatch finds exactly motifMatch(max_mismatch=d)'s
    starts, and score = informative - mismatches."""
    m = _motif_bytes(motif, 0)
    sets = [_IUPAC_SETS[chr(ch).upper()] for ch in m]
    w = np.array([[0, 0, 0, 0] if s == 15 else [(s >> b) & 1 for b in range(4)] for s in sets], dtype=np.int64)
    return w, sum(1 for s in sets if s != 15)


def pwm_revcomp(matrix) -> np.ndarray:
    """The matrix of the other strand: rows reversed, A <-> T and C <-> G swapped."""
    return _pwm_matrix(matrix)[::-1, ::-1].copy()


def pwm_score_distribution(matrix, background=_UNIFORM):
    """(lowest, p): p[k] is the probability that m independent bases drawn from `background` score lowest + k, exactly on the
    integer lattice -- one convolution per row; lowest is the sum of the row minima, lowest + len(p) - 1 that of the maxima."""
    w, bg = _pwm_matrix(matrix), _background(background)
    lo = w.min(axis=1)
    p = np.ones(1, dtype=np.float64)
    for row, base in zip(w, lo):
        shift = (row - base).tolist()
        q = np.zeros(p.size + max(shift), dtype=np.float64)
        for b in range(4):
            q[shift[b]:shift[b] + p.size] += bg[b] * p
        p = q
    return int(lo.sum()), p


def pwm_threshold(matrix, pvalue: float, background=_UNIFORM) -> int:
    """The smallest integer t with P(score >= t) <= pvalue for independent bases drawn from `background` (A, C, G, T), from
    the exact score distribution (pwm_score_distribution).  One above the highest score when even that one is likelier than
    pvalue."""
    if not 0 < float(pvalue) < 1:
        raise ValueError("pvalue must lie strictly between 0 and 1")
    lowest, p = pwm_score_distribution(matrix, background)
    tail = np.cumsum(p[::-1])[::-1]                               # tail[k] = P(score >= lowest + k), summed from the top
    ok = np.flatnonzero(tail <= float(pvalue))
    return lowest + (int(ok[0]) if ok.size else p.size)


def _pwm_args(matrices, threshold, pvalue, strand, background=None):
    _check_strand(strand)
    if (threshold is None) == (pvalue is None):
        raise ValueError("give exactly one of threshold and pvalue")
    ms = [_pwm_matrix(m, f"matrix {i}") for i, m in enumerate(matrices)]
    if pvalue is not None:
        ps = [float(pvalue)] * len(ms) if isinstance(pvalue, (int, float, np.integer, np.floating)) else [float(x) for x in pvalue]
        if len(ps) != len(ms):
            raise ValueError("need one pvalue per matrix")
        ts = [pwm_threshold(m, x) if background is None else pwm_threshold(m, x, background) for m, x in zip(ms, ps)]
    elif isinstance(threshold, (int, np.integer)):
        ts = [int(threshold)] * len(ms)
    else:
        ts = [int(t) for t in threshold]
        if len(ts) != len(ms):
            raise ValueError("need one threshold per matrix")
    for i, (m, t) in enumerate(zip(ms, ts)):
        lowest = int(m.min(axis=1).sum())
        if t <= lowest:
            raise ValueError(f"matrix {i}: threshold {t} does not exceed the sum of its row minima, {lowest}: every start would match")
        if not t < 2 ** 31:
            raise ValueError(f"matrix {i}: threshold {t} does not fit an int32")
    # the minus strand: the reverse-complemented matrix on the SAME genome, in the same pass
    sent, tags = [], []
    for i, (m, t) in enumerate(zip(ms, ts)):
        if strand != "-":
            sent.append((m, t)); tags.append((i, "+"))
        if strand != "+":
            sent.append((pwm_revcomp(m), t)); tags.append((i, "-"))
    return ms, sent, tags


def _pwm_run(ctx, g, ms, sent, tags) -> list:
    """Per matrix the hits (record, lo, hi, strand, score), sorted by (record, lo, strand)."""
    ctx.pwm_match(g, [m for m, _ in sent], [t for _, t in sent])
    out = [[] for _ in ms]
    for h in ctx.pwm_matches().tolist():
        i, st = tags[h[0]]
        out[i].append((h[1], h[2], h[2] + ms[i].shape[0] - 1, st, h[3]))
    for lst in out:
        lst.sort(key=lambda t: (t[0], t[1], t[3]))              # ("+" sorts before "-")
    return out


def _pwm_background(background, threshold):
    """background= of the searches, checked: None (uniform, as pwm_threshold's default), four probabilities, or the string
    "genome" (the base composition of the open subject, measured on the device by genome_background once it is open)."""
    if background is None:
        return None
    if threshold is not None:
        raise ValueError("background has an effect only together with pvalue: give pvalue, not threshold")
    if isinstance(background, str):
        if background != "genome":
            raise ValueError(f"background must be four probabilities or 'genome', not {background!r}")
        return background
    return _background(background)


def pwmMatch_batch(matrices, genome_or_path, *, threshold=None, pvalue=None, strand: str = "+", background=None, ctx=None) -> list:
    """Many matrices in ONE pass over the genome (kgma_pwm_match): per matrix the list of
    (record_index, identifier, lo, hi, strand, score) -- 0-based record, 1-based inclusive lo:hi in forward coordinates --
    sorted by (record, lo, strand).  `threshold` / `pvalue`: one number for all matrices or one per matrix.  Semantics: pwmMatch.
    `genome_or_path`: a FASTA or .2bit path, or a device genome that is already open (it stays open).  `background`: pwmMatch."""
    matrices, bg = list(matrices), _pwm_background(background, threshold)
    ms, sent, tags = _pwm_args(matrices, threshold, pvalue, strand, None if isinstance(bg, str) else bg)
    if not isinstance(genome_or_path, (str, _GenomeView, _lib.Genome)):
        raise TypeError("Invalid subject sequence type")
    ctx = ctx or default_context()
    g, src, owned = _open_subject(ctx, genome_or_path)
    try:
        if isinstance(bg, str):
            ms, sent, tags = _pwm_args(matrices, threshold, pvalue, strand, genome_background(g, ctx=ctx))
        res = _pwm_run(ctx, g, ms, sent, tags)
        ids = {c: _identifier(src, c) for c in {t[0] for lst in res for t in lst}}
    finally:
        if owned:
            g.free()
    return [[(c, ids[c], lo, hi, st, sc) for c, lo, hi, st, sc in lst] for lst in res]


def pwmMatch(matrix, subject_seq, *, threshold=None, pvalue=None, strand: str = "+", background=None, ctx=None):
    """Every place at which `matrix` -- 1 ... 64 rows of four integer weights (A, C, G, T; each -32768 ... 32767) -- laid on the
    subject scores at least the threshold: score(s) = sum over the rows i of matrix[i][t[s + i]], overlapping places included,
    none spanning two records.  Case is folded; a genome N scores its row's minimum, so an assembly gap never looks like a signal
    and a row of four equal weights (a spacer) costs nothing.  Give exactly one of `threshold` (an integer that exceeds the sum of
    the row minima) and `pvalue` (the threshold becomes pwm_threshold(matrix, pvalue, background)).  `background` has an effect only
    together with `pvalue` (ValueError with `threshold`): None is the uniform one, four probabilities (A, C, G, T) are handed to
    pwm_threshold, and the string "genome" is genome_background(subject), the subject's own base composition measured on the
    device.  The subject may hold A/C/G/T/N only (KgmaError KGMA_E_BADBASE otherwise).
    strand: "+" the matrix as given; "-" its reverse complement (pwm_revcomp), searched on the same genome and reported at the
    forward lo:hi it covers; "both" the two together (a matrix equal to its own reverse complement is reported on both strands).
    A `subject_seq` of residues (bytes, or a Record) returns [(lo, hi, strand, score)] sorted by (lo, strand); a FASTA path or
    an open device genome returns pwmMatch_batch(...)[0].  An empty list when there is no hit."""
    if isinstance(subject_seq, (Record, bytes, bytearray, memoryview)):
        bg = _pwm_background(background, threshold)
        ms, sent, tags = _pwm_args([matrix], threshold, pvalue, strand, None if isinstance(bg, str) else bg)
        seq = bytes(subject_seq.sequence if isinstance(subject_seq, Record) else subject_seq)
        ctx = ctx or default_context()
        g = ctx.genome_from_host([seq])
        try:
            if isinstance(bg, str):
                ms, sent, tags = _pwm_args([matrix], threshold, pvalue, strand, genome_background(g, ctx=ctx))
            res = _pwm_run(ctx, g, ms, sent, tags)[0]
        finally:
            g.free()
        return [(lo, hi, st, sc) for _, lo, hi, st, sc in res]
    return pwmMatch_batch([matrix], subject_seq, threshold=threshold, pvalue=pvalue, strand=strand, background=background, ctx=ctx)[0]


def findRSS_pwm(genome_or_path, sites_or_matrix, *, pvalue: float = 1e-6, strand: str = "both", background=None, ctx=None):
    """Recombination signal sequences by a position weight matrix: `sites_or_matrix` is a list of example sites (equal-length
    A/C/G/T sequences, made into a log-odds matrix by pwm_from_sequences) or a ready matrix; every place of the genome that
    scores at least the exact p <= pvalue threshold is returned as pwmMatch does.  Unlike findRSS's mismatch count it weighs
    the all but invariant CAC of the heptamer above the positions that drift."""
    first = sites_or_matrix[0] if isinstance(sites_or_matrix, (list, tuple)) and len(sites_or_matrix) else None
    if isinstance(first, (str, bytes, bytearray, memoryview, Record)):
        matrix = pwm_from_sequences(sites_or_matrix)
    else:
        matrix = sites_or_matrix
    return pwmMatch(matrix, genome_or_path, pvalue=pvalue, strand=strand, background=background, ctx=ctx)


# ---- amino-acid profile search in all six reading frames (kgma_codon_match) --------------------------------------------------

AMINO_ACIDS = "ACDEFGHIKLMNPQRSTVWY*"      # the 21 columns of an amino-acid profile; '*' is the stop
PROT_MAX_ROWS = 64
# NCBI translation tables as 64 letters in the order TTT, TTC, TTA, TTG, TCT, ... GGG (bases in the order T, C, A, G)
GENETIC_CODES = {1: "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"}
_AA_COLUMN = {ch: i for i, ch in enumerate(AMINO_ACIDS)}
_TCAG_OF_BASE = (2, 1, 3, 0)               # where A, C, G, T stand in T, C, A, G
_COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def genetic_code(table=1) -> np.ndarray:
    """A genetic code as kgma_codon_fold takes it: 64 column numbers (0 ... 20, into AMINO_ACIDS) indexed by the codon
    16 b0 + 4 b1 + b2 with A 0, C 1, G 2, T 3.  `table`: the number of a shipped NCBI table (1, the standard code), any
    NCBI-style string of 64 letters in TCAG order (TTT, TTC, TTA, TTG, TCT, ...; '*' the stop), or such an array itself."""
    if isinstance(table, np.ndarray):
        if table.shape != (64,) or table.dtype.kind not in "iu" or (table < 0).any() or (table > 20).any():
            raise ValueError("a genetic code array holds 64 column numbers 0 ... 20")
        return table.astype(np.int64)
    if isinstance(table, (int, np.integer)):
        if int(table) not in GENETIC_CODES:
            raise ValueError(f"genetic code {int(table)} is not shipped (have {sorted(GENETIC_CODES)}): pass its 64 letters in TCAG order")
        table = GENETIC_CODES[int(table)]
    if isinstance(table, (bytes, bytearray)):
        table = bytes(table).decode("ascii", "replace")
    if not isinstance(table, str):
        raise TypeError("genetic code: a table number or a string of 64 letters")
    letters = table.upper()
    if len(letters) != 64:
        raise ValueError(f"a genetic code has 64 letters, not {len(letters)}")
    for i, ch in enumerate(letters):
        if ch not in _AA_COLUMN:
            raise ValueError(f"genetic code, letter {i + 1}: {ch!r} is none of {AMINO_ACIDS}")
    T = _TCAG_OF_BASE
    return np.array([_AA_COLUMN[letters[16 * T[c >> 4] + 4 * T[(c >> 2) & 3] + T[c & 3]]] for c in range(64)], dtype=np.int64)


_code_of = genetic_code                   # (the functions below have a parameter of that name)


def _codon_codes(seq: bytes) -> np.ndarray:
    """Codon code 0 ... 63, or 64 with a residue other than A/C/G/T, of every whole codon of `seq` from its first residue."""
    t = np.frombuffer(seq.upper(), dtype=np.uint8)
    t = t[:t.size - t.size % 3]
    b = np.full(256, 4, dtype=np.int64)
    b[list(b"ACGT")] = (0, 1, 2, 3)
    x = b[t].reshape(-1, 3)
    return np.where((x > 3).any(axis=1), 64, 16 * x[:, 0] + 4 * x[:, 1] + x[:, 2])


def translate(seq, frame: int = 1, genetic_code=1) -> str:
    """The amino acids (letters of AMINO_ACIDS, '*' the stop) of reading frame `frame` of `seq` (bytes / str / Record; case
    folded): 1, 2, 3 begin at the first, second, third residue; -1, -2, -3 read the reverse complement from its first,
    second, third residue.  A codon that holds any residue other than A/C/G/T is 'X', also where every base at that place
    gives the same amino acid: CTN is X, not Leu.  A trailing part of a codon is dropped."""
    if frame not in (1, 2, 3, -1, -2, -3):
        raise ValueError("frame is one of 1, 2, 3, -1, -2, -3")
    s = _query_bytes(seq)
    if frame < 0:
        s = s.translate(_COMPLEMENT)[::-1]
    col = _code_of(genetic_code)
    codes = _codon_codes(s[abs(frame) - 1:])
    letters = np.frombuffer((AMINO_ACIDS + "X").encode(), dtype=np.uint8)
    return letters[np.where(codes == 64, 21, col[np.minimum(codes, 63)])].tobytes().decode()


def _prot_matrix(matrix, which: str = "profile") -> np.ndarray:
    """The checks on one amino-acid profile, made before any device call: an (m, 21) int64 array."""
    if isinstance(matrix, (str, bytes, bytearray, memoryview, Record)) or matrix is None:
        raise TypeError("Invalid profile type")
    a = np.asarray(matrix)
    if a.dtype.kind not in "iu":
        raise TypeError(f"{which}: the weights must be integers (scale and round a log-odds matrix: prot_matrix_from_sequences)")
    if a.ndim != 2 or a.shape[1] != len(AMINO_ACIDS):
        raise ValueError(f"{which}: need rows of 21 weights ({AMINO_ACIDS}), got shape {a.shape}")
    if not 1 <= a.shape[0] <= PROT_MAX_ROWS:
        raise ValueError(f"{which} has {a.shape[0]} rows (1 ... {PROT_MAX_ROWS})")
    a = a.astype(np.int64)
    bad = np.argwhere((a < PWM_WEIGHT_MIN) | (a > PWM_WEIGHT_MAX))
    if bad.size:
        raise ValueError(f"{which}, row {int(bad[0][0]) + 1}: weight {int(a[tuple(bad[0])])} is outside {PWM_WEIGHT_MIN} ... {PWM_WEIGHT_MAX}")
    return a


def prot_pattern(pattern: str):
    """The 0/-1 profile of a PROSITE-style pattern and its length in residues: (matrix, m), matrix (m, 21) over AMINO_ACIDS.
    Elements, separated by '-' (the separator may be left out): a residue `W`; a set `[VIFY]` (any of them); an excluded set
    `{PG}` (anything but them -- the stop included unless it is listed); `x` (anything, the stop included: a row of 21 zeros,
    which costs nothing); `*` the stop; each may be followed by a repeat count `(n)`, as in `x(3)`.  Letters are those of
    AMINO_ACIDS, in either case.  A position scores 0 where the element admits the amino acid and -1 where it does not, so
    score = -mismatches and protMatch(..., max_mismatch=d) is the threshold -d.  Ranges `x(2,4)` and the anchors `<` `>`
    have no fixed-length form and are refused (ValueError)."""
    if not isinstance(pattern, str):
        raise TypeError("a pattern is a string")
    text = pattern.strip()
    if text.endswith("."):
        text = text[:-1]
    if not text:
        raise ValueError("empty pattern")
    rows, i = [], 0

    def letters(body, what):
        if not body:
            raise ValueError(f"pattern, position {i + 1}: an empty {what}")
        cols = []
        for ch in body.upper():
            if ch not in _AA_COLUMN:
                raise ValueError(f"pattern, position {i + 1}: {ch!r} is none of {AMINO_ACIDS}" + (" (x stands alone)" if ch == "X" else ""))
            cols.append(_AA_COLUMN[ch])
        return cols

    while i < len(text):
        ch = text[i]
        if ch == "-":
            i += 1
            continue
        row = np.full(len(AMINO_ACIDS), -1, dtype=np.int64)
        if ch in "[{":
            close = text.find("]" if ch == "[" else "}", i)
            if close < 0:
                raise ValueError(f"pattern, position {i + 1}: {ch!r} is not closed")
            cols = letters(text[i + 1:close], "set")
            if ch == "[":
                row[cols] = 0
            else:
                row[:] = 0
                row[cols] = -1
            end = close + 1
        elif ch in "xX":
            row[:] = 0
            end = i + 1
        else:
            row[letters(ch, "element")] = 0
            end = i + 1
        n = 1
        if end < len(text) and text[end] == "(":
            close = text.find(")", end)
            count = text[end + 1:close] if close > 0 else ""
            if not count.isdigit() or int(count) < 1:
                raise ValueError(f"pattern, position {end + 1}: a repeat count is one positive number, as in x(3)")
            n, end = int(count), close + 1
        rows += [row] * n
        if len(rows) > PROT_MAX_ROWS:
            raise ValueError(f"the pattern has more than {PROT_MAX_ROWS} positions")
        i = end
    if not rows:
        raise ValueError("empty pattern")
    return np.stack(rows), len(rows)


def prot_matrix_from_sequences(aa_seqs, *, pseudocount: float = 1.0, background=None, scale: float = 100) -> np.ndarray:
    """Log-odds amino-acid profile of equal-length example peptides (the 20 amino-acid letters, either case): the (m, 21)
    int64 array whose first 20 columns are np.rint(scale * log2(((count + pseudocount * bg) / (n + pseudocount)) / bg)) in
    the order of AMINO_ACIDS and whose stop column is the row's minimum.  `background`: 20 positive probabilities that sum to
    1 (None: 1/20 each).  With scale = 100 the weights are centibits, like pwm_from_sequences'.  ValueError when a weight
    leaves the int16 range (a count of 0 without a pseudocount, a scale too large)."""
    rows = []
    for q in aa_seqs:
        s = (q.decode("ascii", "replace") if isinstance(q, (bytes, bytearray)) else q).upper() if isinstance(q, (str, bytes, bytearray)) else None
        if s is None:
            raise TypeError("a peptide is a str or bytes")
        rows.append(s)
    if not rows:
        raise ValueError("need at least one sequence")
    m = len(rows[0])
    if not 1 <= m <= PROT_MAX_ROWS:
        raise ValueError(f"the sequences have {m} residues (1 ... {PROT_MAX_ROWS})")
    if any(len(r) != m for r in rows):
        raise ValueError("the sequences differ in length")
    bg = np.full(20, 0.05) if background is None else np.asarray(background, dtype=np.float64)
    if bg.shape != (20,) or not np.isfinite(bg).all() or (bg <= 0).any() or not math.isclose(float(bg.sum()), 1.0, rel_tol=0, abs_tol=1e-9):
        raise ValueError("background: twenty positive probabilities (ACDEFGHIKLMNPQRSTVWY) that sum to 1")
    if not (math.isfinite(pseudocount) and pseudocount >= 0 and math.isfinite(scale) and scale > 0):
        raise ValueError("pseudocount must be >= 0 and scale > 0")
    count = np.zeros((m, 20), dtype=np.float64)
    for r in rows:
        for i, ch in enumerate(r):
            if _AA_COLUMN.get(ch, 20) >= 20:
                raise ValueError("the sequences may hold the 20 amino-acid letters only")
            count[i, _AA_COLUMN[ch]] += 1
    with np.errstate(divide="ignore"):
        w = np.rint(scale * np.log2(((count + pseudocount * bg) / (len(rows) + pseudocount)) / bg))
    if not np.isfinite(w).all() or (w < PWM_WEIGHT_MIN).any() or (w > PWM_WEIGHT_MAX).any():
        i = int(np.argwhere(~np.isfinite(w) | (w < PWM_WEIGHT_MIN) | (w > PWM_WEIGHT_MAX))[0][0])
        raise ValueError(f"row {i + 1}: a weight leaves {PWM_WEIGHT_MIN} ... {PWM_WEIGHT_MAX} (give a pseudocount or a smaller scale)")
    w = w.astype(np.int64)
    return np.concatenate([w, w.min(axis=1, keepdims=True)], axis=1)


def prot_fold(matrix, *, genetic_code=1, x_weight=None, minus: bool = False) -> np.ndarray:
    """The (m, 65) codon matrix kgma_codon_match searches one strand with (kgma_codon_fold): entry 16 b0 + 4 b1 + b2 of row i
    is matrix[i][amino acid of the codon]; entry 64, a codon with an N, is x_weight[i] -- by default the row's minimum over
    its 21 columns, so an assembly gap never looks like a signal.  minus: the matrix of the other strand (rows reversed,
    each codon read as its reverse complement)."""
    a = _prot_matrix(matrix)
    x = a.min(axis=1) if x_weight is None else np.asarray(x_weight, dtype=np.int64)
    return _lib.codon_fold(a, _code_of(genetic_code), x, minus)


def prot_score_distribution(matrix, background=_UNIFORM, genetic_code=1):
    """(lowest, p): p[k] is the probability that m independent codons score lowest + k, a codon's probability being the
    product of its three base frequencies in `background` (A, C, G, T) -- exactly, on the integer lattice, one convolution
    per row."""
    a, bg, col = _prot_matrix(matrix), _background(background), _code_of(genetic_code)
    c = np.arange(64)
    pc = bg[c >> 4] * bg[(c >> 2) & 3] * bg[c & 3]
    total, p = 0, np.ones(1, dtype=np.float64)
    for row in a:
        w = row[col]                                             # the weight of each codon
        base = int(w.min())
        mass = np.bincount(w - base, weights=pc)
        p = np.convolve(p, mass)
        total += base
    return total, p


def prot_threshold(matrix, pvalue: float, background=_UNIFORM, genetic_code=1) -> int:
    """The smallest integer t with P(score >= t) <= pvalue for independent codons of independent bases drawn from `background`
    (A, C, G, T; the default is uniform), from the exact score distribution (prot_score_distribution).  One above the highest
    score when even that one is likelier than pvalue."""
    if not 0 < float(pvalue) < 1:
        raise ValueError("pvalue must lie strictly between 0 and 1")
    lowest, p = prot_score_distribution(matrix, background, genetic_code)
    tail = np.cumsum(p[::-1])[::-1]
    ok = np.flatnonzero(tail <= float(pvalue))
    return lowest + (int(ok[0]) if ok.size else p.size)


def _prot_args(profiles, threshold, max_mismatch, pvalue, strand, code, background=None):
    _check_strand(strand)
    given = [x is not None for x in (threshold, max_mismatch, pvalue)]
    is_pattern = [isinstance(p, str) for p in profiles]
    if sum(given) > 1 or (sum(given) == 0 and not all(is_pattern)):
        raise ValueError("give exactly one of threshold, max_mismatch and pvalue (a pattern alone means max_mismatch=0)")
    if max_mismatch is not None and not all(is_pattern):
        raise ValueError("max_mismatch counts the mismatches of a pattern: give a matrix a threshold or a pvalue")
    ms = [prot_pattern(p)[0] if isinstance(p, str) else _prot_matrix(p, f"profile {i}") for i, p in enumerate(profiles)]

    def per_matrix(x, what, conv):
        if isinstance(x, (int, float, np.integer, np.floating)):
            return [conv(x)] * len(ms)
        xs = [conv(v) for v in x]
        if len(xs) != len(ms):
            raise ValueError(f"need one {what} per profile")
        return xs

    if pvalue is not None:
        bg = _UNIFORM if background is None else background
        ts = [prot_threshold(m, x, bg, code) for m, x in zip(ms, per_matrix(pvalue, "pvalue", float))]
    elif threshold is not None:
        ts = per_matrix(threshold, "threshold", int)
    else:
        ds = per_matrix(0 if max_mismatch is None else max_mismatch, "max_mismatch", int)
        for i, (m, d) in enumerate(zip(ms, ds)):
            informative = int((m.min(axis=1) < 0).sum())
            if not 0 <= d < informative:
                raise ValueError(f"pattern {i}: max_mismatch {d} must be at least 0 and smaller than its {informative} positions other than x")
        ts = [-d for d in ds]
    sent, tags = [], []
    for i, (m, t) in enumerate(zip(ms, ts)):
        plus = prot_fold(m, genetic_code=code)
        lowest = int(plus.min(axis=1).sum())
        if t <= lowest:
            raise ValueError(f"profile {i}: threshold {t} does not exceed the sum of its row minima, {lowest}: every start would match")
        if not t < 2 ** 31:
            raise ValueError(f"profile {i}: threshold {t} does not fit an int32")
        # the minus strand: the matrix folded for it, on the SAME genome, in the same pass
        if strand != "-":
            sent.append((plus, t)); tags.append((i, "+"))
        if strand != "+":
            sent.append((prot_fold(m, genetic_code=code, minus=True), t)); tags.append((i, "-"))
    return ms, sent, tags


def _prot_run(ctx, g, ms, sent, tags) -> list:
    """Per profile the hits (record, lo, hi, strand, frame, score), sorted by (record, lo, strand)."""
    ctx.codon_match(g, [m for m, _ in sent], [t for _, t in sent])
    out = [[] for _ in ms]
    length = {}
    for h in ctx.codon_matches().tolist():
        i, st = tags[h[0]]
        c, lo = h[1], h[2]
        hi = lo + 3 * ms[i].shape[0] - 1
        if st == "+":
            frame = (lo - 1) % 3 + 1
        else:
            if c not in length:
                length[c] = g.contig_len(c)
            frame = -((length[c] - hi) % 3 + 1)
        out[i].append((c, lo, hi, st, frame, h[3]))
    for lst in out:
        lst.sort(key=lambda t: (t[0], t[1], t[3]))              # ("+" sorts before "-")
    return out


def _prot_checked(profiles, threshold, max_mismatch, pvalue, strand, genetic_code, background):
    """The argument checks of protMatch, made before the device is touched: (profiles, genetic code, background)."""
    profiles, bg, code = list(profiles), _pwm_background(background, None if pvalue is not None else 0), _code_of(genetic_code)
    _prot_args(profiles, threshold, max_mismatch, pvalue, strand, code, None if isinstance(bg, str) else bg)
    return profiles, code, bg


def _prot_search(ctx, g, profiles, threshold, max_mismatch, pvalue, strand, code, bg) -> list:
    if isinstance(bg, str):                                      # "genome": the open subject's own composition
        bg = genome_background(g, ctx=ctx)
    return _prot_run(ctx, g, *_prot_args(profiles, threshold, max_mismatch, pvalue, strand, code, bg))


def protMatch_batch(profiles, genome_or_path, *, threshold=None, max_mismatch=None, pvalue=None, strand: str = "+", genetic_code=1,
                    background=None, ctx=None) -> list:
    """Many profiles or patterns, on the strands asked for, in ONE pass over the genome (kgma_codon_match): per profile the
    list of (record_index, identifier, lo, hi, strand, frame, score) -- 0-based record, 1-based inclusive nucleotide lo:hi in
    forward coordinates -- sorted by (record, lo, strand).  `threshold` / `max_mismatch` / `pvalue`: one number for all or
    one per profile.  Semantics: protMatch.  `genome_or_path`: a FASTA or .2bit path, or a device genome that is already open
    (it stays open)."""
    profiles, code, bg = _prot_checked(profiles, threshold, max_mismatch, pvalue, strand, genetic_code, background)
    if not isinstance(genome_or_path, (str, _GenomeView, _lib.Genome)):
        raise TypeError("Invalid subject sequence type")
    ctx = ctx or default_context()
    g, src, owned = _open_subject(ctx, genome_or_path)
    try:
        res = _prot_search(ctx, g, profiles, threshold, max_mismatch, pvalue, strand, code, bg)
        ids = {c: _identifier(src, c) for c in {t[0] for lst in res for t in lst}}
    finally:
        if owned:
            g.free()
    return [[(c, ids[c], lo, hi, st, fr, sc) for c, lo, hi, st, fr, sc in lst] for lst in res]


def protMatch(profile_or_pattern, subject, *, threshold=None, max_mismatch=None, pvalue=None, strand: str = "+", genetic_code=1,
              background=None, ctx=None):
    """Every place of the subject that could encode the protein signal, in every reading frame of the strands asked for.
    `profile_or_pattern`: a PROSITE-style pattern string (prot_pattern; score = -mismatches) or an amino-acid profile of
    1 ... 64 rows of 21 integer weights (AMINO_ACIDS: ACDEFGHIKLMNPQRSTVWY and '*', the stop; each -32768 ... 32767).  Laid at
    the nucleotide start s, score(s) = sum over the rows i of profile[i][amino acid of the codon t[s + 3i .. s + 3i + 2]];
    every start is scored, so the three frames of a strand are found in one pass, overlapping places included, none spanning
    two records.  Case is folded.  A codon that holds an N is the amino acid X and scores its row's minimum over the 21
    columns -- also where all four bases give the same amino acid: CTN is X, not Leu.  The subject may hold A/C/G/T/N only
    (KgmaError KGMA_E_BADBASE otherwise).
    Give one of `threshold` (an integer that exceeds the sum of the row minima), `max_mismatch` (patterns only: the threshold
    -d; d smaller than the number of positions other than x; a pattern with none of the three means 0) and `pvalue` (the
    threshold becomes prot_threshold(profile, pvalue, background, genetic_code); `background` None is uniform, four
    probabilities (A, C, G, T) are used as given, "genome" is genome_background(subject)).  `genetic_code`: genetic_code()'s
    argument.
    strand: "+" as written; "-" the profile read on the reverse complement -- the codon matrix folded for the minus strand,
    searched on the same genome -- reported at the forward lo:hi it covers; "both" the two together.  frame is
    (lo - 1) mod 3 + 1 on the plus strand and -((L - hi) mod 3 + 1) on the minus strand, L the record's length: translate's.
    A `subject` of residues (bytes, or a Record) returns [(lo, hi, strand, frame, score)] sorted by (lo, strand); a FASTA or
    .2bit path or an open device genome returns protMatch_batch(...)[0].  An empty list when there is no hit.
    A profile of rows 0 for every amino acid and -1 for the stop, at threshold 0, finds every stop-free stretch of m codons."""
    if isinstance(subject, (Record, bytes, bytearray, memoryview)):
        profiles, code, bg = _prot_checked([profile_or_pattern], threshold, max_mismatch, pvalue, strand, genetic_code, background)
        seq = bytes(subject.sequence if isinstance(subject, Record) else subject)
        ctx = ctx or default_context()
        g = ctx.genome_from_host([seq])
        try:
            res = _prot_search(ctx, g, profiles, threshold, max_mismatch, pvalue, strand, code, bg)[0]
        finally:
            g.free()
        return [(lo, hi, st, fr, sc) for _, lo, hi, st, fr, sc in res]
    return protMatch_batch([profile_or_pattern], subject, threshold=threshold, max_mismatch=max_mismatch, pvalue=pvalue, strand=strand,
                           genetic_code=genetic_code, background=background, ctx=ctx)[0]


# ---- threshold calibration (kgma_window_dists, kgma_mutation_dists): the working form of src/DistanceTesting.jl --------------

_M64 = (1 << 64) - 1
_GOLDEN64 = 0x9E3779B97F4A7C15
# mutation_dict (src/DistanceTesting.jl:38-42), in its order
_MUT = {ord("A"): b"CGT", ord("C"): b"AGT", ord("G"): b"CAT", ord("T"): b"CGA"}


def _mix64(z):
    """The splitmix64 finaliser on numpy uint64 (scalars or arrays; wraps mod 2^64)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _seq_bytes(seq) -> bytes:
    if isinstance(seq, Record):
        return bytes(seq.sequence)
    return seq.encode() if isinstance(seq, str) else bytes(seq)


def mutate_seq(seq, mut_rate, *, seed: int = 42, stream=(0, 0, 0)) -> bytes:
    """`mutate_seq` (src/DistanceTesting.jl:57-67): a copy of `seq` in which every residue is substituted with probability
    `mut_rate` by one of the three other bases, in mutation_dict's order.  The host mirror of the rule kgma_mutation_dists
    applies on the device (kgma.h): `stream` = (i, r, t) is the (sequence, rate, trial) index of the copy, so
    mutation_dists(seqs, ...)[i, r, t] is the distance of mutate_seq(seqs[i], rates[r], seed=seed, stream=(i, r, t)).
    An unsubstituted residue keeps its byte (and case); a substituted one is upper case.  A residue outside A/C/G/T (either
    case) raises KeyError, substituted or not (the reference looks mutation_dict up only when it substitutes).

    DEVIATION (documented in DESIGN.md): the reference draws from Julia's global RNG (`rand(1)[1] <= mut_rate`;
    `rand(mutation_dict[...])`), which cannot be reproduced outside Julia.  This uses a counter-based hash of (seed, stream,
    position), so the result agrees statistically but not bitwise."""
    s = _seq_bytes(seq)
    rate = float(mut_rate)
    if not (0.0 <= rate <= 1.0):
        raise ValueError(f"mut_rate = {mut_rate} is not in [0, 1]")
    a = np.frombuffer(s, dtype=np.uint8)
    up = a & 0xDF
    ok = (up == 65) | (up == 67) | (up == 71) | (up == 84)
    if not bool(ok.all()):
        j = int(np.flatnonzero(~ok)[0])
        raise KeyError(f"position {j + 1}: residue {s[j:j + 1]!r} is not one of A/C/G/T (mutation_dict has no other key)")
    G = np.uint64(_GOLDEN64)
    with np.errstate(over="ignore"):
        K = np.uint64(int(seed) & _M64)
        for idx in stream:
            K = _mix64(K + G * np.uint64(int(idx) + 1))
        z = _mix64(K + G * np.arange(1, a.size + 1, dtype=np.uint64))
    P = np.uint64(int(np.floor(np.ldexp(rate, 53))))
    hit = (z >> np.uint64(11)) < P
    pick = (((z & np.uint64(0x7FF)) * np.uint64(3)) >> np.uint64(11)).astype(np.int64)
    lut = np.zeros((256, 3), dtype=np.uint8)
    for b, row in _MUT.items():
        lut[b] = np.frombuffer(row, dtype=np.uint8)
    out = a.copy()
    out[hit] = lut[up[hit], pick[hit]]
    return out.tobytes()


def sample_window_starts(record_lens, W: int, n_samples: int, seed: int):
    """(contig, start): windows of W residues drawn from the records of the given lengths -- 0-based record (int32), 1-based
    start (int64).  The valid windows are all (record, s) with 1 <= s <= L - W + 1; a record shorter than W has none.  At most
    `n_samples` of them: every one once, in order.  Otherwise `np.random.default_rng(seed).integers(0, total, n_samples)`
    mapped through the records' cumulative window counts, sorted (duplicates stay).  A pure host function."""
    lens = np.asarray(list(record_lens), dtype=np.int64)
    counts = np.maximum(lens - int(W) + 1, 0)
    cum = np.cumsum(counts)
    total = int(cum[-1]) if cum.size else 0
    if total <= int(n_samples):
        draws = np.arange(total, dtype=np.int64)
    else:
        draws = np.sort(np.random.default_rng(seed).integers(0, total, int(n_samples)).astype(np.int64))
    contig = np.searchsorted(cum, draws, side="right")
    start = draws - (cum[contig] - counts[contig]) + 1 if draws.size else draws
    return contig.astype(np.int32), start.astype(np.int64)


def off_lattice_threshold(est: float, scale: float) -> float:
    """The threshold halfway between the two attainable distances around `est`: an S/N KFV's distances are the lattice
    D / scale (D an integer, scale = 2 k N^2: Context.kfv_scale), and (floor(est * scale) + 0.5) / scale decides exactly the
    windows `est` decides unless est lies on the lattice itself -- then the windows AT est count as below -- while no window
    lies within the 2^-30 guard band of it ("at threshold", kgma_set_refs)."""
    return (math.floor(est * scale) + 0.5) / scale


def _calib_subject(ctx, genome_or_path):
    if not isinstance(genome_or_path, (str, _GenomeView, _lib.Genome)):
        raise TypeError("expected a FASTA or .2bit path or an open device genome")
    g, _src, owned = _open_subject(ctx, genome_or_path)
    return g, owned


def window_dists(genome_or_path, RV, windowsize: int, k: int, contig, start, *, n_refs: Optional[int] = None, ctx=None):
    """(D, dist) of the windows of `windowsize` residues at `start[i]` (1-based) of record `contig[i]` (0-based) to the KFV
    `RV`: kgma_window_dists.  `genome_or_path`: a FASTA path, a .2bit path or an open device genome (it stays open; pass
    Genome.revcomp() for the minus strand, in its own coordinates).  Answers "how far off is this locus?" without a
    whole-genome scan.  Sets the context's references to (RV, windowsize)."""
    ctx = ctx or default_context()
    ctx.set_refs(int(k), [np.asarray(RV, dtype=np.float64)], [int(windowsize)], [1.0], None if n_refs is None else [int(n_refs)])
    g, owned = _calib_subject(ctx, genome_or_path)
    try:
        return ctx.window_dists(g, 1, contig, start)
    finally:
        if owned:
            g.free()


def estimate_threshold_from_genome(genome_or_path, RV, windowsize, k: int, *, n_samples: int = 100_000, seed: int = 42,
                                   buffer: float = 8, quantile: Optional[float] = None, off_lattice: bool = True,
                                   n_refs=None, ctx=None):
    """estimate_optimal_threshold (src/DistanceTesting.jl:8-32) with the genome's own windows in the place of `randdnaseq`:
    the mean distance to the KFV of `n_samples` windows drawn from the genome (sample_window_starts; all of them when the
    genome has no more), minus `buffer` -- math.fsum(d) / n - buffer, independent of order.  A real genome is not uniform
    (repeats, skewed composition, runs of N that the scan counts as T), so this is the distribution the scan actually tests.
    quantile=q (0 < q <= 1): instead the ceil(q n)-th smallest sampled distance minus `buffer`, no interpolation.
    `RV` and `windowsize` may be lists (the cluster case; every KFV with its own window size and the same draw rule): a list
    is returned then.  off_lattice (default) with an S/N KFV: the result is moved to (floor(est * scale) + 0.5) / scale,
    halfway between two attainable distances, so that no window can be "at threshold" in kgma_set_refs's sense and the chain
    replay has no pair to decide.  Pass the result as KmerDistThr / KmerDistThrs; findGenes' own default
    stays estimate_optimal_threshold.  Sets the context's references."""
    many = isinstance(windowsize, (list, tuple, np.ndarray))
    RVs = [np.asarray(r, dtype=np.float64) for r in (RV if many else [RV])]
    Ws = [int(w) for w in (windowsize if many else [windowsize])]
    if len(RVs) != len(Ws):
        raise ValueError("need one window size per KFV")
    if quantile is not None and not (0.0 < float(quantile) <= 1.0):
        raise ValueError(f"quantile = {quantile} is not in (0, 1]")
    nr = None if n_refs is None else [int(x) for x in (n_refs if many else [n_refs])]
    ctx = ctx or default_context()
    ctx.set_refs(int(k), RVs, Ws, [1.0] * len(Ws), nr)
    g, owned = _calib_subject(ctx, genome_or_path)
    out = []
    try:
        lens = [g.contig_len(c) for c in range(g.n_contigs)]
        for j, W in enumerate(Ws):
            contig, start = sample_window_starts(lens, W, n_samples, seed)
            if contig.size == 0:
                raise ValueError(f"no record holds a window of {W} residues")
            _D, d = ctx.window_dists(g, j + 1, contig, start)
            n = int(d.size)
            if quantile is None:
                est = math.fsum(d.tolist()) / n - buffer
            else:
                est = float(np.sort(d)[math.ceil(float(quantile) * n) - 1]) - buffer
            if off_lattice and not ctx.kfv_is_float(j + 1):
                scale = ctx.kfv_scale(j + 1)
                est = off_lattice_threshold(est, scale)
            out.append(est)
    finally:
        if owned:
            g.free()
    return out if many else out[0]


def mutation_dists(ref_path_or_seqs, RV, k: int, *, rates=None, n_trials: int = 42, seed: int = 42,
                   n_refs: Optional[int] = None, ctx=None) -> np.ndarray:
    """The working form of gen_sub_vs_ref (src/DistanceTesting.jl:69-84, which refers to an undefined `vgene`): for every
    sequence i (the records of a FASTA path, or a list of bytes / str / Record), rate r and trial t the distance
    kmer_dist(mutate_seq(seq_i, rates[r]), RV, k), as a Float64 array [n_seqs, n_rates, n_trials] -- how far a gene may have
    diverged and still fall below a threshold.  One device call (kgma_mutation_dists); the mutated copies are never
    materialised, and entry [i, r, t] is reproduced on the host by mutate_seq(seq_i, rates[r], seed=seed, stream=(i, r, t)).
    rates: default 0:0.0125:1.  Sets the context's references."""
    if rates is None:
        rates = np.arange(0, 1 + 1e-9, 0.0125)
    rates = np.asarray(rates, dtype=np.float64)
    seqs = [r.sequence for r in read_fasta(ref_path_or_seqs)] if isinstance(ref_path_or_seqs, str) else [_seq_bytes(s) for s in ref_path_or_seqs]
    ctx = ctx or default_context()
    # (the window size plays no part here: a sequence's own length decides its number of k-mers)
    ctx.set_refs(int(k), [np.asarray(RV, dtype=np.float64)], [int(k) + 1], [1.0], None if n_refs is None else [int(n_refs)])
    return ctx.mutation_dists(seqs, 1, rates, n_trials, seed)[1]


def gen_sub_vs_ref(num_seeds: int = 42, stepsize: float = 0.0125, *, k: int = 6, RKV: str, ctx=None) -> np.ndarray:
    """`gen_sub_vs_ref` (src/DistanceTesting.jl:69-84) with the reference's signature: the reference file's own sequences
    against its KFV, [n_seqs, n_rates, num_seeds] (trial t stands for the reference's seed t + 1)."""
    return mutation_dists(RKV, refprep.gen_ref_ws_cons(RKV, k)[0], k, rates=np.arange(0, 1 + 1e-9, stepsize), n_trials=num_seeds, ctx=ctx)


# ---- the same for the strobemer engine (kgma_strobe_window_dists, kgma_strobe_mutation_dists) ------------------------------------
# Strobemer_findGenes says "there is not distance threshold estimation yet"; its default KmerDistThr = 30 is the k-mer engine's.

def strobe_window_dists(genome_or_path, RV, windowsize: int, contig, start, *, s: int, w_min: int, w_max: int, q: int,
                        n_refs: Optional[int] = None, ctx=None):
    """(D, dist) of the strobemer scan's windows with start `start[i]` (1-based) of record `contig[i]` (0-based) to the
    strobemer KFV `RV` (gen_ref_ws_cons_strobe): kgma_strobe_window_dists.  A window is what StrobeGMA!'s count vector holds
    after step start - 1: W - k + 1 randstrobes (k = w_max + s - 1), for start >= 2 the W - k that start at start ..
    start + W - k - 1 plus the record's randstrobe W - k + 1, which never leaves.  Valid starts: 1 ... max(1, L - W) on a
    record of L >= W residues.  dist is on the engine's scale, D / (2 k N^2): the numbers KmerDistThr is compared with.
    `genome_or_path` as window_dists.  Sets the context's reference to (RV, windowsize)."""
    ctx = ctx or default_context()
    ctx.set_strobe_ref(s, w_min, w_max, q, np.asarray(RV, dtype=np.float64), int(windowsize), 1.0, n_refs)
    g, owned = _calib_subject(ctx, genome_or_path)
    try:
        return ctx.strobe_window_dists(g, contig, start)
    finally:
        if owned:
            g.free()


def estimate_strobe_threshold_from_genome(genome_or_path, RV, windowsize, *, s: int, w_min: int, w_max: int, q: int,
                                          n_samples: int = 100_000, seed: int = 42, buffer: float = 0,
                                          quantile: Optional[float] = None, off_lattice: bool = True, n_refs=None, ctx=None):
    """estimate_threshold_from_genome for the strobemer engine, by its rules: math.fsum(d) / n - buffer over the distances of
    `n_samples` of the genome's own windows (all of them when it has no more), or with quantile=q (0 < q <= 1) the
    ceil(q n)-th smallest minus `buffer`; then off_lattice_threshold on the engine's scale 2 k N^2, k = w_max + s - 1.  The
    windows are drawn by sample_window_starts(lens, W + 1, ...): windows of W + 1 residues have exactly the scan's valid starts
    1 .. L - W (a record of exactly W residues has its first window only, which the scan never tests: it is not drawn).
    buffer defaults to 0, not to the 8 of estimate_optimal_threshold: that figure was chosen for the k-mer distance, the
    strobemer distance lives on another lattice (4^(2s) bins, scale 2 (w_max + s - 1) N^2), and nothing has been measured
    for it.  Pass the result as KmerDistThr of Strobemer_findGenes.  Sets the context's reference."""
    if quantile is not None and not (0.0 < float(quantile) <= 1.0):
        raise ValueError(f"quantile = {quantile} is not in (0, 1]")
    W = int(windowsize)
    ctx = ctx or default_context()
    ctx.set_strobe_ref(s, w_min, w_max, q, np.asarray(RV, dtype=np.float64), W, 1.0, None if n_refs is None else int(n_refs))
    g, owned = _calib_subject(ctx, genome_or_path)
    try:
        lens = [g.contig_len(c) for c in range(g.n_contigs)]
        contig, start = sample_window_starts(lens, W + 1, n_samples, seed)
        if contig.size == 0:
            raise ValueError(f"no record holds a tested window of {W} residues (none is longer than {W})")
        _D, d = ctx.strobe_window_dists(g, contig, start)
        n = int(d.size)
        if quantile is None:
            est = math.fsum(d.tolist()) / n - buffer
        else:
            est = float(np.sort(d)[math.ceil(float(quantile) * n) - 1]) - buffer
        return off_lattice_threshold(est, ctx.kfv_scale(1)) if off_lattice else est
    finally:
        if owned:
            g.free()


def strobe_mutation_dists(ref_path_or_seqs, RV, *, s: int, w_min: int, w_max: int, q: int, rates=None, n_trials: int = 42,
                          seed: int = 42, n_refs: Optional[int] = None, ctx=None) -> np.ndarray:
    """mutation_dists for the strobemer engine: for every sequence i, rate r and trial t the distance of the strobemer KFV `RV`
    to the randstrobe counts of mutate_seq(seq_i, rates[r], seed=seed, stream=(i, r, t)), on the engine's scale
    1 / (2 (w_max + s - 1)), as a Float64 array [n_seqs, n_rates, n_trials].  One device call (kgma_strobe_mutation_dists); the
    copies are never materialised.  rates: default 0:0.0125:1.  Sets the context's reference."""
    if rates is None:
        rates = np.arange(0, 1 + 1e-9, 0.0125)
    rates = np.asarray(rates, dtype=np.float64)
    seqs = [r.sequence for r in read_fasta(ref_path_or_seqs)] if isinstance(ref_path_or_seqs, str) else [_seq_bytes(x) for x in ref_path_or_seqs]
    ctx = ctx or default_context()
    # (the window size plays no part here: a sequence's own length decides its number of randstrobes)
    ctx.set_strobe_ref(s, w_min, w_max, q, np.asarray(RV, dtype=np.float64), int(w_max) + int(s), 1.0, n_refs)
    return ctx.strobe_mutation_dists(seqs, rates, n_trials, seed)[1]


def test_strobe_2_mer_dists(Rkv: str, num_seeds: int = 42, stepsize: float = 0.0125, *, s: int = 2, w_min: int = 3, w_max: int = 5,
                            q: int = 5, ctx=None) -> np.ndarray:
    """`test_strobe_2_mer_dists` (src/StrobemerGMA/MonteCarloBenchmark.jl:2-23) with the reference's signature, finished: RKV
    is the randstrobe count of the file's FIRST record (N = 1; the engine's ungapped_strobe_2_mer_count -- the reference's
    `strobe_2_mer_count` is not defined), and that record stands for the `vgene` the reference leaves undefined.  Returns a Float64 array [n_rates, num_seeds], rates 0:stepsize:1 (column t stands for the reference's seed
    t + 1; row 0, rate 0, is the record's distance to itself: 0).  Values are on the engine's scale 1 / (2 k), k = w_max + s - 1;
    the reference multiplies by 1 / (2 getK(RKV)) = 1 / (4 s) instead: its figure is this one times k / (2 s)."""
    rec = read_fasta(Rkv)[0].sequence
    RKV = refprep.ungapped_strobe_2_mer_count(rec, s, w_min, w_max, q)
    d = strobe_mutation_dists([rec], RKV, s=s, w_min=w_min, w_max=w_max, q=q, rates=np.arange(0, 1 + 1e-9, stepsize),
                              n_trials=num_seeds, n_refs=1, ctx=ctx)
    return d[0]


test_strobe_2_mer_dists.__test__ = False          # (the reference's name; not a pytest test)


# ---- gene assignment: which reference gene is each hit closest to? (kgma_assign_seqs, kgma_assign_ranges) -----------------------
class Assignment(NamedTuple):
    """One reference a hit was aligned to (the hit aligner's model, reference global, the hit's ends free)."""
    ref_id: str          # the reference's FASTA identifier ("" for references given as bare sequences)
    ref_index: int       # 0-based position in the reference batch
    score: int           # optimum semi-global score
    identity: float      # n_eq / (n_eq + n_x + n_ins + n_del); 0.0 when the alignment has no such column
    n_eq: int            # '=' columns
    n_x: int             # 'X' columns
    n_ins: int           # 'I' columns: a reference residue against a gap
    n_del: int           # 'D' columns inside the alignment (the hit's free overhang at either end is not counted)
    q_lo: int            # the hit's residues q_lo .. q_hi (1-based) are what lies between the two overhangs
    q_hi: int


def _assignment(ref_id: str, ref: int, score: int, n_eq: int, n_x: int, n_ins: int, n_del: int, q_lo: int, q_hi: int) -> Assignment:
    d = n_eq + n_x + n_ins + n_del
    return Assignment(ref_id, ref, score, n_eq / d if d else 0.0, n_eq, n_x, n_ins, n_del, q_lo, q_hi)


def _assign_refs(ref_path_or_seqs):
    """(identifiers, sequences) of a reference FASTA path or a list of Record / bytes / str."""
    recs = read_fasta(ref_path_or_seqs) if isinstance(ref_path_or_seqs, str) else list(ref_path_or_seqs)
    ids, seqs = [], []
    for r in recs:
        if isinstance(r, Record):
            parts = r.description.split(None, 1)
            ids.append(parts[0] if parts else "")
        else:
            ids.append("")
        seqs.append(_seq_bytes(r))
    if not seqs:
        raise ValueError("no reference sequences")
    return ids, seqs


def _assignments(ids, out) -> list:
    return [[_assignment(ids[int(a["ref"])], *(int(a[f]) for f in ("ref", "score", "n_eq", "n_x", "n_ins", "n_del", "q_lo", "q_hi")))
             for a in row] for row in out]


def annotated_header(description: str, best: Assignment) -> str:
    """A hit's header with its best reference appended after the last existing field (a minus-strand hit's ` | Strand = -`
    included): ` | Ref = <id> | Identity = <3 decimals>`."""
    return f"{description} | Ref = {best.ref_id} | Identity = {best.identity:.3f}"


def _check_prescreen(prescreen, top: int, n_refs: int) -> None:
    if isinstance(prescreen, bool) or not isinstance(prescreen, (int, np.integer)):
        raise ValueError(f"prescreen = {prescreen!r} is neither None nor an integer")
    if not int(top) <= int(prescreen) <= min(n_refs, _lib.KMAT_MAX_NEAR):
        raise ValueError(f"prescreen = {prescreen} is not one of top = {top} .. {min(n_refs, _lib.KMAT_MAX_NEAR)} "
                         f"(min(number of references, {_lib.KMAT_MAX_NEAR}))")


def assignGenes(hits, ref_path_or_seqs, *, top: int = 1, gap_open_score: int = -69, gap_extend_score: int = -1,
                annotate: bool = False, prescreen: Optional[int] = None, prescreen_k: int = 6, ctx=None):
    """Names every hit's nearest reference genes.  `hits`: the records findGenes / findGenes_cluster_mode / Strobemer_findGenes
    return (or bare sequences); their bodies are the queries -- a minus-strand hit's body is already in reference orientation,
    so both strands work without coordinates.  `ref_path_or_seqs`: a FASTA path or a list of Record / bytes / str.  Every hit
    is scored against every reference on the device (kgma_assign_seqs), its `top` references -- higher score first, the earlier
    reference among equal scores -- are aligned with a traceback, and per hit the list of their Assignment tuples is returned.
    annotate=True returns instead copies of the records with ` | Ref = <id> | Identity = <x.xxx>` of the best reference
    appended to the header (hits must be records then).
    prescreen=n (top <= n <= min(number of references, 128)) aligns a hit only against its n nearest references by k-mer
    distance at k = prescreen_k (kgma_assign_seqs_screened): what is returned is then the best among those candidates, and a
    residue outside A/C/G/T/N raises BadBaseError where the unscreened call counts it as N.  None is the unscreened call."""
    hits = list(hits)
    ids, seqs = _assign_refs(ref_path_or_seqs)
    if not 1 <= int(top) <= len(seqs):
        raise ValueError(f"top = {top} is not one of 1 .. {len(seqs)} (the number of references)")
    if prescreen is not None:
        _check_prescreen(prescreen, top, len(seqs))
    if annotate and not all(isinstance(h, Record) for h in hits):
        raise TypeError("annotate=True needs hit records")
    queries = [_seq_bytes(h) for h in hits]
    if not hits:
        return []
    ctx = ctx or default_context()
    if prescreen is None:
        out, _ = ctx.assign_seqs(seqs, queries, gap_open_score, gap_extend_score, int(top))
    else:
        out = ctx.assign_seqs_screened(seqs, queries, gap_open_score, gap_extend_score, int(top), int(prescreen_k), int(prescreen))[0]
    res = _assignments(ids, out)
    if annotate:
        return [Record(annotated_header(h.description, a[0]), h.sequence) for h, a in zip(hits, res)]
    return res


def assign_ranges(genome_or_path, contig, lo, hi, ref_path_or_seqs, *, top: int = 1, gap_open_score: int = -69,
                  gap_extend_score: int = -1, prescreen: Optional[int] = None, prescreen_k: int = 6, ctx=None) -> list:
    """assignGenes for ranges of a resident genome, which never leave the device: query i is residues lo[i] .. hi[i] (1-based
    inclusive) of record contig[i] (0-based) of `genome_or_path` -- a FASTA or .2bit path, or a device genome that is already
    open (it stays open), as for motifMatch.  Per range the list of its `top` Assignment tuples (kgma_assign_ranges).
    prescreen / prescreen_k: as in assignGenes (kgma_assign_ranges_screened)."""
    if not isinstance(genome_or_path, (str, _GenomeView, _lib.Genome)):
        raise TypeError("Invalid subject sequence type")
    ids, seqs = _assign_refs(ref_path_or_seqs)
    if not 1 <= int(top) <= len(seqs):
        raise ValueError(f"top = {top} is not one of 1 .. {len(seqs)} (the number of references)")
    if prescreen is not None:
        _check_prescreen(prescreen, top, len(seqs))
    ctx = ctx or default_context()
    g, _src, owned = _open_subject(ctx, genome_or_path)
    try:
        if prescreen is None:
            out, _ = ctx.assign_ranges(g, seqs, contig, lo, hi, gap_open_score, gap_extend_score, int(top))
        else:
            out = ctx.assign_ranges_screened(g, seqs, contig, lo, hi, gap_open_score, gap_extend_score, int(top), int(prescreen_k),
                                             int(prescreen))[0]
    finally:
        if owned:
            g.free()
    return _assignments(ids, out)


# ---- all-pairs k-mer distances (kgma_kmer_dist_matrix, kgma_kmer_nearest) ---------------------------------------------------------
def kmer_dist_matrix(seqs_a, seqs_b=None, k: int = 6, *, integer: bool = False, ctx=None) -> np.ndarray:
    """kmer_dist(a, b, k) (src/Kmers.jl:54-56) of every sequence of `seqs_a` to every sequence of `seqs_b`, on the device: the
    Float64 matrix [n_a, n_b], bit for bit the reference's values; integer=True returns instead the exact int32
    D = sum_x (c_a[x] - c_b[x])^2 (dist = (1 / 2k) * D).  Either side: a FASTA path or a list of Record / bytes / str.
    seqs_b=None: every sequence of A against every other (symmetric, zero diagonal).  1 <= k <= 10; sequences of at most
    32767 residues; a residue outside A/C/G/T/N raises BadBaseError (the reference's KeyError)."""
    _ids, a = _assign_refs(seqs_a)
    b = None if seqs_b is None else _assign_refs(seqs_b)[1]
    ctx = ctx or default_context()
    D, dist = ctx.kmer_dist_matrix(a, b, int(k))
    return D if integer else dist


def kmer_dist_matrix_ranges(genome_or_path, contig, lo, hi, ref_path_or_seqs, k: int = 6, *, integer: bool = False, ctx=None) -> np.ndarray:
    """kmer_dist_matrix with ranges of a resident genome as the A side: row i is residues lo[i] .. hi[i] (1-based inclusive;
    hi = lo - 1: empty) of record contig[i] (0-based) of `genome_or_path` -- a FASTA or .2bit path, or a device genome that is
    already open (it stays open), as for assign_ranges.  Only residues inside a requested range can raise BadBaseError."""
    if not isinstance(genome_or_path, (str, _GenomeView, _lib.Genome)):
        raise TypeError("Invalid subject sequence type")
    _ids, b = _assign_refs(ref_path_or_seqs)
    ctx = ctx or default_context()
    g, _src, owned = _open_subject(ctx, genome_or_path)
    try:
        D, dist = ctx.kmer_dist_matrix_ranges(g, contig, lo, hi, b, int(k))
    finally:
        if owned:
            g.free()
    return D if integer else dist


def nearest_refs(hits, ref_path_or_seqs, *, k: int = 6, n: int = 1, ctx=None) -> list:
    """Per hit (a record or a bare sequence) the list of its `n` nearest references by k-mer distance, nearest first, the earlier
    reference among equal distances: (ref_id, ref_index, dist) tuples.  The distance matrix never leaves the device
    (kgma_kmer_nearest)."""
    hits = list(hits)
    ids, seqs = _assign_refs(ref_path_or_seqs)
    if not 1 <= int(n) <= min(len(seqs), _lib.KMAT_MAX_NEAR):
        raise ValueError(f"n = {n} is not one of 1 .. {min(len(seqs), _lib.KMAT_MAX_NEAR)} (min(number of references, {_lib.KMAT_MAX_NEAR}))")
    queries = [_seq_bytes(h) for h in hits]
    if not hits:
        return []
    ctx = ctx or default_context()
    index, D = ctx.kmer_nearest(queries, seqs, int(k), int(n))
    half_inv_k = 1.0 / (2 * int(k))
    return [[(ids[int(r)], int(r), half_inv_k * float(d)) for r, d in zip(ri, di)] for ri, di in zip(index, D)]


# ---- distance landscape: bin minima and threshold sweep of a scan, reduced on the device ----
class LandscapeTrack(NamedTuple):
    """One record of api.dist_landscape.  The first three fields are the track: bin b covers the windows whose starts, in the
    scanned orientation, are b * bin + 2 .. min((b + 1) * bin + 1, L - W + 1) (window 1 is never tested); bin_argmin is the
    FORWARD start of the first window, in scan order, that attains bin_min."""
    identifier: str
    bin_min: np.ndarray
    bin_argmin: np.ndarray
    strand: str
    bin: int
    windowsize: int
    length: int


class ThresholdSweep(NamedTuple):
    thresholds: np.ndarray
    windows_below: np.ndarray
    dips_below: np.ndarray


def _landscape_scan(genome_or_path, RV, windowsize, k, n_refs, strand, ctx, reduce) -> None:
    """The single-engine scan with the distances kept on the device, per strand: reduce(view, strand) runs after each."""
    _check_strand(strand)
    # (any finite threshold serves: the distances do not depend on it, and only the device part of the scan runs)
    ctx.set_refs(int(k), [np.asarray(RV, dtype=np.float64)], [int(windowsize)], [1.0], None if n_refs is None else [int(n_refs)])
    owned = not isinstance(genome_or_path, _GenomeView)
    view = genome_or_path if not owned else _GenomeView(ctx, genome_or_path)

    def run(v, sd):
        ctx.scan_device(v.genome, _lib.MODE_SINGLE, _lib.F_RETURN_DISTS)
        reduce(v, sd)

    try:
        _for_strands(view, strand, run)
    finally:
        if owned:
            view.free()


def dist_landscape(genome_or_path, RV, windowsize: int, k: int, *, bin: Optional[int] = None, n_refs: Optional[int] = None,
                   strand: str = "+", ctx=None) -> List[LandscapeTrack]:
    """The distance landscape of a genome against the KFV `RV`: per record (identifier, bin_min, bin_argmin, ...), the smallest
    window distance of every `bin` consecutive windows (default: windowsize) and the start of the first window attaining it.
    The scan keeps its distances on the device and kgma_dist_bins reduces them there: 16 bytes per bin come to the host
    instead of 8 per window.  `genome_or_path`: a FASTA or .2bit path, an open device genome (it stays open) or records.
    strand "-": the reverse complement of every record is scanned and bin_argmin is mapped to the forward start of the same
    window, L - s - W + 2 (strand_range of the window); the bins keep the scan's order, so bin 0 lies at the record's END.
    "both": the plus tracks, then the minus tracks.  Sets the context's references."""
    ctx = ctx or default_context()
    W = int(windowsize)
    width = W if bin is None else int(bin)
    if width < 1:
        raise ValueError(f"bin = {bin}")
    out: List[LandscapeTrack] = []

    def reduce(v, sd):
        bmin, barg, off = ctx.dist_bins(1, width)
        for c in range(v.genome.n_contigs):
            L = v.genome.contig_len(c)
            m, a = bmin[off[c]:off[c + 1]].copy(), barg[off[c]:off[c + 1]].copy()
            if sd == "-":
                a = L - a - W + 2
            out.append(LandscapeTrack(v.identifier(c), m, a, sd, width, W, L))

    _landscape_scan(genome_or_path, RV, W, k, n_refs, strand, ctx, reduce)
    return out


def default_sweep_thresholds(ctx, RV, windowsize: int, n: int = _lib.SWEEP_MAX_THRESHOLDS) -> np.ndarray:
    """Up to `n` thresholds from 0 up to the mean distance of random sequences of `windowsize` residues to the KFV
    (refprep.estimate_optimal_threshold with buffer 0).  S/N KFV: each lies halfway between two lattice points, (D + 0.5) / scale
    (off_lattice_threshold), D spread evenly, so no window lies on a threshold; Float64 KFV: evenly spaced.  The context's
    references must be set (kfv 1)."""
    top = float(refprep.estimate_optimal_threshold(RV, int(windowsize), buffer=0, ctx=ctx))
    if ctx.kfv_is_float(1):
        return np.linspace(top / n, top, n)
    scale = ctx.kfv_scale(1)
    D = np.unique(np.round(np.linspace(0, math.floor(top * scale), n)).astype(np.int64))
    return (D + 0.5) / scale


def threshold_sweep(genome_or_path, RV, windowsize: int, k: int, thresholds=None, *, n_refs: Optional[int] = None,
                    strand: str = "+", ctx=None) -> ThresholdSweep:
    """(thresholds, windows_below, dips_below): for every threshold the exact number of tested windows whose distance lies
    below it and the exact number of dips -- maximal runs of such windows, what a scan at that threshold would find -- in ONE
    scan and one pass over its distances on the device (kgma_dist_sweep).  thresholds: finite, strictly increasing, at most
    4096; None: default_sweep_thresholds.  strand "both" adds the two strands' counts.  Sets the context's references."""
    ctx = ctx or default_context()
    _check_strand(strand)
    if thresholds is None:
        ctx.set_refs(int(k), [np.asarray(RV, dtype=np.float64)], [int(windowsize)], [1.0], None if n_refs is None else [int(n_refs)])
        thresholds = default_sweep_thresholds(ctx, RV, windowsize)
    thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
    state = dict(thr=thr, below=np.zeros(thr.size, dtype=np.int64), dips=np.zeros(thr.size, dtype=np.int64))

    def reduce(v, sd):
        below, dips = ctx.dist_sweep(thr, 1)
        state["below"] += below
        state["dips"] += dips

    _landscape_scan(genome_or_path, RV, windowsize, k, n_refs, strand, ctx, reduce)
    return ThresholdSweep(state["thr"], state["below"], state["dips"])


def threshold_for_dips(sweep, n: int) -> Optional[float]:
    """The largest threshold of a sweep (thresholds, windows_below, dips_below) with at most `n` dips; None if every one has more.
    (The dips need not grow with the threshold: neighbouring dips merge.)"""
    thr, dips = np.asarray(sweep[0]), np.asarray(sweep[2])
    ok = np.nonzero(dips <= int(n))[0]
    return float(thr[ok[-1]]) if ok.size else None


def best_loci(track, n: int, sep: Optional[int] = None) -> list:
    """The `n` best loci of a track (api.dist_landscape), threshold-free: (record, window start, dist) with record the index
    into `track`.  GREEDY OVER BIN MINIMA, not over all windows: the bins are sorted by (minimum, record, argmin) and taken in
    that order; a bin is dropped when its argmin lies fewer than `sep` windows (default: the track's windowsize) from an
    accepted locus of the same record.  A second locus inside one bin is therefore never seen; choose bin <= sep.  Host only."""
    track = list(track)
    if not track or int(n) <= 0:
        return []
    sep = int(track[0].windowsize if sep is None else sep)
    rec = np.concatenate([np.full(len(t[1]), i, dtype=np.int64) for i, t in enumerate(track)])
    mins = np.concatenate([np.asarray(t[1], dtype=np.float64) for t in track])
    args = np.concatenate([np.asarray(t[2], dtype=np.int64) for t in track])
    taken: dict = {}
    out = []
    for i in np.lexsort((args, rec, mins)):
        r, a = int(rec[i]), int(args[i])
        if any(abs(a - b) < sep for b in taken.get(r, ())):
            continue
        taken.setdefault(r, []).append(a)
        out.append((r, a, float(mins[i])))
        if len(out) == int(n):
            break
    return out


def write_bedgraph(track, path) -> None:
    """One line per bin: record identifier, 0-based start and end of the bin's window STARTS (forward coordinates, half-open),
    minimum (repr of the double).  Lines of a record ascend; a minus-strand track is written in forward order."""
    with open(path, "w") as f:
        for t in track:
            nwin = t.length - t.windowsize + 1
            rows = []
            for b, m in enumerate(t.bin_min):
                lo, hi = b * t.bin + 2, min((b + 1) * t.bin + 1, nwin)            # window starts, 1-based inclusive, scan order
                if t.strand == "-":
                    lo, hi = t.length - hi - t.windowsize + 2, t.length - lo - t.windowsize + 2
                rows.append((lo - 1, hi, m))
            for lo0, hi0, m in (reversed(rows) if t.strand == "-" else rows):
                f.write(f"{t.identifier}\t{lo0}\t{hi0}\t{float(m)!r}\n")


# ---- k-mer counts of the resident genome (kgma_genome_kmer_count): spectra, backgrounds, composition tracks ----
class CompositionTrack(NamedTuple):
    """One record of api.composition_track: bin b holds the k-mers that START at the 0-based residues b * bin ..
    min((b + 1) * bin, length) - 1; counts[b] are their 4^k counts (natural k-mer value), skipped[b] the starts left out."""
    identifier: str
    counts: np.ndarray
    skipped: np.ndarray
    bin: int
    k: int
    length: int


def _count_flags(skip_n: bool, skip_masked: bool, by_start: bool) -> int:
    return ((_lib.COUNT_SKIP_N if skip_n else 0) | (_lib.COUNT_SKIP_MASKED if skip_masked else 0)
            | (_lib.COUNT_BY_START if by_start else 0))


def _count_view(ctx, genome_or_path):
    """(view, owned) of a FASTA or .2bit path, an open device genome (it stays open), a _GenomeView or records."""
    if isinstance(genome_or_path, _GenomeView):
        return genome_or_path, False
    if genome_or_path is None or isinstance(genome_or_path, (bytes, bytearray, memoryview, Record, int, float)):
        raise TypeError("Invalid subject sequence type")
    return _GenomeView(ctx, genome_or_path), True


def _check_count_k(k) -> int:
    if not 1 <= int(k) <= 10:
        raise ValueError(f"k = {k}: the k-mer count serves k = 1 ... 10")
    return int(k)


def genome_kmer_count(genome_or_path, k: int, ranges=None, *, skip_n: bool = False, skip_masked: bool = False,
                      by_start: bool = False, ctx=None):
    """(counts, skipped) of kgma_genome_kmer_count: counts int64 [n, 4^k], row r = kmer_count(view(seq, lo:hi), k)
    (src/Kmers.jl:14-28; index = natural k-mer value, first base most significant) of the r-th of `ranges`, (record, lo, hi)
    triples with a 0-based record and 1-based inclusive lo:hi; None: one whole-record range per record.  The residues are read
    where they lie on the device.  skip_n: a k-mer with a byte outside A/C/G/T is left out and counted in skipped[r] (default:
    N counts as T, anything else is a BadBaseError); skip_masked: so is a k-mer with a lower-case (soft-masked) byte;
    by_start: a k-mer belongs to the range it starts in, also when it ends behind hi, so ranges that tile a record sum to the
    record's count.  `genome_or_path`: a FASTA or .2bit path, an open device genome (it stays open) or records."""
    k = _check_count_k(k)
    ctx = ctx or default_context()
    view, owned = _count_view(ctx, genome_or_path)
    try:
        g = view.genome
        if ranges is None:
            ranges = [(c, 1, g.contig_len(c)) for c in range(g.n_contigs)]
        ranges = [(int(c), int(lo), int(hi)) for c, lo, hi in ranges]
        return ctx.genome_kmer_count(g, k, [r[0] for r in ranges], [r[1] for r in ranges], [r[2] for r in ranges],
                                     _count_flags(skip_n, skip_masked, by_start))
    finally:
        if owned:
            view.free()


def revcomp_kmer_permutation(k: int) -> np.ndarray:
    """perm[x] = the natural value of the reverse complement of the k-mer of value x: the spectrum of the minus strand is
    spectrum[perm]."""
    x = np.arange(4 ** int(k), dtype=np.int64)
    y = np.zeros_like(x)
    for _ in range(int(k)):
        y = (y << 2) | (3 - (x & 3))
        x = x >> 2
    return y


def genome_spectrum(genome_or_path, k: int, *, skip_n: bool = True, skip_masked: bool = False, strand: str = "+", ctx=None) -> np.ndarray:
    """The k-mer spectrum of a genome: int64 [4^k], the whole-record counts summed over the records (no k-mer spans two).
    strand "-": the spectrum of the reverse complements, formed on the host by the reverse-complement permutation of the index
    (no second pass, no reversed genome); "both": the sum of the two."""
    _check_strand(strand)
    counts, _ = genome_kmer_count(genome_or_path, k, skip_n=skip_n, skip_masked=skip_masked, ctx=ctx)
    plus = np.asarray(counts, dtype=np.int64).reshape(-1, 4 ** int(k)).sum(axis=0)
    if strand == "+":
        return plus
    minus = plus[revcomp_kmer_permutation(k)]
    return minus if strand == "-" else plus + minus


def genome_background(genome_or_path, *, skip_masked: bool = False, strand: str = "both", ctx=None) -> np.ndarray:
    """The base composition of a genome as four probabilities (A, C, G, T), measured on the device: usable wherever
    `background=` is accepted (pwm_threshold, pwm_score_distribution, pwm_from_sequences, pwmMatch).  N and other codes are
    left out; "both" symmetrises A/T and C/G.  ValueError when a base does not occur (a background needs positive
    probabilities)."""
    n = genome_spectrum(genome_or_path, 1, skip_n=True, skip_masked=skip_masked, strand=strand, ctx=ctx).astype(np.float64)
    if (n <= 0).any():
        raise ValueError(f"genome_background: base {'ACGT'[int(np.argmin(n))]} does not occur: a background needs four positive probabilities")
    return n / n.sum()


def composition_track(genome_or_path, bin: int, k: int = 1, *, skip_n: bool = True, skip_masked: bool = False, ctx=None) -> List[CompositionTrack]:
    """Per record a CompositionTrack: the k-mer counts of every `bin` consecutive starts (the last bin of a record may be
    shorter), a k-mer belonging to the bin it starts in (by_start) -- the material of GC, CpG and N / masked-share tracks
    (gc_fraction, cpg_obs_exp, track.skipped).  One device call, split where ranges * 4^k would pass the call's cap."""
    k = _check_count_k(k)
    width = int(bin)
    if width < 1:
        raise ValueError(f"bin = {bin}")
    ctx = ctx or default_context()
    view, owned = _count_view(ctx, genome_or_path)
    try:
        g = view.genome
        lens = [g.contig_len(c) for c in range(g.n_contigs)]
        nbins = [(L + width - 1) // width for L in lens]
        contig = np.repeat(np.arange(len(lens), dtype=np.int32), nbins)
        lo = np.concatenate([np.arange(n, dtype=np.int64) * width + 1 for n in nbins]) if lens else np.zeros(0, dtype=np.int64)
        hi = np.minimum(lo + width - 1, np.repeat(np.asarray(lens, dtype=np.int64), nbins))
        flags = _count_flags(skip_n, skip_masked, True)
        per_call = max(1, _lib.SPECTRUM_MAX_COUNTS >> (2 * k))
        parts = [ctx.genome_kmer_count(g, k, contig[i:i + per_call], lo[i:i + per_call], hi[i:i + per_call], flags)
                 for i in range(0, contig.size, per_call)]
        counts = np.concatenate([p[0] for p in parts]) if parts else np.zeros((0, 4 ** k), dtype=np.int64)
        skipped = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, dtype=np.int64)
        off = np.concatenate(([0], np.cumsum(nbins))).astype(np.int64)
        return [CompositionTrack(view.identifier(c), counts[off[c]:off[c + 1]], skipped[off[c]:off[c + 1]], width, k, lens[c])
                for c in range(len(lens))]
    finally:
        if owned:
            view.free()


def _first_base_counts(track) -> np.ndarray:
    """[n_bins, 4]: the counted k-mers of every bin by their first base."""
    c = np.asarray(track.counts, dtype=np.float64)
    return c.reshape(c.shape[0], 4, -1).sum(axis=2)


def gc_fraction(track) -> np.ndarray:
    """(C + G) / counted per bin of a CompositionTrack; at k > 1 the base is the k-mer's first.  NaN where nothing was counted."""
    m = _first_base_counts(track)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (m[:, 1] + m[:, 2]) / m.sum(axis=1)


def cpg_obs_exp(track) -> np.ndarray:
    """CpG observed / expected per bin of a k = 2 CompositionTrack: n_CG * counted / (n_C* * n_G*), the marginals being those
    of the first base.  NaN where a factor of the denominator is 0."""
    if track.k != 2:
        raise ValueError("cpg_obs_exp needs a k = 2 track")
    m = _first_base_counts(track)
    c = np.asarray(track.counts, dtype=np.float64)
    den = m[:, 1] * m[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, c[:, 4 * 1 + 2] * m.sum(axis=1) / den, np.nan)


def write_composition_bedgraph(tracks, values, path) -> None:
    """One line per bin: record identifier, 0-based half-open range of the bin's starts, value (repr of the double).  `values`:
    one array per track (gc_fraction(track), cpg_obs_exp(track), track.skipped / bin, ...).  The analogue of write_bedgraph."""
    tracks, values = list(tracks), list(values)
    if len(tracks) != len(values):
        raise ValueError("need one array of values per track")
    with open(path, "w") as f:
        for t, v in zip(tracks, values):
            v = np.asarray(v, dtype=np.float64).reshape(-1)
            if v.size != len(t.counts):
                raise ValueError(f"{t.identifier}: {v.size} values for {len(t.counts)} bins")
            for b, x in enumerate(v.tolist()):
                f.write(f"{t.identifier}\t{b * t.bin}\t{min((b + 1) * t.bin, t.length)}\t{float(x)!r}\n")


def fasta_id_to_cumulative_len_dict(fasta_file_path) -> dict:
    """src/ExactMatch.jl:146-158: the full description line of every record -> the summed length of the records BEFORE it
    (what the scan reports as GenomePos).  Given an open device genome the headers and lengths come from its handle;
    given a path the file is read on the host, as the reference does (a .2bit path -- told by its first four bytes -- gives
    its record names and dnaSizes from the file's index, after the library's parser has validated the file)."""
    if isinstance(fasta_file_path, _GenomeView):
        g = fasta_file_path.genome
        pairs = [(fasta_file_path.descriptions[c], g.contig_len(c)) for c in range(g.n_contigs)]
    elif isinstance(fasta_file_path, _lib.Genome):
        g = fasta_file_path
        pairs = [(g.header(c), g.contig_len(c)) for c in range(g.n_contigs)]
    elif isinstance(fasta_file_path, str) and _lib.is_twobit(fasta_file_path):
        pairs = twobit_names_and_lengths(fasta_file_path)              # (record name, dnaSize) from the file's index: host only
    elif isinstance(fasta_file_path, str):
        pairs = [(r.description, len(r.sequence)) for r in read_fasta(fasta_file_path)]
    else:
        raise TypeError("expected a FASTA or .2bit path or an open device genome")
    out, total = {}, 0
    for desc, n in pairs:
        out[desc] = total
        total += n
    return out


def write_results(KmerGMA_result_vec: Sequence[Record], file_path: str, width: int = 95) -> None:
    """`write_results` (src/API.jl:234-241): APPENDS to file_path."""
    write_fasta(KmerGMA_result_vec, file_path, width=width, append=True)
    log.info("writing complete")
