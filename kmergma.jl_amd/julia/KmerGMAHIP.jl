# KmerGMAHIP.jl -- Julia shim over libkgma (include/kgma.h): drop-in replacements for the scan engines of
# KmerGMA.jl with the SAME keyword signatures, so `findGenes` / `findGenes_cluster_mode` (src/API.jl:83-94,
# :201-216) can call them instead of `ac_gma_testing!` / `Omn_KmerGMA!`, and `record_KmerGMA!`
# (src/MultiThread/GenomeMiner.jl:8-98) for callers that scan one record at a time.
#
# NOTE: Julia is not installed in the build container nor on the GPU box, so this file has never been
# executed.  It is deliberately thin (marshalling only) and mirrors, call for call, the Python ctypes host
# (kmergma_amd/_lib.py, kmergma_amd/api.py) that IS tested against the same library.
#
# What stays in Julia (exactly the reference's own code): reference preparation (gen_ref_ws_cons /
# cluster_ref_API), re-alignment of hits (BioAlignments.pairalign + cigar_to_UnitRange) and FASTA.Record
# construction.  What moves to the GPU: FASTA parsing + encoding (kgma_genome_from_fasta: the file is mapped
# and goes to the device ONCE; no LongDNA copy of the genome is made on the host) and the per-record body of
# the engines (src/GenomeMiner.jl:32-107, src/OmnGenomeMiner.jl:55-160).  Residues are read back only for the
# hits: `kgma_genome_fetch` serves the alignment segments, `kgma_genome_fetch_batch` the record bodies of all hits at once.
# Every 1 <= k <= 15 is served (kgma_set_refs); the dense refVec of the reference is passed as it is at every k (at k >= 11
# the library keeps only its non-zero entries).

module KmerGMAHIP

using KmerGMA, FASTX, BioSequences, BioAlignments, Mmap, Printf

const libkgma = get(ENV, "KGMA_LIB", joinpath(@__DIR__, "..", "libkgma.so"))

struct KgmaHit            # must match kgma_hit in include/kgma.h (64 bytes)
    contig::Int32
    kfv::Int32
    cmi::Int64
    lo::Int64
    hi::Int64
    genome_pos::Int64
    dist::Float64
    D::Int64
    flags::UInt32
    reserved::UInt32
end

const KGMA_MODE_SINGLE = Int32(0)
const KGMA_MODE_OMN = Int32(1)
const KGMA_MODE_STROBE = Int32(2)
const KGMA_F_RETURN_DISTS = UInt32(1)
const KGMA_F_CHAIN_REPLAY = UInt32(4)   # ties decided by the reference's running Float64 distance (kgma.h)
const KGMA_E_BADBASE = 4
const KGMA_E_BOUNDS = 5

mutable struct Context
    h::Ptr{Cvoid}
    function Context(device::Integer = 0)
        r = Ref{Ptr{Cvoid}}(C_NULL)
        st = ccall((:kgma_create, libkgma), Cint, (Cint, Ref{Ptr{Cvoid}}), device, r)
        st == 0 || error("kgma_create failed: " * unsafe_string(ccall((:kgma_status_string, libkgma), Cstring, (Cint,), st)))
        ctx = new(r[])
        finalizer(c -> (c.h == C_NULL || ccall((:kgma_destroy, libkgma), Cvoid, (Ptr{Cvoid},), c.h); c.h = C_NULL), ctx)
        return ctx
    end
end

const DEFAULT_CTX = Ref{Union{Nothing, Context}}(nothing)
default_context() = (DEFAULT_CTX[] === nothing && (DEFAULT_CTX[] = Context(0)); DEFAULT_CTX[])

function check(ctx::Context, st::Integer)
    st == 0 && return
    msg = unsafe_string(ccall((:kgma_last_error, libkgma), Cstring, (Ptr{Cvoid},), ctx.h))
    st == KGMA_E_BADBASE && throw(KeyError(msg))        # NUCLEOTIDE_BITS lookup, src/Consts.jl:22-28
    st == KGMA_E_BOUNDS && throw(BoundsError(msg))      # src/OmnGenomeMiner.jl:84-86
    error("libkgma status $st: $msg")
end

# ---- the genome lives on the device; the host keeps a handle ------------------------------------------------
mutable struct DeviceGenome
    ctx::Context
    h::Ptr{Cvoid}
end

# FASTA file -> device (replaces `open(FASTA.Reader, genome_path)` + getSeq, src/GenomeMiner.jl:31-35): the library reads
# the file straight into its pinned staging buffers (kgma_genome_from_fasta_file), strips the line breaks and encodes the
# residues on the GPU
function genome_from_fasta(ctx::Context, genome_path::String)
    g = Ref{Ptr{Cvoid}}(C_NULL)
    check(ctx, ccall((:kgma_genome_from_fasta_file, libkgma), Cint, (Ptr{Cvoid}, Cstring, Ref{Ptr{Cvoid}}), ctx.h, genome_path, g))
    return DeviceGenome(ctx, g[])
end

# UCSC .2bit file -> device (kgma_genome_from_2bit_file): the packed bytes and the N / soft-mask interval lists are shipped as they
# are (a quarter of the FASTA text's bytes) and expanded to the resident text by one kernel; mask = false ignores the soft-mask
# blocks (all upper case, as twoBitToFa -noMask).  Record names come back through kgma_genome_header like FASTA header lines.
const KGMA_2BIT_NOMASK = UInt32(1)
function genome_from_2bit(ctx::Context, genome_path::String; mask::Bool = true)
    g = Ref{Ptr{Cvoid}}(C_NULL)
    check(ctx, ccall((:kgma_genome_from_2bit_file, libkgma), Cint, (Ptr{Cvoid}, Cstring, UInt32, Ref{Ptr{Cvoid}}),
                     ctx.h, genome_path, mask ? UInt32(0) : KGMA_2BIT_NOMASK, g))
    return DeviceGenome(ctx, g[])
end

# a genome file by its content: the .2bit signature (either byte order; the library refuses a byte-swapped file with its own
# message) in the first four bytes, else FASTA -- the file's name is not looked at
function genome_from_path(ctx::Context, genome_path::String)
    head = open(io -> read(io, 4), genome_path)
    twobit = head == UInt8[0x43, 0x27, 0x41, 0x1a] || head == UInt8[0x1a, 0x41, 0x27, 0x43]
    return twobit ? genome_from_2bit(ctx, genome_path) : genome_from_fasta(ctx, genome_path)
end

# one record (record_KmerGMA!): its residues as FASTX holds them
function genome_from_record(ctx::Context, record::FASTA.Record)
    s = Vector{UInt8}(FASTA.sequence(String, record))
    g = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve s begin
        check(ctx, ccall((:kgma_genome_from_host, libkgma), Cint,
                         (Ptr{Cvoid}, Ptr{Ptr{UInt8}}, Ptr{Int64}, Int64, Ref{Ptr{Cvoid}}),
                         ctx.h, [pointer(s)], Int64[length(s)], 1, g))
    end
    return DeviceGenome(ctx, g[])
end

# the records of `g` reverse-complemented on the device (kgma_genome_revcomp): a new genome with the same record lengths and
# header lines.  Results on it are in the reversed records' coordinates: position p there is L - p + 1 on `g`.
function genome_revcomp(g::DeviceGenome)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(g.ctx, ccall((:kgma_genome_revcomp, libkgma), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), g.ctx.h, g.h, r))
    return DeviceGenome(g.ctx, r[])
end

contig_len(g::DeviceGenome, contig::Integer) = ccall((:kgma_genome_contig_len, libkgma), Int64, (Ptr{Cvoid}, Int64), g.h, contig)

# lo:hi of a record of length L in the coordinates of its reverse complement (its own inverse)
strand_range(L::Integer, r::UnitRange) = (L - last(r) + 1):(L - first(r) + 1)

check_strand(strand::String) = strand in ("+", "-", "both") || throw(ArgumentError("strand must be \"+\", \"-\" or \"both\""))

# run(genome, minus::Bool) on `g` and / or on its reverse complement; with "both" the reversed genome is made after the
# forward results have been taken and freed before returning (two genomes on the device at the peak)
function for_strands(run::Function, g::DeviceGenome, strand::String)
    strand != "-" && run(g, false)
    if strand != "+"
        rc = genome_revcomp(g)
        try
            run(rc, true)
        finally
            free!(rc)
        end
    end
    return nothing
end

free!(g::DeviceGenome) = (g.h == C_NULL || ccall((:kgma_genome_free, libkgma), Cvoid, (Ptr{Cvoid}, Ptr{Cvoid}), g.ctx.h, g.h); g.h = C_NULL; nothing)

function identifier(g::DeviceGenome, contig::Integer)
    txt = Ref{Cstring}(C_NULL); n = Ref{Int64}(0)
    st = ccall((:kgma_genome_header, libkgma), Cint, (Ptr{Cvoid}, Int64, Ref{Cstring}, Ref{Int64}), g.h, contig, txt, n)
    st == 0 || error("the genome has no FASTA headers")
    hdr = unsafe_string(Ptr{UInt8}(txt[]), n[])
    return String(first(split(hdr, (' ', '\t'); limit = 2)))     # FASTA.identifier: up to the first whitespace
end

# view(seq, lo:hi) as a LongDNA{4} (the residues travel back from the device: hits only)
function subseq(g::DeviceGenome, contig::Integer, lo::Integer, hi::Integer)
    hi < lo && return KmerGMA.Seq("")
    buf = Vector{UInt8}(undef, hi - lo + 1)
    check(g.ctx, ccall((:kgma_genome_fetch, libkgma), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{UInt8}),
                       g.ctx.h, g.h, contig, lo, hi - lo + 1, buf))
    return KmerGMA.Seq(String(buf))
end

# view(seq, lo:hi) of every hit in ONE device gather + ONE download (kgma_genome_fetch_batch)
function hit_bodies(g::DeviceGenome, hits)
    n = length(hits)
    n == 0 && return KmerGMA.Seq[]
    contigs = Int64[h.contig for h in hits]
    pos = Int64[h.lo for h in hits]
    lens = Int64[max(h.hi - h.lo + 1, 0) for h in hits]
    buf = Vector{UInt8}(undef, max(sum(lens), 1))
    check(g.ctx, ccall((:kgma_genome_fetch_batch, libkgma), Cint,
                       (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{UInt8}, Int64),
                       g.ctx.h, g.h, n, contigs, pos, lens, buf, length(buf)))
    offs = cumsum(vcat(0, lens))
    return [KmerGMA.Seq(String(buf[offs[i]+1:offs[i+1]])) for i in 1:n]
end

function fetch_hits(ctx::Context)
    n = Ref{Int64}(0)
    check(ctx, ccall((:kgma_get_hits, libkgma), Cint, (Ptr{Cvoid}, Ptr{KgmaHit}, Int64, Ref{Int64}), ctx.h, C_NULL, 0, n))
    hits = Vector{KgmaHit}(undef, n[])
    check(ctx, ccall((:kgma_get_hits, libkgma), Cint, (Ptr{Cvoid}, Ptr{KgmaHit}, Int64, Ref{Int64}), ctx.h, hits, n[], n))
    return hits
end

function fetch_dists!(ctx::Context, kfv::Integer, dist_vec)
    n = Ref{Int64}(0)
    check(ctx, ccall((:kgma_get_dists, libkgma), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Ref{Int64}), ctx.h, kfv, C_NULL, 0, n))
    buf = Vector{Float64}(undef, n[])
    check(ctx, ccall((:kgma_get_dists, libkgma), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Ref{Int64}), ctx.h, kfv, buf, n[], n))
    append!(dist_vec, buf)
end

# kmer_dist(seq, KFV, k) (src/Kmers.jl:58-60) of many sequences against one KFV in one device batch:
# what cluster_ref_API (ReferenceGeneration.jl:101) and estimate_optimal_threshold (DistanceTesting.jl:14,27)
# compute one sequence at a time.
function kmer_dist_batch(ctx::Context, seqs::Vector{<:AbstractString}, KFV::Vector{Float64}, k::Int)
    length(KFV) == 4^k || error("the KFV must have 4^k entries")
    text = Vector{UInt8}(join(seqs))
    offsets = Int64[0; cumsum(Int64[ncodeunits(s) for s in seqs])]
    out = Vector{Float64}(undef, length(seqs))
    check(ctx, ccall((:kgma_kmer_dist_batch, libkgma), Cint,
                     (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{UInt8}, Ptr{Int64}, Int64, Ptr{Float64}),
                     ctx.h, k, KFV, text, offsets, length(seqs), out))
    return out
end

# alignment callback: the library calls this in reference order with the candidate range and
# expects the aligned range back (Alignment.jl:33-52 / OmnGenomeMiner.jl:130-136).
mutable struct AlignState
    genome::DeviceGenome
    consensus::Vector{KmerGMA.Seq}
    windowsize::Int            # > 0: single engine (view(consensus, 1:windowsize)); 0: cluster engine
    score_model
    keep::Bool
    out::Vector
end

function align_trampoline(user::Ptr{Cvoid}, contig::Int32, kfv::Int32, lo::Int64, hi::Int64, L::Int64,
                          out_lo::Ptr{Int64}, out_hi::Ptr{Int64})::Cvoid
    st = unsafe_pointer_to_objref(user)::AlignState
    segment = subseq(st.genome, contig, lo, hi)                        # view(seq, lo:hi)
    cons = kfv == 0 ? view(st.consensus[1], 1:st.windowsize) : st.consensus[kfv]
    aligned_obj = pairalign(SemiGlobalAlignment(), cons, segment, st.score_model)
    st.keep && push!(st.out, aligned_obj)
    r = cigar_to_UnitRange(aligned_obj)
    unsafe_store!(out_lo, max(1, lo + first(r) - 1))
    unsafe_store!(out_hi, min(lo + last(r) - 1, L))
    return
end

scan_flags(do_return_dists::Bool, float_chain::Bool) =
    (do_return_dists ? KGMA_F_RETURN_DISTS : UInt32(0)) | (float_chain ? KGMA_F_CHAIN_REPLAY : UInt32(0))

# the body shared by ac_gma_testing! and record_KmerGMA!: scan `g` with the single engine and build the records
function single_engine!(ctx::Context, g::DeviceGenome, ident::Function; refVec, consensus_refseq, k, windowsize, thr, buff,
                        do_align, result_align_vec, gap_open_score, gap_extend_score, do_return_dists, dist_vec,
                        do_return_align, get_hit_loci, hit_loci_vec, resultVec, n_refs, with_genome_pos::Bool, float_chain::Bool,
                        minus::Bool = false, set_refs::Bool = true)
    # (minus: `g` is the reverse complement of the caller's genome -- hits come back in its coordinates and are reported in
    #  forward coordinates with " | Strand = -"; the body stays the reversed genome's lo:hi, the gene in reference orientation)
    if set_refs
        nref = n_refs === nothing ? C_NULL : Int64[n_refs]
        check(ctx, ccall((:kgma_set_refs, libkgma), Cint,
            (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}),
            ctx.h, k, 1, collect(Float64, refVec), Int64[windowsize], Float64[thr], nref))
    end
    st = AlignState(g, [consensus_refseq], windowsize,
        AffineGapScoreModel(EDNAFULL, gap_open = gap_open_score, gap_extend = gap_extend_score),
        do_return_align, result_align_vec)
    cb = do_align ? @cfunction(align_trampoline, Cvoid,
        (Ptr{Cvoid}, Int32, Int32, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64})) : C_NULL
    GC.@preserve st begin
        check(ctx, ccall((:kgma_scan, libkgma), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Int64, UInt32, Ptr{Cvoid}, Ptr{Cvoid}),
            ctx.h, g.h, KGMA_MODE_SINGLE, buff, 0, scan_flags(do_return_dists, float_chain), cb, pointer_from_objref(st)))
    end
    hits = fetch_hits(ctx)
    bodies = hit_bodies(g, hits)
    for (h, body) in zip(hits, bodies)
        seq_UnitRange = Int(h.lo):Int(h.hi)
        minus && (seq_UnitRange = strand_range(contig_len(g, h.contig), seq_UnitRange))
        # the reference's record format: src/Alignment.jl:69-80 (append_hit!, do_overlap = false);
        # record_KmerGMA! omits GenomePos (src/MultiThread/GenomeMiner.jl:87-93)
        header = ident(h.contig) *
            " | dist = " * string(round(h.dist, digits = 2)) *
            " | MatchPos = $seq_UnitRange" *
            (with_genome_pos ? " | GenomePos = $(h.genome_pos)" : "") *
            " | Len = " * string(last(seq_UnitRange) - first(seq_UnitRange) + 1) *
            (minus ? " | Strand = -" : "")
        push!(resultVec, FASTA.Record(header, body))
        get_hit_loci && push!(hit_loci_vec, first(seq_UnitRange) + h.genome_pos)
    end
    do_return_dists && fetch_dists!(ctx, 1, dist_vec)
    return nothing
end

"""
    ac_gma_testing!(; kwargs...)   -- same keywords as KmerGMA.ac_gma_testing! (src/GenomeMiner.jl:4-23)
plus `n_refs` (number of reference sequences averaged into refVec; inferred when omitted) and `float_chain`
(default true: rounding-dependent ties decided by the reference's running Float64 distance, KGMA_F_CHAIN_REPLAY), and
`strand`: "+" (default, the reference's scan), "-" (the same scan over the reverse complement of every record, made on the
device; hits reported in forward coordinates, lo:hi -> (L - hi + 1):(L - lo + 1), with " | Strand = -" appended to the header
and the gene in reference orientation as the body) or "both" (the plus results, then the minus results; not de-duplicated,
a palindromic region may be reported twice).  With `do_return_align` the BioAlignments objects of minus hits are those of the
gene-oriented segments.
"""
function ac_gma_testing!(; genome_path::String, refVec::Vector{Float64}, consensus_refseq::KmerGMA.Seq,
    k::Int64 = 6, windowsize::Int64 = 289, thr::Union{Int64, Float64} = 33.5, buff::Int64 = 50,
    mask::UInt64 = unsigned(4095), Nt_bits = NUCLEOTIDE_BITS, ScaleFactor::Float64 = 1/6,
    do_align::Bool = true, result_align_vec = [], gap_open_score::Int = -69, gap_extend_score::Int = -1,
    do_return_dists::Bool = false, dist_vec = Float64[], do_return_align::Bool = false,
    get_hit_loci::Bool = false, hit_loci_vec::Vector{Int} = Int[],
    resultVec::Vector{FASTA.Record} = FASTA.Record[], n_refs::Union{Nothing, Int} = nothing,
    float_chain::Bool = true, strand::String = "+", ctx::Context = default_context())

    check_strand(strand)
    mask == unsigned(4^k - 1) || error("mask must be 4^k - 1")
    g = genome_from_fasta(ctx, genome_path)
    try
        for_strands(g, strand) do gs, minus
            single_engine!(ctx, gs, c -> identifier(gs, c); refVec, consensus_refseq, k, windowsize, thr, buff, do_align,
                result_align_vec, gap_open_score, gap_extend_score, do_return_dists, dist_vec, do_return_align,
                get_hit_loci, hit_loci_vec, resultVec, n_refs, with_genome_pos = true, float_chain, minus,
                set_refs = !(minus && strand == "both"))
        end
    finally
        free!(g)
    end
    return nothing
end

"""
    record_KmerGMA!(; kwargs...)   -- same keywords as KmerGMA.record_KmerGMA! (src/MultiThread/GenomeMiner.jl:8-23):
one record in, hits pushed to `resultVec_vec[Threads.threadid()]`, headers without GenomePos.  `refVec` may be the
reference's SVector or a plain Vector; `curr_kmer_freq_vec` (the per-thread count buffers) is accepted and unused:
the counts live on the device.  Use one Context per Julia thread (a context is not thread-safe).
"""
function record_KmerGMA!(; record::FASTA.Record, refVec, curr_kmer_freq_vec = nothing, consensus_refseq::KmerGMA.Seq,
    resultVec_vec::Vector{Vector{FASTA.Record}}, k::Int64 = 6, windowsize::Int64 = 289,
    thr::Union{Int64, Float64} = 30, buff::Int64 = 50, mask::UInt64 = unsigned(4095), Nt_bits = NUCLEOTIDE_BITS,
    ScaleFactor::Float64 = 1/6, initial_scale_factor::Float64 = 1/12, do_align::Bool = true,
    score_model::AffineGapScoreModel{Int64} = AffineGapScoreModel(EDNAFULL, gap_open = -69, gap_extend = -1),
    n_refs::Union{Nothing, Int} = nothing, float_chain::Bool = true, ctx::Context = default_context())

    mask == unsigned(4^k - 1) || error("mask must be 4^k - 1")
    g = genome_from_record(ctx, record)
    try
        single_engine!(ctx, g, c -> FASTA.identifier(record); refVec, consensus_refseq, k, windowsize, thr, buff, do_align,
            result_align_vec = [], gap_open_score = score_model.gap_open, gap_extend_score = score_model.gap_extend,
            do_return_dists = false, dist_vec = Float64[], do_return_align = false, get_hit_loci = false,
            hit_loci_vec = Int[], resultVec = resultVec_vec[Threads.threadid()], n_refs, with_genome_pos = false, float_chain)
    finally
        free!(g)
    end
    return nothing
end

"""
    Omn_KmerGMA!(; kwargs...)   -- same keywords as KmerGMA.Omn_KmerGMA! (src/OmnGenomeMiner.jl:7-30)
plus `n_refs::Vector{Int}` (reference count per cluster), `float_chain` and `strand` ("+", "-" or "both": as
ac_gma_testing!; with "both" every KFV's distances are its plus vector followed by its minus vector).
"""
function Omn_KmerGMA!(; genome_path::String, refVecs::Vector{Vector{Float64}}, windowsizes::Vector{Int64},
    consensus_seqs::Vector{KmerGMA.Seq}, resultVec::Vector{FASTA.Record}, k::Int64 = 6, ScaleFactor::Real = 1/6,
    mask::UInt64 = unsigned(4095), thr_vec = Float64[35, 31, 38, 34, 27, 27], buff::Int64 = 50,
    Nt_bits = NUCLEOTIDE_BITS, align_hits::Bool = true, align_vec = [], gap_open_score::Int = -200,
    gap_extend_score::Int = -1, genome_pos::Int64 = 0, get_hit_loci::Bool = false,
    hit_loci_vec::Vector{Int} = Int[], get_aligns::Bool = false, do_return_dists::Bool = false,
    dist_vec_vec::Vector{Vector{Float64}} = [Float64[] for _ in 1:6],
    n_refs::Union{Nothing, Vector{Int}} = nothing, float_chain::Bool = true, strand::String = "+",
    ctx::Context = default_context())

    check_strand(strand)
    m = length(windowsizes)
    refmat = reduce(vcat, refVecs[1:m])                  # m x 4^k, row-major as the C side expects
    nref = n_refs === nothing ? C_NULL : Int64.(n_refs)
    check(ctx, ccall((:kgma_set_refs, libkgma), Cint,
        (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}),
        ctx.h, k, m, refmat, Int64.(windowsizes), Float64.(thr_vec[1:m]), nref))
    g0 = genome_from_fasta(ctx, genome_path)
    try
        for_strands(g0, strand) do g, minus
            st = AlignState(g, consensus_seqs, 0,
                AffineGapScoreModel(EDNAFULL, gap_open = gap_open_score, gap_extend = gap_extend_score),
                get_aligns, align_vec)
            cb = align_hits ? @cfunction(align_trampoline, Cvoid,
                (Ptr{Cvoid}, Int32, Int32, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64})) : C_NULL
            GC.@preserve st begin
                check(ctx, ccall((:kgma_scan, libkgma), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Int64, UInt32, Ptr{Cvoid}, Ptr{Cvoid}),
                    ctx.h, g.h, KGMA_MODE_OMN, buff, genome_pos, scan_flags(do_return_dists, float_chain),
                    cb, pointer_from_objref(st)))
            end
            hits = fetch_hits(ctx)
            bodies = hit_bodies(g, hits)
            for (h, body) in zip(hits, bodies)
                seq_UnitRange = Int(h.lo):Int(h.hi)
                minus && (seq_UnitRange = strand_range(contig_len(g, h.contig), seq_UnitRange))
                # record construction as in src/OmnGenomeMiner.jl:141-149
                push!(resultVec, FASTA.Record(
                    identifier(g, h.contig) *
                        " | Dist = " * string(round(h.dist, digits = 2)) *
                        " | KFV = $(h.kfv)" *
                        " | MatchPos = $seq_UnitRange" *
                        " | GenomePos = $(h.genome_pos)" *
                        " | Len = " * string(last(seq_UnitRange) - first(seq_UnitRange) + 1) *
                        (minus ? " | Strand = -" : ""),
                    body))
                get_hit_loci && push!(hit_loci_vec, first(seq_UnitRange) + h.genome_pos)
            end
            if do_return_dists
                for j in 1:m; fetch_dists!(ctx, j, dist_vec_vec[j]) end
            end
        end
    finally
        free!(g0)
    end
    return nothing
end

struct KgmaAlignment
    contig::Int32
    kfv::Int32
    lo::Int64
    hi::Int64
    first::Int64
    last::Int64
end

"""
    StrobeGMA!(; kwargs...)   -- same keywords as KmerGMA.StrobeGMA! (src/StrobemerGMA/StrobeGenomeMiner.jl:5-24)
plus `n_refs` and `float_chain`.  The scan, the re-alignment of process_hit! (src/Alignment.jl:83-111: EDNAFULL with the gap
scores of `score_model`) and its `score_threshold` gate run on the device (kgma_set_strobe_ref + kgma_strobe_scan); with
`do_return_align` the kept candidates are aligned once more on the host, only to hand BioAlignments objects back.
"""
function StrobeGMA!(; genome_path::String, refVec, consensus_refseq::KmerGMA.Seq,
    s::Int = 2, w_min::Int = 3, w_max::Int = 5, q::Int = 5, windowsize::Int64 = 289,
    thr::Union{Int64, Float64} = 33.5, ScaleFactor::Float64 = 0.166666666666666666666666666667, buff::Int64 = 50,
    do_align::Bool = true,
    score_model::AffineGapScoreModel{Int64} = AffineGapScoreModel(EDNAFULL, gap_open = -69, gap_extend = -5),
    score_threshold::Int = 0, do_return_dists::Bool = false, do_return_align::Bool = false, get_hit_loci::Bool = false,
    dist_vec = Float64[], result_align_vec = [], hit_loci_vec = Int[], genome_pos::Int = 0,
    resultVec::Vector{FASTA.Record} = FASTA.Record[], n_refs::Union{Nothing, Int} = nothing,
    float_chain::Bool = true, ctx::Context = default_context())

    genome_pos == 0 || error("StrobeGMA! starts genome_pos at 0 (StrobeGenomeMiner.jl:147)")
    check(ctx, ccall((:kgma_set_strobe_ref, libkgma), Cint,
        (Ptr{Cvoid}, Int32, Int32, Int32, Int64, Ptr{Float64}, Int64, Float64, Int64),
        ctx.h, s, w_min, w_max, q, collect(Float64, refVec), windowsize, Float64(thr), n_refs === nothing ? 0 : n_refs))
    g = genome_from_fasta(ctx, genome_path)
    try
        cons = do_align ? Vector{UInt8}(string(consensus_refseq)) : UInt8[]
        check(ctx, ccall((:kgma_strobe_scan, libkgma), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Int64, UInt32, Ptr{UInt8}, Int64, Int32, Int32, Int64),
            ctx.h, g.h, buff, scan_flags(do_return_dists, float_chain), do_align ? pointer(cons) : C_NULL, length(cons),
            score_model.gap_open, score_model.gap_extend, score_threshold))
        hits = fetch_hits(ctx)
        bodies = hit_bodies(g, hits)
        for (h, body) in zip(hits, bodies)
            seq_UnitRange = Int(h.lo):Int(h.hi)
            header = identifier(g, h.contig) *                         # append_hit! (src/Alignment.jl:69-80), do_overlap = false
                " | dist = " * string(round(h.dist, digits = 2)) *
                " | MatchPos = $seq_UnitRange" *
                " | GenomePos = $(h.genome_pos)" *
                " | Len = " * string(last(seq_UnitRange) - first(seq_UnitRange) + 1)
            push!(resultVec, FASTA.Record(header, body))
            get_hit_loci && push!(hit_loci_vec, h.lo + h.genome_pos)
        end
        if do_align && do_return_align
            n = Ref{Int64}(0)
            check(ctx, ccall((:kgma_get_alignments, libkgma), Cint, (Ptr{Cvoid}, Ptr{KgmaAlignment}, Int64, Ref{Int64}, Ptr{Int64}, Ptr{Int64}),
                             ctx.h, C_NULL, 0, n, C_NULL, C_NULL))
            al = Vector{KgmaAlignment}(undef, n[])
            check(ctx, ccall((:kgma_get_alignments, libkgma), Cint, (Ptr{Cvoid}, Ptr{KgmaAlignment}, Int64, Ref{Int64}, Ptr{Int64}, Ptr{Int64}),
                             ctx.h, al, n[], n, C_NULL, C_NULL))
            for a in al
                push!(result_align_vec, pairalign(SemiGlobalAlignment(), view(consensus_refseq, 1:windowsize),
                                                  subseq(g, a.contig, a.lo, a.hi), score_model))
            end
        end
        do_return_dists && fetch_dists!(ctx, 1, dist_vec)
    finally
        free!(g)
    end
    return nothing
end

struct KgmaMatch          # kgma_match: 0-based query and contig, 1-based start
    query::Int32
    contig::Int32
    start::Int64
end

query_text(q::FASTA.Record) = FASTA.sequence(String, q)        # convert_to_search_query, src/ExactMatch.jl:46-58
query_text(q) = string(q)

# kgma_exact_match + kgma_get_matches: every occurrence of every query in every record, sorted by (query, contig, start)
function exact_matches(g::DeviceGenome, queries::Vector{String}, overlap::Bool)
    ctx = g.ctx
    text = Vector{UInt8}(join(queries))
    offsets = Int64[0; cumsum(Int64[ncodeunits(q) for q in queries])]
    check(ctx, ccall((:kgma_exact_match, libkgma), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt8}, Ptr{Int64}, Int32, Int32),
                     ctx.h, g.h, text, offsets, length(queries), overlap ? 1 : 0))
    n = Ref{Int64}(0)
    check(ctx, ccall((:kgma_get_matches, libkgma), Cint, (Ptr{Cvoid}, Ptr{KgmaMatch}, Int64, Ref{Int64}), ctx.h, C_NULL, 0, n))
    out = Vector{KgmaMatch}(undef, n[])
    check(ctx, ccall((:kgma_get_matches, libkgma), Cint, (Ptr{Cvoid}, Ptr{KgmaMatch}, Int64, Ref{Int64}), ctx.h, out, n[], n))
    return out
end

"""
    exactMatch_batch(queries, genome; overlap = true)   -- `genome`: a FASTA path or an open DeviceGenome
exactMatch (src/ExactMatch.jl:100-121) for all queries in one pass over the genome: per query the Dict of record identifier =>
match ranges, or "no match".
"""
function exactMatch_batch(queries::Vector, genome::Union{String, DeviceGenome}; overlap::Bool = true, ctx::Context = default_context())
    g = genome isa String ? genome_from_fasta(ctx, genome) : genome
    try
        qs = String[query_text(q) for q in queries]
        dicts = [Dict{String, Vector{UnitRange{Int64}}}() for _ in qs]
        last_contig = fill(Int32(-1), length(qs))
        for m in exact_matches(g, qs, overlap)
            d, id = dicts[m.query + 1], identifier(g, m.contig)
            m.contig == last_contig[m.query + 1] || (d[id] = UnitRange{Int64}[]; last_contig[m.query + 1] = m.contig)
            push!(d[id], m.start:m.start + ncodeunits(qs[m.query + 1]) - 1)
        end
        return Any[isempty(d) ? "no match" : d for d in dicts]
    finally
        genome isa String && free!(g)
    end
end

"""
    exactMatch(query, genome; overlap = true)   -- KmerGMA.exactMatch's reader method (src/ExactMatch.jl:100-121) on the device
"""
exactMatch(query, genome::Union{String, DeviceGenome}; overlap::Bool = true, ctx::Context = default_context()) =
    exactMatch_batch([query], genome; overlap = overlap, ctx = ctx)[1]

struct KgmaMotifHit       # kgma_motif_hit: 0-based motif and contig, 1-based start
    motif::Int32
    contig::Int32
    start::Int64
    mismatches::Int32
    reserved::Int32
end

const HumanRSSV = "CACAGTG" * "N"^12 * "ACAAAAACC"            # src/RSS.jl:14-15
const HumanRSSD = "CACAGTG" * "N"^23 * "ACAAAAACC"

"""
    motifMatch(motifs, genome; max_mismatch = 0)   -- `genome`: a FASTA path or an open DeviceGenome
IUPAC motifs (1 ... 64 symbols) with at most `max_mismatch` (one number, or one per motif) non-matching positions, all in one
pass over the genome (kgma_motif_match): per motif the vector of (record identifier, range, mismatches).  A genome base matches
a symbol whose set holds it; a genome N matches only a motif N.  For the minus strand pass the reverse complement of the motif:
its matches are in forward coordinates.
"""
function motifMatch(motifs::Vector, genome::Union{String, DeviceGenome}; max_mismatch = 0, ctx::Context = default_context())
    g = genome isa String ? genome_from_fasta(ctx, genome) : genome
    try
        ms = String[query_text(m) for m in motifs]
        text = Vector{UInt8}(join(ms))
        offsets = Int64[0; cumsum(Int64[ncodeunits(m) for m in ms])]
        ds = max_mismatch isa Integer ? fill(Int32(max_mismatch), length(ms)) : Int32.(max_mismatch)
        check(ctx, ccall((:kgma_motif_match, libkgma), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt8}, Ptr{Int64}, Int32, Ptr{Int32}),
                         ctx.h, g.h, text, offsets, length(ms), ds))
        n = Ref{Int64}(0)
        check(ctx, ccall((:kgma_get_motif_matches, libkgma), Cint, (Ptr{Cvoid}, Ptr{KgmaMotifHit}, Int64, Ref{Int64}), ctx.h, C_NULL, 0, n))
        hits = Vector{KgmaMotifHit}(undef, n[])
        check(ctx, ccall((:kgma_get_motif_matches, libkgma), Cint, (Ptr{Cvoid}, Ptr{KgmaMotifHit}, Int64, Ref{Int64}), ctx.h, hits, n[], n))
        out = [Tuple{String, UnitRange{Int64}, Int}[] for _ in ms]
        for h in hits
            push!(out[h.motif + 1], (identifier(g, h.contig), h.start:h.start + ncodeunits(ms[h.motif + 1]) - 1, Int(h.mismatches)))
        end
        return out
    finally
        genome isa String && free!(g)
    end
end
motifMatch(motif, genome::Union{String, DeviceGenome}; max_mismatch::Integer = 0, ctx::Context = default_context()) =
    motifMatch([motif], genome; max_mismatch = max_mismatch, ctx = ctx)[1]

struct KgmaApproxHit      # kgma_approx_hit: 0-based query and contig, the 1-based inclusive range start:end
    query::Int32
    contig::Int32
    start::Int64
    stop::Int64
    edits::Int32
    reserved::Int32
end

struct KgmaApproxStats    # kgma_approx_stats
    tile::Int32
    wg_bases::Int32
    words::Int32
    n_launches::Int32
    n_ends::Int64
    n_hits::Int64
    search_ms::Float64
    starts_ms::Float64
end

function approx_stats(ctx::Context)
    s = Ref{KgmaApproxStats}()
    check(ctx, ccall((:kgma_get_approx_stats, libkgma), Cint, (Ptr{Cvoid}, Ref{KgmaApproxStats}), ctx.h, s))
    return s[]
end

"""
    approxMatch(queries, genome; max_edits = 1, all_ends = false)   -- `genome`: a FASTA path or an open DeviceGenome
IUPAC queries (1 ... 64 symbols) within `max_edits` (one number, or one per query) substitutions, inserted and deleted bases of a
substring of a record, all in one pass over the genome (kgma_approx_match): per query the vector of (record identifier, range,
edits) -- per run of consecutive matching ends the best one, or every matching end with `all_ends`; the range is the shortest
substring ending there that attains the edits.  Symbols match as in motifMatch.  For the minus strand pass the reverse
complement of the query: its hits are in forward coordinates.
"""
function approxMatch(queries::Vector, genome::Union{String, DeviceGenome}; max_edits = 1, all_ends::Bool = false,
                     ctx::Context = default_context())
    g = genome isa String ? genome_from_fasta(ctx, genome) : genome
    try
        qs = String[query_text(q) for q in queries]
        text = Vector{UInt8}(join(qs))
        offsets = Int64[0; cumsum(Int64[ncodeunits(q) for q in qs])]
        es = max_edits isa Integer ? fill(Int32(max_edits), length(qs)) : Int32.(max_edits)
        check(ctx, ccall((:kgma_approx_match, libkgma), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt8}, Ptr{Int64}, Int32, Ptr{Int32}, Int32),
                         ctx.h, g.h, text, offsets, length(qs), es, all_ends ? 0 : 1))
        n = Ref{Int64}(0)
        check(ctx, ccall((:kgma_get_approx_matches, libkgma), Cint, (Ptr{Cvoid}, Ptr{KgmaApproxHit}, Int64, Ref{Int64}), ctx.h, C_NULL, 0, n))
        hits = Vector{KgmaApproxHit}(undef, n[])
        check(ctx, ccall((:kgma_get_approx_matches, libkgma), Cint, (Ptr{Cvoid}, Ptr{KgmaApproxHit}, Int64, Ref{Int64}), ctx.h, hits, n[], n))
        out = [Tuple{String, UnitRange{Int64}, Int}[] for _ in qs]
        for h in hits
            push!(out[h.query + 1], (identifier(g, h.contig), h.start:h.stop, Int(h.edits)))
        end
        return out
    finally
        genome isa String && free!(g)
    end
end
approxMatch(query, genome::Union{String, DeviceGenome}; max_edits::Integer = 1, all_ends::Bool = false, ctx::Context = default_context()) =
    approxMatch([query], genome; max_edits = max_edits, all_ends = all_ends, ctx = ctx)[1]

struct KgmaPwmHit         # kgma_pwm_hit: 0-based matrix and contig, the 1-based start
    matrix::Int32
    contig::Int32
    start::Int64
    score::Int32
    reserved::Int32
end

struct KgmaPwmStats       # kgma_pwm_stats
    lane_starts::Int32
    wave_starts::Int32
    wg_starts::Int32
    n_launches::Int32
    n_candidates::Int64
    n_hits::Int64
    search_ms::Float64
end

function pwm_stats(ctx::Context)
    s = Ref{KgmaPwmStats}()
    check(ctx, ccall((:kgma_get_pwm_stats, libkgma), Cint, (Ptr{Cvoid}, Ref{KgmaPwmStats}), ctx.h, s))
    return s[]
end

"The matrix of the other strand: rows reversed, A <-> T and C <-> G swapped (`matrix` is m x 4, columns A, C, G, T)."
pwm_revcomp(matrix::AbstractMatrix{<:Integer}) = matrix[end:-1:1, end:-1:1]

"""
    pwmMatch(matrices, genome; threshold)   -- `genome`: a FASTA path or an open DeviceGenome
Position weight matrices (m x 4 integer weights, columns A, C, G, T, 1 <= m <= 64, each weight an Int16) laid on every start of
every record, all in one pass over the genome (kgma_pwm_match): per matrix the vector of (record identifier, range, score) with
score = the sum of the weights of the residues under the rows >= `threshold` (one number, or one per matrix; it must exceed the
sum of the row minima).  A genome N scores its row's minimum.  For the minus strand pass `pwm_revcomp(matrix)`: its hits are in
forward coordinates.
"""
function pwmMatch(matrices::Vector{<:AbstractMatrix{<:Integer}}, genome::Union{String, DeviceGenome}; threshold,
                  ctx::Context = default_context())
    all(m -> size(m, 2) == 4, matrices) || throw(ArgumentError("a matrix has four columns: A, C, G, T"))
    g = genome isa String ? genome_from_fasta(ctx, genome) : genome
    try
        weights = Int16[]
        for m in matrices, i in 1:size(m, 1), b in 1:4
            push!(weights, Int16(m[i, b]))                    # rows of four, matrices back to back (InexactError: a weight out of range)
        end
        offsets = Int64[0; cumsum(Int64[size(m, 1) for m in matrices])]
        ts = threshold isa Integer ? fill(Int32(threshold), length(matrices)) : Int32.(threshold)
        length(ts) == length(matrices) || throw(ArgumentError("need one threshold per matrix"))
        check(ctx, ccall((:kgma_pwm_match, libkgma), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int16}, Ptr{Int64}, Int32, Ptr{Int32}),
                         ctx.h, g.h, weights, offsets, length(matrices), ts))
        n = Ref{Int64}(0)
        check(ctx, ccall((:kgma_get_pwm_matches, libkgma), Cint, (Ptr{Cvoid}, Ptr{KgmaPwmHit}, Int64, Ref{Int64}), ctx.h, C_NULL, 0, n))
        hits = Vector{KgmaPwmHit}(undef, n[])
        check(ctx, ccall((:kgma_get_pwm_matches, libkgma), Cint, (Ptr{Cvoid}, Ptr{KgmaPwmHit}, Int64, Ref{Int64}), ctx.h, hits, n[], n))
        out = [Tuple{String, UnitRange{Int64}, Int}[] for _ in matrices]
        for h in hits
            m = size(matrices[h.matrix + 1], 1)
            push!(out[h.matrix + 1], (identifier(g, h.contig), h.start:(h.start + m - 1), Int(h.score)))
        end
        return out
    finally
        genome isa String && free!(g)
    end
end
pwmMatch(matrix::AbstractMatrix{<:Integer}, genome::Union{String, DeviceGenome}; threshold::Integer, ctx::Context = default_context()) =
    pwmMatch([matrix], genome; threshold = threshold, ctx = ctx)[1]

# ---- protMatch: amino-acid profiles in all reading frames (kgma_codon_match, kgma_codon_fold) -------------------------------

struct KgmaCodonHit       # kgma_codon_hit: 0-based matrix and contig, the 1-based nucleotide start
    matrix::Int32
    contig::Int32
    start::Int64
    score::Int32
    reserved::Int32
end

struct KgmaCodonStats     # kgma_codon_stats
    lane_starts::Int32
    wave_starts::Int32
    wg_starts::Int32
    n_launches::Int32
    n_candidates::Int64
    n_hits::Int64
    search_ms::Float64
end

function codon_stats(ctx::Context)
    s = Ref{KgmaCodonStats}()
    check(ctx, ccall((:kgma_get_codon_stats, libkgma), Cint, (Ptr{Cvoid}, Ref{KgmaCodonStats}), ctx.h, s))
    return s[]
end

const AMINO_ACIDS = "ACDEFGHIKLMNPQRSTVWY*"        # the 21 columns of an amino-acid profile; '*' is the stop
const GENETIC_CODE_1 = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"   # NCBI table 1, TCAG order

"""
    genetic_code(letters = GENETIC_CODE_1)
64 column numbers (0 ... 20, into AMINO_ACIDS) indexed by the codon 16 b0 + 4 b1 + b2 (A 0, C 1, G 2, T 3), from an NCBI-style
string of 64 letters in TCAG order: what kgma_codon_fold takes.
"""
function genetic_code(letters::AbstractString = GENETIC_CODE_1)
    length(letters) == 64 || throw(ArgumentError("a genetic code has 64 letters"))
    tcag = (2, 1, 3, 0)                                # where A, C, G, T stand in T, C, A, G
    code = Vector{UInt8}(undef, 64)
    for c in 0:63
        i = 16 * tcag[(c >> 4) + 1] + 4 * tcag[((c >> 2) & 3) + 1] + tcag[(c & 3) + 1]
        col = findfirst(==(uppercase(letters[i + 1])), AMINO_ACIDS)
        col === nothing && throw(ArgumentError("genetic code: letter $(i + 1) is none of $AMINO_ACIDS"))
        code[c + 1] = UInt8(col - 1)
    end
    return code
end

"""
    codon_fold(profile; code = genetic_code(), x_weight = minimum(profile, dims = 2), minus = false)
The m x 65 codon matrix of one strand (kgma_codon_fold; host only) from an m x 21 amino-acid profile (columns AMINO_ACIDS):
entry 64 (0-based) of a row, a codon with an N, is `x_weight`; `minus`: the rows reversed, each codon read as its reverse complement.
"""
function codon_fold(profile::AbstractMatrix{<:Integer}; code::Vector{UInt8} = genetic_code(),
                    x_weight = vec(minimum(profile, dims = 2)), minus::Bool = false)
    size(profile, 2) == 21 || throw(ArgumentError("a profile has 21 columns: $AMINO_ACIDS"))
    m = size(profile, 1)
    aa = Int16[profile[i, a] for i in 1:m for a in 1:21]   # rows of 21
    out = Vector{Int16}(undef, 65 * m)
    st = ccall((:kgma_codon_fold, libkgma), Cint, (Ptr{Int16}, Int32, Ptr{UInt8}, Ptr{Int16}, Int32, Ptr{Int16}),
               aa, m, code, Int16.(x_weight), minus ? 1 : 0, out)
    st == 0 || throw(ArgumentError("kgma_codon_fold: 1 ... 64 rows and code entries 0 ... 20"))
    return permutedims(reshape(Int.(out), 65, m))          # m x 65
end

"""
    protMatch(profiles, genome; threshold, strand = "+", code = genetic_code())   -- `genome`: a FASTA path or an open DeviceGenome
Amino-acid profiles (m x 21 integer weights, columns AMINO_ACIDS, 1 <= m <= 64) laid on every nucleotide start of every record in
every reading frame of the strands asked for, all in one pass over the genome (kgma_codon_match): per profile the vector of
(record identifier, range, strand, frame, score) with score >= `threshold` (one number, or one per profile; it must exceed the sum
of the row minima).  A codon with an N scores its row's minimum.  Ranges are forward coordinates; frame is (lo - 1) mod 3 + 1 on the
plus strand and -((L - hi) mod 3 + 1) on the minus strand.
"""
function protMatch(profiles::Vector{<:AbstractMatrix{<:Integer}}, genome::Union{String, DeviceGenome}; threshold, strand::String = "+",
                   code::Vector{UInt8} = genetic_code(), ctx::Context = default_context())
    strand in ("+", "-", "both") || throw(ArgumentError("strand is \"+\", \"-\" or \"both\""))
    ts = threshold isa Integer ? fill(Int32(threshold), length(profiles)) : Int32.(threshold)
    length(ts) == length(profiles) || throw(ArgumentError("need one threshold per profile"))
    g = genome isa String ? genome_from_fasta(ctx, genome) : genome
    try
        weights, rows, sent_t, tags = Int16[], Int64[], Int32[], Tuple{Int, String}[]
        for (i, p) in enumerate(profiles), st in ("+", "-")
            (strand == "both" || strand == st) || continue
            W = codon_fold(p; code = code, minus = st == "-")
            for r in 1:size(W, 1), e in 1:65
                push!(weights, Int16(W[r, e]))                # rows of 65, matrices back to back
            end
            push!(rows, size(W, 1)); push!(sent_t, ts[i]); push!(tags, (i, st))
        end
        offsets = Int64[0; cumsum(rows)]
        check(ctx, ccall((:kgma_codon_match, libkgma), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int16}, Ptr{Int64}, Int32, Ptr{Int32}),
                         ctx.h, g.h, weights, offsets, length(rows), sent_t))
        n = Ref{Int64}(0)
        check(ctx, ccall((:kgma_get_codon_matches, libkgma), Cint, (Ptr{Cvoid}, Ptr{KgmaCodonHit}, Int64, Ref{Int64}), ctx.h, C_NULL, 0, n))
        hits = Vector{KgmaCodonHit}(undef, n[])
        check(ctx, ccall((:kgma_get_codon_matches, libkgma), Cint, (Ptr{Cvoid}, Ptr{KgmaCodonHit}, Int64, Ref{Int64}), ctx.h, hits, n[], n))
        out = [Tuple{String, UnitRange{Int64}, String, Int, Int}[] for _ in profiles]
        for h in hits
            i, st = tags[h.matrix + 1]
            lo = h.start
            hi = lo + 3 * size(profiles[i], 1) - 1
            L = ccall((:kgma_genome_contig_len, libkgma), Int64, (Ptr{Cvoid}, Int64), g.h, h.contig)
            frame = st == "+" ? Int(mod(lo - 1, 3) + 1) : -Int(mod(L - hi, 3) + 1)
            push!(out[i], (identifier(g, h.contig), lo:hi, st, frame, Int(h.score)))
        end
        return out
    finally
        genome isa String && free!(g)
    end
end
protMatch(profile::AbstractMatrix{<:Integer}, genome::Union{String, DeviceGenome}; threshold::Integer, strand::String = "+",
          code::Vector{UInt8} = genetic_code(), ctx::Context = default_context()) =
    protMatch([profile], genome; threshold = threshold, strand = strand, code = code, ctx = ctx)[1]

# ---- threshold calibration (the working form of src/DistanceTesting.jl): kgma_window_dists, kgma_mutation_dists -------------

"""
    window_dists(g, kfv, contig, start) -> (D, dist)
The distance to KFV `kfv` (1-based, of the references last given to the context) of the windows that begin at `start[i]` (1-based)
of record `contig[i]` (0-based); the window size is that KFV's.  D: the exact integer distance of an S/N KFV.
"""
function window_dists(g::DeviceGenome, kfv::Integer, contig::Vector{Int32}, start::Vector{Int64})
    ctx = g.ctx
    n = length(contig)
    length(start) == n || throw(ArgumentError("need one start per contig"))
    D = Vector{Int64}(undef, n); dist = Vector{Float64}(undef, n)
    check(ctx, ccall((:kgma_window_dists, libkgma), Cint,
                     (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Ptr{Int32}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}),
                     ctx.h, g.h, kfv, n, contig, start, D, dist))
    return D, dist
end

"""
    mutation_dists(ctx, seqs, kfv, rates; n_trials = 42, seed = 42) -> (D, dist), each [trial, rate, sequence]
kmer_dist(mutate_seq(seq, rate), KFV, k) for every sequence, rate and trial (the inner step of gen_sub_vs_ref), the mutated
copies never materialised.  The substitutions come from a counter-based hash (include/kgma.h), not from Julia's RNG.
"""
function mutation_dists(ctx::Context, seqs::Vector{String}, kfv::Integer, rates::Vector{Float64}; n_trials::Integer = 42, seed::Integer = 42)
    text = Vector{UInt8}(join(seqs))
    offsets = Int64[0; cumsum(Int64[ncodeunits(s) for s in seqs])]
    D = Array{Int64}(undef, n_trials, length(rates), length(seqs)); dist = Array{Float64}(undef, n_trials, length(rates), length(seqs))
    check(ctx, ccall((:kgma_mutation_dists, libkgma), Cint,
                     (Ptr{Cvoid}, Int32, Ptr{UInt8}, Ptr{Int64}, Int64, Ptr{Float64}, Int32, Int32, UInt64, Ptr{Int64}, Ptr{Float64}),
                     ctx.h, kfv, text, offsets, length(seqs), rates, length(rates), n_trials, seed % UInt64, D, dist))
    return D, dist
end

"""
    strobe_window_dists(g, contig, start) -> (D, dist)
The same for the strobemer reference last given to the context (kgma_set_strobe_ref): the strobemer scan's window with start
`start[i]` (1 ... max(1, L - W)) of record `contig[i]` -- W - k + 1 randstrobes, the record's permanent one included for start >= 2.
dist = D / (2 k N^2), k = w_max + s - 1.
"""
function strobe_window_dists(g::DeviceGenome, contig::Vector{Int32}, start::Vector{Int64})
    ctx = g.ctx
    n = length(contig)
    length(start) == n || throw(ArgumentError("need one start per contig"))
    D = Vector{Int64}(undef, n); dist = Vector{Float64}(undef, n)
    check(ctx, ccall((:kgma_strobe_window_dists, libkgma), Cint,
                     (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Int32}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}),
                     ctx.h, g.h, n, contig, start, D, dist))
    return D, dist
end

"""
    strobe_mutation_dists(ctx, seqs, rates; n_trials = 42, seed = 42) -> (D, dist), each [trial, rate, sequence]
The distance of the strobemer reference to the randstrobe counts of mutate_seq(seq, rate) for every sequence, rate and trial: the
working form of test_strobe_2_mer_dists (src/StrobemerGMA/MonteCarloBenchmark.jl:2-23).
"""
function strobe_mutation_dists(ctx::Context, seqs::Vector{String}, rates::Vector{Float64}; n_trials::Integer = 42, seed::Integer = 42)
    text = Vector{UInt8}(join(seqs))
    offsets = Int64[0; cumsum(Int64[ncodeunits(s) for s in seqs])]
    D = Array{Int64}(undef, n_trials, length(rates), length(seqs)); dist = Array{Float64}(undef, n_trials, length(rates), length(seqs))
    check(ctx, ccall((:kgma_strobe_mutation_dists, libkgma), Cint,
                     (Ptr{Cvoid}, Ptr{UInt8}, Ptr{Int64}, Int64, Ptr{Float64}, Int32, Int32, UInt64, Ptr{Int64}, Ptr{Float64}),
                     ctx.h, text, offsets, length(seqs), rates, length(rates), n_trials, seed % UInt64, D, dist))
    return D, dist
end

# ---- gene assignment (kgma_assign_seqs, kgma_assign_ranges) ---------------------------------------------------------------------
"One reference a hit was aligned to: mirrors kgma_assignment (include/kgma.h), `ref` 0-based as in the C ABI."
struct KgmaAssignment
    ref::Int32; score::Int32; n_eq::Int32; n_x::Int32; n_ins::Int32; n_del::Int32; q_lo::Int32; q_hi::Int32
end
const Assignment = NamedTuple{(:ref_id, :ref_index, :score, :identity, :n_eq, :n_x, :n_ins, :n_del, :q_lo, :q_hi),
                              Tuple{String, Int, Int, Float64, Int, Int, Int, Int, Int, Int}}

function assignment(ids::Vector{String}, a::KgmaAssignment)
    d = a.n_eq + a.n_x + a.n_ins + a.n_del
    return Assignment((ids[a.ref + 1], a.ref + 1, a.score, d == 0 ? 0.0 : a.n_eq / d, a.n_eq, a.n_x, a.n_ins, a.n_del, a.q_lo, a.q_hi))
end

function assign_refs(ref)
    recs = ref isa String ? open(collect, FASTA.Reader, ref) : ref
    ids = String[r isa FASTA.Record ? String(FASTA.identifier(r)) : "" for r in recs]
    seqs = String[r isa FASTA.Record ? String(FASTA.sequence(r)) : String(r) for r in recs]
    return ids, seqs
end

pack_seqs(seqs::Vector{String}) = (Vector{UInt8}(join(seqs)), Int64[0; cumsum(Int64[ncodeunits(s) for s in seqs])])

"""
    assignGenes(hits, ref; top = 1, gap_open_score = -69, gap_extend_score = -1, annotate = false) -> Vector{Vector{Assignment}}
Names every hit's nearest reference genes: every hit record's body against every reference (a FASTA path or records) under the
hit aligner's model on the device, per hit its `top` references (higher score first, the earlier reference among equal scores)
with the column counts of that alignment; `ref_index` is 1-based here.  `annotate = true` returns copies of the records with
` | Ref = <id> | Identity = <x.xxx>` appended to the description instead.
"""
function assignGenes(hits::Vector{FASTA.Record}, ref; top::Integer = 1, gap_open_score::Integer = -69, gap_extend_score::Integer = -1,
                     annotate::Bool = false, ctx::Context = default_context())
    ids, refs = assign_refs(ref)
    isempty(hits) && return annotate ? FASTA.Record[] : Vector{Assignment}[]
    rtext, roff = pack_seqs(refs)
    qtext, qoff = pack_seqs(String[String(FASTA.sequence(h)) for h in hits])
    out = Matrix{KgmaAssignment}(undef, top, length(hits))            # [t, hit]: the C ABI's out[hit * top + t]
    check(ctx, ccall((:kgma_assign_seqs, libkgma), Cint,
                     (Ptr{Cvoid}, Ptr{UInt8}, Ptr{Int64}, Int32, Ptr{UInt8}, Ptr{Int64}, Int64, Int32, Int32, Int32, Ptr{KgmaAssignment}, Ptr{Int32}),
                     ctx.h, rtext, roff, length(refs), qtext, qoff, length(hits), gap_open_score, gap_extend_score, top, out, C_NULL))
    res = [Assignment[assignment(ids, out[t, i]) for t in 1:top] for i in eachindex(hits)]
    annotate || return res
    return [FASTA.Record(string(FASTA.description(h), " | Ref = ", a[1].ref_id, " | Identity = ", @sprintf("%.3f", a[1].identity)),
                         FASTA.sequence(h)) for (h, a) in zip(hits, res)]
end

"""
    assign_ranges(g, contig, lo, hi, ref; top = 1, ...) -> Vector{Vector{Assignment}}
The same for ranges lo[i]:hi[i] (1-based, inclusive) of record contig[i] (0-based, as in the C ABI) of an open DeviceGenome.
"""
function assign_ranges(g::DeviceGenome, contig::Vector{Int32}, lo::Vector{Int64}, hi::Vector{Int64}, ref; top::Integer = 1,
                       gap_open_score::Integer = -69, gap_extend_score::Integer = -1)
    ctx = g.ctx
    n = length(contig)
    length(lo) == n == length(hi) || throw(ArgumentError("need one lo and one hi per contig"))
    ids, refs = assign_refs(ref)
    rtext, roff = pack_seqs(refs)
    out = Matrix{KgmaAssignment}(undef, top, n)
    check(ctx, ccall((:kgma_assign_ranges, libkgma), Cint,
                     (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt8}, Ptr{Int64}, Int32, Int64, Ptr{Int32}, Ptr{Int64}, Ptr{Int64}, Int32, Int32, Int32,
                      Ptr{KgmaAssignment}, Ptr{Int32}),
                     ctx.h, g.h, rtext, roff, length(refs), n, contig, lo, hi, gap_open_score, gap_extend_score, top, out, C_NULL))
    return [Assignment[assignment(ids, out[t, i]) for t in 1:top] for i in 1:n]
end

# ---- all-pairs k-mer distances (kgma_kmer_dist_matrix, kgma_kmer_nearest) and the prescreened assignment ------------------------
"""
    kmer_dist_matrix(seqs_a, seqs_b = nothing; k = 6, integer = false) -> Matrix
`kmer_dist(a, b, k)` of every sequence of `seqs_a` to every sequence of `seqs_b` on the device (`nothing`: A against A): the
Float64 matrix [a, b], bit for bit the package's values, or with `integer = true` the exact Int32 D = Σ (c_a − c_b)².
"""
function kmer_dist_matrix(seqs_a::Vector{String}, seqs_b::Union{Nothing, Vector{String}} = nothing; k::Integer = 6, integer::Bool = false,
                          ctx::Context = default_context())
    atext, aoff = pack_seqs(seqs_a)
    nb = seqs_b === nothing ? length(seqs_a) : length(seqs_b)
    btext, boff = seqs_b === nothing ? (C_NULL, C_NULL) : pack_seqs(seqs_b)
    D = Matrix{Int32}(undef, nb, length(seqs_a))                      # [b, a]: the C ABI's row-major D[a][b]
    dist = Matrix{Float64}(undef, nb, length(seqs_a))
    check(ctx, ccall((:kgma_kmer_dist_matrix, libkgma), Cint,
                     (Ptr{Cvoid}, Int32, Ptr{UInt8}, Ptr{Int64}, Int64, Ptr{UInt8}, Ptr{Int64}, Int32, Ptr{Int32}, Ptr{Float64}),
                     ctx.h, k, atext, aoff, length(seqs_a), btext, boff, seqs_b === nothing ? 0 : nb, D, dist))
    return integer ? permutedims(D) : permutedims(dist)
end

"The same with ranges lo[i]:hi[i] (1-based, inclusive; hi = lo - 1: empty) of record contig[i] (0-based) of an open DeviceGenome as A."
function kmer_dist_matrix_ranges(g::DeviceGenome, contig::Vector{Int32}, lo::Vector{Int64}, hi::Vector{Int64}, seqs_b::Vector{String};
                                 k::Integer = 6, integer::Bool = false)
    btext, boff = pack_seqs(seqs_b)
    D = Matrix{Int32}(undef, length(seqs_b), length(contig))
    dist = Matrix{Float64}(undef, length(seqs_b), length(contig))
    check(g.ctx, ccall((:kgma_kmer_dist_matrix_ranges, libkgma), Cint,
                       (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Ptr{Int32}, Ptr{Int64}, Ptr{Int64}, Ptr{UInt8}, Ptr{Int64}, Int32, Ptr{Int32}, Ptr{Float64}),
                       g.ctx.h, g.h, k, length(contig), contig, lo, hi, btext, boff, length(seqs_b), D, dist))
    return integer ? permutedims(D) : permutedims(dist)
end

"""
    nearest_refs(hits, ref; k = 6, n = 1) -> Vector{Vector{Tuple{String, Int, Float64}}}
Per hit its `n` nearest references by k-mer distance, nearest first, the earlier reference among equal distances:
(ref_id, ref_index (1-based), dist).  The matrix stays on the device (kgma_kmer_nearest; kgma_kmer_nearest_ranges takes ranges).
"""
function nearest_refs(hits::Vector{FASTA.Record}, ref; k::Integer = 6, n::Integer = 1, ctx::Context = default_context())
    ids, refs = assign_refs(ref)
    qtext, qoff = pack_seqs(String[String(FASTA.sequence(h)) for h in hits])
    rtext, roff = pack_seqs(refs)
    index = Matrix{Int32}(undef, n, length(hits))
    Dn = Matrix{Int32}(undef, n, length(hits))
    check(ctx, ccall((:kgma_kmer_nearest, libkgma), Cint,
                     (Ptr{Cvoid}, Int32, Ptr{UInt8}, Ptr{Int64}, Int64, Ptr{UInt8}, Ptr{Int64}, Int32, Int32, Ptr{Int32}, Ptr{Int32}),
                     ctx.h, k, qtext, qoff, length(hits), rtext, roff, length(refs), n, index, Dn))
    return [[(ids[index[t, i] + 1], Int(index[t, i]) + 1, (1.0 / (2k)) * Dn[t, i]) for t in 1:n] for i in eachindex(hits)]
end

"""
    assignGenes_screened(hits, ref; prescreen = 8, prescreen_k = 6, top = 1, ...) -> Vector{Vector{Assignment}}
`assignGenes` over every hit's `prescreen` nearest references by k-mer distance only (kgma_assign_seqs_screened; the ranges form
is kgma_assign_ranges_screened with kgma_assign_ranges' arguments plus screen_k and n_near).  A residue outside A/C/G/T/N is an
error here, whereas `assignGenes` counts it as N.
"""
function assignGenes_screened(hits::Vector{FASTA.Record}, ref; prescreen::Integer = 8, prescreen_k::Integer = 6, top::Integer = 1,
                              gap_open_score::Integer = -69, gap_extend_score::Integer = -1, ctx::Context = default_context())
    ids, refs = assign_refs(ref)
    isempty(hits) && return Vector{Assignment}[]
    rtext, roff = pack_seqs(refs)
    qtext, qoff = pack_seqs(String[String(FASTA.sequence(h)) for h in hits])
    out = Matrix{KgmaAssignment}(undef, top, length(hits))
    check(ctx, ccall((:kgma_assign_seqs_screened, libkgma), Cint,
                     (Ptr{Cvoid}, Ptr{UInt8}, Ptr{Int64}, Int32, Ptr{UInt8}, Ptr{Int64}, Int64, Int32, Int32, Int32, Int32, Int32,
                      Ptr{KgmaAssignment}, Ptr{Int32}, Ptr{Int32}),
                     ctx.h, rtext, roff, length(refs), qtext, qoff, length(hits), gap_open_score, gap_extend_score, top, prescreen_k, prescreen,
                     out, C_NULL, C_NULL))
    return [Assignment[assignment(ids, out[t, i]) for t in 1:top] for i in eachindex(hits)]
end

# ---- distance landscape (kgma_dist_layout, kgma_dist_bins, kgma_dist_sweep): reductions over the distances the last scan kept ------
# (like the rest of this shim these three calls have not been executed: no Julia on the build machines; the Python binding in
#  _lib.py makes the same calls with the same argument types and is what the tests run)
"dist_layout(ctx) -> offsets: record c's values are offset[c] + 1 : offset[c + 1] of the distance vector; value i is window start i + 1."
function dist_layout(ctx::Context)
    n = Ref{Int64}(0)
    check(ctx, ccall((:kgma_dist_layout, libkgma), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int64, Ptr{Int64}), ctx.h, C_NULL, 0, n))
    offset = Vector{Int64}(undef, n[])
    check(ctx, ccall((:kgma_dist_layout, libkgma), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int64, Ptr{Int64}), ctx.h, offset, n[], n))
    return offset
end

"""
    dist_bins(ctx; kfv = 1, bin = 1) -> (bin_min, bin_argmin, bin_offset)
Minimum and window start (1-based, within the record) of the first window attaining it, per `bin` consecutive windows of every
record; record c's bins are bin_offset[c] + 1 : bin_offset[c + 1].  Needs a scan with the distances kept.
"""
function dist_bins(ctx::Context; kfv::Integer = 1, bin::Integer = 1)
    offset = Vector{Int64}(undef, length(dist_layout(ctx)))
    n = Ref{Int64}(0)
    sig = (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64})
    check(ctx, ccall((:kgma_dist_bins, libkgma), Cint, sig, ctx.h, kfv, bin, C_NULL, C_NULL, offset, 0, n))
    bmin, barg = Vector{Float64}(undef, n[]), Vector{Int64}(undef, n[])
    check(ctx, ccall((:kgma_dist_bins, libkgma), Cint, sig, ctx.h, kfv, bin, bmin, barg, offset, n[], n))
    return bmin, barg, offset
end

"dist_sweep(ctx, thresholds; kfv = 1) -> (windows_below, dips_below) per threshold (finite, strictly increasing, at most 4096)."
function dist_sweep(ctx::Context, thresholds::Vector{Float64}; kfv::Integer = 1)
    below, dips = Vector{Int64}(undef, length(thresholds)), Vector{Int64}(undef, length(thresholds))
    check(ctx, ccall((:kgma_dist_sweep, libkgma), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}),
                     ctx.h, kfv, thresholds, length(thresholds), below, dips))
    return below, dips
end

# ---- k-mer counts of the resident genome (kgma_genome_kmer_count) ---------------------------------------------------------------
# (not executed either; _lib.py's Context.genome_kmer_count makes the same call with the same argument types)
const KGMA_COUNT_SKIP_N = UInt32(1)
const KGMA_COUNT_SKIP_MASKED = UInt32(2)
const KGMA_COUNT_BY_START = UInt32(4)

"""
    genome_kmer_count(g, k, contig, lo, hi; skip_n = false, skip_masked = false, by_start = false) -> (counts, skipped)
`counts[:, r]` is `kmer_count(view(seq, lo[r]:hi[r]), k)` of record `contig[r]` (0-based; lo:hi 1-based inclusive, hi = lo - 1 is
empty) of the resident genome -- 4^k Int64, k-mer value + 1 as the row index, first base most significant --, `skipped[r]` the
considered starts the flags left out.  skip_n: a k-mer with a byte outside A/C/G/T is skipped (default: N counts as T, anything
else is the reference's KeyError); skip_masked: so is one with a lower-case byte; by_start: a k-mer belongs to the range it
starts in.  1 <= k <= 10.
"""
function genome_kmer_count(g::DeviceGenome, k::Integer, contig::Vector{Int32}, lo::Vector{Int64}, hi::Vector{Int64};
                           skip_n::Bool = false, skip_masked::Bool = false, by_start::Bool = false)
    flags = (skip_n ? KGMA_COUNT_SKIP_N : UInt32(0)) | (skip_masked ? KGMA_COUNT_SKIP_MASKED : UInt32(0)) |
            (by_start ? KGMA_COUNT_BY_START : UInt32(0))
    counts = Matrix{Int64}(undef, 4^k, length(contig))
    skipped = Vector{Int64}(undef, length(contig))
    check(g.ctx, ccall((:kgma_genome_kmer_count, libkgma), Cint,
                       (Ptr{Cvoid}, Ptr{Cvoid}, Int32, UInt32, Int64, Ptr{Int32}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
                       g.ctx.h, g.h, k, flags, length(contig), contig, lo, hi, counts, skipped))
    return counts, skipped
end

export ac_gma_testing!, Omn_KmerGMA!, record_KmerGMA!, StrobeGMA!, exactMatch, exactMatch_batch, motifMatch, approxMatch, pwmMatch, pwm_revcomp, protMatch, codon_fold, genetic_code, HumanRSSV, HumanRSSD, Context
export dist_layout, dist_bins, dist_sweep
export window_dists, mutation_dists, strobe_window_dists, strobe_mutation_dists, assignGenes, assign_ranges
export kmer_dist_matrix, kmer_dist_matrix_ranges, nearest_refs, assignGenes_screened
export genome_kmer_count

end # module
