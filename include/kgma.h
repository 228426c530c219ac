/*
 * kgma.h -- C ABI of libkgma: the MI355X (gfx950) implementation of KmerGMA.jl's
 * sliding-window k-mer-distance genome scan.
 *
 * Drop-in boundary.  The reference (Julia, no FFI of its own) exposes the scan as two
 * keyword-only engine functions that API.jl and the tests call directly:
 *
 *   ac_gma_testing!(; genome_path, refVec, consensus_refseq, k, windowsize, thr, buff, mask,
 *                     Nt_bits, ScaleFactor, do_align, ..., resultVec)       src/GenomeMiner.jl:4-23
 *   Omn_KmerGMA!(;    genome_path, refVecs, windowsizes, consensus_seqs, resultVec, k, ScaleFactor,
 *                     mask, thr_vec, buff, ..., dist_vec_vec)               src/OmnGenomeMiner.jl:7-30
 *
 * A Julia shim with those signatures `ccall`s the entry points below (INTEGRATION.md shows the
 * binding); the per-record body of both engines (src/GenomeMiner.jl:32-107,
 * src/OmnGenomeMiner.jl:55-160) is what this library replaces.  FASTA parsing, reference
 * preparation, BioAlignments re-alignment and FASTA-record construction stay on the host.
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary: every call returns a KGMA_* status (0 = OK);
 *     kgma_last_error() gives the message for the last failing call on that context.
 *   - all sequence coordinates are 1-BASED and inclusive, exactly as in the reference.
 *   - the caller owns every buffer it passes in; the library copies what it keeps.
 *   - a context is bound to one GPU and is not thread-safe; use one context per host thread/task.
 *   - there is NO CPU fallback: kgma_create fails with KGMA_E_NODEVICE when no gfx950 device
 *     (or no HIP runtime) is available.
 */
#ifndef KGMA_H
#define KGMA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KGMA_VERSION_MAJOR 0
#define KGMA_VERSION_MINOR 1

/* status codes */
enum {
    KGMA_OK = 0,
    KGMA_E_ARG = 1,         /* invalid argument (also k >= windowsize: error() at src/API.jl:70,177) */
    KGMA_E_NODEVICE = 2,    /* no usable HIP device / runtime                                      */
    KGMA_E_HIP = 3,         /* a HIP runtime call failed                                           */
    KGMA_E_BADBASE = 4,     /* residue outside A/C/G/T/N (either case): KeyError, src/Consts.jl:22-28 */
    KGMA_E_BOUNDS = 5,      /* record shorter than k-1 in the cluster engine: BoundsError, src/OmnGenomeMiner.jl:84-86 */
    KGMA_E_UNSUPPORTED = 6, /* parameters outside what the device path implements                  */
    KGMA_E_OVERFLOW = 7,    /* a device-side record buffer overflowed even after regrowth           */
    KGMA_E_NOMEM = 8,
    KGMA_E_STATE = 9        /* call sequence error (e.g. scan before set_refs)                      */
};

/* engine selector for kgma_scan */
enum {
    KGMA_MODE_SINGLE = 0,   /* ac_gma_testing!  src/GenomeMiner.jl:4-109   (uses KFV 1 only)          */
    KGMA_MODE_OMN = 1,      /* Omn_KmerGMA!     src/OmnGenomeMiner.jl:7-162 (all KFVs, lock-step)     */
    KGMA_MODE_STROBE = 2    /* StrobeGMA!       src/StrobemerGMA/StrobeGenomeMiner.jl:5-95 (after kgma_set_strobe_ref) */
};

/* flags for kgma_scan */
enum {
    KGMA_F_RETURN_DISTS = 1u << 0,  /* do_return_dists: keep the per-window distances on the device
                                       for kgma_get_dists (8 B per window per KFV)                   */
    KGMA_F_NO_TIE_RESOLVE = 1u << 1,/* keep exact-arithmetic tie-breaking (first tied window) instead of
                                       replaying the reference's Float64 rounding over tied minima   */
    KGMA_F_CHAIN_REPLAY = 1u << 2   /* (kgma_scan) decide every rounding-dependent choice the way the
                                       reference's running Float64 value does: for each (record, KFV) in
                                       which exact arithmetic has a tie -- equal minima, a minimum equal
                                       to the stale running minimum, a window exactly at the threshold --
                                       the reference's Float64 update (GenomeMiner.jl:46-47,70-77) is
                                       re-run from the record's first window and the decisions are taken
                                       from those values.  The chain runs ON THE DEVICE (a variant of the
                                       scan kernel forms every window's increment in the reference's
                                       operation order; the host adds one integer per 4096-window chunk and
                                       the raw increments where the value may change binade or is wanted:
                                       kgma_device.h): stream8_kernel's chain variant for k = 5 ... 7 and KFVs whose entries
                                       are S * (1/N) or S / N bit for bit, the generic chain kernel (kgma_generic.hip: it
                                       forms the increments from the caller's own Float64 table) for every other k, window
                                       and KFV; host threads (about 1.8 ns per window) only when a walk fails a check or
                                       the device buffers do not fit.  kgma_stats.chain_* report both.  No dip is
                                       left KGMA_HIT_TIE / KGMA_HIT_AT_THRESHOLD.  CONVENTION: the first
                                       window's sqeuclidean is summed left to right; Julia leaves the order of
                                       that @simd reduction to the machine, so "identical to the reference"
                                       means identical under this convention (it is order-free when N is a
                                       power of two).  Ignored with KGMA_F_NO_TIE_RESOLVE and by
                                       kgma_replay_dips (no residues on that rank).                    */
};

/* flags in kgma_hit.flags / kgma_dip.flags */
enum {
    KGMA_HIT_TIE = 1u << 0,        /* the dip's minimum is attained at >=2 positions that are not one
                                      contiguous plateau: exact arithmetic reports the FIRST; the
                                      reference's choice there depends on Float64 rounding noise     */
    KGMA_HIT_AT_THRESHOLD = 1u << 1,/* the window before the dip, or its exit window, has a distance
                                      within a relative 2^-30 of thr (the guard band described at
                                      kgma_set_refs): whether the reference sees it below thr is
                                      Float64 rounding noise; the library counts it as NOT below       */
    KGMA_HIT_TIE_RESOLVED = 1u << 2,/* a tie of the kind above, decided the way the reference's Float64
                                      update decides it (host replay over the tied stretch; the order is
                                      independent of the chain's history, see kgma_api.cpp)           */
    KGMA_HIT_CHAIN = 1u << 3        /* the dip belongs to a (record, KFV) pair decided by the Float64 chain
                                      replay (KGMA_F_CHAIN_REPLAY): window choice, threshold side and
                                      kgma_hit.dist are the reference's running Float64 value          */
};

typedef struct kgma_ctx kgma_ctx;
typedef struct kgma_genome kgma_genome;

/* One accepted hit, in the reference's emission order.
 * single engine: cmi = CMI after `CMI += 1` (GenomeMiner.jl:92) = best window start + k - 1;
 * cluster engine: cmi = CMIs[ind] (OmnGenomeMiner.jl:117,123) = best window start - 1.
 * lo:hi = seq_UnitRange (after the align callback if one was given). */
typedef struct {
    int32_t contig;      /* 0-based index of the record in the genome                          */
    int32_t kfv;         /* 1-based KFV index (cluster engine); 0 for the single engine        */
    int64_t cmi;
    int64_t lo, hi;
    int64_t genome_pos;  /* GenomeMiner.jl:25,106 / OmnGenomeMiner.jl:25,159                   */
    double dist;         /* currminim = D / (2 k N^2)                                          */
    int64_t D;           /* exact integer squared distance sum_x (S[x] - N c[x])^2             */
    uint32_t flags;
    uint32_t reserved;
} kgma_hit;

/* One dip (maximal run of tested windows with d < thr) as found by the device, before the
 * host-side hit state machine.  Window starts are 1-based. */
typedef struct {
    int32_t contig;
    int32_t kfv;          /* 1-based */
    int64_t start, end;   /* first / last window start of the run                               */
    int64_t argmin;       /* first window start attaining the minimum                           */
    int64_t D_min;
    int64_t exit_pos;     /* end + 1 if that window was tested (dip closed), else 0 (open at contig end) */
    int64_t D_exit;       /* D of the exit window (valid if exit_pos != 0)                      */
    uint32_t flags;
    uint32_t reserved;
} kgma_dip;

typedef struct {
    int64_t bases_scanned;     /* sum of contig lengths handed to the last scan                 */
    int64_t windows_scanned;   /* windows evaluated (all KFVs)                                  */
    int64_t n_dips, n_hits;
    int64_t n_tie_flagged;     /* dips left with KGMA_HIT_TIE (rounding-ambiguous, unresolved)      */
    int64_t n_at_threshold;    /* tested windows inside the threshold guard band (all KFVs)         */
    double pack_ms, scan_ms;   /* device time of the last pack / scan kernels (hipEvents)       */
    double replay_ms;          /* host time of the hit state machine                            */
    int64_t device_bytes;      /* device memory held by the context + current genome            */
    int32_t n_tiles, n_launches;
    double chain_ms;           /* wall time of the Float64 chain replay (KGMA_F_CHAIN_REPLAY: selection, chain kernels,
                                  downloads, host walk), 0 if none ran                                          */
    int64_t n_chain_pairs;     /* (record, KFV) pairs it re-ran                                                */
    int64_t chain_windows;     /* windows it walked (sum over the pairs)                                       */
    int64_t chain_device_pairs;/* ... of them walked by the chain kernel on the device (the rest: host threads)         */
    double chain_device_ms;    /* device time of the chain kernels (hipEvents; part of chain_ms)                      */
    int64_t chain_raw_steps;   /* 64-window steps whose increments the host added one by one (wanted windows, binade
                                  changes); every other step reached the host as part of one integer add per chunk    */
    double chain_max_drift;    /* largest |chain value - exact distance| seen, relative to the exact distance at the stream
                                  starts of the device chain (it is only used while this stays below 2^-31 there) and to
                                  max(exact distance, thr) at the first windows and dip minima of the chained pairs         */
    int32_t chain_band_log2;   /* the guard band around thr the last kgma_scan ended with: 2^-30 unless the chain's drift
                                  exceeded half of it and the scan was repeated with a wider one (kgma_scan's drift policy) */
    int32_t chain_rescans;     /* ... and how often it was repeated (0, 1 or 2)                                              */
    double overlap_ms;         /* kgma_repack_scan_hits on a large genome re-encodes the records group by group on a few CUs
                                  BESIDE the scan launches of the previous groups: wall time of that pack + scan region (then
                                  pack_ms / scan_ms are the SUMS of the groups' kernel times, n_launches their number); 0 when
                                  pack and scan ran one after the other                                                       */
} kgma_stats;

/* Host-side stand-in for `pairalign` + `cigar_to_UnitRange` (src/Alignment.jl:33-52,
 * src/OmnGenomeMiner.jl:130-136): given a candidate range lo:hi (1-based) on `contig` for KFV
 * `kfv` (0 for the single engine) it must write the aligned range.  Called on the calling
 * thread, in reference order, interleaved with the hit state machine (the cluster engine feeds
 * the result back into its overlap checks, OmnGenomeMiner.jl:126,139,152). NULL = no alignment. */
typedef void (*kgma_align_fn)(void *user, int32_t contig, int32_t kfv, int64_t lo, int64_t hi,
                              int64_t seq_len, int64_t *out_lo, int64_t *out_hi);

int kgma_version(void);
const char *kgma_status_string(int status);
const char *kgma_last_error(const kgma_ctx *ctx);

/* Create a context on HIP device `device_ordinal`. */
int kgma_create(int device_ordinal, kgma_ctx **out);
void kgma_destroy(kgma_ctx *ctx);

/* Upload the reference KFV(s).  ref: m x 4^k row-major Float64 (refVec / refVecs, natural k-mer
 * index order: first base most significant, src/Kmers.jl:37-43).  windowsizes[m], thr[m].
 * refVec::Vector{Float64} (src/GenomeMiner.jl:6, src/OmnGenomeMiner.jl:9) may be any vector, and so may `ref`:
 *   - a KFV that is S/N with integer S (every KFV gen_ref_ws_cons / cluster_ref_API produce is one: an average of N integer
 *     histograms) is scanned in EXACT integers, S = round(ref*N).  n_refs[m] gives N per KFV; n_refs == NULL: N is inferred
 *     (smallest N <= 2^20 with every ref*N within a relative 1e-14 of an integer);
 *   - any other finite vector (weighted averages, smoothed or hand-edited profiles; also a KFV that is not S/n_refs for the
 *     n_refs given) is scanned in Float64 by the generic kernel.  Window q's distance (q = 0, 1, ... within its record) lies
 *     within an ABSOLUTE bound of the exact rational distance d_q = (1/2k) sum (ref - c_q)^2, and so does the reference's
 *     running value:  u [(max(P, n) + 5) A / 2k + (q + 4) M / k],  u = 2^-53, P the KFV's non-zero entries, n the k-mers per
 *     window, A = sum ref^2 + 2 sum_{p in window} |ref[K_p]| + n + 2 pairs at its largest over the record's windows up to q,
 *     M the sum over the steps up to q of (1 + c[r]) + |ref[l]| + |ref[r]| + c[l] ("The Float64 scan in exact
 *     arithmetic"; measured: the device at most 0.05 of it, the reference 0.3).  That is a relative 1e-13 ... 1e-11 where the
 *     distance is of the order of A -- an ordinary profile -- and no relative statement at all where the KFV nearly equals a
 *     window's own counts: there the distance is smaller than the bound and the value is rounding noise.  What the scan itself
 *     computes is never below zero: a sum the rounding took below zero is 0.0 in kgma_get_dists, in the dips and hits of a
 *     default-mode scan and (as D = 0) in kgma_get_first_window.  The decisions rounding noise could take either way in the
 *     reference -- a window within a relative 2^-30 of thr, two minima within 2^-30 of each other -- are flagged exactly like
 *     the integer form's exact ties (KGMA_HIT_AT_THRESHOLD / KGMA_HIT_TIE), and KGMA_F_CHAIN_REPLAY decides them from the
 *     reference's own running value (replayed on the device from the caller's table, bit for bit).  That value is the
 *     reference's with its sign: a chain-decided hit (KGMA_HIT_CHAIN) at such a window may carry a dist, and a D, a few ulps
 *     of the window's terms below zero, as the reference's own hit does.  kgma_hit.D / kgma_dip.D_* are round(d * 2kN^2) with
 *     N a power of two (kgma_kfv_scale), kgma_hit.dist the Float64 distance.
 * Requires 1 <= k <= 15 (a k-mer is at most 30 bits of the 2-bit genome), k < min(windowsizes) (src/API.jl:70,177) and at most
 * 65535 k-mers per window (windowsize - k + 1; the reference itself has no bound, src/ReferenceGeneration.jl:35-40);
 * KGMA_E_UNSUPPORTED otherwise, and for S/N KFVs whose largest possible D = sum S^2 + N^2 n^2 does not fit 61 bits.
 * At k >= 11 the library reads `ref` once for its non-zero entries and keeps no 4^k copy, on the host or on the device
 * (kgma_set_refs_sparse takes those entries directly: a dense KFV at k = 15 is 8 GiB).
 * Threshold semantics: with D the exact integer form of the distance (d = D / (2 k N^2)) a window
 * is below thr iff D < T, T = ceil(thr * 2kN^2 * (1 - 2^-30)).  The 2^-30 guard band stands for the
 * rounding noise of the reference's rolling Float64 chain (GenomeMiner.jl:77): windows whose exact
 * distance is that close to thr count as NOT below and are reported (KGMA_HIT_AT_THRESHOLD,
 * kgma_stats.n_at_threshold).  Away from the distance lattice T = ceil(thr * 2kN^2) exactly. */
int kgma_set_refs(kgma_ctx *ctx, int32_t k, int32_t m, const double *ref, const int64_t *windowsizes,
                  const double *thr, const int64_t *n_refs);

/* The same references given by their non-zero entries: KFV j has nnz[j] entries, keys[] / vals[] hold them KFV after KFV.  Keys are
 * natural k-mer values (0-based, first base most significant: the reference's index - 1), strictly increasing within a KFV; every
 * other entry is 0.  Exactly kgma_set_refs on the dense vectors (S/N inference, the Float64 form, every error and message), for
 * 1 <= k <= 15; KGMA_E_ARG for a key >= 4^k or out of order. */
int kgma_set_refs_sparse(kgma_ctx *ctx, int32_t k, int32_t m, const int64_t *nnz, const uint32_t *keys, const double *vals,
                         const int64_t *windowsizes, const double *thr, const int64_t *n_refs);

/* Change thresholds only (thr[m]). */
int kgma_set_thresholds(kgma_ctx *ctx, const double *thr);

/* Build a device-resident genome from host ASCII records (raw FASTA residue bytes, either case;
 * line breaks already removed).  The bytes are copied to the device and packed there to 2-bit
 * codes (A0 C1 G2 T3 N->3, src/Consts.jl:22-28; 16 residues per 32-bit word -- plus a copy as two
 * bit-planes, made the first time a scan picks a kernel that reads it).  Residues outside A/C/G/T/N are recorded
 * per record; kgma_scan raises KGMA_E_BADBASE for those the reference would have looked up. */
int kgma_genome_from_host(kgma_ctx *ctx, const uint8_t *const *contig_ascii, const int64_t *contig_len,
                          int64_t n_contigs, kgma_genome **out);

/* Build a device-resident genome straight from FASTA text (the whole file in host memory, e.g.
 * mmap-ed): replaces FASTX parsing + getSeq (src/GenomeMiner.jl:31-35).  The host only locates the
 * header lines; line breaks are stripped and records laid out on the device, then packed as in
 * kgma_genome_from_host.  Multi-line records, blank lines and CR/LF are accepted.
 * kgma_genome_header returns record `contig`'s header line (without '>', not NUL-counted). */
int kgma_genome_from_fasta(kgma_ctx *ctx, const uint8_t *text, int64_t n, kgma_genome **out);
/* The same from a file: `open(FASTA.Reader, genome_path)` (src/GenomeMiner.jl:31).  The text is read with pread() straight into
 * the pinned staging buffers (no mapping to fault in page by page: a 400 MB file in the page cache is resident and packed in
 * 12 ms instead of 17). */
int kgma_genome_from_fasta_file(kgma_ctx *ctx, const char *path, kgma_genome **out);
int kgma_genome_header(const kgma_genome *g, int64_t contig, const char **text, int64_t *len);

/* Build a device-resident genome from a UCSC .2bit file (the form assemblies are distributed in: hg38.2bit).  The file is 2 bits
 * per base on disk, with its runs of N and its soft-masked runs as interval lists; the packed bytes and the lists are shipped as
 * they are (0.25 byte per base over the link instead of the 1 byte of FASTA text) and expanded to the ordinary resident text by
 * one kernel (twobit_unpack_kernel: one pass, 0.25 B read + 1 B written per base), then packed as in kgma_genome_from_host.
 * Residue i of a record is N inside an N block, else the letter of its 2-bit code, and lower case inside a mask block (an N
 * there is `n`): what twoBitToFa writes.  The result is an ordinary genome; kgma_genome_header returns a record's name.
 * flags: KGMA_2BIT_NOMASK ignores the mask blocks (all upper case: twoBitToFa -noMask).
 * The whole file is validated on the host before any device work.  KGMA_E_UNSUPPORTED: a byte-swapped file, a version above 1
 * (0: 32-bit record offsets, 1: 64-bit), more tiles than one launch of the kernel takes.  KGMA_E_ARG: a wrong signature; an index,
 * a table or packed data that run past the end of the file; a block that ends behind its record; sums that leave 64 bits; more
 * records than a genome holds; a path that cannot be opened as a regular file.  kgma_last_error names record and field.  Block
 * lists need not be sorted or disjoint: they are normalised (empty blocks dropped, sorted, overlapping and adjacent ones merged).
 * KGMA_E_HIP / KGMA_E_NOMEM as kgma_genome_from_host (nothing is left allocated). */
enum { KGMA_2BIT_NOMASK = 1u << 0 };
int kgma_genome_from_2bit_file(kgma_ctx *ctx, const char *path, uint32_t flags, kgma_genome **out);
/* Device time of twobit_unpack_kernel in the last kgma_genome_from_2bit_file of the context (hipEvents around the launch), in
 * milliseconds; 0 if the file had no records.  KGMA_E_STATE before the first such call. */
int kgma_get_2bit_unpack_ms(kgma_ctx *ctx, double *ms);
/* HOST-side (no device, no context): what the parser of kgma_genome_from_2bit_file makes of a file -- the same validation, status
 * codes and messages (`err`, NUL-terminated, may be NULL).  Block counts are those of the normalised lists. */
typedef struct {
    int32_t version;
    int32_t reserved;
    int64_t n_records;
    int64_t total_bases;
    int64_t n_blocks;       /* N blocks, all records */
    int64_t mask_blocks;    /* mask blocks, all records */
    int64_t packed_bytes;   /* sum of ceil(dnaSize / 4) */
} kgma_twobit_info;
int kgma_twobit_inspect(const char *path, kgma_twobit_info *info, char *err, int64_t err_cap);

/* Build a synthetic genome on the device (benchmarks; no PCIe traffic): n_contigs records of the
 * given lengths, base i of record c = splitmix64(seed + c, i) >> 62 written as ASCII 'A','C','G','T',
 * then `n_plants` copies of `plant` (ASCII, length plant_len) written at the given (contig,
 * 1-based position) pairs, then packed like kgma_genome_from_host. */
int kgma_genome_synthetic(kgma_ctx *ctx, const int64_t *contig_len, int64_t n_contigs, uint64_t seed,
                          const uint8_t *plant, int64_t plant_len, const int64_t *plant_contig,
                          const int64_t *plant_pos, int64_t n_plants, kgma_genome **out);

/* Copy `len` ASCII bases of record `contig` starting at 1-based `pos` back to the host
 * (used to build the FASTA body of a hit: view(seq, seq_UnitRange)). */
int kgma_genome_fetch(kgma_ctx *ctx, const kgma_genome *g, int64_t contig, int64_t pos, int64_t len,
                      uint8_t *out);
/* The same for n ranges in ONE device gather + ONE download (the FASTA bodies of all hits of a scan:
 * GenomeMiner.jl:100-103 / OmnGenomeMiner.jl:143-150 build one record per hit).  The ranges are written
 * back to back into `out` (range i at the sum of len[0..i-1]); out_cap >= the sum of len. */
int kgma_genome_fetch_batch(kgma_ctx *ctx, const kgma_genome *g, int64_t n, const int64_t *contig,
                            const int64_t *pos, const int64_t *len, uint8_t *out, int64_t out_cap);
int64_t kgma_genome_num_contigs(const kgma_genome *g);
int64_t kgma_genome_contig_len(const kgma_genome *g, int64_t contig);
int64_t kgma_genome_total_bases(const kgma_genome *g);
void kgma_genome_free(kgma_ctx *ctx, kgma_genome *g);

/* Overwrite `len` ASCII residues of record `contig` starting at 1-based `pos` with host bytes
 * (used to plant genes / runs of N in synthetic genomes).  Call kgma_genome_repack afterwards. */
int kgma_genome_poke(kgma_ctx *ctx, kgma_genome *g, int64_t contig, int64_t pos, int64_t len,
                     const uint8_t *bytes);

/* Re-run the ASCII -> 2-bit pack kernel of a resident genome (after kgma_genome_poke, and in
 * benchmarks that time pack + scan). */
int kgma_genome_repack(kgma_ctx *ctx, kgma_genome *g);

/* A new device-resident genome whose record c is the reverse complement of record c of `g` (same number of
 * records, same lengths, same header lines).  Made on the device from the resident residue text: no host copy
 * (one kernel, 1 byte read and 1 written per base, then the pack kernel as in kgma_genome_from_host).  No counterpart
 * in the reference, whose engines read every record left to right only: scanning the new genome finds the genes of
 * the reverse strand.  The complement keeps the case: A<->T, C<->G, M<->K, R<->Y, V<->B, H<->D; W, S, N and '-' are
 * their own complements; any other byte is copied, so a residue outside the alphabet is reported (KGMA_E_BADBASE) by
 * the same scans as on `g`, at its mirrored position.
 * COORDINATES of every result on the new genome (hits, dips, matches, alignments, kgma_genome_fetch) are those of the
 * REVERSED records: position p there is position L - p + 1 of the source record (L its length), so a range lo:hi there
 * is (L - hi + 1):(L - lo + 1) on `g`, and its residues are the reverse complement of that source range.  genome_pos
 * keeps its meaning (the records' order and lengths are the source's).
 * `g` is left untouched; it may have no records, and records of length 0.  The result is an ordinary genome (its own
 * device memory, about the size of `g`'s; a fresh identity for the scan caches) and is freed with kgma_genome_free.
 * KGMA_E_ARG for null arguments; KGMA_E_HIP / KGMA_E_NOMEM as kgma_genome_from_host (nothing is left allocated). */
int kgma_genome_revcomp(kgma_ctx *ctx, const kgma_genome *g, kgma_genome **out);
/* The kernel of kgma_genome_revcomp alone: overwrites the residue text of `rc` -- a genome with the record lengths of `g`,
 * such as an earlier kgma_genome_revcomp(g) -- with the reverse complement of `g`'s current text (after kgma_genome_poke on
 * `g`; benchmarks time this call).  Queued on the context's stream; call kgma_genome_repack(rc) afterwards, as after
 * kgma_genome_poke.  KGMA_E_ARG when the record lengths differ or g == rc. */
int kgma_genome_revcomp_into(kgma_ctx *ctx, const kgma_genome *g, kgma_genome *rc);

/* Scan every record of `g`.  mode: KGMA_MODE_*.  buff: `buff`.
 * (What "identical to the reference" means: every window's distance is the exact value; the hit list is the one
 * the reference's Float64 arithmetic produces wherever that does not hang on rounding noise.  Where it does -- dips
 * reported with KGMA_HIT_TIE / KGMA_HIT_AT_THRESHOLD, windows counted in kgma_stats.n_at_threshold -- exact arithmetic's
 * choice is returned unless KGMA_F_CHAIN_REPLAY is passed, which takes those decisions from a replay of the reference's
 * running value and leaves nothing flagged.  So: identical to a sequential IEEE-754 evaluation of the reference with the
 * flag (first window summed left to right, see the flag); without it, identical whenever n_tie_flagged == 0 &&
 * n_at_threshold == 0.)
 * genome_pos0 is the cluster
 * engine's `genome_pos` keyword (OmnGenomeMiner.jl:25); ignored (0) by the single engine.
 * Results are kept in the context until the next scan. */
int kgma_scan(kgma_ctx *ctx, const kgma_genome *g, int32_t mode, int64_t buff, int64_t genome_pos0,
              uint32_t flags, kgma_align_fn align, void *align_user);

/* Device part of kgma_scan only (kernels + record download, no hit state machine); used by
 * benchmarks and by callers that replay dips themselves. */
int kgma_scan_device(kgma_ctx *ctx, const kgma_genome *g, int32_t mode, uint32_t flags);

/* Results of the last scan.  Two-call pattern: out == NULL or cap too small -> *n is set to the
 * required count (status KGMA_OK when out == NULL, KGMA_E_ARG when cap is too small). */
int kgma_get_hits(kgma_ctx *ctx, kgma_hit *out, int64_t cap, int64_t *n);
int kgma_get_dips(kgma_ctx *ctx, kgma_dip *out, int64_t cap, int64_t *n);
/* D of the first window of every record for KFV `kfv` (1-based): out[n_contigs], -1 = record skipped. */
int kgma_get_first_window(kgma_ctx *ctx, int32_t kfv, int64_t *out, int64_t cap, int64_t *n);
/* Per-window distances of KFV `kfv` (1-based) in the order the reference push!es them
 * (GenomeMiner.jl:79 / OmnGenomeMiner.jl:111); needs KGMA_F_RETURN_DISTS. */
int kgma_get_dists(kgma_ctx *ctx, int32_t kfv, double *out, int64_t cap, int64_t *n);

/* Distance landscape: reductions over the vector of kgma_get_dists on the device, where the scan left it (it stays there until the
 * next scan), so that a genome's 8 B per window per KFV need not come to the host.
 *
 * Layout.  The vector holds record after record; a record with nwin evaluated windows has nwin - 1 values, and value i (0-based in
 * the record) is the distance of window start i + 2 (window 1 is never tested).  kgma_dist_layout: record c's values are
 * offset[c] .. offset[c + 1] of the vector, *n = records + 1 (two-call pattern).  Host only; valid after any scan, with or without
 * KGMA_F_RETURN_DISTS (KGMA_E_STATE before the first).
 *
 * kgma_dist_bins: every record is cut into bins of `bin` consecutive values (the last bin of a record may be shorter, a record
 * without values has none; bins never cross a record).  bin_min[b] is the smallest value of bin b, bit for bit as the scan wrote
 * it (also for a Float64 KFV); bin_argmin[b] the window start (1-based, within the record) of the FIRST value attaining it.
 * Record c's bins are bin_offset[c] .. bin_offset[c + 1] (records + 1 entries, or NULL).  Two-call pattern on bin_min / bin_argmin
 * (both NULL: *n_bins and bin_offset alone, no device work; cap counts bins).
 *
 * kgma_dist_sweep: for n_thr finite, strictly increasing thresholds (1 .. KGMA_SWEEP_MAX_THRESHOLDS), windows_below[j] is the exact
 * number of values d < thr[j], dips_below[j] the exact number of maximal runs of consecutive values of one record below thr[j]:
 * the dips kgma_get_dips lists for a scan at that threshold when no window lies at the threshold itself.  Comparisons only (a value
 * equal to a threshold is not below it), one pass for the whole list.
 *
 * All three: KGMA_E_UNSUPPORTED for strobemer references (their distance vector follows another window convention).  The two
 * device calls: KGMA_E_STATE when the last scan kept no distances, KGMA_E_ARG for kfv outside the KFVs the last scan evaluated,
 * bin < 1, n_thr out of range, or a threshold that is not finite or not above the one before it.  The values are taken as
 * non-negative doubles, as every scan writes them (the integer forms by construction, the Float64 form because it writes 0.0
 * for a distance whose rounding noise went below zero: kgma_set_refs).  Nothing stays allocated after a call; the results of the scan are untouched. */
#define KGMA_SWEEP_MAX_THRESHOLDS 4096
int kgma_dist_layout(kgma_ctx *ctx, int64_t *offset, int64_t cap, int64_t *n);
int kgma_dist_bins(kgma_ctx *ctx, int32_t kfv, int64_t bin, double *bin_min, int64_t *bin_argmin, int64_t *bin_offset /* records + 1, or NULL */,
                   int64_t cap, int64_t *n_bins);
int kgma_dist_sweep(kgma_ctx *ctx, int32_t kfv, const double *thr, int64_t n_thr, int64_t *windows_below /* n_thr */,
                    int64_t *dips_below /* n_thr */);
/* The last kgma_dist_bins (bins_ms: the bin kernel, combine_ms: the pass that joins bins spread over workgroups, n_bins) and the
 * last kgma_dist_sweep (sweep_ms; sweep_slots: threshold slots of the kernel form that ran: 64, 512 or 4096): device time by
 * hipEvents.  n_values (values read per kernel) and n_launches describe the later of the two.  All zero before the first call. */
typedef struct {
    double bins_ms, combine_ms, sweep_ms;
    int64_t n_values, n_bins;
    int32_t n_launches, sweep_slots;
} kgma_landscape_stats;
int kgma_get_landscape_stats(kgma_ctx *ctx, kgma_landscape_stats *out);

int kgma_get_stats(kgma_ctx *ctx, kgma_stats *out);

/* Distance-bound prefilter of the last scan (one integer KFV, k = 5 or 6, 8-bit count-table kernel, no distance output).
 * A window's distance has the exact lower bound D >= sumS2 - 2N sumS + N^2 n (sumS: the sum of S over the window's k-mer
 * positions), so a cheap pass over the genome names the GRANULES (16 consecutive window starts of a record, granule g =
 * windows 16g + 1 ... 16g + 16) that may hold a window at or below the threshold band; the exact scan then runs over
 * streams built around them instead of over every window.  Results are those of the full scan.  The scan falls back to
 * the full scan (same results) when the candidate list overflows, when the candidate streams outnumber the regular ones
 * or when they cover too large a part of the windows; a fallback is remembered for the (genome, references, thresholds)
 * triple and later scans of it skip the filter.  KGMA_FILTER=0 switches the filter off. */
enum { KGMA_FILTER_OK = 0, KGMA_FILTER_OVERFLOW = 1, KGMA_FILTER_STREAMS = 2, KGMA_FILTER_FRACTION = 3, KGMA_FILTER_REMEMBERED = 4 };
typedef struct kgma_filter_stats {
    int32_t ran;             /* the filter kernel ran in the last scan */
    int32_t fell_back;       /* the full scan ran although the filter applies */
    int32_t reason;          /* KGMA_FILTER_*: why it fell back */
    int32_t form;            /* the filter kernel's form: S entry bytes (1, 2) | table copies (1, 32) << 8; 0: it did not run.
                              * Bit 16: it read the block sums that the step's pack wrote (kgma_repack_scan_hits / kgma_step_begin
                              * with KGMA_FUSE_SUMS != 0) instead of cutting and looking up the k-mers itself */
    int64_t granules;        /* candidate granules */
    int64_t regions;         /* merged, padded regions (every record's first windows included) */
    int64_t streams;         /* candidate streams the exact kernel walked */
    int64_t windows;         /* windows in candidate streams */
    int64_t positions;       /* ... plus the streams' warm-up positions */
    int64_t total_windows;   /* windows of the records */
    int64_t bound;           /* U: a granule is a candidate when its sum of S reaches it */
    double filter_ms;        /* filter kernel time */
} kgma_filter_stats;
int kgma_get_filter_stats(kgma_ctx *ctx, kgma_filter_stats *out);
/* The last scan's candidate granules (0-based record, 0-based granule), sorted; two-call pattern as kgma_get_hits. */
int kgma_get_filter_candidates(kgma_ctx *ctx, int32_t *contig, int64_t *granule, int64_t cap, int64_t *n);
/* Block sums of record `contig` as the last step whose pack computed them left them (bit 16 of kgma_filter_stats.form): out[i] =
 * the sum of S over the k-mers that start at 0-based positions 16 b ... 16 b + 15 of the record, b = first_block + i, and do not
 * pass the record's last k-mer.  A record has 2 * ceil(len / 32) blocks.  KGMA_E_STATE: no such step has run on this genome. */
int kgma_get_block_sums(kgma_ctx *ctx, const kgma_genome *genome, int64_t contig, int64_t first_block, int64_t n, uint32_t *out);
/* The sparse step pack (tests and KGMA_GEOM_DEBUG).  A step whose pack carries the block sums, on a genome without a bit-plane
 * copy, does not write the device's 2-bit copy of the genome in full (KGMA_SPARSE_PACK=0: it does): it packs only the blocks of
 * 32 768 bases that its own candidate streams and chained records read, and leaves the genome KGMA_INTER_PARTIAL.  Every other
 * reader of the copy completes it first (one full pack) and leaves it KGMA_INTER_FULL, so no call ever sees the difference.
 * *state: KGMA_INTER_*; *demand_blocks: the blocks the last step packed on demand (0 after any full pack).  Either may be null.
 * KGMA_SPARSE_POISON=1 (tests): a sparse step fills the copy with a byte pattern before it packs its blocks. */
enum { KGMA_INTER_FULL = 0, KGMA_INTER_PARTIAL = 1 };
/* The block sums of a genome: none yet; written by the last step's pack; or DEFERRED -- that step's pack made the prefilter's test
 * itself and stored none: kgma_get_block_sums (and whatever changes the resident text) has them written first, for the text and
 * the reference of that step. */
enum { KGMA_BSUM_NONE = 0, KGMA_BSUM_WRITTEN = 1, KGMA_BSUM_DEFERRED = 2 };
/* The last step (kgma_repack_scan_hits): did its pack make the prefilter's granule test itself (no filter kernel, no block sums
 * stored; KGMA_PACK_TEST=0: never), and if so: the units (128 plane words) a wave took at a time, the units in all, those that went
 * word by word, and the chunks (half units) encoded a second time to prime a run. */
typedef struct kgma_pack_test_stats {
    int32_t tested;
    int32_t run;
    int64_t units;
    int64_t slow_units;
    int64_t primed_chunks;
} kgma_pack_test_stats;
int kgma_get_pack_test_stats(kgma_ctx *ctx, kgma_pack_test_stats *out);
int kgma_genome_inter_state(const kgma_genome *genome, int32_t *state, int64_t *demand_blocks);

/* HOST-side helper (not on the device path; a Julia host keeps using BioAlignments.jl): semi-global
 * affine-gap alignment of `a` (global; the consensus) against `b` (leading/trailing residues of b
 * free), EDNAFULL scores, gap of length L scoring gap_open_score + L*gap_extend_score
 * (AffineGapScoreModel, src/GenomeMiner.jl:28).  Writes the CIGAR text ('=','X','I','D') that
 * cigar_to_UnitRange (src/Alignment.jl:13-30) consumes. */
int kgma_host_semiglobal_cigar(const uint8_t *a, int64_t m, const uint8_t *b, int64_t n,
                               int32_t gap_open_score, int32_t gap_extend_score, char *cigar,
                               int64_t cigar_cap, int64_t *score_out);

/* HOST-side helper (no device): the reference's running Float64 distance kmerDist (src/GenomeMiner.jl:46-47,70-77; the same
 * update in src/OmnGenomeMiner.jl:73-74,101-108) of one sequence, from its first window on, sampled at the windows of
 * the given intervals (1-based window starts, sorted, disjoint): what KGMA_F_CHAIN_REPLAY runs for the (record, KFV) pairs
 * that contain a rounding-dependent tie.  1 <= k <= 15; `ref` is the dense 4^k vector.  Two-call pattern via cap / *n_out as
 * elsewhere. */
int kgma_host_chain_values(const uint8_t *seq, int64_t len, const double *ref, int32_t k, int64_t windowsize,
                           const int64_t *win_lo, const int64_t *win_hi, int64_t n_intervals, double *out, int64_t cap,
                           int64_t *n_out);

/* The reference's running Float64 distance of record `contig` for KFV `kfv` (1-based) at the windows of the given intervals
 * (1-based window starts, sorted, disjoint) -- kgma_host_chain_values computed by the chain kernel on the resident genome:
 * what KGMA_F_CHAIN_REPLAY runs for its (record, KFV) pairs.  Window 1's value is the first window's
 * ScaleFactor * 0.5 * sqeuclidean (summed left to right on the host); every later value is bit for bit what a sequential
 * IEEE-754 evaluation of src/GenomeMiner.jl:70-72 gives.  Served for every k, window and KFV (by one of the two chain kernels);
 * KGMA_E_UNSUPPORTED only when the device chain is switched off (KGMA_CHAIN=host) or its walk failed a check.  Two-call pattern
 * via cap / *n_out. */
int kgma_chain_values(kgma_ctx *ctx, const kgma_genome *genome, int64_t contig, int32_t kfv, const int64_t *win_lo,
                      const int64_t *win_hi, int64_t n_intervals, double *out, int64_t cap, int64_t *n_out);

/* HOST half of the device chain, exposed for tests: walks caller-supplied chunk records (the layout of
 * kgma_device.h's ChainChunk: int64 A0, uint32 info, uint32 raw; `pool` = entries and raw increments in 16-byte units) exactly as the product does with
 * the kernel's output.  KGMA_E_STATE: the value drifted more than 2^-31 from the exact distance at a stream start. */
int kgma_chain_chunk_steps(void);   /* 64-position steps per chunk (kgma_device.h: KGMA_CHAIN_STEPS) */
int kgma_host_chain_walk(double first, double scale, int32_t nk, int64_t n_streams, const int64_t *win0, const int32_t *n_valid,
                         const int64_t *chunk_base, const int64_t *D0, const void *chunks, int64_t n_chunks, const void *pool,
                         int64_t pool_units, const int64_t *win_lo, const int64_t *win_hi, int64_t n_intervals, double *out,
                         int64_t cap, int64_t *n_out, double *max_drift);

/* ---- scans sharded INSIDE a record (one process per GPU; kmergma_amd.parallel.scan_sharded) ----------
 * A rank scans its slice of the records with kgma_scan_device, decides the ties that need its residues
 * (kgma_resolve_ties_local), and ships kgma_get_dips + kgma_get_dip_last_min (+ kgma_get_first_window for
 * the records whose first window it owns) to rank 0, which translates the dips to whole-record window
 * coordinates, joins the dips that straddle a slice boundary and runs the reference's hit state machine
 * (GenomeMiner.jl:82-104 / OmnGenomeMiner.jl:113-156) over them with kgma_replay_dips.  first_D is
 * [m][n_records] (D of each record's first window, -1 for skipped records); dips must be sorted by
 * (record, KFV, start).  Hits then come from kgma_get_hits as usual. */
int kgma_resolve_ties_local(kgma_ctx *ctx, const kgma_genome *genome);
/* Residue source for kgma_replay_dips: rank 0 has no genome for the dips other GPUs found, so a dip whose minimum
 * EQUALS the stale running minimum left by an earlier dip (GenomeMiner.jl:93-103) -- a tie only the hit state machine
 * can see -- is decided by asking the caller for the residues of the stretch in between: fn must write `len` residue
 * characters of record `contig` starting at 1-based `pos` and return 0 (anything else: the tie stays KGMA_HIT_TIE).
 * NULL (default): such ties stay flagged.  (KGMA_F_CHAIN_REPLAY needs kgma_set_chain_source below.) */
typedef int (*kgma_fetch_fn)(void *user, int32_t contig, int64_t pos, int64_t len, uint8_t *out);
/* Chain-value source for kgma_replay_dips with KGMA_F_CHAIN_REPLAY: rank 0 holds no residues, so the reference's running
 * Float64 value (src/GenomeMiner.jl:46-47,70-77) of the (record, KFV) pairs that need it is produced where the residues
 * are.  fn receives the pairs (0-based record, 1-based KFV) and, per pair, the sorted disjoint window intervals
 * win_lo/win_hi[iv_begin[p] .. iv_begin[p+1]) whose values are wanted (the first is always window 1), and writes one
 * Float64 per wanted window, pair after pair, in window order; it returns 0 on success.  A multi-GPU host serves it by
 * running kgma_chain_export on every rank's slices of the record (in whole-record window order a slice ends one
 * transition before the next begins) and walking the pieces in order with kgma_host_chain_walk, each piece starting on
 * the value the previous one ended on (kmergma_amd.parallel.scan_sharded).  NULL (default): kgma_replay_dips ignores the
 * flag, ties stay flagged. */
typedef int (*kgma_chain_fn)(void *user, int64_t n_pairs, const int32_t *contig, const int32_t *kfv, const int64_t *iv_begin,
                             const int64_t *win_lo, const int64_t *win_hi, double *values);
int kgma_set_chain_source(kgma_ctx *ctx, kgma_chain_fn fn, void *user);
/* 2 k N^2 of KFV `kfv` (1-based): exact distance = D / scale (what kgma_host_chain_walk checks the chain against); N as given
 * to or inferred by kgma_set_refs. */
int kgma_kfv_scale(kgma_ctx *ctx, int32_t kfv, double *scale, int64_t *n_refs);
/* 1 if KFV `kfv` (1-based) is scanned as a general Float64 vector (kgma_set_refs: not S/n_refs), 0 for the exact-integer form.
 * Callers that join dips themselves (parallel.merge_payloads across slice boundaries) compare the D values of a Float64 KFV
 * with the library's near-tie tolerance |a - b| <= max(|a|, |b|) * 2^-30 + 2 instead of ==. */
int kgma_kfv_is_float(kgma_ctx *ctx, int32_t kfv, int32_t *is_float);
/* The tested windows inside the threshold guard band found by the last scan (0-based record, 1-based KFV, window start):
 * they travel with the dips, because the chain replay samples the running value at them.  kgma_set_att hands the merged
 * list to the NEXT kgma_replay_dips. */
int kgma_get_att(kgma_ctx *ctx, int32_t *contig, int32_t *kfv, int64_t *pos, int64_t cap, int64_t *n);
int kgma_set_att(kgma_ctx *ctx, const int32_t *contig, const int32_t *kfv, const int64_t *pos, int64_t n);
/* The chain kernel's output for windows 1 .. last_window of one record and KFV, for a caller that joins the pieces of a
 * record cut across GPUs: the streams (kgma_chain_export_copy: first window, windows, first chunk, exact D of the first
 * window), the chunk records and the pool exactly as kgma_host_chain_walk takes them; the steps that hold a window of
 * win_lo/win_hi are raw.  *first = the Float64 distance of the record's window 1 (summed left to right). */
int kgma_chain_export(kgma_ctx *ctx, const kgma_genome *genome, int64_t contig, int32_t kfv, int64_t last_window,
                      const int64_t *win_lo, const int64_t *win_hi, int64_t n_intervals, int64_t *n_streams, int64_t *n_chunks,
                      int64_t *pool_units, double *first);
int kgma_chain_export_copy(kgma_ctx *ctx, int64_t *win0, int32_t *n_valid, int64_t *chunk_base, int64_t *D0, void *chunks, void *pool);
int kgma_set_residue_source(kgma_ctx *ctx, kgma_fetch_fn fn, void *user);
int kgma_get_dip_last_min(kgma_ctx *ctx, int64_t *out, int64_t cap, int64_t *n);   /* last window attaining each dip's minimum */
int kgma_replay_dips(kgma_ctx *ctx, int32_t mode, int64_t buff, int64_t genome_pos0, uint32_t flags, int64_t n_records,
                     const int64_t *record_len, const int64_t *first_D, const kgma_dip *dips, const int64_t *dip_last_min,
                     int64_t n_dips, kgma_align_fn align, void *align_user);

/* Batched re-alignment of hits ON THE DEVICE (single engine; replaces the per-hit
 * pairalign(SemiGlobalAlignment(), consensus, view(seq, lo:hi), AffineGapScoreModel(EDNAFULL, ...)) +
 * cigar_to_UnitRange of src/Alignment.jl:13-30,41-46 for hosts without BioAlignments): same algorithm and
 * tie-breaking as kgma_host_semiglobal_cigar, one wave per hit, segments read from the resident genome.
 * first_out/last_out receive cigar_to_UnitRange's (first, last); the caller maps them to the record as the
 * reference does: max(lo + first - 1, 1) : min(lo + last - 1, L).  Segments up to 8191 residues. */
int kgma_align_hits_device(kgma_ctx *ctx, const kgma_genome *genome, const uint8_t *consensus, int64_t m,
                           int32_t gap_open_score, int32_t gap_extend_score, int64_t n_hits, const int32_t *contig,
                           const int64_t *lo, const int64_t *hi, int64_t *first_out, int64_t *last_out, int64_t *score_out);

/* The scan with the hits' re-alignment done ON THE DEVICE in batches, for hosts that do not bring their
 * own aligner: replaces, per hit, pairalign(SemiGlobalAlignment(), consensus, view(seq, range),
 * AffineGapScoreModel(EDNAFULL, gap_open, gap_extend)) + cigar_to_UnitRange (src/Alignment.jl:13-30,41-46 for the single
 * engine, against consensus[1:windowsize]; src/OmnGenomeMiner.jl:130-136 for the cluster engine, against the whole
 * consensus_seqs[ind]).  consensus[j] / consensus_len[j]: one sequence per KFV (the single engine uses entry 0).
 * Single engine: the hits of the scan are aligned in one batch.  Cluster engine: the aligned range feeds back into the
 * overlap checks (OmnGenomeMiner.jl:126,139,152), but WHICH range is aligned depends only on a dip's best window and KFV,
 * so every dip's candidate range is aligned speculatively in one batch per KFV right after the scan and the hit state
 * machine looks the results up where the reference calls pairalign; a range that was not speculated is aligned by the
 * host restatement (kgma_host_semiglobal_cigar) and counted in n_host.  Hits then come from kgma_get_hits (lo:hi =
 * aligned range); kgma_get_alignments lists the alignments the state machine consumed, in order (first, last =
 * cigar_to_UnitRange's result relative to lo). */
typedef struct {
    int32_t contig;
    int32_t kfv;          /* 1-based; 0 for the single engine */
    int64_t lo, hi;       /* the range that was aligned */
    int64_t first, last;  /* cigar_to_UnitRange of the alignment (1-based, relative to lo; last < first: empty) */
} kgma_alignment;
int kgma_scan_aligned(kgma_ctx *ctx, const kgma_genome *g, int32_t mode, int64_t buff, int64_t genome_pos0, uint32_t flags,
                      const uint8_t *const *consensus, const int64_t *consensus_len, int32_t gap_open_score, int32_t gap_extend_score);
int kgma_get_alignments(kgma_ctx *ctx, kgma_alignment *out, int64_t cap, int64_t *n, int64_t *n_device, int64_t *n_host);

/* kgma_genome_repack + kgma_scan (no align callback) + kgma_get_hits in one call, for callers that run the
 * whole step in a loop (bench.py): out must hold `cap` hits; if more were found KGMA_E_ARG is returned and
 * *n holds the number needed (the scan results stay valid: call kgma_get_hits with a larger buffer). */
int kgma_repack_scan_hits(kgma_ctx *ctx, kgma_genome *genome, int32_t mode, int64_t buff, int64_t genome_pos0,
                          uint32_t flags, kgma_hit *out, int64_t cap, int64_t *n);

/* Reference preparation on the device: n sequences given as residue characters
 * seqs[offsets[i] .. offsets[i+1]) (either case; anything outside A/C/G/T/N -> KGMA_E_BADBASE, the
 * reference's KeyError), 1 <= k <= 10.
 *   kgma_kmer_count_batch: bins[i*4^k + x] = kmer_count(seq_i, k)[x+1] (src/Kmers.jl:14-28; Float64 bins,
 *     k-mer value = first base most significant; a sequence shorter than k counts nothing).
 *   kgma_kmer_dist_batch:  out[i] = kmer_dist(seq_i, KFV, k) = (1/2k)*sqeuclidean(kmer_count(seq_i,k), KFV)
 *     (src/Kmers.jl:58-60), as called per reference sequence by cluster_ref_API
 *     (src/ReferenceGeneration.jl:101) and per trial by estimate_optimal_threshold
 *     (src/DistanceTesting.jl:14,27).  Float64, fixed summation order: exact for integer-valued KFVs,
 *     otherwise equal to the reference up to the rounding of its (unordered) @simd reduction. */
int kgma_kmer_count_batch(kgma_ctx *ctx, int32_t k, const uint8_t *seqs, const int64_t *offsets, int64_t n, double *bins);
int kgma_kmer_dist_batch(kgma_ctx *ctx, int32_t k, const double *kfv, const uint8_t *seqs, const int64_t *offsets, int64_t n,
                         double *out);

/* ---- the strobemer engine: StrobeGMA! / Strobemer_findGenes (src/StrobemerGMA/StrobeGenomeMiner.jl) ------------------------------
 * Upload the reference of the strobemer method (gen_ref_ws_cons of src/StrobemerGMA/StrobeRefGen.jl): ref[4^(2s)] Float64 in the
 * reference's bin order (bin = first s-mer * 4^s + second s-mer, natural values: as_UInt of the ungapped randstrobe), one window
 * size, one threshold.  s, w_min, w_max, q are get_strobe_2_mer's parameters (src/StrobemerGMA/Strobemers.jl:45-65); a strobemer
 * spans k = w_max + s - 1 residues.  Read literally, the reference picks as second s-mer the one at the LAST offset in
 * w_min..w_max whose score (as_UInt(first) + as_UInt(s-mer)) % q is 0, at w_min if none is (`min_score::Int = 2 << 63` is 0), and
 * its scan re-enters the window's own last strobemer: after step i the counts are the W - k strobemers starting at i+1 .. i+W-k
 * plus one permanent copy of the record's strobemer W-k+1.  That is what the device computes (kgma_strobe.hip), in exact integers:
 * the KFV must be S/N with integer S (same inference from n_refs / the entries and same threshold band as kgma_set_refs).
 * Served: 1 <= s <= 3, 1 <= w_min <= w_max, k <= 16, q >= 1, k < windowsize, windowsize - k + 1 <= 65535.  KGMA_E_ARG where the
 * reference would throw (s < 1, w_min < 1, w_min > w_max, q < 1, k >= windowsize); KGMA_E_UNSUPPORTED for the rest (s > 3, k > 16,
 * longer windows, a KFV that is not S/N).  The call REPLACES the context's references: a k-mer scan after it, or a strobe scan
 * after kgma_set_refs, returns KGMA_E_STATE.  kgma_set_thresholds works as for k-mer references. */
int kgma_set_strobe_ref(kgma_ctx *ctx, int32_t s, int32_t w_min, int32_t w_max, int64_t q, const double *ref, int64_t windowsize,
                        double thr, int64_t n_refs /* 0: infer */);

/* The strobemer scan of every record, with the optional re-alignment of process_hit! (src/Alignment.jl:83-111) on the device.
 * consensus == NULL: do_align = false.  Otherwise every candidate range max(CMI - buff, 1) : min(CMI + W - 1 + buff, L) is aligned
 * against consensus[1:windowsize] (semi-global, EDNAFULL, affine gaps; StrobeGMA!'s default scores are -69 / -5) in one device
 * batch, a candidate whose alignment score is below score_threshold is dropped -- goal_ind and currminim were updated all the
 * same, as in the reference, where the gate does not feed back into the state machine -- and the others get the aligned range.
 * Results through the usual getters: kgma_get_hits (kfv = 0, cmi = CMI after `CMI += 1` = the best window's step + 1, genome_pos
 * advancing by the length of every record that is not shorter than the window), kgma_get_dips, kgma_get_first_window,
 * kgma_get_dists (KGMA_F_RETURN_DISTS: one value per step i >= 1 in record order, L - W - 1 per record), kgma_get_stats,
 * kgma_get_alignments (the alignments of the hits that passed the gate), kgma_scan_kernel_name ("strobe_kernel<2>").
 * Without KGMA_F_CHAIN_REPLAY every decision is taken on exact integers (first of tied windows, strict comparisons, windows inside
 * the threshold band count as not below) and the rounding-dependent dips are flagged KGMA_HIT_TIE / KGMA_HIT_AT_THRESHOLD, a minimum
 * equal to the stale running minimum included.  With it, every record that holds a flagged dip or an at-threshold window is decided
 * by a HOST replay of the reference's sequential Float64 loop over the record's residues (fetched from the device; first window
 * summed left to right, increments in the reference's operation order): its hits carry KGMA_HIT_CHAIN and the running value as
 * dist.  kgma_scan(KGMA_MODE_STROBE) is this call without a consensus (an align callback is refused with KGMA_E_UNSUPPORTED: the
 * gate needs the alignment's score, which the callback does not return); kgma_scan_device(KGMA_MODE_STROBE) is its device part.
 * NOT served for strobemer references (KGMA_E_UNSUPPORTED): kgma_chain_values, kgma_chain_export, kgma_replay_dips,
 * kgma_resolve_ties_local, kgma_scan_aligned, kgma_repack_scan_hits, kgma_step_begin / kgma_step_end. */
int kgma_strobe_scan(kgma_ctx *ctx, const kgma_genome *g, int64_t buff, uint32_t flags, const uint8_t *consensus, int64_t consensus_len,
                     int32_t gap_open_score, int32_t gap_extend_score, int64_t score_threshold);

/* ---- exact sequence search: exactMatch (src/ExactMatch.jl:89-121) ------------------------------------------------------------------
 * Every occurrence of every query in every record of `g`.  queries[offsets[i] .. offsets[i+1]) is query i: DNA symbols, either
 * case.  Comparison is symbol equality after case folding -- BioSequences' ExactSearchQuery with isequal on DNAAlphabet{4}
 * (convert_to_search_query, src/ExactMatch.jl:46-58): N matches only N, each of M R W S Y K V H D B and '-' only itself; a genome N
 * does NOT match a query T, although the scans' 2-bit code stores N as T.  A match of a query of length m at 1-based start s covers
 * s : s+m-1 and lies inside one record; a query longer than a record has no match there.  overlap != 0: every occurrence
 * (FindAllOverlap, src/ExactMatch.jl:33-43); overlap == 0: the leftmost occurrence, then the leftmost one starting behind its end,
 * and so on (FindAll, src/ExactMatch.jl:20-30).  All queries are served in one pass over the genome: the number of kernel launches
 * does not depend on n_queries (queries of A/C/G/T only are filtered on the 2-bit copy of the genome and verified against the
 * residue text, the others -- and every query when a record holds a symbol outside A/C/G/T/N, or under the testing switch
 * KGMA_EXACT_ASCII=1 -- are compared on the residue text: at most one launch of each kind, repeated once when the matches outgrow
 * the device buffer, which starts at 64 Ki matches and is kept between calls; KGMA_E_NOMEM, the buffer it had still in place and
 * the context usable, if the larger buffer cannot be had, as in the three searches below; KGMA_E_OVERFLOW if the matches outgrow
 * the regrown buffer).
 * KGMA_E_ARG: an empty query, or a query symbol outside the 16-symbol alphabet.  KGMA_E_BADBASE: a genome residue outside it, in any
 * record (the reference decodes every record before it searches, getSeq at src/ExactMatch.jl:109); kgma_last_error names the first
 * such record and position.
 * The call needs no references and leaves the KFVs and the hits, dips and distances of the last scan as they are; of kgma_stats it
 * sets bases_scanned, scan_ms (hipEvents around the launches) and n_launches.  kgma_get_matches returns the matches of the last
 * call sorted by (query, contig, start), with the two-call pattern of kgma_get_hits. */
typedef struct {
    int32_t query;       /* 0-based index of the query                                         */
    int32_t contig;      /* 0-based index of the record                                        */
    int64_t start;       /* 1-based position of the match's first symbol                       */
} kgma_match;
int kgma_exact_match(kgma_ctx *ctx, const kgma_genome *g, const uint8_t *queries, const int64_t *offsets /* n_queries + 1 */,
                     int32_t n_queries, int32_t overlap);
int kgma_get_matches(kgma_ctx *ctx, kgma_match *out, int64_t cap, int64_t *n);

/* IUPAC motif search with mismatches on a resident genome (the working form of the reference's src/RSS.jl, whose RSS_dist counts
 * every N of a spacer as a mismatch).  Motif i is motifs[offsets[i] .. offsets[i+1]), 1 ... 64 symbols of ACGTRYSWKMBDHVN in either
 * case; each symbol stands for a set of bases, N for all four.  Laid at 1-based start s of a record of length L (s + m - 1 <= L; no
 * match spans two records), position j of the motif MATCHES when the set of the genome residue (case folded; N = all four) is a
 * subset of the symbol's set: a base A/C/G/T matches a symbol that contains it, a genome N matches only a motif N.  mism(s) is the
 * number of non-matching positions, and every s with mism(s) <= max_mismatch[i] is reported, overlapping ones included.
 * 0 <= max_mismatch[i] <= 15, and it must be smaller than the number of informative (non-N) positions of the motif -- otherwise
 * every start would match (an all-N motif is refused the same way).  The minus strand is served by passing the reverse-complemented
 * motif: it is searched on the same genome and its matches are in forward coordinates.
 * All motifs are served by ONE kernel launch over the bit-plane copy of the genome (made on first use, 0.25 byte per base; each
 * 32-bit operation serves 32 starts, candidates are verified and counted on the residue text), repeated once when the hits outgrow
 * the device buffer (KGMA_E_NOMEM, context still usable, if the larger buffer cannot be had; KGMA_E_OVERFLOW if it overflows again).
 * KGMA_E_ARG: an empty motif or one of more than 64 symbols, a symbol outside the 15 codes, a max_mismatch out of range;
 * kgma_last_error names motif and position.  KGMA_E_BADBASE: a genome residue outside A/C/G/T/N, in any record (the 2-bit copies
 * are not faithful there); kgma_last_error names the first such record and position.
 * The call needs no references and leaves the KFVs, the hits, dips and distances of the last scan and the matches of the last
 * kgma_exact_match as they are; of kgma_stats it sets bases_scanned, scan_ms (hipEvents around the launches) and n_launches.
 * kgma_get_motif_matches returns the hits of the last call sorted by (motif, contig, start), with the two-call pattern of
 * kgma_get_hits; after a call that failed, for whatever reason, it returns none. */
typedef struct {
    int32_t motif;       /* 0-based index of the motif                                         */
    int32_t contig;      /* 0-based index of the record                                        */
    int64_t start;       /* 1-based position of the motif's first symbol                       */
    int32_t mismatches;  /* non-matching positions, <= max_mismatch of the motif               */
    int32_t reserved;
} kgma_motif_hit;
int kgma_motif_match(kgma_ctx *ctx, const kgma_genome *g, const uint8_t *motifs, const int64_t *offsets /* n_motifs + 1 */,
                     int32_t n_motifs, const int32_t *max_mismatch /* n_motifs */);
int kgma_get_motif_matches(kgma_ctx *ctx, kgma_motif_hit *out, int64_t cap, int64_t *n);

/* ---- approxMatch: semi-global edit-distance search on a resident genome (kernels: kgma_approx.hip) -----------------------------
 * Query i is queries[offsets[i] .. offsets[i+1]): 1 ... 64 symbols of ACGTRYSWKMBDHVN in either case.  A genome residue MATCHES a
 * symbol by kgma_motif_match's rule: case folded, its set must be a subset of the symbol's set -- a base A/C/G/T matches a symbol
 * that contains it, a genome N matches only a query N.
 * For a record t[1..L] and a query q[1..m], score(j) = min over 1 <= s <= j+1 of ed(q, t[s..j]): unit costs (substitution,
 * insertion, deletion 1 each), the empty substring allowed -- Sellers' semi-global dynamic programme, the query global, the start
 * in the text free.  Nothing spans two records.  Every end j with score(j) <= max_edits[i] is a MATCHING END.  Each carries a
 * start: the largest s with ed(q, t[s..j]) == score(j), the shortest substring that attains the score; the covered range is
 * start : j (start = j + 1 cannot occur under the limits below).  A RUN is a maximal set of consecutive matching ends of one
 * (query, record).  best_only != 0 reports per run the end with the smallest score, on a tie the smallest end; best_only == 0
 * reports every matching end.
 * 0 <= max_edits[i] <= 15, and it must be smaller than the number of informative (non-N) symbols of query i -- otherwise every
 * position would match.  The minus strand is served by passing the reverse-complemented query: it is searched on the same genome,
 * start : end are forward coordinates and every canonical choice (shortest substring, smallest end of a run) is made on the
 * forward text.
 * All queries are served by ONE launch of the search kernel (Myers' bit vectors over the residue text, a lane per `tile` end
 * positions, restarted m + max_edits columns before them) and one of the start kernel (the anchored recurrence backwards from each
 * reported end); the search is repeated once when the ends outgrow the device buffer (KGMA_E_NOMEM, context still usable, if the
 * larger buffer cannot be had; KGMA_E_OVERFLOW if it overflows again).  The bit vectors are one 32-bit word when no query of the
 * batch is longer than 32 symbols, else two (the measuring switch KGMA_APPROX_WORDS=2 asks for two words in every case).
 * KGMA_E_ARG: an empty query or one of more than 64 symbols, a symbol outside the 15 codes, a max_edits out of range;
 * kgma_last_error names query and position.  KGMA_E_BADBASE: a genome residue outside A/C/G/T/N, in any record; kgma_last_error
 * names the first such record and position.
 * The call needs no references and leaves the KFVs, the hits, dips and distances of the last scan and the matches of the last
 * kgma_exact_match / kgma_motif_match as they are; of kgma_stats it sets bases_scanned, scan_ms (hipEvents around the launches)
 * and n_launches.  kgma_get_approx_matches returns the hits of the last call sorted by (query, contig, end), with the two-call
 * pattern of kgma_get_hits; after a call that failed, for whatever reason, it returns none. */
typedef struct {
    int32_t query;       /* 0-based index of the query                                         */
    int32_t contig;      /* 0-based index of the record                                        */
    int64_t start, end;  /* 1-based, inclusive: the covered range                               */
    int32_t edits;       /* score(end), <= max_edits of the query                              */
    int32_t reserved;
} kgma_approx_hit;
typedef struct {
    int32_t tile;        /* end positions a lane of the search kernel owns                     */
    int32_t wg_bases;    /* end positions a workgroup owns                                     */
    int32_t words;       /* 32-bit words of the bit vectors of the form that ran               */
    int32_t n_launches;  /* kernel launches of the call (search, a repeated search, starts)    */
    int64_t n_ends;      /* matching ends before the run reduction                             */
    int64_t n_hits;      /* reported hits                                                      */
    double search_ms;    /* hipEvents around the search launch(es)                             */
    double starts_ms;    /* ... around the start kernel                                        */
} kgma_approx_stats;
int kgma_approx_match(kgma_ctx *ctx, const kgma_genome *g, const uint8_t *queries, const int64_t *offsets /* n_queries + 1 */,
                      int32_t n_queries, const int32_t *max_edits /* n_queries */, int32_t best_only);
int kgma_get_approx_matches(kgma_ctx *ctx, kgma_approx_hit *out, int64_t cap, int64_t *n);
int kgma_get_approx_stats(kgma_ctx *ctx, kgma_approx_stats *out);

/* ---- pwmMatch: position-weight-matrix search on a resident genome (kernel: kgma_pwm.hip) --------------------------------------
 * Matrix i is rows row_offsets[i] .. row_offsets[i+1] - 1 of `weights`: m = 1 ... 64 rows of four integer weights in the order
 * A, C, G, T, each in -32768 ... 32767 (the int16_t of the interface), the matrices back to back.  Every score fits an int32, its
 * magnitude is at most 2^21.
 * Laid at the 1-based start s of a record t[1..L], s + m - 1 <= L, score(s) = sum over the rows i = 0 ... m - 1 of
 * W[i][t[s + i]].  Nothing spans two records.  Case is folded.  A genome N scores the row's minimum over A/C/G/T: an assembly gap
 * never looks like a signal, and a row of four equal weights (a spacer) costs nothing.  Every s with score(s) >= threshold[i] is a
 * hit, overlapping ones included.
 * threshold[i] must exceed the sum of the row minima of matrix i -- otherwise every start would match; a threshold above the sum
 * of the row maxima is legal and finds nothing.  The minus strand is served by passing the reverse-complemented matrix (rows
 * reversed, A<->T and C<->G swapped): it is searched on the same genome, in the same pass, and its starts are forward
 * coordinates.  The 0/1 matrix of an IUPAC motif (1 where the symbol's set holds the base, four 0 for N) with the threshold
 * informative - d finds exactly the starts of kgma_motif_match with max_mismatch d, and score = informative - mismatches.
 * All matrices are served by ONE launch (a workgroup per `wg_starts` consecutive starts of a record, a wave per `wave_starts` of
 * them, `lane_starts` consecutive starts per lane; the host folds the constant rows into the threshold and every other row with
 * the row behind it into a table indexed by two residues); the search is repeated once when the hits outgrow the device buffer,
 * which starts at 64 Ki hits and is kept between calls (KGMA_E_NOMEM, context still usable, if the larger buffer cannot be had;
 * KGMA_E_OVERFLOW if it overflows again).
 * KGMA_E_ARG: a null pointer, a matrix of no rows or of more than 64, a threshold that does not exceed the sum of the row
 * minima; kgma_last_error names the matrix.  KGMA_E_BADBASE: a genome residue outside A/C/G/T/N, in any record, exactly as in
 * kgma_motif_match.
 * The call needs no references and leaves the KFVs, the hits, dips and distances of the last scan and the matches of the last
 * kgma_exact_match / kgma_motif_match / kgma_approx_match as they are; of kgma_stats it sets bases_scanned, scan_ms (hipEvents
 * around the launches) and n_launches.  kgma_get_pwm_matches returns the hits of the last call sorted by (matrix, contig,
 * start), with the two-call pattern of kgma_get_hits; after a call that failed, for whatever reason, it returns none. */
typedef struct {
    int32_t matrix;      /* 0-based index of the matrix                                        */
    int32_t contig;      /* 0-based index of the record                                        */
    int64_t start;       /* 1-based                                                            */
    int32_t score;       /* score(start), >= threshold of the matrix                           */
    int32_t reserved;
} kgma_pwm_hit;          /* 24 bytes */
typedef struct {
    int32_t lane_starts; /* consecutive starts a lane owns                                     */
    int32_t wave_starts; /* ... a wave owns                                                    */
    int32_t wg_starts;   /* ... a workgroup owns                                               */
    int32_t n_launches;  /* kernel launches of the call (the search, a repeated search)        */
    int64_t n_candidates; /* starts the kernel emitted: it scores exactly, so = n_hits         */
    int64_t n_hits;      /* reported hits                                                      */
    double search_ms;    /* hipEvents around the search launch(es)                             */
} kgma_pwm_stats;
int kgma_pwm_match(kgma_ctx *ctx, const kgma_genome *g, const int16_t *weights /* rows of 4, matrices back to back */,
                   const int64_t *row_offsets /* n_matrices + 1, in rows */, int32_t n_matrices, const int32_t *threshold /* n_matrices */);
int kgma_get_pwm_matches(kgma_ctx *ctx, kgma_pwm_hit *out, int64_t cap, int64_t *n);
int kgma_get_pwm_stats(kgma_ctx *ctx, kgma_pwm_stats *out);

/* ---- protMatch: codon-weight-matrix search on a resident genome, all three reading frames (kernel: kgma_codon.hip) -------------
 * The device searches with a CODON WEIGHT MATRIX.  Matrix i is rows row_offsets[i] .. row_offsets[i+1] - 1 of `weights`:
 * m = 1 ... 64 rows of KGMA_CODON_ENTRIES = 65 integer weights, each in -32768 ... 32767 (the int16_t of the interface), the
 * matrices back to back.  Entry 16 b0 + 4 b1 + b2 of a row (A 0, C 1, G 2, T 3) is the weight of the codon b0 b1 b2 read left to
 * right on the plus strand; entry 64 is the weight of a codon that holds any residue other than A/C/G/T -- an N, that is.  Case is
 * folded as everywhere else.
 * Laid at the 1-based NUCLEOTIDE start s of a record t[1..L], s + 3m - 1 <= L,
 *     score(s) = sum over the rows i = 0 ... m - 1 of row_i[codon(t[s + 3i], t[s + 3i + 1], t[s + 3i + 2])].
 * Every start is scored, so the three reading frames of the strand are searched in one pass; nothing spans two records.  Every
 * score fits an int32, its magnitude is at most 64 * 32768 = 2^21.  Every s with score(s) >= threshold[i] is a hit, overlapping
 * ones included.
 * threshold[i] must exceed the sum of the row minima of matrix i (each over the 65 entries) -- otherwise every start would
 * match; a threshold above the sum of the row maxima is legal and finds nothing.
 * The kernel knows nothing of genetic codes or strands: kgma_codon_fold (below) turns an amino-acid profile into the codon
 * matrix of one strand, and a minus-strand search is a plus-strand search with another matrix, on the same genome, in the same
 * pass, its starts in forward coordinates.
 * All matrices are served by ONE launch (a workgroup per `wg_starts` consecutive starts of a record, a wave per `wave_starts` of
 * them, `lane_starts` consecutive starts per lane; the workgroup keeps one codon code per residue position in LDS; the host takes
 * the rows of 65 equal weights out and into the threshold); the search is repeated once when the hits outgrow the device buffer,
 * which starts at 64 Ki hits and is kept between calls (KGMA_E_NOMEM, context still usable, if the larger buffer cannot be had;
 * KGMA_E_OVERFLOW if it overflows again).
 * KGMA_E_ARG: a null pointer, a matrix of no rows or of more than 64, a threshold that does not exceed the sum of the row
 * minima; kgma_last_error names the matrix.  KGMA_E_BADBASE: a genome residue outside A/C/G/T/N, in any record, exactly as in
 * kgma_motif_match; kgma_last_error names the first such record and residue.
 * The call needs no references and leaves the KFVs, the hits, dips and distances of the last scan and the matches of the last
 * kgma_exact_match / kgma_motif_match / kgma_approx_match / kgma_pwm_match as they are; of kgma_stats it sets bases_scanned,
 * scan_ms (hipEvents around the launches) and n_launches.  kgma_get_codon_matches returns the hits of the last call sorted by
 * (matrix, contig, start), with the two-call pattern of kgma_get_hits; after a call that failed, for whatever reason, it returns
 * none.
 *
 * kgma_codon_fold (host only: it needs no context and no GPU) makes the codon matrix of one strand from an amino-acid profile.
 * aa_weights: m rows of KGMA_CODON_AA_COLUMNS = 21 weights, the columns in the order ACDEFGHIKLMNPQRSTVWY*, '*' the stop.
 * code: the genetic code, 64 bytes: code[16 b0 + 4 b1 + b2] is the column (0 ... 20) the codon b0 b1 b2 translates to.
 * x_weight: per row the weight of a codon that holds a residue other than A/C/G/T (entry 64).
 * minus == 0:  out[i][c] = aa_weights[i][code[c]],                          out[i][64] = x_weight[i];
 * minus != 0:  out[i][c] = aa_weights[m - 1 - i][code[revcomp(c)]],         out[i][64] = x_weight[m - 1 - i],
 * where revcomp(b0 b1 b2) = (3 - b2)(3 - b1)(3 - b0): the rows are reversed and each codon is read as its reverse complement, so
 * that a hit of the folded matrix at the forward start s is the profile read on the minus strand over s .. s + 3m - 1.
 * KGMA_E_ARG: a null pointer, m outside 1 ... 64, a code entry above 20. */
#define KGMA_CODON_ENTRIES 65
#define KGMA_CODON_MAX_ROWS 64
#define KGMA_CODON_AA_COLUMNS 21
typedef struct {
    int32_t matrix;      /* 0-based index of the matrix                                        */
    int32_t contig;      /* 0-based index of the record                                        */
    int64_t start;       /* 1-based nucleotide position of the first codon's first residue     */
    int32_t score;       /* score(start), >= threshold of the matrix                           */
    int32_t reserved;
} kgma_codon_hit;        /* 24 bytes */
typedef struct {
    int32_t lane_starts; /* consecutive starts a lane owns                                     */
    int32_t wave_starts; /* ... a wave owns                                                    */
    int32_t wg_starts;   /* ... a workgroup owns                                               */
    int32_t n_launches;  /* kernel launches of the call (the search, a repeated search)        */
    int64_t n_candidates; /* starts the kernel emitted: it scores exactly, so = n_hits         */
    int64_t n_hits;      /* reported hits                                                      */
    double search_ms;    /* hipEvents around the search launch(es)                             */
} kgma_codon_stats;
int kgma_codon_match(kgma_ctx *ctx, const kgma_genome *g, const int16_t *weights /* rows of 65, matrices back to back */,
                     const int64_t *row_offsets /* n_matrices + 1, in rows */, int32_t n_matrices, const int32_t *threshold /* n_matrices */);
int kgma_get_codon_matches(kgma_ctx *ctx, kgma_codon_hit *out, int64_t cap, int64_t *n);
int kgma_get_codon_stats(kgma_ctx *ctx, kgma_codon_stats *out);
int kgma_codon_fold(const int16_t *aa_weights /* m rows of 21 */, int32_t m, const uint8_t *code /* 64 */, const int16_t *x_weight /* m */,
                    int32_t minus, int16_t *out /* m rows of 65 */);

/* Threshold calibration: the working form of src/DistanceTesting.jl on the device (kernels: kgma_calib.hip).  Both calls need
 * the references of kgma_set_refs (KGMA_E_STATE before it, or after kgma_set_strobe_ref), serve 1 <= k <= 10 (references at
 * k >= 11 are kept sparse: KGMA_E_UNSUPPORTED) and leave the references, the thresholds and the results of the last scan,
 * kgma_exact_match and kgma_motif_match untouched; of kgma_stats they set only scan_ms (hipEvents around the launch) and
 * n_launches.  kgma_scan_kernel_name afterwards names the form that ran: "calib_kernel<window|mutation,lds|global,int|f64>" --
 * counters in LDS for k <= 7, in a per-workgroup global table (left all-zero) for k = 8 ... 10; integer or Float64 form.
 *
 * kgma_window_dists: the distance of n arbitrary windows of a resident genome to KFV `kfv` (1-based).  Window i is the W
 * residues start[i] .. start[i] + W - 1 (1-based) of record contig[i] (0-based), W the window size kgma_set_refs was given for
 * that KFV; it holds W - k + 1 k-mers.  Residues go through the reference's code table (A0 C1 G2 T3, N -> 3, either case) as in
 * every scan; the definition does not depend on the engine.  The list may be unsorted, hold duplicates, or be empty.  A genome
 * made by kgma_genome_revcomp is used in its own coordinates.
 *   S/N KFV:      D_out[i] = sum_x (S[x] - N c[x])^2 exactly (the quantity kgma_hit.D holds), formed from the window's k-mer
 *                 positions alone, D = sumS2 - 2 N sum_j S[x_j] + N^2 sum_j c[x_j]: the work is proportional to W, not to 4^k.
 *                 dist_out[i] = (double)D / scale, scale as kgma_kfv_scale returns it: the bits the scans report as `dist`
 *                 without chain replay.
 *   Float64 KFV:  dist_out[i] = (1 / 2k) sum_x (ref[x] - c[x])^2 by a dense pass in one fixed order -- lane t of 256 sums the
 *                 bins t, t + 256, ... of the device index order (first base least significant) in increasing order, a wave's
 *                 64 lanes are combined by a shuffle tree (distances 32 ... 1), the four waves in order, times RN(1 / 2k);
 *                 within (4^k + 4) 2^-53 (relative) of the exact value.  D_out[i] = llround(dist * scale).
 * Either output may be NULL.  KGMA_E_ARG: kfv or a contig out of range, or a window that does not lie inside its record
 * (kgma_last_error names the index).  KGMA_E_BADBASE: a residue outside A/C/G/T/N INSIDE a requested window (kgma_last_error
 * names record and position; the outputs are then unspecified); such a residue elsewhere in the genome is no error.
 *
 * kgma_mutation_dists: for every (sequence i, rate r, trial t) the distance of the whole mutated sequence to the KFV,
 * kmer_dist(mutate_seq(seq_i, rates[r]), KFV, k) -- the inner step of gen_sub_vs_ref (src/DistanceTesting.jl:69-84) -- in the
 * forms and with the scale above; results at [(i * n_rates + r) * n_trials + t].  Sequence i is seqs[offsets[i] ..
 * offsets[i + 1]); its own length decides the number of k-mers (shorter than k: nothing is counted, D = sumS2).  The mutated
 * copy is never materialised: each lane forms the codes it needs.  The mutation is a counter-based hash, so that the host
 * reproduces any single trial exactly (it cannot reproduce Julia's RNG: results agree with the reference statistically):
 *   mix64(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)
 *   G = 0x9E3779B97F4A7C15;  K = mix64(mix64(mix64(seed + G (i + 1)) + G (r + 1)) + G (t + 1))          (all mod 2^64)
 *   residue j (0-based): z = mix64(K + G (j + 1)); substituted iff (z >> 11) < floor(rate * 2^53) -- a rate of 0 never
 *   substitutes, a rate of 1 always does; the new base is MUT[b][((z & 0x7FF) * 3) >> 11] with MUT in the order of
 *   mutation_dict (:38-42): A -> C G T, C -> A G T, G -> C A T, T -> C G A.  r enters the key: the same rate at another index of
 *   `rates` draws other substitutions.  A result does not depend on the sequences, rates or trials that follow it.
 * KGMA_E_ARG: a rate outside [0, 1] or not finite, n_rates < 1, n_trials < 1.  KGMA_E_BADBASE: a residue outside A/C/G/T in
 * either case, N included (mutation_dict has no other key); kgma_last_error names sequence and position.  KGMA_E_UNSUPPORTED:
 * a sequence whose sumS2 + N^2 n^2 leaves 61 bits, or more than 2^28 distances in one call. */
int kgma_window_dists(kgma_ctx *ctx, const kgma_genome *g, int32_t kfv /* 1-based */, int64_t n,
                      const int32_t *contig /* 0-based */, const int64_t *start /* 1-based */,
                      int64_t *D_out /* n, may be NULL */, double *dist_out /* n, may be NULL */);
int kgma_mutation_dists(kgma_ctx *ctx, int32_t kfv, const uint8_t *seqs, const int64_t *offsets /* n_seqs + 1 */,
                        int64_t n_seqs, const double *rates, int32_t n_rates, int32_t n_trials, uint64_t seed,
                        int64_t *D_out, double *dist_out /* [n_seqs][n_rates][n_trials], either may be NULL */);

/* The same two calls for the strobemer engine (kernel: strobe_calib_kernel, kgma_calib.hip), whose reference docstring reads "there
 * is not distance threshold estimation yet" and whose default KmerDistThr = 30 is the k-mer engine's: the strobemer distance
 * lives on another lattice -- 4^(2s) bins, D / scale with scale = 2 k N^2, k = w_max + s - 1, which is exactly what
 * kgma_kfv_scale(ctx, 1, ...) returns after kgma_set_strobe_ref.  Both calls need the reference of kgma_set_strobe_ref
 * (KGMA_E_STATE before it, or after kgma_set_refs; kgma_window_dists and kgma_mutation_dists in turn keep refusing a strobemer
 * reference), leave the reference, the threshold and the hits, dips, distances, alignments, matches and motif matches of earlier
 * calls untouched, and set of kgma_stats only scan_ms and n_launches.  kgma_scan_kernel_name afterwards:
 * "strobe_calib_kernel<window|mutation,s>".  Either output may be NULL.  D is exact in int64: D = sumS2 - 2 N sum_j S[x_j] +
 * N^2 sum_j c[x_j] over the item's randstrobes j, x_j their bins (first * 4^s + second, the rule kgma_strobe_scan counts by),
 * with 4^(2s) 32-bit counters in LDS; dist_out = (double)D / scale.
 *
 * kgma_strobe_window_dists: window i is THE SCAN'S window with start start[i] (1-based) of record contig[i] (0-based), W the
 * window size kgma_set_strobe_ref was given, read as literally as the scan reads the reference: the window with start 1 holds the
 * W - k + 1 randstrobes that start at residues 1 .. W - k + 1 of the record; a window with start q >= 2 holds the W - k
 * randstrobes that start at q .. q + W - k - 1 PLUS one permanent copy of the record's randstrobe at residue W - k + 1 (the
 * reference's update re-enters the previous window's last randstrobe, so that one never leaves).  W - k + 1 items either way.
 * Valid starts: 1 <= start <= max(1, L - W) on a record of L >= W residues -- the first window and the windows the scan tests
 * (its steps 1 .. L - W - 1, start = step + 1).  D_out[i] is exactly what kgma_hit.D, kgma_get_first_window (start 1) and, divided
 * by the scale, kgma_get_dists report for that window.  The list may be unsorted, hold duplicates, or be empty; a genome made by
 * kgma_genome_revcomp is used in its own coordinates.  KGMA_E_ARG: a null list, a contig out of range, a record shorter than W, a
 * start outside the range above (kgma_last_error names the index).  KGMA_E_BADBASE: a residue outside A/C/G/T/N among the residues
 * a requested window's items read -- residues q .. q + W - 2 of the record and, for q >= 2, the k residues W - k + 1 .. W of the
 * permanent item; for q = 1, residues 1 .. W -- (kgma_last_error names record and position; the outputs are then unspecified);
 * such a residue elsewhere in the genome is no error.
 *
 * kgma_strobe_mutation_dists: for every (sequence i, rate r, trial t) the distance of the reference to the randstrobe counts of
 * the whole mutated sequence: all len - k + 1 randstrobes and no permanent item (len < k: D = sumS2).  The mutation rule, the key
 * derivation, the layout [(i * n_rates + r) * n_trials + t] and the argument errors are those of kgma_mutation_dists; the working
 * form of test_strobe_2_mer_dists (src/StrobemerGMA/MonteCarloBenchmark.jl:2-23).  KGMA_E_UNSUPPORTED: a sequence whose
 * sumS2 + N^2 n^2 leaves 61 bits, or more than 2^28 distances in one call. */
int kgma_strobe_window_dists(kgma_ctx *ctx, const kgma_genome *g, int64_t n, const int32_t *contig /* 0-based */,
                             const int64_t *start /* 1-based */, int64_t *D_out /* n, may be NULL */, double *dist_out /* n, may be NULL */);
int kgma_strobe_mutation_dists(kgma_ctx *ctx, const uint8_t *seqs, const int64_t *offsets /* n_seqs + 1 */, int64_t n_seqs,
                               const double *rates, int32_t n_rates, int32_t n_trials, uint64_t seed,
                               int64_t *D_out, double *dist_out /* [n_seqs][n_rates][n_trials], either may be NULL */);

/* ---- gene assignment: which reference gene is each hit closest to? (kgma_assign.hip, kgma_assign.cpp) ----
 * Every query (a hit's residues) is aligned against every reference of a batch under the hit aligner's model -- the one of
 * kgma_host_semiglobal_cigar(reference, query): Gotoh affine gaps, the reference global, the query's ends free, a gap of length L
 * scoring gap_open_score + L * gap_extend_score, EDNAFULL over A/C/G/T/N, any byte outside A/C/G/T in either case counting as N
 * (there is no KGMA_E_BADBASE here).  A score-only kernel fills the n_queries x n_refs matrix; per query the `top` references are
 * chosen -- higher score first, lower reference index among equal scores -- and only those pairs are aligned with a traceback
 * (match, then deletion, then insertion; a gap extended where extending and opening tie), whose columns are counted:
 * out[q * top + t] describes query q's (t+1)-th best reference.  The CIGAR letters mean what kgma_host_semiglobal_cigar writes
 * ('=' / 'X': a reference residue against an equal / other query residue, N never equal; 'I': a reference residue against a gap;
 * 'D': a query residue against a gap), and the counts are those of its CIGAR for that pair.
 *
 * kgma_assign_seqs takes the queries from the host (query q = queries[query_offsets[q] .. query_offsets[q + 1])), kgma_assign_ranges
 * from the resident genome (query q = residues lo[q] .. hi[q], 1-based inclusive, of record contig[q], 0-based).  The references
 * are refs[ref_offsets[r] .. ref_offsets[r + 1]).  `scores`, when not NULL, receives the whole matrix, row-major.
 * n_queries == 0: KGMA_OK.  KGMA_E_ARG: a null pointer, n_refs < 1, top < 1 or top > n_refs, an empty reference or query,
 * offsets that decrease, a range outside its record, a positive gap score.  KGMA_E_UNSUPPORTED: a reference or query longer than
 * 8191 residues (KGMA_ASSIGN_MAX_LEN), more than 2^30 pairs in one call, or gap scores with
 * -gap_open_score - 8192 * gap_extend_score > 2^27: beyond that a cell could come within reach of the kernel's "no alignment"
 * sentinel, -2^29.  kgma_last_error names the offending item.  Nothing stays allocated after the call, whatever it returns;
 * it needs no kgma_set_refs. */
#define KGMA_ASSIGN_MAX_LEN 8191
typedef struct {
    int32_t ref;        /* 0-based index into the reference batch */
    int32_t score;      /* optimum semi-global score of (reference global, query ends free) */
    int32_t n_eq, n_x;  /* '=' and 'X' columns */
    int32_t n_ins;      /* 'I' columns: a reference residue against a gap */
    int32_t n_del;      /* 'D' columns NOT in a leading or trailing D run (those are the query's free overhang) */
    int32_t q_lo, q_hi; /* 1-based query positions left after removing the leading / trailing D runs; q_hi < q_lo: none */
} kgma_assignment;
int kgma_assign_seqs(kgma_ctx *ctx, const uint8_t *refs, const int64_t *ref_offsets /* n_refs + 1 */, int32_t n_refs,
                     const uint8_t *queries, const int64_t *query_offsets /* n_queries + 1 */, int64_t n_queries,
                     int32_t gap_open_score, int32_t gap_extend_score, int32_t top,
                     kgma_assignment *out /* n_queries * top */, int32_t *scores /* n_queries * n_refs, or NULL */);
int kgma_assign_ranges(kgma_ctx *ctx, const kgma_genome *genome, const uint8_t *refs, const int64_t *ref_offsets /* n_refs + 1 */,
                       int32_t n_refs, int64_t n_queries, const int32_t *contig /* 0-based */, const int64_t *lo,
                       const int64_t *hi /* 1-based inclusive */, int32_t gap_open_score, int32_t gap_extend_score, int32_t top,
                       kgma_assignment *out, int32_t *scores);
/* The last assignment call of the context: device time of its score launches and of its trace launches (hipEvents), the pairs
 * scored, their DP cells (sum of reference length x query length), the pairs traced and the kernel launches.  All zero before the
 * first call and after a call that failed or had no queries. */
typedef struct {
    double score_ms, trace_ms;
    int64_t n_pairs, n_cells, n_traced;
    int32_t n_score_launches, n_trace_launches;
} kgma_assign_stats;
int kgma_get_assign_stats(kgma_ctx *ctx, kgma_assign_stats *out);

/* ---- all-pairs k-mer distances (kgma_kmat.hip, kgma_kmat.cpp) ----
 * D[a][b] = sum_x (c_a[x] - c_b[x])^2 with c_s = kmer_count(s, k) (src/Kmers.jl:14-28: residues through A0 C1 G2 T3 N3 in either
 * case, nothing counted for a sequence shorter than k), an exact integer, and dist[a][b] = RN(1 / 2k) * (double)D: bit for bit
 * kmer_dist(a, b, k) (src/Kmers.jl:54-56).  Both matrices are row-major [n_a][n_b]; either pointer may be NULL.
 *
 * kgma_kmer_dist_matrix takes A from the host (sequence i = a[a_off[i] .. a_off[i + 1])); b == NULL means B = A (the symmetric
 * matrix, zero diagonal; b_off and n_b are ignored).  kgma_kmer_dist_matrix_ranges takes A from the resident genome: residues
 * lo[i] .. hi[i] (1-based inclusive) of record contig[i] (0-based); hi = lo - 1 is an empty range.  B is always uploaded.
 * kgma_kmer_nearest / kgma_kmer_nearest_ranges keep the matrix on the device and return per row of A its n_near nearest of B, in
 * the order (D ascending, index in B ascending): index[n_a][n_near] and D_near[n_a][n_near] (either may be NULL); b == NULL in
 * kgma_kmer_nearest is B = A as well (a sequence's nearest is then itself, at D = 0).
 *
 * Every residue of every sequence is looked up, also of one shorter than k; a byte outside A/C/G/T/N is KGMA_E_BADBASE (the
 * reference's KeyError), and kgma_last_error names the side, the sequence and the position.  In a genome only the residues inside
 * a requested range count.  KGMA_E_ARG: a null pointer, k < 1, offsets that decrease, a range outside its record, n_a < 0,
 * n_b < 1, n_near outside 1 .. min(n_b, KGMA_KMAT_MAX_NEAR).  KGMA_E_UNSUPPORTED: k > 10, a sequence of more than
 * KGMA_KMAT_MAX_LEN residues (a count must fit 16 bits and D 31), more than 2^30 pairs in one call.  n_a == 0: KGMA_OK.  Nothing
 * stays allocated after a call, whatever it returns; the calls need no kgma_set_refs and leave references, hits and every
 * earlier result untouched. */
#define KGMA_KMAT_MAX_LEN 32767
#define KGMA_KMAT_MAX_NEAR 128
int kgma_kmer_dist_matrix(kgma_ctx *ctx, int32_t k, const uint8_t *a, const int64_t *a_off /* n_a + 1 */, int64_t n_a,
                          const uint8_t *b /* NULL: B = A */, const int64_t *b_off /* n_b + 1 */, int32_t n_b,
                          int32_t *D, double *dist);
int kgma_kmer_dist_matrix_ranges(kgma_ctx *ctx, const kgma_genome *genome, int32_t k, int64_t n_a, const int32_t *contig /* 0-based */,
                                 const int64_t *lo, const int64_t *hi /* 1-based inclusive */, const uint8_t *b, const int64_t *b_off,
                                 int32_t n_b, int32_t *D, double *dist);
int kgma_kmer_nearest(kgma_ctx *ctx, int32_t k, const uint8_t *a, const int64_t *a_off, int64_t n_a, const uint8_t *b,
                      const int64_t *b_off, int32_t n_b, int32_t n_near, int32_t *index, int32_t *D_near);
int kgma_kmer_nearest_ranges(kgma_ctx *ctx, const kgma_genome *genome, int32_t k, int64_t n_a, const int32_t *contig, const int64_t *lo,
                             const int64_t *hi, const uint8_t *b, const int64_t *b_off, int32_t n_b, int32_t n_near, int32_t *index,
                             int32_t *D_near);
/* The last of the four calls above on the context (a screened assignment counts: it makes one): device time of the matrix launches
 * (the |c_a|^2 pass and the matrix kernel) and of the select launch (hipEvents), the pairs, the launches, and the form that ran:
 * form 0 = count tables in LDS (k <= 7), 1 = one table per workgroup in global memory (k >= 8); tile = sequences of B per
 * workgroup, chunks = workgroups that share a tile.  All zero before the first call and after a call that failed or was empty. */
typedef struct {
    double kmat_ms, select_ms;
    int64_t n_pairs;
    int32_t n_launches, form, tile, chunks;
} kgma_kmat_stats;
int kgma_get_kmat_stats(kgma_ctx *ctx, kgma_kmat_stats *out);

/* kgma_assign_seqs / kgma_assign_ranges with a k-mer prescreen: kgma_kmer_nearest(screen_k, queries, references, n_near) chooses
 * every query's candidates, the score kernel runs over those n_near pairs per query only, and selection and traceback are as in
 * the unscreened calls.  out[q * top + t] is the (t+1)-th best AMONG THE CANDIDATES (higher score first, lower reference index
 * among equal scores); with n_near == n_refs it is the unscreened call's `out`.  cand (n_queries * n_near, or NULL) receives the
 * candidates' reference indices in (D, index) order, scores (n_queries * n_near, or NULL) their scores in the same order.
 * 1 <= top <= n_near <= min(n_refs, KGMA_KMAT_MAX_NEAR), 1 <= screen_k <= 10 (KGMA_E_ARG / KGMA_E_UNSUPPORTED as above);
 * lengths follow KGMA_ASSIGN_MAX_LEN.  The k-mer pass follows kmer_count: a byte outside A/C/G/T/N in a query (inside its range)
 * or a reference is KGMA_E_BADBASE here, whereas the unscreened calls keep counting such bytes as N.  kgma_get_kmat_stats and
 * kgma_get_assign_stats both describe the call. */
int kgma_assign_seqs_screened(kgma_ctx *ctx, const uint8_t *refs, const int64_t *ref_offsets, int32_t n_refs, const uint8_t *queries,
                              const int64_t *query_offsets, int64_t n_queries, int32_t gap_open_score, int32_t gap_extend_score,
                              int32_t top, int32_t screen_k, int32_t n_near, kgma_assignment *out /* n_queries * top */,
                              int32_t *cand /* n_queries * n_near, or NULL */, int32_t *scores /* n_queries * n_near, or NULL */);
int kgma_assign_ranges_screened(kgma_ctx *ctx, const kgma_genome *genome, const uint8_t *refs, const int64_t *ref_offsets, int32_t n_refs,
                                int64_t n_queries, const int32_t *contig, const int64_t *lo, const int64_t *hi, int32_t gap_open_score,
                                int32_t gap_extend_score, int32_t top, int32_t screen_k, int32_t n_near, kgma_assignment *out,
                                int32_t *cand, int32_t *scores);

/* ---- k-mer counts of the resident genome (kgma_spectrum.hip, kgma_spectrum.cpp) ----
 * counts[r * 4^k + x] = how often the k-mer of value x (first base most significant: the order of kgma_kmer_count_batch and of
 * kgma_set_refs) begins at a considered start of range r: residues lo[r] .. hi[r] (1-based inclusive) of record contig[r] (0-based)
 * of length L; hi = lo - 1 is an empty range.  Ranges may be unsorted, overlapping or duplicated; each has its own row.
 *
 * Considered starts: every p with lo <= p and p + k - 1 <= hi -- the row is kmer_count(view(seq, lo:hi), k) (src/Kmers.jl:14-28).
 * With KGMA_COUNT_BY_START: every p in lo .. hi with p + k - 1 <= L: a k-mer belongs to the range it starts in, so the rows of
 * ranges that tile a record sum to the record's whole count.
 *
 * flags == 0 (or BY_START alone): residues go through the reference's code table, A0 C1 G2 T3 and N -> 3, in either case.  Every
 * residue the range covers is looked up, also when the range is shorter than k (BY_START: lo .. min(hi + k - 1, L)); a byte
 * outside A/C/G/T/N among them is KGMA_E_BADBASE (the reference's KeyError) and kgma_last_error names the smallest (record,
 * position) among such bytes; such a byte outside every requested range is no error.  For a whole record (lo = 1, hi = L) the row
 * equals kgma_kmer_count_batch of the same bytes, value for value.
 * KGMA_COUNT_SKIP_N: a considered start whose k residues hold a byte outside A/C/G/T (either case) is not counted but counted in
 * n_skipped[r]; there is no KGMA_E_BADBASE in this mode, IUPAC codes are skipped like N.
 * KGMA_COUNT_SKIP_MASKED: a considered start whose k residues hold a lower-case byte (the soft-mask of a .2bit genome) is not
 * counted either and goes to n_skipped[r] too.  The flags combine freely; without SKIP_N an N in either case still counts as T and
 * a byte outside A/C/G/T/N is still KGMA_E_BADBASE, masked or not.
 * INVARIANT: the sum of row r plus n_skipped[r] is the number of considered starts of range r.
 *
 * 1 <= k <= 10.  KGMA_E_UNSUPPORTED: k > 10; n_ranges * 4^k > 2^28 (2 GiB of counts).  KGMA_E_ARG: a null pointer (n_skipped may
 * be NULL), k < 1, unknown flag bits, a record out of range, lo < 1, hi > L or hi < lo - 1 (kgma_last_error names the range).
 * n_ranges == 0: KGMA_OK.  KGMA_E_NOMEM leaves the context usable.  The call needs no kgma_set_refs; nothing stays allocated after
 * it; it leaves references, thresholds, hits, dips, distances, alignments and the matches of the four searches untouched.  Of
 * kgma_stats it sets scan_ms and n_launches only; kgma_scan_kernel_name afterwards names the form that ran,
 * "spectrum_kernel<wg>", "spectrum_kernel<wave>" or "spectrum_kernel<global>". */
enum { KGMA_COUNT_SKIP_N = 1u << 0, KGMA_COUNT_SKIP_MASKED = 1u << 1, KGMA_COUNT_BY_START = 1u << 2 };
int kgma_genome_kmer_count(kgma_ctx *ctx, const kgma_genome *g, int32_t k, uint32_t flags, int64_t n_ranges,
                           const int32_t *contig /* 0-based */, const int64_t *lo, const int64_t *hi /* 1-based inclusive */,
                           int64_t *counts /* n_ranges * 4^k, row-major */, int64_t *n_skipped /* n_ranges, or NULL */);
/* The last kgma_genome_kmer_count on the context: device time of the rows' memset and the launch (hipEvents), the ranges, the
 * considered starts, and the form that ran: 0 = `wg` (4^k counters in a workgroup's LDS, k <= 7), 1 = `wave` (a table per wave,
 * k <= 4, chosen when the mean range is shorter than a unit of `wg`), 2 = `global` (atomic adds straight into the rows, k >= 8);
 * span = considered starts of a unit of work, n_workgroups = workgroups launched.  All zero before the first call and after a call
 * that failed or had no range. */
typedef struct { double count_ms; int64_t n_ranges, n_positions; int32_t form, span, n_workgroups, n_launches; } kgma_spectrum_stats;
int kgma_get_spectrum_stats(kgma_ctx *ctx, kgma_spectrum_stats *out);

/* kgma_repack_scan_hits in two halves, for step loops that have other work to queue while the GPU scans
 * (bench.py with several ranks: the hit exchange of step i overlaps the scan of step i+1).  kgma_step_begin
 * hands the step to a helper thread owned by the context and returns at once; kgma_step_end waits for it
 * and copies the hits out (same contract as kgma_repack_scan_hits for out/cap/n).  Between the two calls
 * the caller must not use the context or the genome.  One step in flight per context. */
int kgma_step_begin(kgma_ctx *ctx, kgma_genome *genome, int32_t mode, int64_t buff, int64_t genome_pos0, uint32_t flags);
int kgma_step_end(kgma_ctx *ctx, kgma_hit *out, int64_t cap, int64_t *n);

/* The count-table stream kernel sizes its streams so that one round of workgroups fills every CU of the chip
 * (one workgroup takes a CU's whole LDS).  A caller that runs other kernels beside the scan -- the RCCL
 * collective of a multi-rank step loop, whose workgroups wait on their peers while resident -- reserves `n`
 * CUs for them (0 .. half of the device's CUs, queried at kgma_create; default 0): the scan then uses (CUs - n) x the
 * resident waves per CU as its number of streams per round, so that neither kernel
 * waits for the other's workgroups to retire.  Takes effect at the next scan. */
int kgma_set_reserved_cus(kgma_ctx *ctx, int32_t n);

/* Host stream handle (hipStream_t) the context launches on, for callers that time with hipEvents. */
void *kgma_stream(kgma_ctx *ctx);

/* Name of the device kernel the last scan launched ("stream8_kernel<6>" / "stream_kernel<6>" / "scan_kernel<8>"): the
 * count-table stream kernel "stream8_kernel" serves k = 5, 6, 7 (8-bit counters for windows of <= 383 k-mers, up to eight KFVs
 * of neighbouring window sizes per launch; 16-bit counters and 64-bit prefix carries for longer windows -- up to 65535 k-mers --
 * and for prefixes beyond int32, up to four KFVs of one size per launch), the bit-sliced kernel "scan_kernel" the other k up to
 * 2031 k-mers per window, the generic kernel "gen_kernel<k>" / "gen_kernel<f64,k>" (kgma_generic.hip, one KFV per launch) what is
 * left: longer windows at k < 5 and k > 7, and every scan with a general Float64 KFV (the round-1 16-bit kernel
 * "stream_kernel" runs under testing switches only). */
const char *kgma_scan_kernel_name(const kgma_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* KGMA_H */
