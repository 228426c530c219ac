// kgma_device.h -- structures shared between the host side (kgma_api.cpp) and the gfx950 kernels
// (kgma_kernels.hip).  Internal to libkgma; the public boundary is include/kgma.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace kgma {

// Geometry of one scan tile: a workgroup of KGMA_THREADS lanes (4 waves); 253 distinct lane slots
// each own KGMA_R consecutive 32-window words of one record (kgma_kernels.hip explains the halos).
constexpr int KGMA_THREADS = 256;
constexpr int KGMA_R = 2;
constexpr int KGMA_TILE_WORDS = 253 * KGMA_R;                 // words covered by one tile (incl. halos)
constexpr int KGMA_TILE_WINDOWS = KGMA_TILE_WORDS * 32;
constexpr int KGMA_MAX_GROUP = 8;                              // KFVs of one window size per launch
constexpr int KGMA_NPLANES_SMALL = 9;                          // bit-sliced counter width for <= 495 k-mers per window
constexpr int KGMA_NPLANES_LARGE = 11;                         // ... for <= 2031
constexpr int KGMA_MAX_NK_SMALL = 16 * 31 - 1;
constexpr int KGMA_MAX_NK = 16 * 127 - 1;                      // max k-mers per window of the bit-sliced kernel (counter range)
constexpr int KGMA_MAX_NK_WIDE = 65535;                        // ... of the 16-bit count-table kernels (stream8 C16 form, generic kernel)

// One tile of the scan grid (built on the host, read by every workgroup).
struct TileDesc {
    int64_t word_base;   // word index (per plane) of the tile's first base in the plane array
    int64_t win0;        // 1-based window start of local position 0
    int64_t dist_base;   // index into the per-KFV distance array of local position 0 (may be -1)
    int32_t n_valid;     // windows of this tile that exist and are evaluated (1..KGMA_TILE_WINDOWS)
    int32_t first_test;  // first local position that is TESTED against the threshold (1 on a
                         // record's first tile: the first window is never tested, GenomeMiner.jl:57)
    int32_t contig;
    int32_t pad;
};

constexpr int KGMA_MAX_SIZES = 4;                              // distinct window sizes per launch
constexpr int KGMA_MAX_DW = 8;                                 // max spread of k-mers-per-window within a launch

// Parameters of one launch: up to KGMA_MAX_GROUP KFVs whose window sizes differ by <= KGMA_MAX_DW
// (<= KGMA_MAX_SIZES distinct values).  The match loop runs once, for the largest size.
struct GroupParams {
    int32_t n_kfv;                       // KFVs in this launch (<= KGMA_MAX_GROUP)
    int32_t k;                           // k-mer length
    int32_t nk;                          // k-mers per window (W - k + 1) of the LARGEST window of the launch
    int32_t nk_min;                      // ... of the smallest
    int32_t n_sizes;                     // distinct sizes
    int32_t sizes[KGMA_MAX_SIZES];       // distinct k-mers-per-window values, ascending
    int32_t nk_of[KGMA_MAX_GROUP];       // k-mers per window of each KFV
    int32_t nblocks;                     // 16-offset blocks of the match loop
    int32_t debug_skip;                  // timing experiments only (bit 0: no match loop, bit 1: no position phase); 0 in product use
    int32_t stream_slots;                // stream kernels: streams resident per CU the tile table was sized for (all launches of a scan share it)
    int32_t s_fits_u8;                   // every S entry of the launch's KFVs is below 256 (the five-KFV stream8_kernel keeps rows of bytes)
    int32_t s_fits_i16;                  // every S entry of the launch's KFVs fits int16 (stream8_kernel keeps the table as int16)
    int32_t need_wide;                   // a KFV of the launch needs the 64-bit prefix carry (its E = (D - D0) / 2N leaves int32): the 16-bit
                                         // counter form of stream8_kernel serves it whatever its window length
    int32_t kfv_id[KGMA_MAX_GROUP];      // 1-based KFV index reported in records
    int32_t N[KGMA_MAX_GROUP];           // reference count of each KFV
    int64_t T[KGMA_MAX_GROUP];           // integer threshold: window below thr  <=>  D < T
    int64_t T_hi[KGMA_MAX_GROUP];        // T <= D <= T_hi: at threshold (ATT records); T_hi < T: no band
    int64_t sumS2[KGMA_MAX_GROUP];       // sum_x S[x]^2
    double inv_scale[KGMA_MAX_GROUP];    // 2 k N^2 as a double (distance = D / that)
    // chain launches (kgma_device.h: ChainArgs), per KFV slot:
    double chain_invN[4];                // RN(1 / N)
    int32_t chain_form[4];               // how the KFV's Float64 entries follow from S (checked entry by entry on the host):
                                         // 0: RN(S * invN) -- `answer .* (1/N)`, src/ReferenceGeneration.jl:35,40;
                                         // 1: RN(S / N) -- `KFVs[i] ./= lens[i]`, src/ReferenceGeneration.jl:118
};

// Device record kinds (low bits of DevRecord::kind_kfv) and the WIDE flag: the record's two values (minimum, exit) are 64-bit
// quantities kept in (minE_hi : minE) and (exitE_hi : exitE) -- an int64 prefix E from the kernels that carry the prefix in
// 64 bits (windows of more than 2031 k-mers, large N), or the bits of a Float64 distance from the Float64 KFV path.  Records
// without the flag hold int32 E values and leave the two high words unwritten.
enum : int32_t { REC_RUN = 0, REC_EXIT = 1, REC_ATT = 2, REC_FAULT = 3 /* the kernel gave up on a stream (internal error) */, REC_KIND_MASK = 0x3F, REC_WIDE = 0x40 };

// One record emitted by the scan kernel (positions are local to the tile; E is the integer
// prefix (D - D0[tile]) / (2N)).
struct DevRecord {
    int32_t tile;
    int32_t kind_kfv;     // kind | (1-based KFV index << 8)
    int32_t start, end;   // RUN: first/last local position of the under-threshold fragment
                          // EXIT/ATT: start = position
    int32_t minE;         // RUN: minimum E;  EXIT/ATT: E at the position
    int32_t argf, argl;   // RUN: first / last local position attaining minE
    int32_t nmin;         // RUN: number of positions attaining minE
    int32_t exitE;        // RUN: E at end+1 when has_exit
    int32_t has_exit;     // RUN: bit 0 = end+1 was evaluated by the same lane/wave (exitE valid);
                          // bits 1.. = 1 + 16-byte slot of the residues under the tied minimum in the aux region (0: none)
    int32_t minE_hi;      // REC_WIDE records only: high words of the two values
    int32_t exitE_hi;
};
static_assert(sizeof(DevRecord) == 48, "device records are 48 bytes");

// ---- Float64 chain on the device (stream8_kernel<..., CHAIN>; KGMA_F_CHAIN_REPLAY) --------------------------
// The reference's running distance is ONE sequential Float64 value per record and KFV: v' = RN(v + inc)
// (src/GenomeMiner.jl:70-72, src/OmnGenomeMiner.jl:101-108).  The increment of a window is a function of that
// window's exact counts alone, so every lane can form it; what is sequential is the rounding.  Inside one binade
// v is an integer number of ulps, RN(v + inc) = v + a when v is even and v + b when it is odd, with a == b unless
// the sum lands exactly half way between two doubles (then the even neighbour wins and the result is EVEN whatever
// v was).  So a run of windows inside one binade is a translation by the sum of its a's, corrected at the ties by
// the parity the value has there -- a parity that only the run's FIRST tie can inherit from the incoming value.
// A chain stream cuts its positions into steps of 64 and chunks of KGMA_CHAIN_STEPS steps.  A step is RAW when the
// host marked it hot (it holds a window whose value the host wants) or when one of its windows may leave the binade
// (decided on the exact integer D with a guard band): its 64 Float64 increments go to the pool.  Every other step
// is regular, and consecutive regular steps of a chunk are one RUN: a translation for both parities of the incoming
// value (A0, A1 = A0 + dA).  A chunk without a raw step is its one record in the chunk array; a chunk with raw steps
// is "detailed": its record holds the leading run and points at a list of entries in the pool, one per later run and
// per raw step, in order.  The host walks a record's chunks in order: an integer add per run, a hardware add per raw
// increment (kgma_chain.cpp).
#ifndef KGMA_CHAIN_STEPS_LOG2_V
#define KGMA_CHAIN_STEPS_LOG2_V 6
#endif
constexpr int KGMA_CHAIN_STEPS_LOG2 = KGMA_CHAIN_STEPS_LOG2_V;
constexpr int KGMA_CHAIN_STEPS = 1 << KGMA_CHAIN_STEPS_LOG2;   // 64-position steps per chunk (64 steps = 4096 positions; <= 64: one hot bit per step)
constexpr uint32_t KGMA_CHAIN_RAW = 1u << 10;                  // entry: one raw step, `raw` = pool unit of its 64 doubles
constexpr uint32_t KGMA_CHAIN_DETAIL = 1u << 11;               // chunk record: `raw` = pool unit of its entry list
struct ChainChunk {       // a chunk's record, or an entry of a detailed chunk (16 bytes = one pool unit)
    int64_t A0;           // ulps the run adds when the incoming value's mantissa is even
    uint32_t info;        // bits 0-1: dA + 1 (A1 = A0 + dA);  bits 2-9: steps of the run;  KGMA_CHAIN_RAW / KGMA_CHAIN_DETAIL
    uint32_t raw;
};
struct ChainArgs {
    ChainChunk *chunks;           // [all chunks of the launch] (a stream's first chunk: TileDesc::dist_base)
    ChainChunk *pool;             // entries of detailed chunks and raw increments (64 doubles = 32 units per raw step)
    unsigned int *pool_cursor;    // units handed out
    unsigned int pool_cap;        // units available
    const uint32_t *hot;          // one bit per chunk: it has hot steps
    const uint32_t *hot_prefix;   // per word of `hot`: hot chunks before it
    const uint64_t *hot_masks;    // per hot chunk, in chunk order: its hot steps
    int64_t chunk_stride;         // chunk records of KFV slot j of the launch: chunks[first chunk + j * chunk_stride] (hot bits alike)
    double SF;                    // ScaleFactor = 1 / k (src/API.jl:86,204)
    double guard;                 // relative guard band around the powers of two (2^-29)
    double guard_abs;             // ... and an absolute one, as a fraction of the STREAM's first-window distance (2^-30): the host
                                  // checks the running value against the exact one at every stream start, relative to that
                                  // distance -- so that is what bounds the value's ABSOLUTE error inside the stream, also at
                                  // windows whose own distance is tiny (a perfect match inside a record of ordinary distances)
    unsigned int *status;         // bit 0: the pool ran out
};

// Arguments of one scan launch (either kernel).
struct ScanArgs {
    const uint32_t *planes;
    const uint32_t *inter;      // the same genome as 2-bit codes, 16 bases per dword (first base = bits 0-1): two dwords per plane word
    const TileDesc *tiles;
    const int32_t *Stab;        // all KFVs' tables, 4^k int32 each, in the launching kernel's index order
    const int16_t *Sinter;      // stream8_kernel at k = 7: the launch's S tables interleaved per k-mer (rows of NV int16 slots), in global
                                // memory, COMPACTED: only the rows with a non-zero entry, behind row 0 which is all zero
    const uint32_t *Sbits;      // ... and, per 32 k-mers, {bitmap of the non-zero rows, 1 + number of non-zero rows before them}: the row
                                // of k-mer x is Sbits[2 (x / 32) + 1] + popcount(bits below x) if bit x % 32 is set, else 0
    int64_t *D0out;             // [KFV id - 1][n_tiles]
    DevRecord *recs;
    unsigned int *rec_count;
    unsigned int rec_cap;
    int32_t n_tiles;
    double *dist[KGMA_MAX_GROUP];   // per-KFV distance arrays or nullptr
    unsigned long long *n_att;      // stats: tested windows inside the threshold guard band
    unsigned long long *n_cold;     // stats: stream8_kernel steps that left the fast path for the exact counts
    // stream8_kernel launched over a PART of the stream table (the pack / scan overlap of kgma_repack_scan_hits): `tiles`, `D0out`
    // and `n_tiles` are the part's, tile0 its first stream's index in the whole table (added to the records' tile numbers).
    // two-kernel cluster path (kgma_pos.hip): this launch covers tiles [tile0, tile0 + n_chunk_tiles);
    // diff[z] holds, per window size z of the launch, tile_windows int16 per tile of the chunk
    int32_t tile0, n_chunk_tiles;
    int64_t tile_windows;
    int16_t *diff[KGMA_MAX_SIZES];
    int32_t *wave_state;            // stream8_kernel at k = 7 with several KFVs: per-stream cold state (stream8_state_words() words each)
    ChainArgs chain;                // chain launches only (no other kernel reads it)
};

// Parameters of one launch of the generic kernel (kgma_generic.hip): ONE KFV, any 2 <= k <= 10, up to 65535 k-mers per
// window; integer form (S/N KFV, int64 prefix) or Float64 form (any KFV).
struct GenParams {
    int32_t k, nk;                       // k-mer length, k-mers per window
    int32_t N;                           // integer form: reference count
    int32_t kfv_id;                      // 1-based KFV index reported in records
    int32_t n_slots;                     // wave slots of the launch (grid x waves per workgroup): the streams are dealt over them
    int32_t fp;                          // Float64 form
    int64_t T, T_hi, sumS2;              // integer form: thresholds (as GroupParams), sum_x S[x]^2
    double thr_lo, thr_hi;               // Float64 form: below thr <=> d < thr_lo; thr_lo <= d <= thr_hi: at threshold
    double sumR2;                        // Float64 form: sum_x ref[x]^2
    double SF;                           // ScaleFactor = 1 / k
    double inv_scale;                    // integer form: 2 k N^2
    double tie_rel;                      // Float64 form: minima within this relative distance of each other are reported as tied
    const int32_t *S;                    // integer form: the KFV's S table, 2-bit interleaved index order (first base least significant)
    const double *R;                     // Float64 form: the KFV as given, same index order
    uint32_t *ctab;                      // k >= 8: 4^k / 2 dwords of counters per wave slot (global memory)
    // where the wave keeps its counts (generic_set_mode): 0 = 4^k 16-bit counters in LDS (k <= 7), 1 = the same in global memory,
    // 2 = a hash table of the window's distinct k-mers in LDS (k >= 8, windows of at most KGMA_HASH_MAX_NK k-mers): 2^hash_log2m
    // dwords per wave, rebuilt from the window every hash_rebuild steps;  k >= 11 (kgma_generic.hip, "wide" tables): 3 = a hash table
    // of 2^hash_log2m entries of 16 bytes (key, 32-bit count, the KFV's value) per wave in LDS (windows of at most KGMA_WIDE_LDS_MAX_NK
    // k-mers), 4 = the same table in global memory (ctab, 4 << hash_log2m dwords per wave slot);  k = 1: 5 = four 32-bit counters in LDS
    int32_t cmode, hash_log2m, hash_rebuild;
    // k >= 11: the KFV as an open-addressed table of its non-zero entries in global memory (no 4^k table exists): 2^sp_log2 slots,
    // keys in the kernels' index order (0xFFFFFFFF: empty, at least half of the slots), values as 64-bit patterns -- the int32 S entry
    // sign-extended (integer form) or the Float64 entry's bits (Float64 form, chain kernel).  An absent key is 0.
    const uint32_t *sp_keys;
    const uint64_t *sp_vals;
    int32_t sp_log2;
};
constexpr int KGMA_HASH_MAX_NK = 1983;                         // count field of 11 bits: n + 64 <= 2047
constexpr int KGMA_WIDE_MIN_K = 11;                            // k-mers of 2k > 20 bits: the wide tables (cmode 3 / 4) and the sparse KFV
constexpr int KGMA_MAX_K = 15;                                 // 2k <= 30 bits: a k-mer is one dword of the 2-bit genome copy
// cmode 3 up to this many k-mers per window (4096 entries, 64 KiB per wave, 2 waves per CU, >= 23 steps between rebuilds); measured at k = 12,
// 400 Mb: LDS / global 9.3 / 4.6 Gbp/s at n = 989, 4.8 / 3.9 at 1489, 4.6 / 3.1 at 1989, 1.4 / 3.0 at 2989 (EXPERIMENTS)
constexpr int KGMA_WIDE_LDS_MAX_NK = 2048;
constexpr int KGMA_WIDE_LDS_NK_CAP = 8192 - 64 - 1024 - 512;   // ... the most an LDS table can serve: 8192 entries, 128 KiB (one wave per CU)
constexpr uint32_t KGMA_SP_EMPTY = 0xFFFFFFFFu;

// Parameters of one launch of the strobemer kernel (kgma_strobe.hip): the integer form of the generic kernel with a randstrobe
// bin (4^(2s) of them) in the place of the k-mer.  nk is the number of strobemers that slide (W - k); every window holds one more,
// the record's strobemer W - k + 1, which never leaves (StrobeGenomeMiner.jl:50-57 re-enters the window's own last strobemer).
struct StrobeParams {
    int32_t s, w_min, w_max;             // randstrobe parameters (Strobemers.jl:45-65); k = w_max + s - 1 <= 16 residues per strobemer
    int32_t nk;                          // strobemers that slide per window: W - k
    int32_t N;                           // reference count
    int32_t kfv_id;                      // 1-based KFV index reported in records (1)
    int32_t n_slots;                     // wave slots of the launch
    int32_t pad;
    int64_t T, T_hi, sumS2;              // as GenParams
    double inv_scale;                    // 2 k N^2
    const int32_t *S;                    // the KFV's S table, 4^(2s) entries, natural bin order (first * 4^s + second)
    uint32_t zero[4];                    // bit v: v % q == 0, for the sums of two s-mer values (< 2 * 4^s <= 128)
};
constexpr int KGMA_STROBE_MAX_S = 3;                           // 4^(2s) 16-bit counters per wave and the S table fit the LDS; sums fit `zero`
constexpr int KGMA_STROBE_MAX_K = 16;                          // a strobemer's residues are one dword of the 2-bit genome copy
// the zero-score mask words of the bin rule (kgma_strobe_bin.h) for the modulus q >= 1
inline void strobe_zero_mask(int64_t q, uint32_t zero[4])
{
    for (int i = 0; i < 4; i++) zero[i] = 0;
    for (int64_t v = 0; v < 128; v++)
        if (v % q == 0) zero[v >> 5] |= 1u << (v & 31);
}

// Count-table stream kernel (kgma_stream.hip): one wave per stream of consecutive window starts.
constexpr int KGMA_STREAM_MIN_WINDOWS = 2048;                  // shorter streams waste their warm-up (n k-mers)
constexpr int KGMA_STREAM_MAX_WINDOWS = 1 << 19;               // longer genomes take more rounds (100 Gb, one KFV: 24 rounds of 509 k windows
                                                               // 155.1 ms, 12 rounds of 1 M windows 157.3 ms, 48 rounds 154.5 ms)
constexpr int KGMA_STREAM_MAX_K = 7;                           // 4^k 16-bit counters per wave must fit the LDS

// Distance-bound prefilter of the one-KFV scan at k = 5, 6 (kgma_filter.hip).  A GRANULE is 16 consecutive window starts of a
// record; an entry names the granules of one wave iteration that may hold a window with D <= Dmax.
struct FilterEntry {
    int32_t contig;
    int32_t gbase;        // granule of bit 0 of the mask (negative at a record's start: those bits are never set)
    uint64_t mask;
};
static_assert(sizeof(FilterEntry) == 16, "filter entries are 16 bytes");
struct ContigDesc;
struct FilterArgs {
    const uint32_t *inter;        // the 2-bit genome copy the scan reads
    int64_t n_dwords;             // its length
    const TileDesc *tiles;        // the scan's regular stream table: one wave walks one stream's granules
    int32_t n_tiles;
    int32_t nblk;                 // blocks of 16 positions a granule's windows use: floor((n + 14) / 16) + 1
    const ContigDesc *cd;
    const int32_t *S;             // the KFV's S table (4^k int32, the 2-bit copy's index order); every entry in 0 ... 65535
    uint32_t U;                   // candidate: the granule's sum of S reaches U
    unsigned int cap;             // entries the list holds
    FilterEntry *list;
    unsigned int *ctl;            // entries appended (keeps counting past cap)
    const uint16_t *bsum;         // filter_sums_kernel: the block sums pack_sums_kernel wrote beside `inter` in this step (else null)
};

// The step's pack with the prefilter's block sums (kgma_filter.hip: pack_sums_kernel): what pack_kernel writes, plus per dword J of
// `inter` the sum of S over the k-mers that start in it and belong to its record (0 for padding) -- bsum[J], 16 x 255 at most.
struct PackSumsArgs {
    const uint8_t *ascii;
    uint32_t *planes;             // may be null, as for pack_kernel
    uint32_t *inter;
    uint16_t *bsum;               // [2 * total_words]
    const ContigDesc *cd;
    int64_t total_words;
    const int32_t *block_contig;  // record of the first word of every block of 2^block_shift words (pack_kernel's table)
    unsigned long long *first_bad;
    const int32_t *S;             // the KFV's S table as FilterArgs::S, every entry below 256
    int32_t n_contigs;
    int32_t block_shift;
    // the form that makes the prefilter's granule test itself (pack_sums_kernel<K, false, true>; else list is null): FilterArgs' U,
    // nblk, cap, list and ctl -- ctl[1] counts the units that went word by word, ctl[2] the chunks primed -- and
    int32_t nblk;
    int32_t nk;                   // k-mers of a window (a record has len - (nk + K - 1) + 1 windows)
    int32_t run;                  // consecutive units a wave takes at a time
    uint32_t U;
    unsigned int cap;
    FilterEntry *list;
    unsigned int *ctl;
};

// Aux region of the result block: residues under tied minima, gathered on the device (export_kernel)
constexpr int KGMA_AUX_BYTES = 64 << 10;
constexpr int KGMA_RES_HDR = 32;                               // counters at the head of a scan's result block (kgma_api.cpp)
constexpr int KGMA_AUX_MAX_RANGE = 4096;                       // longest residue range gathered speculatively

// One hit to re-align on the device (kgma_align.hip): its segment of the resident residue text.
struct AlignJob {
    int64_t ascii_off;    // byte offset of the segment's first residue
    int32_t n;            // residues
    int32_t pad;
};
constexpr int KGMA_ALIGN_MAX_SEGMENT = 8191;                   // longest segment (LDS rows of the wavefront)
constexpr int KGMA_ALIGN_MAX_CONSENSUS = 65535;

// Per-record info for the pack kernel.
struct ContigDesc {
    int64_t ascii_off;    // byte offset of the record's first residue in the ASCII buffer (32-aligned)
    int64_t word_off;     // word index of the record's first base in the plane array
    int64_t len;          // residues
};


// Exact sequence search (kgma_exact.hip; exactMatch, src/ExactMatch.jl:89-121).  One query of a launch: its case-folded text
// (byte & 0xDF: letters to upper case, '-' to 0x0D) at qtext + text_off, and the leading symbols the kernel tests in registers --
// ASCII kernel: the first min(len, 8) folded bytes, little endian, in pat[0..1] with a byte mask in mask[0..1]; 2-bit kernel: the
// codes of the first min(len, 16) symbols (first symbol = bits 0-1, as the interleaved genome copy) in pat[0] with mask[0].
struct ExactQuery {
    int64_t text_off, len;
    uint32_t pat[2], mask[2];
    int32_t id;           // 0-based query index reported in the matches
    int32_t pad;
};
struct ExactMatch {       // = kgma_match
    int32_t query, contig;
    int64_t start;        // 1-based
};
static_assert(sizeof(ExactMatch) == 16, "matches are 16 bytes");
constexpr int KGMA_EXACT_THREADS = 256;
constexpr int KGMA_EXACT_ITERS = 4;                            // runs of start positions a lane takes per tile
constexpr int KGMA_EXACT_RUN_ASCII = 16;                       // start positions per run: one 16-byte load (+ 8 bytes of the next run)
constexpr int KGMA_EXACT_RUN_2BIT = 32;                        // ... two dwords of the interleaved copy (+ one of the next run)
struct ExactArgs {
    const uint8_t *ascii;
    const uint32_t *inter;
    const ContigDesc *cd;
    const int64_t *tile_prefix;   // [n_contigs + 1]: tiles of the records before record c (a tile never spans two records)
    int32_t n_contigs, n_queries;
    const ExactQuery *queries;
    const uint8_t *qtext;
    ExactMatch *out;
    unsigned long long *ctl;      // [0]: matches found (keeps counting past cap), [1]: smallest (record << 40 | 0-based offset) of a
                                  // residue outside the 16-symbol alphabet (checking launches only)
    unsigned long long cap;
};

// IUPAC motif search with mismatches (kgma_motif.hip; kgma_motif_match).  One motif of a launch: its INFORMATIVE (non-N) positions
// only, as entries `offset | set << 8` (offset 0 ... 63 in the motif, set: bit 0 A, 1 C, 2 G, 3 T of the bases the symbol stands
// for) at info + info_off -- first the n_lo entries with offset < 32, then the n_hi entries with offset >= 32, then one spare entry
// (the kernel reads one entry ahead).
struct MotifDesc {
    int32_t info_off;
    int32_t n_lo, n_hi;
    int32_t len;          // symbols, 1 ... 64
    int32_t max_mm;       // mismatches allowed, 0 ... 15 and < n_lo + n_hi
    int32_t id;           // 0-based motif index reported in the hits
    int32_t pad[2];
};
struct MotifHit {         // = kgma_motif_hit
    int32_t motif, contig;
    int64_t start;        // 1-based
    int32_t mismatches, reserved;
};
static_assert(sizeof(MotifHit) == 24, "motif hits are 24 bytes");
constexpr int KGMA_MOTIF_THREADS = 256;
constexpr int KGMA_MOTIF_ITERS = 4;                            // plane words (32 start positions each) a lane takes per tile
struct MotifArgs {
    const uint32_t *planes;       // the plane copy: a {hi, lo} word pair per 32 bases (N stored as T)
    const uint8_t *ascii;
    const ContigDesc *cd;
    const int64_t *tile_prefix;   // [n_contigs + 1]: tiles of the records before record c (a tile never spans two records)
    int32_t n_contigs, n_motifs;
    const MotifDesc *motifs;
    const uint32_t *info;
    MotifHit *out;
    unsigned long long *ctl;      // [0]: hits found (keeps counting past cap)
    unsigned long long cap;
};

// Reverse complement of the residue text (kgma_revcomp.hip; kgma_genome_revcomp).  Source and destination have the same layout.
constexpr int KGMA_REVCOMP_THREADS = 256;
constexpr int KGMA_REVCOMP_ITERS = 4;                          // 16-byte chunks a lane takes per tile (a tile: 16 KiB of a record's slot)
struct RevcompArgs {
    const uint8_t *src;           // the source genome's residue text
    uint8_t *dst;                 // the destination's: every byte of every record's slot is written
    const ContigDesc *cd;
    const int64_t *tile_prefix;   // [n_contigs + 1]: tiles of the records before record c (a tile never spans two records)
    int32_t n_contigs;
    int32_t pad;
};

// .2bit ingest (kgma_twobit.hip; kgma_genome_from_2bit_file): the packed bases of every record as they lie in the file, four per
// byte, and the normalised N / mask block lists -> the resident residue text.  Tiled as the reverse complement above.
constexpr int KGMA_TWOBIT_THREADS = 256;
constexpr int KGMA_TWOBIT_ITERS = 4;                           // 16-byte chunks a lane takes per tile (a tile: 16 KiB of a record's slot)
struct TwobitBlock { uint32_t start, end; };                   // residues start .. end - 1 of the record (0-based)
struct TwobitArgs {
    const uint8_t *packed;        // record c's packed bytes at packed + packed_off[c]: 16-byte aligned, padded to a multiple of 16
    uint8_t *dst;                 // the genome's residue text: every byte of every record's slot is written
    const ContigDesc *cd;
    const int64_t *tile_prefix;   // [n_contigs + 1]: tiles of the records before record c (a tile never spans two records)
    const int64_t *packed_off;    // [n_contigs]
    const int64_t *n_prefix;      // [n_contigs + 1]: record c's N blocks are blk[n_prefix[c] .. n_prefix[c + 1])
    const int64_t *m_prefix;      // [n_contigs + 1]: its mask blocks blk[m_prefix[c] .. m_prefix[c + 1])
    const TwobitBlock *blk;       // per record: disjoint, increasing, not adjacent
    int32_t n_contigs;
    int32_t pad;
};

// Distances of chosen windows / of mutated copies (kgma_calib.hip; kgma_window_dists, kgma_mutation_dists).  An item is a run
// of residues of `text`: window source -- item i is the W residues at text + item_off[i]; mutation source -- item
// (i * n_rates + r) * n_trials + t is sequence i, text + item_off[i] .. item_off[i + 1], under the trial key of (i, r, t).
struct CalibArgs {
    const uint8_t *text;          // the genome's residue text / the uploaded sequences
    const int64_t *item_off;      // window source: [n_items] byte offsets; mutation source: [n_seqs + 1]
    int64_t n_items;
    int64_t W;                    // window source: residues per window
    int32_t k, fp;                // k-mer length (1 ... 10); Float64 form
    int32_t n_rates, n_trials;    // mutation source
    uint64_t seed;                // mutation source
    const uint64_t *P;            // mutation source: [n_rates] floor(rate * 2^53)
    const int32_t *S;             // integer form: the KFV's S table, device index order (first base least significant)
    const double *R;              // Float64 form: the KFV as given, same index order
    int64_t N, sumS2;             // integer form
    double scale;                 // integer form: 2 k N^2 (dist = D / scale)
    double half_inv_k;            // Float64 form: RN(1 / 2k)
    uint32_t *scratch;            // k >= 8: 4^k counters per workgroup, all zero between items and launches
    int64_t *D_out;               // integer form: [n_items]
    double *dist_out;             // [n_items]
    unsigned long long *first_bad;   // smallest byte offset in `text` of a residue outside the source's alphabet
};
int calib_grid(int k, int64_t n_items, int n_cus);   // workgroups of a launch = rows of CalibArgs::scratch
// The strobemer form (strobe_calib_kernel; kgma_strobe_window_dists, kgma_strobe_mutation_dists): the integer form above with the
// randstrobe bin (StrobeParams, kgma_strobe_bin.h) in the place of the k-mer and 4^(2s) 32-bit counters in LDS.  `c` is read as
// above with k = w_max + s - 1 and S in natural bin order; fp, R, half_inv_k and scratch are not used.  An item of the window
// source holds W - k + 1 strobemers: those at residues 0 .. W - k - 1 of the window, and the one at residue W - k of the window's
// RECORD (its permanent item, which for the record's first window is the window's own last strobemer).
struct StrobeCalibArgs {
    CalibArgs c;
    const int64_t *rec_off;       // window source: [n_items] byte offset in `text` of the first residue of the item's record
    int32_t s, w_min, w_max, pad;
    uint32_t zero[4];             // strobe_zero_mask
};
// Gene assignment (kgma_assign.hip; kgma_assign_seqs, kgma_assign_ranges): queries x references, semi-global scores, then the
// column counts of every query's chosen references.  One launch covers the queries of one LENGTH CLASS (its LDS is sized by
// max_n, the longest query of the class) and a chunk of its pairs / jobs.
struct AssignArgs {
    const uint8_t *text;          // range source: the genome's residue text; sequence source: the uploaded queries
    const ContigDesc *cd;         // range source: the genome's record table
    const int32_t *q_contig;      // range source: [n_queries] record (0-based)
    const int64_t *q_pos;         // range source: [n_queries] first residue (1-based); sequence source: byte offset in `text`
    const int32_t *q_n;           // [n_queries] residues, 1 ... max_n for the queries of this launch
    const uint8_t *refs;          // the references' residues, one after the other
    const int64_t *ref_off;       // [n_refs + 1]
    int32_t n_refs;
    int32_t go, ge;               // penalties (positive)
    int32_t max_n;
    int64_t first;                // score: first pair of the launch (pair p: query q = items[p / n_cols], column p % n_cols);
                                  // trace: first job of the launch
    const int32_t *items;         // score: the class's queries
    int32_t *scores;              // score: [n_queries][n_cols]
    const int32_t *cand;          // score: nullptr -- a column IS its reference (n_cols = n_refs); otherwise the screened call's
    int32_t n_cols, pad;          //        candidate table [n_queries][n_cols]: column c of query q is reference cand[q * n_cols + c]
    const int32_t *job_q, *job_r; // trace: query and reference of every job
    uint8_t *trace;               // trace: trace_stride bytes per workgroup of the launch
    int64_t trace_stride;
    int32_t *out;                 // trace: 8 int32 per job = kgma_assignment
};
constexpr int KGMA_ASSIGN_LEN_MAX = 8191;                      // longest query or reference (LDS rows of the wavefront)
constexpr int KGMA_ASSIGN_CLASS_BOUNDS[3] = {255, 1023, KGMA_ASSIGN_LEN_MAX};   // longest query of each length class
constexpr int64_t KGMA_ASSIGN_PAIRS_PER_LAUNCH = 1 << 16;      // pairs of one score launch (= its grid)
constexpr int64_t KGMA_ASSIGN_TRACE_BYTES = (int64_t)1 << 30;  // trace bytes of one trace launch at most (one job at least)
int64_t assign_trace_bytes(int m, int n);
size_t assign_lds_bytes(int max_n);

// All-pairs k-mer distances (kgma_kmat.hip; kgma_kmer_dist_matrix, kgma_kmer_nearest and their _ranges forms).  The A side is
// described as AssignArgs describes its queries (a run of an uploaded buffer, or a range of a record of the resident text); B is
// always an uploaded buffer.  D[a][b] = na[a] + |c_b|^2 - 2 * sum_p c_b[x_p], p over the k-mer positions of a.
struct KmatArgs {
    const uint8_t *text;          // range source: the genome's residue text; sequence source: the uploaded A sequences
    const ContigDesc *cd;         // range source: the genome's record table
    const int32_t *q_contig;      // range source: [n_a] record (0-based)
    const int64_t *q_pos;         // range source: [n_a] first residue (1-based); sequence source: byte offset in `text`
    const int32_t *q_n;           // [n_a] residues, 0 ... KGMA_KMAT_LEN_MAX
    const uint8_t *b_text;        // B's residues, one sequence after the other
    const int64_t *b_off;         // [n_b + 1]
    int64_t n_a;
    int32_t n_b, k;
    int64_t rows_per_chunk;       // matrix kernel: rows of A of one blockIdx.y
    uint32_t *na;                 // [n_a] |c_a|^2: written by the norm kernel, read by the matrix kernel
    uint32_t *scratch;            // k >= 8: 4^k counters per workgroup, all zero between sequences and launches
    int32_t *D;                   // [n_a][n_b]
    double *dist;                 // [n_a][n_b] or nullptr
    double half_inv_k;            // RN(1 / 2k)
    unsigned long long *bad;      // [2] side A, side B: smallest (sequence << 16 | 0-based position) of a residue outside A/C/G/T/N
    int32_t n_near, pad;          // select kernel
    int32_t *near_index, *near_D; // select kernel: [n_a][n_near]
};
constexpr int KGMA_KMAT_LEN_MAX = 32767;                       // a count fits 16 bits, D fits 31
constexpr int KGMA_KMAT_THREADS = 256;
constexpr int KGMA_KMAT_MIN_ROWS = 64;                         // rows of a chunk at least (unless A has fewer): amortises a tile's build
constexpr int kmat_tile(int k) { return k <= 5 ? 16 : k == 6 ? 8 : k == 7 ? 4 : 1; }   // sequences of B per workgroup
int kmat_scratch_rows(int k);                                  // k >= 8: workgroups of a launch at most = rows of KmatArgs::scratch

#ifdef HIP_INCLUDE_HIP_HIP_RUNTIME_H                   // (host files that do not see the HIP runtime include this header too)
hipError_t launch_assign(const AssignArgs &a, int source /* 0: genome ranges, 1: uploaded sequences */, bool trace, int grid, hipStream_t st);
hipError_t launch_kmat_norm(const KmatArgs &a, int source, int grid, hipStream_t st);
hipError_t launch_kmat(const KmatArgs &a, int source, int grid_x, int grid_y, hipStream_t st);
hipError_t launch_kmat_select(const KmatArgs &a, hipStream_t st);
hipError_t launch_calib(const CalibArgs &a, int source /* 0: windows, 1: mutated copies */, int grid, hipStream_t st);
hipError_t launch_strobe_calib(const StrobeCalibArgs &a, int source, int grid, hipStream_t st);
#endif

}  // namespace kgma
