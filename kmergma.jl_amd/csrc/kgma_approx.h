// kgma_approx.h -- what kgma_approx.cpp (host) and kgma_approx.hip (kernels) share, and what the context keeps for the search.
#ifndef KGMA_APPROX_H
#define KGMA_APPROX_H

#include "kgma_search.h"

namespace kgma {

// approx_kernel: a lane owns AP_TILE consecutive end positions of one record, a workgroup AP_WG_BASES.  The workgroup stages the
// residues of its ends and the AP_LEAD before them (>= 64 + 15 warm-up columns, a multiple of 16) in LDS as residue classes.
constexpr int AP_THREADS = 128;
constexpr int AP_TILE = 256;
constexpr int AP_WG_BASES = AP_THREADS * AP_TILE;
constexpr int AP_LEAD = 80;
constexpr int AP_MAX_LEN = 64;
constexpr int AP_MAX_EDITS = 15;
static_assert(AP_LEAD >= AP_MAX_LEN + AP_MAX_EDITS && AP_LEAD % 16 == 0 && AP_LEAD <= AP_TILE, "the lead holds the longest warm-up");

// Residue class of a byte of the text, either case: (byte >> 1) & 7 -- A 0, C 1, T 2, G 3, N 7; 4 is what the kernel puts
// where there is no residue (no symbol matches it: it leaves a fresh state fresh).
constexpr int AP_CLASSES = 8;
constexpr uint8_t AP_NO_RESIDUE = 'H';

struct ApproxQuery {
    // peq[c]: bit 64 - m + i is set iff a residue of class c matches symbol i (the query's last symbol is bit 63; the one-word
    // form reads the upper words).  rev[c]: bit i is set iff it matches symbol m - 1 - i (the start kernel's reversed query).
    uint64_t peq[AP_CLASSES], rev[AP_CLASSES];
    int32_t len;          // m, 1 ... 64
    int32_t max_edits;    // 0 ... 15
    int32_t id;           // 0-based query index reported in the hits
    int32_t pad;
};
struct ApproxHit {        // = kgma_approx_hit
    int32_t query, contig;
    int64_t start, end;   // 1-based; the search kernel leaves start 0, the start kernel fills it in
    int32_t edits, reserved;
};
static_assert(sizeof(ApproxHit) == 32, "approx hits are 32 bytes");

struct ApproxArgs {
    const uint8_t *ascii;
    const ContigDesc *cd;
    const int64_t *wg_prefix;     // [n_contigs + 1]: workgroups of the records before record c (none spans two records)
    int32_t n_contigs, n_queries;
    const ApproxQuery *queries;
    ApproxHit *out;
    unsigned long long *ctl;      // [0]: hits counted (also past cap)
    unsigned long long cap;
    int64_t n_hits;               // approx_start_kernel: the hits of `out` to give a start
};

hipError_t launch_approx(const ApproxArgs &a, int words, int64_t n_wg, hipStream_t st);
hipError_t launch_approx_starts(const ApproxArgs &a, hipStream_t st);

// What the context keeps for kgma_approx_match: the device buffer of the hits (kept between calls), the hits and the stats of the
// last call
struct ApproxState {
    HitBuffer<ApproxHit> out;
    std::vector<kgma_approx_hit> hits;
    kgma_approx_stats stats{};
    void release() { out.release(); }
};

// kgma_api.cpp: the state above (released by kgma_destroy)
ApproxState *ctx_approx(kgma_ctx *ctx);

}  // namespace kgma

#endif
