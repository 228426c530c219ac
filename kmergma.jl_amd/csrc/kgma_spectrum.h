// kgma_spectrum.h -- k-mer counting on the resident genome (kgma_genome_kmer_count; semantics: include/kgma.h): what
// kgma_spectrum.cpp (host) and kgma_spectrum.hip (kernels) share, and the call's plan -- argument checks, the considered starts
// of every range, the unit prefix, the form and its geometry -- as one function that needs neither a device nor the HIP runtime.
#ifndef KGMA_SPECTRUM_H
#define KGMA_SPECTRUM_H

#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kgma.h"
#include "kgma_device.h"

namespace kgma {

constexpr int SP_THREADS = 256;                  // a workgroup: four waves
constexpr int SP_FORM_WG = 0, SP_FORM_WAVE = 1, SP_FORM_GLOBAL = 2;
constexpr int SP_WG_SPAN = 8192;                 // considered starts of a unit: `wg` and `global` (a workgroup per unit) ...
constexpr int SP_WAVE_SPAN = 1024;               // ... and `wave` (a wave per unit: a 1000-base bin is one unit)
constexpr int SP_WG_MAX_K = 7, SP_WAVE_MAX_K = 4, SP_MAX_K = 10;
constexpr int64_t SP_MAX_COUNTS = (int64_t)1 << 28;          // n_ranges * 4^k at most: 2 GiB of int64
constexpr int64_t SP_TABLE_MAX = 0x7FFFFFFFll;   // starts of one range a group may take between two flushes (32-bit counters)
constexpr int SP_POS_BITS = 40;                  // the bad-base key: record << 40 | position (1-based)
constexpr uint32_t SP_ALL_FLAGS = KGMA_COUNT_SKIP_N | KGMA_COUNT_SKIP_MASKED | KGMA_COUNT_BY_START;

// residue classes as the kernels keep them in LDS, one byte per residue
constexpr uint32_t SP_CODE = 3u, SP_N = 4u, SP_OTHER = 8u, SP_MASKED = 16u;

struct SpectrumArgs {
    const uint8_t *text;                 // the genome's residue text
    const ContigDesc *cd;                // its record table
    const int32_t *r_contig;             // [n_ranges] record (0-based)
    const int64_t *r_lo;                 // [n_ranges] first residue (1-based) = first considered start
    const int64_t *r_starts;             // [n_ranges] considered starts
    const int64_t *r_cover;              // [n_ranges] residues the range covers, counted from lo
    const int64_t *unit_prefix;          // [n_ranges + 1] units before range r
    int64_t n_ranges, n_units;
    int64_t units_per_group;             // a group (workgroup; `wave`: wave) walks this many consecutive units
    int32_t k, span;
    uint32_t skip_mask;                  // class bits that keep a start from being counted
    int32_t check_bad;                   // a class SP_OTHER among the covered residues is reported in `bad`
    unsigned long long *counts;          // [n_ranges << 2k], zeroed
    unsigned long long *skipped;         // [n_ranges], zeroed
    unsigned long long *bad;             // smallest key of a bad residue, ~0 when there is none
};

struct SpectrumPlan {
    std::vector<int64_t> starts, cover, prefix;   // per range; prefix has n_ranges + 1 entries
    int64_t n_positions = 0, n_units = 0, units_per_group = 0, n_groups = 0, n_workgroups = 0;
    int form = SP_FORM_WG, span = SP_WG_SPAN;
    size_t lds_bytes = 0;
};

inline int sp_groups_per_wg(int form) { return form == SP_FORM_WAVE ? SP_THREADS / 64 : 1; }
// dynamic LDS of a workgroup: per group the table (not `global`) and span + 32 class bytes
inline size_t sp_lds_bytes(int form, int k, int span)
{
    const size_t table = form == SP_FORM_GLOBAL ? 0 : (size_t)4 << (2 * k);
    return (size_t)sp_groups_per_wg(form) * (table + (size_t)span + 32);
}

// The plan of a call.  record_len[c]: the genome's record lengths.  forced_form: -1 or a form (taken where k allows it);
// max_groups: > 0 caps the workgroups (KGMA_SPECTRUM_WGS); n_cus sizes the launch otherwise.  Returns KGMA_OK, or the status
// with `err` set; *empty: nothing to launch.
inline int spectrum_plan(const char *fn, const int64_t *record_len, int64_t n_records, int32_t k, uint32_t flags, int64_t n_ranges,
                         const int32_t *contig, const int64_t *lo, const int64_t *hi, bool have_counts, int forced_form, int max_wgs,
                         int n_cus, SpectrumPlan &P, std::string &err, bool *empty)
{
    char buf[320];
    *empty = false;
    auto fail = [&](int code) { err = buf; return code; };
    if (k < 1) { snprintf(buf, sizeof buf, "%s: k = %d", fn, k); return fail(KGMA_E_ARG); }
    if (k > SP_MAX_K) { snprintf(buf, sizeof buf, "%s: k = %d: the k-mer count serves k = 1 ... %d", fn, k, SP_MAX_K); return fail(KGMA_E_UNSUPPORTED); }
    if (flags & ~SP_ALL_FLAGS) { snprintf(buf, sizeof buf, "%s: unknown flag bits 0x%x", fn, flags & ~SP_ALL_FLAGS); return fail(KGMA_E_ARG); }
    if (n_ranges < 0) { snprintf(buf, sizeof buf, "%s: n_ranges = %lld", fn, (long long)n_ranges); return fail(KGMA_E_ARG); }
    if (n_ranges == 0) { *empty = true; return KGMA_OK; }
    if (!contig || !lo || !hi || !have_counts) { snprintf(buf, sizeof buf, "%s: null ranges or counts", fn); return fail(KGMA_E_ARG); }
    if (n_ranges > (SP_MAX_COUNTS >> (2 * k))) {
        snprintf(buf, sizeof buf, "%s: %lld ranges x 4^%d counts: more than 2^28 counts in one call", fn, (long long)n_ranges, k);
        return fail(KGMA_E_UNSUPPORTED);
    }
    if (n_records >= ((int64_t)1 << (63 - SP_POS_BITS))) {
        snprintf(buf, sizeof buf, "%s: a genome of %lld records", fn, (long long)n_records);
        return fail(KGMA_E_UNSUPPORTED);
    }
    const bool by_start = (flags & KGMA_COUNT_BY_START) != 0;
    P.starts.assign((size_t)n_ranges, 0);
    P.cover.assign((size_t)n_ranges, 0);
    P.n_positions = 0;
    for (int64_t r = 0; r < n_ranges; r++) {
        if (contig[r] < 0 || contig[r] >= n_records) {
            snprintf(buf, sizeof buf, "%s: range %lld: no record %d", fn, (long long)r, contig[r]);
            return fail(KGMA_E_ARG);
        }
        const int64_t L = record_len[contig[r]];
        if (lo[r] < 1 || hi[r] > L || hi[r] < lo[r] - 1) {
            snprintf(buf, sizeof buf, "%s: range %lld: %lld:%lld outside record %d of %lld residues", fn, (long long)r, (long long)lo[r],
                     (long long)hi[r], contig[r], (long long)L);
            return fail(KGMA_E_ARG);
        }
        if (L >= ((int64_t)1 << SP_POS_BITS)) {
            snprintf(buf, sizeof buf, "%s: record %d has %lld residues", fn, contig[r], (long long)L);
            return fail(KGMA_E_UNSUPPORTED);
        }
        // last covered residue and last considered start
        const int64_t last = by_start ? std::min<int64_t>(hi[r] + k - 1, L) : hi[r];
        const int64_t last_start = by_start ? std::min<int64_t>(hi[r], L - k + 1) : hi[r] - k + 1;
        P.cover[(size_t)r] = hi[r] < lo[r] ? 0 : last - lo[r] + 1;
        P.starts[(size_t)r] = hi[r] < lo[r] ? 0 : std::max<int64_t>(0, last_start - lo[r] + 1);
        P.n_positions += P.starts[(size_t)r];
    }
    // the form: `global` where no table fits; `wave` where the mean range is shorter than a unit of `wg`
    int form = k > SP_WG_MAX_K ? SP_FORM_GLOBAL : (k <= SP_WAVE_MAX_K && P.n_positions < n_ranges * (int64_t)SP_WG_SPAN) ? SP_FORM_WAVE : SP_FORM_WG;
    if (forced_form == SP_FORM_GLOBAL || (forced_form == SP_FORM_WG && k <= SP_WG_MAX_K) || (forced_form == SP_FORM_WAVE && k <= SP_WAVE_MAX_K))
        form = forced_form;
    P.form = form;
    P.span = form == SP_FORM_WAVE ? SP_WAVE_SPAN : SP_WG_SPAN;
    // units: `span` consecutive starts of one range; a range with residues and no start keeps one unit (its residues are looked up)
    P.prefix.assign((size_t)n_ranges + 1, 0);
    for (int64_t r = 0; r < n_ranges; r++) {
        const int64_t units = P.starts[(size_t)r] ? (P.starts[(size_t)r] + P.span - 1) / P.span : P.cover[(size_t)r] ? 1 : 0;
        P.prefix[(size_t)r + 1] = P.prefix[(size_t)r] + units;
    }
    P.n_units = P.prefix[(size_t)n_ranges];
    P.lds_bytes = sp_lds_bytes(form, k, P.span);
    if (P.n_units == 0) { P.units_per_group = P.n_groups = P.n_workgroups = 0; return KGMA_OK; }
    // groups: enough to fill the device a few times over, each with a contiguous chunk of units -- never more starts than a
    // 32-bit counter of the table holds between two flushes
    const int per_wg = sp_groups_per_wg(form);
    const int64_t want_wgs = max_wgs > 0 ? max_wgs : (int64_t)std::max(1, n_cus) * (form == SP_FORM_WG && k == 7 ? 2 : 8);
    int64_t upg = (P.n_units + want_wgs * per_wg - 1) / (want_wgs * per_wg);
    upg = std::max<int64_t>(1, std::min<int64_t>(upg, SP_TABLE_MAX / P.span));
    if (upg * (int64_t)P.span > SP_TABLE_MAX) { snprintf(buf, sizeof buf, "%s: a chunk of %lld units overflows a counter", fn, (long long)upg); return fail(KGMA_E_OVERFLOW); }
    P.units_per_group = upg;
    P.n_groups = (P.n_units + upg - 1) / upg;
    P.n_workgroups = (P.n_groups + per_wg - 1) / per_wg;
    if (P.n_workgroups > 0x7FFFFFFFll) { snprintf(buf, sizeof buf, "%s: %lld workgroups exceed one launch", fn, (long long)P.n_workgroups); return fail(KGMA_E_UNSUPPORTED); }
    return KGMA_OK;
}

#ifdef HIP_INCLUDE_HIP_HIP_RUNTIME_H
hipError_t launch_spectrum(const SpectrumArgs &a, int form, int64_t n_workgroups, size_t lds_bytes, hipStream_t st);
#endif

}  // namespace kgma

#endif
