// kgma_spectrum.cpp -- host side of the k-mer counts of the resident genome (kgma_genome_kmer_count, kgma_get_spectrum_stats;
// kernels: kgma_spectrum.hip).
//
// One call: check the arguments and plan the launch (spectrum_plan, kgma_spectrum.h: the considered starts of every range, the
// unit prefix, the form and its geometry), upload the range arrays and the prefix, zero the rows, run the kernel, bring the rows
// and the skip counts down and turn the key of a bad residue into a message.  Every device buffer belongs to the call and is freed
// before it returns, whatever it returns.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <vector>

#include "kgma_assign.h"
#include "kgma_spectrum.h"

using namespace kgma;

static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the rows are added to as unsigned 64-bit words");

namespace {

constexpr unsigned long long NO_BAD = ~0ull;
const char *const FORM_NAME[3] = {"wg", "wave", "global"};

// testing switches, read once: KGMA_SPECTRUM_FORM=wg|wave|global forces a form where k allows it, KGMA_SPECTRUM_WGS=n caps the
// workgroups of a launch (a small genome then makes one workgroup walk several units and ranges)
struct Switches {
    int form = -1, wgs = 0;
    Switches()
    {
        if (const char *e = getenv("KGMA_SPECTRUM_FORM"))
            for (int f = 0; f < 3; f++) if (!strcmp(e, FORM_NAME[f])) form = f;
        if (const char *e = getenv("KGMA_SPECTRUM_WGS")) wgs = std::max(0, atoi(e));
    }
};
const Switches SWITCHES;

// an allocation that fails for want of memory is KGMA_E_NOMEM and leaves the context as it was
#define SP_ALLOC(expr, what)                                                                                  \
    do {                                                                                                      \
        const hipError_t e__ = (expr);                                                                        \
        if (e__ == hipErrorOutOfMemory) {                                                                     \
            (void)hipGetLastError();                                                                          \
            return failf(ctx, KGMA_E_NOMEM, "%s: no device memory for %s", fn, what);                         \
        }                                                                                                     \
        if (e__ != hipSuccess) return failf(ctx, KGMA_E_HIP, "%s: %s failed: %s", fn, #expr, hipGetErrorString(e__)); \
    } while (0)

}  // namespace

extern "C" {

int kgma_genome_kmer_count(kgma_ctx *ctx, const kgma_genome *genome, int32_t k, uint32_t flags, int64_t n_ranges, const int32_t *contig,
                           const int64_t *lo, const int64_t *hi, int64_t *counts, int64_t *n_skipped)
{
    const char *fn = "kgma_genome_kmer_count";
    if (!ctx) return KGMA_E_ARG;
    *ctx_spectrum_stats(ctx) = kgma_spectrum_stats{};
    if (!genome) return failf(ctx, KGMA_E_ARG, "%s: null genome", fn);
    const GenomeText g = genome_text(genome);
    std::vector<int64_t> len((size_t)g.n_contigs);
    for (int64_t c = 0; c < g.n_contigs; c++) len[(size_t)c] = g.cd[c].len;
    SpectrumPlan P;
    std::string err;
    bool empty = false;
    const int rc = spectrum_plan(fn, len.data(), g.n_contigs, k, flags, n_ranges, contig, lo, hi, counts != nullptr, SWITCHES.form,
                                 SWITCHES.wgs, ctx_n_cus(ctx), P, err, &empty);
    if (rc) return ctx_fail(ctx, rc, err.c_str());
    if (empty) return KGMA_OK;
    const size_t n_counts = (size_t)n_ranges << (2 * k);

    int device = 0;
    hipStream_t st = nullptr;
    ctx_device(ctx, &device, &st);
    (void)hipSetDevice(device);
    kgma_spectrum_stats S{};
    S.n_ranges = n_ranges; S.n_positions = P.n_positions; S.form = P.form; S.span = P.span;
    if (P.n_units == 0) {                                          // nothing but empty ranges
        memset(counts, 0, n_counts * sizeof(int64_t));
        if (n_skipped) memset(n_skipped, 0, (size_t)n_ranges * sizeof(int64_t));
    } else {
        DeviceHold hold;
        SpectrumArgs a;
        memset(&a, 0, sizeof a);
        int32_t *d_contig = nullptr;
        int64_t *d_lo = nullptr, *d_starts = nullptr, *d_cover = nullptr, *d_prefix = nullptr;
        unsigned long long *d_counts = nullptr, *d_skipped = nullptr, *d_bad = nullptr;
        SP_ALLOC(hold.alloc(d_counts, n_counts), "the counts");
        SP_ALLOC(hold.alloc(d_skipped, (size_t)n_ranges), "the skip counts");
        SP_ALLOC(hold.upload(d_contig, contig, (size_t)n_ranges, st), "the ranges");
        SP_ALLOC(hold.upload(d_lo, lo, (size_t)n_ranges, st), "the ranges");
        SP_ALLOC(hold.upload(d_starts, P.starts.data(), (size_t)n_ranges, st), "the ranges");
        SP_ALLOC(hold.upload(d_cover, P.cover.data(), (size_t)n_ranges, st), "the ranges");
        SP_ALLOC(hold.upload(d_prefix, P.prefix.data(), (size_t)n_ranges + 1, st), "the unit prefix");
        SP_ALLOC(hold.alloc(d_bad, 1), "the status word");
        for (int e = 0; e < 2; e++) KGMA_TRY(hipEventCreate(&hold.ev[e]));
        a.text = g.d_ascii; a.cd = g.d_cd; a.r_contig = d_contig; a.r_lo = d_lo; a.r_starts = d_starts; a.r_cover = d_cover;
        a.unit_prefix = d_prefix; a.n_ranges = n_ranges; a.n_units = P.n_units; a.units_per_group = P.units_per_group;
        a.k = k; a.span = P.span;
        a.skip_mask = ((flags & KGMA_COUNT_SKIP_N) ? (SP_N | SP_OTHER) : 0u) | ((flags & KGMA_COUNT_SKIP_MASKED) ? SP_MASKED : 0u);
        a.check_bad = (flags & KGMA_COUNT_SKIP_N) ? 0 : 1;
        a.counts = d_counts; a.skipped = d_skipped; a.bad = d_bad;

        KGMA_TRY(hipMemsetAsync(d_bad, 0xFF, sizeof(unsigned long long), st));
        KGMA_TRY(hipEventRecord(hold.ev[0], st));
        KGMA_TRY(hipMemsetAsync(d_counts, 0, n_counts * sizeof(unsigned long long), st));
        KGMA_TRY(hipMemsetAsync(d_skipped, 0, (size_t)n_ranges * sizeof(unsigned long long), st));
        KGMA_TRY(launch_spectrum(a, P.form, P.n_workgroups, P.lds_bytes, st));
        KGMA_TRY(hipEventRecord(hold.ev[1], st));
        unsigned long long bad = NO_BAD;
        KGMA_TRY(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, st));
        KGMA_TRY(hipStreamSynchronize(st));
        if (bad != NO_BAD)
            return failf(ctx, KGMA_E_BADBASE, "%s: record %lld position %lld: residue is not one of A/C/G/T/N (KeyError, Consts.jl:22-28)", fn,
                         (long long)(bad >> SP_POS_BITS), (long long)(bad & ((1ull << SP_POS_BITS) - 1)));
        KGMA_TRY(hipMemcpyAsync(counts, d_counts, n_counts * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        if (n_skipped) KGMA_TRY(hipMemcpyAsync(n_skipped, d_skipped, (size_t)n_ranges * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        KGMA_TRY(hipStreamSynchronize(st));
        float ms = 0;
        KGMA_TRY(hipEventElapsedTime(&ms, hold.ev[0], hold.ev[1]));
        S.count_ms = ms;
        S.n_workgroups = (int32_t)P.n_workgroups;
        S.n_launches = 1;
    }
    kgma_stats *stats = ctx_stats(ctx);
    stats->scan_ms = S.count_ms;
    stats->n_launches = S.n_launches;
    char name[48];
    snprintf(name, sizeof name, "spectrum_kernel<%s>", FORM_NAME[P.form]);
    ctx_set_kernel_name(ctx, name);
    *ctx_spectrum_stats(ctx) = S;
    return KGMA_OK;
}

int kgma_get_spectrum_stats(kgma_ctx *ctx, kgma_spectrum_stats *out)
{
    if (!ctx || !out) return KGMA_E_ARG;
    *out = *ctx_spectrum_stats(ctx);
    return KGMA_OK;
}

}  // extern "C"
