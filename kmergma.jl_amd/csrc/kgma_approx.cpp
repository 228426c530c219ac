// kgma_approx.cpp -- host side of the edit-distance search (kgma_approx_match, kgma_get_approx_matches, kgma_get_approx_stats;
// kernels: kgma_approx.hip).
//
// One call: check the arguments and build each query's Peq tables (for the search kernel, the query at the top of the vector; for
// the start kernel, the reversed query), upload them and the per-record prefix of workgroup counts, run the search kernel -- once
// more with a buffer of the size it counted when the ends outgrow the buffer -- bring the ends down, sort them by (query, contig,
// end), keep the best end of every run when asked to, send the kept ends back, run the start kernel over them and bring them down
// again.  The hit buffer belongs to the context and is kept between calls; everything else is freed before the call returns.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kgma_approx.h"

using namespace kgma;

static_assert(sizeof(kgma_approx_hit) == sizeof(ApproxHit), "kgma_approx_hit is the device record");

namespace {

constexpr int64_t FIRST_CAP = (int64_t)1 << 16;

int failf(kgma_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return ctx_fail(ctx, code, buf);
}

#define A_TRY(expr)                                                                                          \
    do {                                                                                                     \
        const hipError_t e__ = (expr);                                                                       \
        if (e__ != hipSuccess) return failf(ctx, KGMA_E_HIP, "%s: %s failed: %s", fn, #expr, hipGetErrorString(e__)); \
    } while (0)

// base set of an IUPAC symbol (bit 0 A, 1 C, 2 G, 3 T), either case; 0: not one of the 15 symbols
uint32_t iupac_set(uint8_t ch)
{
    switch (ch & 0xDFu) {
    case 'A': return 1;  case 'C': return 2;  case 'G': return 4;  case 'T': return 8;
    case 'R': return 5;  case 'Y': return 10; case 'S': return 6;  case 'W': return 9;
    case 'K': return 12; case 'M': return 3;  case 'B': return 14; case 'D': return 13;
    case 'H': return 11; case 'V': return 7;  case 'N': return 15;
    default: return 0;
    }
}

// residue class (kgma_approx.h) of the bases A C G T, and of N
constexpr int BASE_CLASS[4] = {('A' >> 1) & 7, ('C' >> 1) & 7, ('G' >> 1) & 7, ('T' >> 1) & 7};
constexpr int N_CLASS = ('N' >> 1) & 7;
static_assert(BASE_CLASS[0] == 0 && BASE_CLASS[1] == 1 && BASE_CLASS[2] == 3 && BASE_CLASS[3] == 2 && N_CLASS == 7 &&
                  ((AP_NO_RESIDUE >> 1) & 7) == 4,
              "six different classes");

// Query i of the call: the checks of include/kgma.h and the two Peq tables
int make_query(kgma_ctx *ctx, const char *fn, int32_t i, const uint8_t *sym, int64_t m, int32_t e, ApproxQuery &Q)
{
    if (m < 1 || m > AP_MAX_LEN) return failf(ctx, KGMA_E_ARG, "%s: query %d has %lld symbols (1 ... %d)", fn, i, (long long)m, AP_MAX_LEN);
    if (e < 0 || e > AP_MAX_EDITS) return failf(ctx, KGMA_E_ARG, "%s: query %d: max_edits %d (0 ... %d)", fn, i, e, AP_MAX_EDITS);
    memset(&Q, 0, sizeof Q);
    Q.len = (int32_t)m; Q.max_edits = e; Q.id = i;
    int informative = 0;
    for (int64_t j = 0; j < m; j++) {
        const uint32_t set = iupac_set(sym[j]);
        if (!set) return failf(ctx, KGMA_E_ARG, "%s: query %d, symbol %lld (0x%02x) is not an IUPAC nucleotide code", fn, i, (long long)j + 1, sym[j]);
        if (set != 15u) informative++;
        const uint64_t top = 1ull << (64 - m + j), rev = 1ull << (m - 1 - j);
        for (int b = 0; b < 4; b++)
            if ((set >> b) & 1u) { Q.peq[BASE_CLASS[b]] |= top; Q.rev[BASE_CLASS[b]] |= rev; }
        if (set == 15u) { Q.peq[N_CLASS] |= top; Q.rev[N_CLASS] |= rev; }      // a genome N matches only a query N
    }
    if (e >= informative)
        return failf(ctx, KGMA_E_ARG, "%s: query %d: max_edits %d is not smaller than its %d informative (non-N) symbols: every position would match",
                     fn, i, e, informative);
    return KGMA_OK;
}

// the best end of every run of consecutive ends of one (query, contig): the smallest edits, on a tie the smallest end
void keep_run_minima(std::vector<kgma_approx_hit> &v)
{
    size_t out = 0;
    for (size_t i = 0; i < v.size();) {
        size_t best = i, j = i + 1;
        for (; j < v.size() && v[j].query == v[i].query && v[j].contig == v[i].contig && v[j].end == v[j - 1].end + 1; j++)
            if (v[j].edits < v[best].edits) best = j;
        v[out++] = v[best];
        i = j;
    }
    v.resize(out);
}

}  // namespace

extern "C" {

int kgma_approx_match(kgma_ctx *ctx, const kgma_genome *genome, const uint8_t *queries, const int64_t *offsets, int32_t n_queries,
                      const int32_t *max_edits, int32_t best_only)
{
    const char *fn = "kgma_approx_match";
    if (!ctx || !genome) return KGMA_E_ARG;
    ApproxState *S = ctx_approx(ctx);
    S->hits.clear();                                  // (whatever happens below: a failed call leaves no hits of an earlier one behind)
    S->stats = kgma_approx_stats{};
    if (n_queries < 0 || (n_queries > 0 && (!queries || !offsets || !max_edits))) return failf(ctx, KGMA_E_ARG, "%s: no queries", fn);
    std::vector<ApproxQuery> Q((size_t)n_queries);
    int words = 1;
    for (int32_t i = 0; i < n_queries; i++) {
        const int64_t m = offsets[i + 1] - offsets[i];
        const int rc = make_query(ctx, fn, i, queries + offsets[i], m, max_edits[i], Q[(size_t)i]);
        if (rc) return rc;
        if (m > 32) words = 2;
    }
    if (const char *w = getenv("KGMA_APPROX_WORDS")) if (atoi(w) == 2) words = 2;   // measurements: the two-word form for every query
    int rc = genome_searchable(ctx, genome);
    if (rc) return rc;
    const GenomeText g = genome_text(genome);
    std::vector<int64_t> prefix((size_t)g.n_contigs + 1, 0);
    for (int64_t c = 0; c < g.n_contigs; c++) prefix[(size_t)c + 1] = prefix[(size_t)c] + (g.cd[c].len + AP_WG_BASES - 1) / AP_WG_BASES;
    const int64_t n_wg = prefix[(size_t)g.n_contigs];
    if (n_wg > 0x7FFFFFFFll) return failf(ctx, KGMA_E_UNSUPPORTED, "%s: %lld workgroups exceed one launch", fn, (long long)n_wg);
    kgma_approx_stats T{};
    T.tile = AP_TILE; T.wg_bases = AP_WG_BASES; T.words = words;
    if (n_queries == 0 || n_wg == 0) { S->stats = T; return KGMA_OK; }

    int device = 0;
    hipStream_t st = nullptr;
    ctx_device(ctx, &device, &st);
    (void)hipSetDevice(device);
    DeviceHold hold;
    if (!S->d_out) {
        if (hipMalloc(reinterpret_cast<void **>(&S->d_out), (size_t)FIRST_CAP * sizeof(ApproxHit)) != hipSuccess) {
            (void)hipGetLastError();
            S->d_out = nullptr;
            return failf(ctx, KGMA_E_NOMEM, "%s: no device memory for the hit buffer", fn);
        }
        S->out_cap = FIRST_CAP;
        *ctx_device_bytes(ctx) += FIRST_CAP * (int64_t)sizeof(ApproxHit);
    }
    ApproxArgs a;
    memset(&a, 0, sizeof a);
    ApproxQuery *d_q = nullptr;
    int64_t *d_prefix = nullptr;
    A_TRY(hold.upload(d_q, Q.data(), Q.size(), st));
    A_TRY(hold.upload(d_prefix, prefix.data(), prefix.size(), st));
    A_TRY(hold.alloc(a.ctl, 2));
    for (int e = 0; e < 4; e++) A_TRY(hipEventCreate(&hold.ev[e]));
    a.ascii = g.d_ascii; a.cd = g.d_cd; a.wg_prefix = d_prefix; a.n_contigs = (int32_t)g.n_contigs; a.n_queries = n_queries;
    a.queries = d_q;

    // one launch for the whole batch; ends that do not fit the device buffer: once more with a buffer of the size it counted
    unsigned long long ctl[2] = {0, 0};
    A_TRY(hipEventRecord(hold.ev[0], st));
    for (int attempt = 0;; attempt++) {
        a.out = S->d_out; a.cap = (unsigned long long)S->out_cap;
        A_TRY(hipMemsetAsync(a.ctl, 0, 2 * sizeof(unsigned long long), st));
        A_TRY(launch_approx(a, words, n_wg, st));
        T.n_launches++;
        A_TRY(hipMemcpyAsync(ctl, a.ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
        A_TRY(hipStreamSynchronize(st));
        if (ctl[0] <= (unsigned long long)S->out_cap) break;
        if (attempt == 1) return failf(ctx, KGMA_E_OVERFLOW, "%s: %llu hits overflowed the regrown buffer", fn, ctl[0]);
        // the larger buffer is taken before the old one is given up: without room for it the context stays as it was
        ApproxHit *fresh = nullptr;
        if (ctl[0] > (1ull << 40) || hipMalloc(reinterpret_cast<void **>(&fresh), (size_t)ctl[0] * sizeof(ApproxHit)) != hipSuccess) {
            (void)hipGetLastError();
            return failf(ctx, KGMA_E_NOMEM, "%s: no device memory for %llu hits", fn, ctl[0]);
        }
        (void)hipFree(S->d_out);
        *ctx_device_bytes(ctx) += ((int64_t)ctl[0] - S->out_cap) * (int64_t)sizeof(ApproxHit);
        S->d_out = fresh; S->out_cap = (int64_t)ctl[0];
    }
    A_TRY(hipEventRecord(hold.ev[1], st));
    std::vector<kgma_approx_hit> found((size_t)ctl[0]);
    if (ctl[0]) A_TRY(hipMemcpyAsync(found.data(), S->d_out, found.size() * sizeof(kgma_approx_hit), hipMemcpyDeviceToHost, st));
    A_TRY(hipStreamSynchronize(st));
    std::sort(found.begin(), found.end(), [](const kgma_approx_hit &x, const kgma_approx_hit &y) {
        return x.query != y.query ? x.query < y.query : x.contig != y.contig ? x.contig < y.contig : x.end < y.end;
    });
    T.n_ends = (int64_t)found.size();
    if (best_only) keep_run_minima(found);
    T.n_hits = (int64_t)found.size();

    // the start of every reported end
    float ms = 0;
    if (!found.empty()) {
        a.n_hits = (int64_t)found.size();
        A_TRY(hipMemcpyAsync(S->d_out, found.data(), found.size() * sizeof(kgma_approx_hit), hipMemcpyHostToDevice, st));
        A_TRY(hipEventRecord(hold.ev[2], st));
        A_TRY(launch_approx_starts(a, st));
        T.n_launches++;
        A_TRY(hipEventRecord(hold.ev[3], st));
        A_TRY(hipMemcpyAsync(found.data(), S->d_out, found.size() * sizeof(kgma_approx_hit), hipMemcpyDeviceToHost, st));
        A_TRY(hipStreamSynchronize(st));
        A_TRY(hipEventElapsedTime(&ms, hold.ev[2], hold.ev[3]));
        T.starts_ms = ms;
        for (const kgma_approx_hit &h : found)
            if (h.start < 1 || h.start > h.end)
                return failf(ctx, KGMA_E_STATE, "%s: query %d, record %d, end %lld: no start attains %d edits", fn, h.query, h.contig,
                             (long long)h.end, h.edits);
    }
    A_TRY(hipEventElapsedTime(&ms, hold.ev[0], hold.ev[1]));
    T.search_ms = ms;
    kgma_stats *stats = ctx_stats(ctx);
    stats->scan_ms = T.search_ms + T.starts_ms;
    stats->n_launches = T.n_launches;
    S->stats = T;
    S->hits.swap(found);
    return KGMA_OK;
}

int kgma_get_approx_matches(kgma_ctx *ctx, kgma_approx_hit *out, int64_t cap, int64_t *n)
{
    if (!ctx || !n) return KGMA_E_ARG;
    const std::vector<kgma_approx_hit> &hits = ctx_approx(ctx)->hits;
    *n = (int64_t)hits.size();
    if (!out) return KGMA_OK;
    if (cap < *n) return failf(ctx, KGMA_E_ARG, "kgma_get_approx_matches: capacity %lld < %lld", (long long)cap, (long long)*n);
    if (*n) memcpy(out, hits.data(), (size_t)*n * sizeof(kgma_approx_hit));
    return KGMA_OK;
}

int kgma_get_approx_stats(kgma_ctx *ctx, kgma_approx_stats *out)
{
    if (!ctx || !out) return KGMA_E_ARG;
    *out = ctx_approx(ctx)->stats;
    return KGMA_OK;
}

}  // extern "C"
