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
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kgma_approx.h"

using namespace kgma;

static_assert(sizeof(kgma_approx_hit) == sizeof(ApproxHit), "kgma_approx_hit is the device record");

namespace {

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
    const std::vector<int64_t> prefix = tile_prefix(g.n_contigs, AP_WG_BASES, false, [&](int64_t c) { return g.cd[c].len; });
    const int64_t n_wg = prefix[(size_t)g.n_contigs];
    if ((rc = one_launch(ctx, fn, n_wg, "workgroups"))) return rc;
    kgma_approx_stats T{};
    T.tile = AP_TILE; T.wg_bases = AP_WG_BASES; T.words = words;
    if (n_queries == 0 || n_wg == 0) { S->stats = T; return KGMA_OK; }

    int device = 0;
    hipStream_t st = nullptr;
    ctx_device(ctx, &device, &st);
    (void)hipSetDevice(device);
    DeviceHold hold;
    if ((rc = S->out.reserve(ctx, fn))) return rc;
    ApproxArgs a;
    memset(&a, 0, sizeof a);
    ApproxQuery *d_q = nullptr;
    int64_t *d_prefix = nullptr;
    KGMA_TRY(hold.upload(d_q, Q.data(), Q.size(), st));
    KGMA_TRY(hold.upload(d_prefix, prefix.data(), prefix.size(), st));
    KGMA_TRY(hold.alloc(a.ctl, 2));
    for (int e = 0; e < 4; e++) KGMA_TRY(hipEventCreate(&hold.ev[e]));
    a.ascii = g.d_ascii; a.cd = g.d_cd; a.wg_prefix = d_prefix; a.n_contigs = (int32_t)g.n_contigs; a.n_queries = n_queries;
    a.queries = d_q;

    unsigned long long ctl[2] = {0, 0};
    KGMA_TRY(hipEventRecord(hold.ev[0], st));
    rc = S->out.fill(ctx, fn, "hits", st, a.ctl, ctl, [&](ApproxHit *out, unsigned long long cap, unsigned long long *) {
        a.out = out; a.cap = cap;
        return launch_approx(a, words, n_wg, st);
    }, &T.n_launches);
    if (rc) return rc;
    KGMA_TRY(hipEventRecord(hold.ev[1], st));
    std::vector<kgma_approx_hit> found;
    if ((rc = S->out.fetch(ctx, fn, ctl[0], found))) return rc;
    KGMA_TRY(hipStreamSynchronize(st));            // (the second event has been reached)
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
        KGMA_TRY(hipMemcpyAsync(S->out.d, found.data(), found.size() * sizeof(kgma_approx_hit), hipMemcpyHostToDevice, st));
        KGMA_TRY(hipEventRecord(hold.ev[2], st));
        KGMA_TRY(launch_approx_starts(a, st));
        T.n_launches++;
        KGMA_TRY(hipEventRecord(hold.ev[3], st));
        KGMA_TRY(hipMemcpyAsync(found.data(), S->out.d, found.size() * sizeof(kgma_approx_hit), hipMemcpyDeviceToHost, st));
        KGMA_TRY(hipStreamSynchronize(st));
        KGMA_TRY(hipEventElapsedTime(&ms, hold.ev[2], hold.ev[3]));
        T.starts_ms = ms;
        for (const kgma_approx_hit &h : found)
            if (h.start < 1 || h.start > h.end)
                return failf(ctx, KGMA_E_STATE, "%s: query %d, record %d, end %lld: no start attains %d edits", fn, h.query, h.contig,
                             (long long)h.end, h.edits);
    }
    KGMA_TRY(hipEventElapsedTime(&ms, hold.ev[0], hold.ev[1]));
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
    return ctx ? copy_out(ctx, "kgma_get_approx_matches", ctx_approx(ctx)->hits, out, cap, n) : KGMA_E_ARG;
}

int kgma_get_approx_stats(kgma_ctx *ctx, kgma_approx_stats *out)
{
    if (!ctx || !out) return KGMA_E_ARG;
    *out = ctx_approx(ctx)->stats;
    return KGMA_OK;
}

}  // extern "C"
