// kgma_exact.cpp -- host side of the exact sequence search (kgma_exact_match, kgma_get_matches; exactMatch,
// src/ExactMatch.jl:89-121; kernels: kgma_exact.hip).
//
// One call: check and fold the queries and encode each for both kernels, make the genome's 2-bit copy and residue check current,
// send the queries that are A/C/G/T only through the 2-bit kernel (when no record holds a residue outside A/C/G/T/N) and the others
// through the residue-text kernel, which also reports a residue outside the 16-symbol alphabet; each launch follows the protocol of
// kgma_search.h and appends to one list, which is sorted by (query, contig, start) and, on request, thinned to FindAll's matches.
// Every device buffer belongs to the context and is kept between calls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kgma_exact.h"

using namespace kgma;

static_assert(sizeof(kgma_match) == sizeof(ExactMatch), "kgma_match is the device record");

namespace {

constexpr unsigned long long NO_BAD = ~0ull;

// the 16 symbols of DNAAlphabet{4}, either case
bool exact_symbol(uint8_t ch)
{
    static const char sym[] = "ACGTMRWSYKVHDBN";
    if (ch == '-') return true;
    const uint8_t u = (uint8_t)(ch & 0xDFu);
    return u >= 'A' && u <= 'Z' && strchr(sym, (int)u) != nullptr;
}

// One launch over the whole genome for the queries `qs` (kind: kgma_exact.hip, launch_exact); appends the matches to `found`.
// *bad_out: the residue outside the alphabet that a checking launch met (the caller reports it; the matches are not wanted)
int exact_launch(kgma_ctx *ctx, const char *fn, const GenomeText &g, hipStream_t st, int kind, const std::vector<ExactQuery> &qs,
                 std::vector<kgma_match> &found, unsigned long long *bad_out, int *n_launches)
{
    ExactState *S = ctx_exact(ctx);
    const int64_t nc = g.n_contigs;
    const std::vector<int64_t> prefix = tile_prefix(nc, exact_tile_starts(kind == 2), false, [&](int64_t c) { return g.cd[c].len; });
    const int64_t n_tiles = prefix[(size_t)nc];
    int rc;
    if ((rc = one_launch(ctx, fn, n_tiles, "tiles"))) return rc;
    if ((rc = S->q.reserve(ctx, (int64_t)qs.size()))) return rc;
    if ((rc = S->prefix.reserve(ctx, nc + 1))) return rc;
    if ((rc = S->ctl.reserve(ctx, 2))) return rc;
    if ((rc = S->out.reserve(ctx, fn))) return rc;
    KGMA_TRY(hipMemcpyAsync(S->q.d, qs.data(), qs.size() * sizeof(ExactQuery), hipMemcpyHostToDevice, st));
    KGMA_TRY(hipMemcpyAsync(S->prefix.d, prefix.data(), prefix.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    ExactArgs a{};
    a.ascii = g.d_ascii; a.inter = g.d_inter; a.cd = g.d_cd; a.tile_prefix = S->prefix.d;
    a.n_contigs = (int32_t)nc; a.n_queries = (int32_t)qs.size();
    a.queries = S->q.d; a.qtext = S->text.d;
    unsigned long long ctl[2] = {0ull, NO_BAD};
    rc = S->out.fill(ctx, fn, "matches", st, S->ctl.d, ctl, [&](ExactMatch *out, unsigned long long cap, unsigned long long *d_ctl) {
        a.out = out; a.cap = cap; a.ctl = d_ctl;
        return launch_exact(a, kind, n_tiles, st);
    }, n_launches);
    if (rc) return rc;
    if (ctl[1] != NO_BAD) { *bad_out = ctl[1]; return KGMA_OK; }
    return S->out.fetch(ctx, fn, ctl[0], found);
}

}  // namespace

extern "C" {

int kgma_exact_match(kgma_ctx *ctx, const kgma_genome *gc, const uint8_t *queries, const int64_t *offsets, int32_t n_queries, int32_t overlap)
{
    const char *fn = "kgma_exact_match";
    if (!ctx || !gc) return KGMA_E_ARG;
    if (n_queries < 0 || (n_queries > 0 && (!queries || !offsets))) return failf(ctx, KGMA_E_ARG, "kgma_exact_match: no queries");
    std::vector<uint8_t> text;
    std::vector<ExactQuery> q_ascii, q_2bit;
    std::vector<int64_t> qlen((size_t)n_queries);
    for (int32_t i = 0; i < n_queries; i++) {
        const int64_t b = offsets[i], m = offsets[i + 1] - b;
        if (m < 1) return failf(ctx, KGMA_E_ARG, "kgma_exact_match: query %d is empty", i);
        qlen[(size_t)i] = m;
        ExactQuery Q{};
        Q.text_off = (int64_t)text.size(); Q.len = m; Q.id = i;
        bool acgt = true;
        for (int64_t j = 0; j < m; j++) {
            const uint8_t ch = queries[b + j];
            if (!exact_symbol(ch)) return failf(ctx, KGMA_E_ARG, "kgma_exact_match: query %d, symbol %lld (0x%02x) is outside the DNA alphabet", i, (long long)j + 1, ch);
            const uint8_t u = (uint8_t)(ch & 0xDFu);
            acgt = acgt && (u == 'A' || u == 'C' || u == 'G' || u == 'T');
            text.push_back(u);
        }
        ExactQuery P = Q;      // the same query for the 2-bit kernel
        for (int64_t j = 0; j < std::min<int64_t>(m, 8); j++) {
            Q.pat[j >> 2] |= (uint32_t)text[(size_t)(Q.text_off + j)] << (8 * (j & 3));
            Q.mask[j >> 2] |= 0xFFu << (8 * (j & 3));
        }
        if (acgt)
            for (int64_t j = 0; j < std::min<int64_t>(m, 16); j++) {
                const uint8_t u = text[(size_t)(Q.text_off + j)];
                P.pat[0] |= (u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : 3u) << (2 * j);
                P.mask[0] |= 3u << (2 * j);
            }
        q_ascii.push_back(Q);
        if (acgt) q_2bit.push_back(P);
        else { P.len = 0; q_2bit.push_back(P); }       // len 0: not a 2-bit query
    }
    bool clean = true;                       // no residue outside A/C/G/T/N anywhere: nothing to check, and the 2-bit copy is faithful up to N
    int rc = genome_searchable(ctx, gc, PackedCopy::Inter, &clean);
    if (rc) return rc;
    const GenomeText g = genome_text(gc);
    const char *sw = getenv("KGMA_EXACT_ASCII");     // testing only: every query through the residue-text kernel
    const bool allow_2bit = clean && !(sw && atoi(sw) != 0);
    std::vector<ExactQuery> la, lb;
    for (int32_t i = 0; i < n_queries; i++) {
        if (allow_2bit && q_2bit[(size_t)i].len > 0) lb.push_back(q_2bit[(size_t)i]);
        else la.push_back(q_ascii[(size_t)i]);
    }
    ExactState *S = ctx_exact(ctx);
    int device = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    ctx_device(ctx, &device, &st);
    ctx_events(ctx, &ev0, &ev1);
    if ((rc = S->text.reserve(ctx, (int64_t)text.size() + 8))) return rc;
    if (!text.empty()) KGMA_TRY(hipMemcpyAsync(S->text.d, text.data(), text.size(), hipMemcpyHostToDevice, st));
    std::vector<kgma_match> found;
    unsigned long long bad = NO_BAD;
    int n_launches = 0;
    KGMA_TRY(hipEventRecord(ev0, st));
    if (!la.empty() && (rc = exact_launch(ctx, fn, g, st, clean ? 0 : 1, la, found, &bad, &n_launches))) return rc;
    if (bad == NO_BAD && !lb.empty() && (rc = exact_launch(ctx, fn, g, st, 2, lb, found, &bad, &n_launches))) return rc;
    KGMA_TRY(hipEventRecord(ev1, st));
    KGMA_TRY(hipEventSynchronize(ev1));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ev0, ev1);
    kgma_stats *stats = ctx_stats(ctx);
    stats->scan_ms = ms;
    stats->n_launches = n_launches;
    if (bad != NO_BAD) {
        S->matches.clear();
        return failf(ctx, KGMA_E_BADBASE, "record %lld: residue %lld is outside the DNA alphabet", (long long)(bad >> 40),
                     (long long)(bad & ((1ull << 40) - 1)) + 1);
    }
    std::sort(found.begin(), found.end(), [](const kgma_match &x, const kgma_match &y) {
        return x.query != y.query ? x.query < y.query : x.contig != y.contig ? x.contig < y.contig : x.start < y.start;
    });
    if (!overlap) {
        // FindAll (src/ExactMatch.jl:20-30): the leftmost match, then the leftmost one that starts behind its end
        size_t w = 0;
        int64_t last_end = 0;
        for (size_t i = 0; i < found.size(); i++) {
            const kgma_match &mt = found[i];
            const bool fresh = w == 0 || found[w - 1].query != mt.query || found[w - 1].contig != mt.contig;
            if (!fresh && mt.start <= last_end) continue;
            last_end = mt.start + qlen[(size_t)mt.query] - 1;
            found[w++] = mt;
        }
        found.resize(w);
    }
    S->matches.swap(found);
    return KGMA_OK;
}

int kgma_get_matches(kgma_ctx *ctx, kgma_match *out, int64_t cap, int64_t *n)
{
    return ctx ? copy_out(ctx, "kgma_get_matches", ctx_exact(ctx)->matches, out, cap, n) : KGMA_E_ARG;
}

}  // extern "C"
