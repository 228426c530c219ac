// kgma_pwm.cpp -- host side of the position-weight-matrix search (kgma_pwm_match, kgma_get_pwm_matches, kgma_get_pwm_stats;
// kernel: kgma_pwm.hip).
//
// One call: check the arguments, fold each matrix (the rows of four equal weights become a constant that moves into the threshold,
// every other row and the row behind it one table of 64 sums indexed by two residue classes; a matrix whose threshold lies above
// the sum of its row maxima is not sent at all), upload the matrices, their tables and the per-record prefix of workgroup counts,
// run the kernel by the protocol of kgma_search.h and sort the hits by (matrix, contig, start).  The hit buffer belongs to the
// context and is kept between calls; everything else is freed before the call returns.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "kgma_pwm.h"

using namespace kgma;

static_assert(sizeof(kgma_pwm_hit) == sizeof(PwmHit), "kgma_pwm_hit is the device record");

namespace {

// weight of a row (A, C, G, T) for a residue class of the text (kgma_approx.h: A 0, C 1, T 2, G 3, N 7): a genome N scores the
// row's minimum; the classes no residue of a checked genome has, and the one the kernel puts where there is no residue, score 0
// (no valid start reads them)
int32_t class_weight(const int16_t *row, int cls)
{
    switch (cls) {
    case 0: return row[0];
    case 1: return row[1];
    case 2: return row[3];
    case 3: return row[2];
    case 7: return std::min(std::min(row[0], row[1]), std::min(row[2], row[3]));
    default: return 0;
    }
}

bool constant_row(const int16_t *row) { return row[0] == row[1] && row[1] == row[2] && row[2] == row[3]; }

}  // namespace

extern "C" {

int kgma_pwm_match(kgma_ctx *ctx, const kgma_genome *genome, const int16_t *weights, const int64_t *row_offsets, int32_t n_matrices,
                   const int32_t *threshold)
{
    const char *fn = "kgma_pwm_match";
    if (!ctx || !genome) return KGMA_E_ARG;
    PwmState *S = ctx_pwm(ctx);
    S->hits.clear();                                  // (whatever happens below: a failed call leaves no hits of an earlier one behind)
    S->stats = kgma_pwm_stats{};
    if (n_matrices < 0 || (n_matrices > 0 && (!weights || !row_offsets || !threshold))) return failf(ctx, KGMA_E_ARG, "%s: no matrices", fn);
    std::vector<PwmMatrix> Q;
    std::vector<int32_t> tables;
    int64_t m_min = PW_MAX_ROWS;
    for (int32_t i = 0; i < n_matrices; i++) {
        const int64_t m = row_offsets[i + 1] - row_offsets[i];
        if (m < 1 || m > PW_MAX_ROWS) return failf(ctx, KGMA_E_ARG, "%s: matrix %d has %lld rows (1 ... %d)", fn, i, (long long)m, PW_MAX_ROWS);
        const int16_t *W = weights + 4 * row_offsets[i];
        int64_t lo = 0, hi = 0, konst = 0;
        for (int64_t r = 0; r < m; r++) {
            lo += *std::min_element(W + 4 * r, W + 4 * r + 4);
            hi += *std::max_element(W + 4 * r, W + 4 * r + 4);
            if (constant_row(W + 4 * r)) konst += W[4 * r];
        }
        if ((int64_t)threshold[i] <= lo)
            return failf(ctx, KGMA_E_ARG, "%s: matrix %d: threshold %d does not exceed the sum of its row minima, %lld: every start would match",
                         fn, i, threshold[i], (long long)lo);
        if ((int64_t)threshold[i] > hi) continue;     // legal, and no start reaches it
        PwmMatrix M;
        memset(&M, 0, sizeof M);
        M.rows = (int32_t)m; M.id = i; M.konst = (int32_t)konst; M.thr = (int32_t)((int64_t)threshold[i] - konst);
        M.tab_off = (int32_t)tables.size();
        static const int16_t ZERO[4] = {0, 0, 0, 0};
        for (int64_t r = 0; r < m;) {
            if (constant_row(W + 4 * r)) { r++; continue; }
            // (lo < hi here, so some row is not constant: n_pairs >= 1)
            const int16_t *first = W + 4 * r, *second = r + 1 < m && !constant_row(W + 4 * (r + 1)) ? W + 4 * (r + 1) : ZERO;
            M.col[M.n_pairs++] = (uint8_t)r;
            for (int e = 0; e < PW_PAIR_ENTRIES; e++) tables.push_back(class_weight(first, e & 7) + class_weight(second, e >> 3));
            r += 2;
        }
        m_min = std::min(m_min, m);
        Q.push_back(M);
    }
    int rc = genome_searchable(ctx, genome);
    if (rc) return rc;
    const GenomeText g = genome_text(genome);
    // workgroups of a record: over the starts its shortest matrix has there
    const std::vector<int64_t> prefix = tile_prefix(g.n_contigs, PW_WG_STARTS, false, [&](int64_t c) { return g.cd[c].len; }, m_min);
    const int64_t n_wg = prefix[(size_t)g.n_contigs];
    if ((rc = one_launch(ctx, fn, n_wg, "workgroups"))) return rc;
    kgma_pwm_stats T{};
    T.lane_starts = PW_LANE_STARTS; T.wave_starts = PW_WAVE_STARTS; T.wg_starts = PW_WG_STARTS;
    if (Q.empty() || n_wg == 0) { S->stats = T; return KGMA_OK; }

    int device = 0;
    hipStream_t st = nullptr;
    ctx_device(ctx, &device, &st);
    (void)hipSetDevice(device);
    DeviceHold hold;
    if ((rc = S->out.reserve(ctx, fn))) return rc;
    PwmArgs a;
    memset(&a, 0, sizeof a);
    PwmMatrix *d_q = nullptr;
    int32_t *d_tab = nullptr;
    int64_t *d_prefix = nullptr;
    KGMA_TRY(hold.upload(d_q, Q.data(), Q.size(), st));
    KGMA_TRY(hold.upload(d_tab, tables.data(), tables.size(), st));
    KGMA_TRY(hold.upload(d_prefix, prefix.data(), prefix.size(), st));
    KGMA_TRY(hold.alloc(a.ctl, 2));
    for (int e = 0; e < 2; e++) KGMA_TRY(hipEventCreate(&hold.ev[e]));
    a.ascii = g.d_ascii; a.cd = g.d_cd; a.wg_prefix = d_prefix; a.n_contigs = (int32_t)g.n_contigs; a.n_matrices = (int32_t)Q.size();
    a.matrices = d_q; a.tables = d_tab;

    unsigned long long ctl[2] = {0, 0};
    KGMA_TRY(hipEventRecord(hold.ev[0], st));
    rc = S->out.fill(ctx, fn, "hits", st, a.ctl, ctl, [&](PwmHit *out, unsigned long long cap, unsigned long long *) {
        a.out = out; a.cap = cap;
        return launch_pwm(a, n_wg, st);
    }, &T.n_launches);
    if (rc) return rc;
    KGMA_TRY(hipEventRecord(hold.ev[1], st));
    std::vector<kgma_pwm_hit> found;
    if ((rc = S->out.fetch(ctx, fn, ctl[0], found))) return rc;
    KGMA_TRY(hipStreamSynchronize(st));            // (the second event has been reached)
    std::sort(found.begin(), found.end(), [](const kgma_pwm_hit &x, const kgma_pwm_hit &y) {
        return x.matrix != y.matrix ? x.matrix < y.matrix : x.contig != y.contig ? x.contig < y.contig : x.start < y.start;
    });
    T.n_candidates = T.n_hits = (int64_t)found.size();
    float ms = 0;
    KGMA_TRY(hipEventElapsedTime(&ms, hold.ev[0], hold.ev[1]));
    T.search_ms = ms;
    kgma_stats *stats = ctx_stats(ctx);
    stats->scan_ms = T.search_ms;
    stats->n_launches = T.n_launches;
    S->stats = T;
    S->hits.swap(found);
    return KGMA_OK;
}

int kgma_get_pwm_matches(kgma_ctx *ctx, kgma_pwm_hit *out, int64_t cap, int64_t *n)
{
    return ctx ? copy_out(ctx, "kgma_get_pwm_matches", ctx_pwm(ctx)->hits, out, cap, n) : KGMA_E_ARG;
}

int kgma_get_pwm_stats(kgma_ctx *ctx, kgma_pwm_stats *out)
{
    if (!ctx || !out) return KGMA_E_ARG;
    *out = ctx_pwm(ctx)->stats;
    return KGMA_OK;
}

}  // extern "C"
