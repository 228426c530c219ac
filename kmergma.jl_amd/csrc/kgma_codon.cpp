// kgma_codon.cpp -- host side of the codon-weight-matrix search (kgma_codon_match, kgma_get_codon_matches, kgma_get_codon_stats,
// kgma_codon_fold; kernel: kgma_codon.hip).
//
// One call: check the arguments, take the constant rows of each matrix out (a row of 65 equal weights becomes a constant that
// moves into the threshold; a matrix whose threshold lies above the sum of its row maxima is not sent at all), upload the
// matrices, the tables of their other rows and the per-record prefix of workgroup counts, run the kernel by the protocol of
// kgma_search.h and sort the hits by (matrix, contig, start).  The hit buffer belongs to the context and is kept between calls;
// everything else is freed before the call returns.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "kgma_codon.h"

using namespace kgma;

static_assert(sizeof(kgma_codon_hit) == sizeof(CodonHit), "kgma_codon_hit is the device record");
static_assert(KGMA_CODON_ENTRIES == CD_ENTRIES && KGMA_CODON_MAX_ROWS == CD_MAX_ROWS, "the header's numbers are the kernel's");

namespace {

bool constant_row(const int16_t *row) { return std::all_of(row + 1, row + CD_ENTRIES, [&](int16_t w) { return w == row[0]; }); }

}  // namespace

extern "C" {

int kgma_codon_match(kgma_ctx *ctx, const kgma_genome *genome, const int16_t *weights, const int64_t *row_offsets, int32_t n_matrices,
                     const int32_t *threshold)
{
    const char *fn = "kgma_codon_match";
    if (!ctx || !genome) return KGMA_E_ARG;
    CodonState *S = ctx_codon(ctx);
    S->hits.clear();                                  // (whatever happens below: a failed call leaves no hits of an earlier one behind)
    S->stats = kgma_codon_stats{};
    if (n_matrices < 0 || (n_matrices > 0 && (!weights || !row_offsets || !threshold))) return failf(ctx, KGMA_E_ARG, "%s: no matrices", fn);
    std::vector<CodonMatrix> Q;
    std::vector<int16_t> tables;
    int64_t m_min = CD_MAX_ROWS;
    for (int32_t i = 0; i < n_matrices; i++) {
        const int64_t m = row_offsets[i + 1] - row_offsets[i];
        if (m < 1 || m > CD_MAX_ROWS) return failf(ctx, KGMA_E_ARG, "%s: matrix %d has %lld rows (1 ... %d)", fn, i, (long long)m, CD_MAX_ROWS);
        const int16_t *W = weights + CD_ENTRIES * row_offsets[i];
        int64_t lo = 0, hi = 0, konst = 0;
        for (int64_t r = 0; r < m; r++) {
            const int16_t *row = W + CD_ENTRIES * r;
            lo += *std::min_element(row, row + CD_ENTRIES);
            hi += *std::max_element(row, row + CD_ENTRIES);
            if (constant_row(row)) konst += row[0];
        }
        if ((int64_t)threshold[i] <= lo)
            return failf(ctx, KGMA_E_ARG, "%s: matrix %d: threshold %d does not exceed the sum of its row minima, %lld: every start would match",
                         fn, i, threshold[i], (long long)lo);
        if ((int64_t)threshold[i] > hi) continue;     // legal, and no start reaches it
        CodonMatrix M;
        memset(&M, 0, sizeof M);
        M.rows = (int32_t)m; M.id = i; M.konst = (int32_t)konst; M.thr = (int32_t)((int64_t)threshold[i] - konst);
        M.tab_off = (int32_t)tables.size();
        for (int64_t r = 0; r < m; r++) {
            const int16_t *row = W + CD_ENTRIES * r;
            if (constant_row(row)) continue;
            // (lo < hi here, so some row is not constant: n_rows >= 1)
            M.col[M.n_rows++] = (uint8_t)r;
            tables.insert(tables.end(), row, row + CD_ENTRIES);
            tables.resize(tables.size() + (CD_TAB_STRIDE - CD_ENTRIES), 0);
        }
        m_min = std::min(m_min, m);
        Q.push_back(M);
    }
    int rc = genome_searchable(ctx, genome);
    if (rc) return rc;
    const GenomeText g = genome_text(genome);
    // workgroups of a record: over the starts its shortest matrix has there
    const std::vector<int64_t> prefix = tile_prefix(g.n_contigs, CD_WG_STARTS, false, [&](int64_t c) { return g.cd[c].len; }, 3 * m_min);
    const int64_t n_wg = prefix[(size_t)g.n_contigs];
    if ((rc = one_launch(ctx, fn, n_wg, "workgroups"))) return rc;
    kgma_codon_stats T{};
    T.lane_starts = CD_LANE_STARTS; T.wave_starts = CD_WAVE_STARTS; T.wg_starts = CD_WG_STARTS;
    if (Q.empty() || n_wg == 0) { S->stats = T; return KGMA_OK; }

    int device = 0;
    hipStream_t st = nullptr;
    ctx_device(ctx, &device, &st);
    (void)hipSetDevice(device);
    DeviceHold hold;
    if ((rc = S->out.reserve(ctx, fn))) return rc;
    CodonArgs a;
    memset(&a, 0, sizeof a);
    CodonMatrix *d_q = nullptr;
    int16_t *d_tab = nullptr;
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
    rc = S->out.fill(ctx, fn, "hits", st, a.ctl, ctl, [&](CodonHit *out, unsigned long long cap, unsigned long long *) {
        a.out = out; a.cap = cap;
        return launch_codon(a, n_wg, st);
    }, &T.n_launches);
    if (rc) return rc;
    KGMA_TRY(hipEventRecord(hold.ev[1], st));
    std::vector<kgma_codon_hit> found;
    if ((rc = S->out.fetch(ctx, fn, ctl[0], found))) return rc;
    KGMA_TRY(hipStreamSynchronize(st));            // (the second event has been reached)
    std::sort(found.begin(), found.end(), [](const kgma_codon_hit &x, const kgma_codon_hit &y) {
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

int kgma_get_codon_matches(kgma_ctx *ctx, kgma_codon_hit *out, int64_t cap, int64_t *n)
{
    return ctx ? copy_out(ctx, "kgma_get_codon_matches", ctx_codon(ctx)->hits, out, cap, n) : KGMA_E_ARG;
}

int kgma_get_codon_stats(kgma_ctx *ctx, kgma_codon_stats *out)
{
    if (!ctx || !out) return KGMA_E_ARG;
    *out = ctx_codon(ctx)->stats;
    return KGMA_OK;
}

int kgma_codon_fold(const int16_t *aa_weights, int32_t m, const uint8_t *code, const int16_t *x_weight, int32_t minus, int16_t *out)
{
    if (!aa_weights || !code || !x_weight || !out || m < 1 || m > CD_MAX_ROWS) return KGMA_E_ARG;
    for (int c = 0; c < 64; c++)
        if (code[c] >= KGMA_CODON_AA_COLUMNS) return KGMA_E_ARG;
    for (int32_t i = 0; i < m; i++) {
        // the row a codon at row i of the plus strand is scored by, and the codon it is read as on the searched strand
        const int32_t src = minus ? m - 1 - i : i;
        int16_t *row = out + (int64_t)CD_ENTRIES * i;
        for (int c = 0; c < 64; c++) {
            const int b0 = c >> 4, b1 = (c >> 2) & 3, b2 = c & 3;
            const int read = minus ? 16 * (3 - b2) + 4 * (3 - b1) + (3 - b0) : c;
            row[c] = aa_weights[(int64_t)KGMA_CODON_AA_COLUMNS * src + code[read]];
        }
        row[CD_AMBIGUOUS] = x_weight[src];
    }
    return KGMA_OK;
}

}  // extern "C"
