// kgma_assign.cpp -- host side of gene assignment (kgma_assign_seqs, kgma_assign_ranges; kernels: kgma_assign.hip).
//
// One call: check the arguments, upload the references and the query descriptors, sort the queries into LENGTH CLASSES (a launch's
// LDS is sized by its longest query, so one 8191-residue query must not cut the occupancy of thousands of short ones), run the
// score kernel over every class in chunks of KGMA_ASSIGN_PAIRS_PER_LAUNCH pairs, bring the n_queries x n_refs matrix down, choose
// every query's top references on the host (the matrix is small: a partial sort per row), run the trace kernel over the chosen
// pairs -- again per class, in chunks whose trace bytes fit KGMA_ASSIGN_TRACE_BYTES -- and bring the assignments down.  Every
// device buffer belongs to the call and is freed before it returns.
//
// The screened calls (kgma_assign_seqs_screened, kgma_assign_ranges_screened) first ask kgma_kmat.cpp for every query's n_near
// nearest references by k-mer distance; the matrix then has n_near columns, column c of query q being reference cand[q][c].
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "kgma_assign.h"

using namespace kgma;

static_assert(sizeof(kgma_assignment) == 8 * sizeof(int32_t), "assign_trace_kernel writes 8 int32 per job");
static_assert(KGMA_ASSIGN_MAX_LEN == kgma::KGMA_ASSIGN_LEN_MAX, "kgma.h and kgma_device.h agree on the longest sequence");

namespace {

int check_refs(kgma_ctx *ctx, const char *fn, const uint8_t *refs, const int64_t *ref_offsets, int32_t n_refs, int32_t go, int32_t ge,
               int32_t top, int64_t n_queries, const void *out)
{
    if (!refs || !ref_offsets) return failf(ctx, KGMA_E_ARG, "%s: null references", fn);
    if (n_refs < 1) return failf(ctx, KGMA_E_ARG, "%s: n_refs = %d", fn, n_refs);
    if (top < 1 || top > n_refs) return failf(ctx, KGMA_E_ARG, "%s: top = %d is not one of 1 .. n_refs = %d", fn, top, n_refs);
    if (n_queries < 0) return failf(ctx, KGMA_E_ARG, "%s: n_queries = %lld", fn, (long long)n_queries);
    if (n_queries > 0 && !out) return failf(ctx, KGMA_E_ARG, "%s: null output", fn);
    if (go > 0 || ge > 0) return failf(ctx, KGMA_E_ARG, "%s: gap scores %d, %d: a gap score is not positive", fn, go, ge);
    if (-(int64_t)go - 8192 * (int64_t)ge > ((int64_t)1 << 27))
        return failf(ctx, KGMA_E_UNSUPPORTED, "%s: gap scores %d, %d: -gap_open_score - 8192 * gap_extend_score exceeds 2^27 (a cell could reach the no-alignment sentinel)",
                     fn, go, ge);
    for (int32_t r = 0; r < n_refs; r++) {
        const int64_t m = ref_offsets[r + 1] - ref_offsets[r];
        if (m < 0) return failf(ctx, KGMA_E_ARG, "%s: ref_offsets[%d] > ref_offsets[%d]", fn, r, r + 1);
        if (m == 0) return failf(ctx, KGMA_E_ARG, "%s: reference %d is empty", fn, r);
        if (m > KGMA_ASSIGN_MAX_LEN) return failf(ctx, KGMA_E_UNSUPPORTED, "%s: reference %d has %lld residues (max %d)", fn, r, (long long)m, KGMA_ASSIGN_MAX_LEN);
    }
    if (n_queries * (int64_t)n_refs > ((int64_t)1 << 30))
        return failf(ctx, KGMA_E_UNSUPPORTED, "%s: %lld queries x %d references: more than 2^30 pairs in one call", fn, (long long)n_queries, n_refs);
    return KGMA_OK;
}

#define A_TRY(expr)                                                                                          \
    do {                                                                                                     \
        const hipError_t e__ = (expr);                                                                       \
        if (e__ != hipSuccess) return failf(ctx, KGMA_E_HIP, "%s: %s failed: %s", fn, #expr, hipGetErrorString(e__)); \
    } while (0)

// cand == nullptr: every reference is a column (n_cols = n_refs); otherwise cand[q * n_cols + c] names column c of query q
int run(kgma_ctx *ctx, const char *fn, const Queries &Q, const uint8_t *refs, const int64_t *ref_offsets, int32_t n_refs, int32_t go,
        int32_t ge, int32_t top, kgma_assignment *out, int32_t *scores, const int32_t *cand = nullptr, int32_t n_cols = 0)
{
    const int64_t H = (int64_t)Q.n.size();
    if (!cand) n_cols = n_refs;
    int device = 0;
    hipStream_t st = nullptr;
    ctx_device(ctx, &device, &st);
    (void)hipSetDevice(device);
    DeviceHold hold;

    // length classes: the class's queries, and all classes' lists one after the other (`items`)
    constexpr int NC = (int)(sizeof KGMA_ASSIGN_CLASS_BOUNDS / sizeof KGMA_ASSIGN_CLASS_BOUNDS[0]);
    std::vector<int32_t> items[NC];
    int class_max[NC] = {};
    for (int64_t q = 0; q < H; q++) {
        int c = 0;
        while (Q.n[(size_t)q] > KGMA_ASSIGN_CLASS_BOUNDS[c]) c++;
        items[c].push_back((int32_t)q);
        class_max[c] = std::max(class_max[c], (int)Q.n[(size_t)q]);
    }
    std::vector<int32_t> all_items;
    int64_t item0[NC];
    for (int c = 0; c < NC; c++) { item0[c] = (int64_t)all_items.size(); all_items.insert(all_items.end(), items[c].begin(), items[c].end()); }

    const int64_t rbase = ref_offsets[0];
    std::vector<int64_t> roff((size_t)n_refs + 1);
    for (int32_t r = 0; r <= n_refs; r++) roff[(size_t)r] = ref_offsets[r] - rbase;

    AssignArgs a;
    memset(&a, 0, sizeof a);
    uint8_t *d_refs = nullptr, *d_text = nullptr;
    int64_t *d_roff = nullptr, *d_pos = nullptr;
    int32_t *d_n = nullptr, *d_contig = nullptr, *d_items = nullptr, *d_scores = nullptr, *d_cand = nullptr;
    A_TRY(hold.upload(d_refs, refs + rbase, (size_t)roff[(size_t)n_refs], st));
    A_TRY(hold.upload(d_roff, roff.data(), roff.size(), st));
    A_TRY(hold.upload(d_pos, Q.pos.data(), (size_t)H, st));
    A_TRY(hold.upload(d_n, Q.n.data(), (size_t)H, st));
    A_TRY(hold.upload(d_items, all_items.data(), (size_t)H, st));
    if (Q.source == 0) {
        A_TRY(hold.upload(d_contig, Q.contig, (size_t)H, st));
        a.text = Q.g.d_ascii; a.cd = Q.g.d_cd; a.q_contig = d_contig;
    } else {
        A_TRY(hold.upload(d_text, Q.text, (size_t)Q.bytes, st));
        a.text = d_text;
    }
    if (cand) A_TRY(hold.upload(d_cand, cand, (size_t)(H * n_cols), st));
    A_TRY(hold.alloc(d_scores, (size_t)(H * n_cols)));
    for (hipEvent_t &e : hold.ev) A_TRY(hipEventCreate(&e));
    a.q_pos = d_pos; a.q_n = d_n; a.refs = d_refs; a.ref_off = d_roff; a.n_refs = n_refs; a.go = -go; a.ge = -ge;
    a.scores = d_scores; a.cand = d_cand; a.n_cols = n_cols;

    kgma_assign_stats S{};
    // ---- score pass -------------------------------------------------------------------------------------------
    A_TRY(hipEventRecord(hold.ev[0], st));
    for (int c = 0; c < NC; c++) {
        const int64_t pairs = (int64_t)items[c].size() * n_cols;
        a.max_n = class_max[c];
        a.items = d_items + item0[c];
        for (int64_t p = 0; p < pairs; p += KGMA_ASSIGN_PAIRS_PER_LAUNCH) {
            a.first = p;
            A_TRY(launch_assign(a, Q.source, false, (int)std::min<int64_t>(KGMA_ASSIGN_PAIRS_PER_LAUNCH, pairs - p), st));
            S.n_score_launches++;
        }
    }
    A_TRY(hipEventRecord(hold.ev[1], st));
    std::vector<int32_t> own;
    int32_t *mat = scores;
    if (!mat) { own.resize((size_t)(H * n_cols)); mat = own.data(); }
    A_TRY(hipMemcpyAsync(mat, d_scores, (size_t)(H * n_cols) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    A_TRY(hipStreamSynchronize(st));

    // ---- selection: per query the `top` references, higher score first, lower index among equal scores ------------
    // jobs are laid out class by class (a trace launch has one LDS size); job_slot says where a job's result belongs in `out`
    std::vector<int32_t> job_q, job_r;
    std::vector<int64_t> job_slot;
    int64_t job0[NC + 1];
    std::vector<int32_t> order((size_t)n_cols);
    for (int c = 0; c < NC; c++) {
        job0[c] = (int64_t)job_q.size();
        for (int32_t q : items[c]) {
            const int32_t *row = mat + (int64_t)q * n_cols;
            const int32_t *name = cand ? cand + (int64_t)q * n_cols : nullptr;     // a column's reference (the column itself without)
            std::iota(order.begin(), order.end(), 0);
            std::partial_sort(order.begin(), order.begin() + top, order.end(), [row, name](int32_t x, int32_t y) {
                return row[x] != row[y] ? row[x] > row[y] : name ? name[x] < name[y] : x < y;
            });
            for (int32_t t = 0; t < top; t++) {
                job_q.push_back(q); job_r.push_back(name ? name[order[(size_t)t]] : order[(size_t)t]); job_slot.push_back((int64_t)q * top + t);
            }
        }
    }
    job0[NC] = (int64_t)job_q.size();
    const int64_t J = job0[NC];

    // ---- trace pass ---------------------------------------------------------------------------------------------
    int32_t *d_jq = nullptr, *d_jr = nullptr, *d_out = nullptr;
    uint8_t *d_trace = nullptr;
    A_TRY(hold.upload(d_jq, job_q.data(), (size_t)J, st));
    A_TRY(hold.upload(d_jr, job_r.data(), (size_t)J, st));
    A_TRY(hold.alloc(d_out, (size_t)J * 8));
    int64_t stride[NC], chunk[NC], trace_bytes = 0;
    for (int c = 0; c < NC; c++) {
        stride[c] = chunk[c] = 0;
        const int64_t nj = job0[c + 1] - job0[c];
        if (!nj) continue;
        int max_m = 1;
        for (int64_t j = job0[c]; j < job0[c + 1]; j++) max_m = std::max<int>(max_m, (int)(roff[(size_t)job_r[(size_t)j] + 1] - roff[(size_t)job_r[(size_t)j]]));
        stride[c] = (assign_trace_bytes(max_m, class_max[c]) + 255) & ~(int64_t)255;
        chunk[c] = std::max<int64_t>(1, std::min<int64_t>(nj, KGMA_ASSIGN_TRACE_BYTES / stride[c]));
        trace_bytes = std::max(trace_bytes, chunk[c] * stride[c]);
    }
    A_TRY(hold.alloc(d_trace, (size_t)trace_bytes));
    a.job_q = d_jq; a.job_r = d_jr; a.trace = d_trace; a.out = d_out;
    A_TRY(hipEventRecord(hold.ev[2], st));
    for (int c = 0; c < NC; c++) {
        a.max_n = class_max[c];
        a.trace_stride = stride[c];
        for (int64_t j = job0[c]; j < job0[c + 1]; j += chunk[c]) {
            a.first = j;
            A_TRY(launch_assign(a, Q.source, true, (int)std::min<int64_t>(chunk[c], job0[c + 1] - j), st));
            S.n_trace_launches++;
        }
    }
    A_TRY(hipEventRecord(hold.ev[3], st));
    std::vector<kgma_assignment> res((size_t)J);
    A_TRY(hipMemcpyAsync(res.data(), d_out, (size_t)J * sizeof(kgma_assignment), hipMemcpyDeviceToHost, st));
    A_TRY(hipStreamSynchronize(st));
    for (int64_t j = 0; j < J; j++) out[job_slot[(size_t)j]] = res[(size_t)j];

    float ms = 0;
    A_TRY(hipEventElapsedTime(&ms, hold.ev[0], hold.ev[1]));
    S.score_ms = ms;
    A_TRY(hipEventElapsedTime(&ms, hold.ev[2], hold.ev[3]));
    S.trace_ms = ms;
    S.n_pairs = H * n_cols;
    S.n_traced = J;
    if (cand) {
        for (int64_t p = 0; p < H * n_cols; p++) S.n_cells += (int64_t)Q.n[(size_t)(p / n_cols)] * (roff[(size_t)cand[p] + 1] - roff[(size_t)cand[p]]);
    } else {
        int64_t sum_n = 0;
        for (int32_t n : Q.n) sum_n += n;
        S.n_cells = sum_n * roff[(size_t)n_refs];
    }
    *ctx_assign_stats(ctx) = S;
    return KGMA_OK;
}

// The queries of the two sources, validated.  *empty: n_queries == 0 (KGMA_OK, nothing to do).
int seq_queries(kgma_ctx *ctx, const char *fn, const uint8_t *queries, const int64_t *query_offsets, int64_t n_queries, Queries &Q)
{
    if (!queries || !query_offsets) return failf(ctx, KGMA_E_ARG, "%s: null queries", fn);
    Q.source = 1;
    Q.pos.resize((size_t)n_queries);
    Q.n.resize((size_t)n_queries);
    const int64_t base = query_offsets[0];
    for (int64_t q = 0; q < n_queries; q++) {
        const int64_t n = query_offsets[q + 1] - query_offsets[q];
        if (n < 0) return failf(ctx, KGMA_E_ARG, "%s: query_offsets[%lld] > query_offsets[%lld]", fn, (long long)q, (long long)q + 1);
        if (n == 0) return failf(ctx, KGMA_E_ARG, "%s: query %lld is empty", fn, (long long)q);
        if (n > KGMA_ASSIGN_MAX_LEN) return failf(ctx, KGMA_E_UNSUPPORTED, "%s: query %lld has %lld residues (max %d)", fn, (long long)q, (long long)n, KGMA_ASSIGN_MAX_LEN);
        Q.pos[(size_t)q] = query_offsets[q] - base;
        Q.n[(size_t)q] = (int32_t)n;
    }
    Q.text = queries + base;
    Q.bytes = query_offsets[n_queries] - base;
    return KGMA_OK;
}

int range_queries(kgma_ctx *ctx, const char *fn, const kgma_genome *genome, int64_t n_queries, const int32_t *contig, const int64_t *lo,
                  const int64_t *hi, Queries &Q)
{
    if (!contig || !lo || !hi) return failf(ctx, KGMA_E_ARG, "%s: null ranges", fn);
    Q.source = 0;
    Q.g = genome_text(genome);
    Q.contig = contig;
    Q.pos.resize((size_t)n_queries);
    Q.n.resize((size_t)n_queries);
    for (int64_t q = 0; q < n_queries; q++) {
        if (contig[q] < 0 || contig[q] >= Q.g.n_contigs) return failf(ctx, KGMA_E_ARG, "%s: query %lld: no record %d", fn, (long long)q, contig[q]);
        const int64_t L = Q.g.cd[contig[q]].len, n = hi[q] - lo[q] + 1;
        if (n == 0) return failf(ctx, KGMA_E_ARG, "%s: query %lld is empty (%lld:%lld)", fn, (long long)q, (long long)lo[q], (long long)hi[q]);
        if (lo[q] < 1 || hi[q] > L || n < 0)
            return failf(ctx, KGMA_E_ARG, "%s: query %lld: range %lld:%lld outside record %d of %lld residues", fn, (long long)q, (long long)lo[q],
                         (long long)hi[q], contig[q], (long long)L);
        if (n > KGMA_ASSIGN_MAX_LEN) return failf(ctx, KGMA_E_UNSUPPORTED, "%s: query %lld has %lld residues (max %d)", fn, (long long)q, (long long)n, KGMA_ASSIGN_MAX_LEN);
        Q.pos[(size_t)q] = lo[q];
        Q.n[(size_t)q] = (int32_t)n;
    }
    return KGMA_OK;
}

int check_screen(kgma_ctx *ctx, const char *fn, int32_t n_refs, int32_t top, int32_t screen_k, int32_t n_near)
{
    if (n_refs >= 1 && (n_near < 1 || n_near > n_refs || n_near > KGMA_KMAT_MAX_NEAR))
        return failf(ctx, KGMA_E_ARG, "%s: n_near = %d is not one of 1 .. min(n_refs = %d, %d)", fn, n_near, n_refs, KGMA_KMAT_MAX_NEAR);
    if (n_refs >= 1 && top > n_near) return failf(ctx, KGMA_E_ARG, "%s: top = %d exceeds n_near = %d", fn, top, n_near);
    if (screen_k < 1) return failf(ctx, KGMA_E_ARG, "%s: screen_k = %d", fn, screen_k);
    if (screen_k > 10) return failf(ctx, KGMA_E_UNSUPPORTED, "%s: screen_k = %d: the prescreen serves k = 1 ... 10", fn, screen_k);
    return KGMA_OK;
}

// The prescreen, then the assignment over its candidates
int run_screened(kgma_ctx *ctx, const char *fn, const Queries &Q, const uint8_t *refs, const int64_t *ref_offsets, int32_t n_refs, int32_t go,
                 int32_t ge, int32_t top, int32_t screen_k, int32_t n_near, kgma_assignment *out, int32_t *cand, int32_t *scores)
{
    std::vector<int64_t> roff((size_t)n_refs + 1);
    for (int32_t r = 0; r <= n_refs; r++) roff[(size_t)r] = ref_offsets[r] - ref_offsets[0];
    std::vector<int32_t> own;
    if (!cand) { own.resize(Q.n.size() * (size_t)n_near); cand = own.data(); }
    int rc = kmat_run(ctx, fn, screen_k, Q, "query", refs + ref_offsets[0], roff.data(), n_refs, "reference", n_near, nullptr, nullptr, cand, nullptr);
    if (rc) return rc;
    rc = run(ctx, fn, Q, refs, ref_offsets, n_refs, go, ge, top, out, scores, cand, n_near);
    if (rc) *ctx_kmat_stats(ctx) = kgma_kmat_stats{};
    return rc;
}

}  // namespace

extern "C" {

int kgma_assign_seqs(kgma_ctx *ctx, const uint8_t *refs, const int64_t *ref_offsets, int32_t n_refs, const uint8_t *queries,
                     const int64_t *query_offsets, int64_t n_queries, int32_t gap_open_score, int32_t gap_extend_score, int32_t top,
                     kgma_assignment *out, int32_t *scores)
{
    static const char fn[] = "kgma_assign_seqs";
    if (!ctx) return KGMA_E_ARG;
    *ctx_assign_stats(ctx) = kgma_assign_stats{};
    int rc = check_refs(ctx, fn, refs, ref_offsets, n_refs, gap_open_score, gap_extend_score, top, n_queries, out);
    if (rc) return rc;
    if (n_queries == 0) return KGMA_OK;
    Queries Q;
    if ((rc = seq_queries(ctx, fn, queries, query_offsets, n_queries, Q))) return rc;
    return run(ctx, fn, Q, refs, ref_offsets, n_refs, gap_open_score, gap_extend_score, top, out, scores);
}

int kgma_assign_ranges(kgma_ctx *ctx, const kgma_genome *genome, const uint8_t *refs, const int64_t *ref_offsets, int32_t n_refs,
                       int64_t n_queries, const int32_t *contig, const int64_t *lo, const int64_t *hi, int32_t gap_open_score,
                       int32_t gap_extend_score, int32_t top, kgma_assignment *out, int32_t *scores)
{
    static const char fn[] = "kgma_assign_ranges";
    if (!ctx) return KGMA_E_ARG;
    *ctx_assign_stats(ctx) = kgma_assign_stats{};
    if (!genome) return failf(ctx, KGMA_E_ARG, "%s: null genome", fn);
    int rc = check_refs(ctx, fn, refs, ref_offsets, n_refs, gap_open_score, gap_extend_score, top, n_queries, out);
    if (rc) return rc;
    if (n_queries == 0) return KGMA_OK;
    Queries Q;
    if ((rc = range_queries(ctx, fn, genome, n_queries, contig, lo, hi, Q))) return rc;
    return run(ctx, fn, Q, refs, ref_offsets, n_refs, gap_open_score, gap_extend_score, top, out, scores);
}

int kgma_assign_seqs_screened(kgma_ctx *ctx, const uint8_t *refs, const int64_t *ref_offsets, int32_t n_refs, const uint8_t *queries,
                              const int64_t *query_offsets, int64_t n_queries, int32_t gap_open_score, int32_t gap_extend_score,
                              int32_t top, int32_t screen_k, int32_t n_near, kgma_assignment *out, int32_t *cand, int32_t *scores)
{
    static const char fn[] = "kgma_assign_seqs_screened";
    if (!ctx) return KGMA_E_ARG;
    *ctx_assign_stats(ctx) = kgma_assign_stats{};
    *ctx_kmat_stats(ctx) = kgma_kmat_stats{};
    int rc = check_refs(ctx, fn, refs, ref_offsets, n_refs, gap_open_score, gap_extend_score, top, n_queries, out);
    if (rc || (rc = check_screen(ctx, fn, n_refs, top, screen_k, n_near))) return rc;
    if (n_queries == 0) return KGMA_OK;
    Queries Q;
    if ((rc = seq_queries(ctx, fn, queries, query_offsets, n_queries, Q))) return rc;
    return run_screened(ctx, fn, Q, refs, ref_offsets, n_refs, gap_open_score, gap_extend_score, top, screen_k, n_near, out, cand, scores);
}

int kgma_assign_ranges_screened(kgma_ctx *ctx, const kgma_genome *genome, const uint8_t *refs, const int64_t *ref_offsets, int32_t n_refs,
                                int64_t n_queries, const int32_t *contig, const int64_t *lo, const int64_t *hi, int32_t gap_open_score,
                                int32_t gap_extend_score, int32_t top, int32_t screen_k, int32_t n_near, kgma_assignment *out,
                                int32_t *cand, int32_t *scores)
{
    static const char fn[] = "kgma_assign_ranges_screened";
    if (!ctx) return KGMA_E_ARG;
    *ctx_assign_stats(ctx) = kgma_assign_stats{};
    *ctx_kmat_stats(ctx) = kgma_kmat_stats{};
    if (!genome) return failf(ctx, KGMA_E_ARG, "%s: null genome", fn);
    int rc = check_refs(ctx, fn, refs, ref_offsets, n_refs, gap_open_score, gap_extend_score, top, n_queries, out);
    if (rc || (rc = check_screen(ctx, fn, n_refs, top, screen_k, n_near))) return rc;
    if (n_queries == 0) return KGMA_OK;
    Queries Q;
    if ((rc = range_queries(ctx, fn, genome, n_queries, contig, lo, hi, Q))) return rc;
    return run_screened(ctx, fn, Q, refs, ref_offsets, n_refs, gap_open_score, gap_extend_score, top, screen_k, n_near, out, cand, scores);
}

int kgma_get_assign_stats(kgma_ctx *ctx, kgma_assign_stats *out)
{
    if (!ctx || !out) return KGMA_E_ARG;
    *out = *ctx_assign_stats(ctx);
    return KGMA_OK;
}

}  // extern "C"
