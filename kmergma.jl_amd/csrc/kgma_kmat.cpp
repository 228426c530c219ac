// kgma_kmat.cpp -- host side of the all-pairs k-mer distances (kgma_kmer_dist_matrix, kgma_kmer_nearest and their _ranges forms;
// kernels: kgma_kmat.hip).
//
// One call: check the arguments, upload B and the descriptors of A (and A itself unless it lies in a resident genome), run the norm
// kernel (|c_a|^2 and A's residue check) and the matrix kernel, then either bring the matrix down or run the select kernel and
// bring down only its n_near columns.  Every device buffer belongs to the call and is freed before it returns.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kgma_assign.h"

using namespace kgma;

static_assert(KGMA_KMAT_MAX_LEN == kgma::KGMA_KMAT_LEN_MAX, "kgma.h and kgma_device.h agree on the longest sequence");
static_assert(2ll * KGMA_KMAT_MAX_LEN * KGMA_KMAT_MAX_LEN < (1ll << 31), "D fits an int32");

namespace {

constexpr unsigned long long NO_BAD = ~0ull;
constexpr int64_t MAX_PAIRS = (int64_t)1 << 30;

#define K_TRY(expr)                                                                                          \
    do {                                                                                                     \
        const hipError_t e__ = (expr);                                                                       \
        if (e__ != hipSuccess) return failf(ctx, KGMA_E_HIP, "%s: %s failed: %s", fn, #expr, hipGetErrorString(e__)); \
    } while (0)

// k, n_a, n_b, n_near: what can be said before any pointer is read.  *empty: there is nothing to do (KGMA_OK).
int check_scalars(kgma_ctx *ctx, const char *fn, int32_t k, int64_t n_a, int64_t n_b, bool nearest, int32_t n_near, bool *empty)
{
    *empty = false;
    if (k < 1) return failf(ctx, KGMA_E_ARG, "%s: k = %d", fn, k);
    if (k > 10) return failf(ctx, KGMA_E_UNSUPPORTED, "%s: k = %d: the distance matrix serves k = 1 ... 10", fn, k);
    if (n_a < 0) return failf(ctx, KGMA_E_ARG, "%s: n_a = %lld", fn, (long long)n_a);
    if (n_b < 1) return failf(ctx, KGMA_E_ARG, "%s: n_b = %lld", fn, (long long)n_b);
    if (nearest && (n_near < 1 || n_near > n_b || n_near > KGMA_KMAT_MAX_NEAR))
        return failf(ctx, KGMA_E_ARG, "%s: n_near = %d is not one of 1 .. min(n_b = %lld, %d)", fn, n_near, (long long)n_b, KGMA_KMAT_MAX_NEAR);
    if (n_a == 0) { *empty = true; return KGMA_OK; }
    if (n_a * n_b > MAX_PAIRS)
        return failf(ctx, KGMA_E_UNSUPPORTED, "%s: %lld x %lld sequences: more than 2^30 pairs in one call", fn, (long long)n_a, (long long)n_b);
    return KGMA_OK;
}

// Offsets of n sequences: lengths 0 ... KGMA_KMAT_MAX_LEN.  rel: the offsets from the first one's.
int check_offsets(kgma_ctx *ctx, const char *fn, const char *side, const char *name, const int64_t *off, int64_t n, std::vector<int64_t> &rel)
{
    rel.resize((size_t)n + 1);
    for (int64_t i = 0; i < n; i++) {
        const int64_t len = off[i + 1] - off[i];
        if (len < 0) return failf(ctx, KGMA_E_ARG, "%s: %s[%lld] > %s[%lld]", fn, name, (long long)i, name, (long long)i + 1);
        if (len > KGMA_KMAT_MAX_LEN)
            return failf(ctx, KGMA_E_UNSUPPORTED, "%s: %s sequence %lld has %lld residues (max %d)", fn, side, (long long)i, (long long)len, KGMA_KMAT_MAX_LEN);
        rel[(size_t)i] = off[i] - off[0];
    }
    rel[(size_t)n] = off[n] - off[0];
    return KGMA_OK;
}

int a_from_ranges(kgma_ctx *ctx, const char *fn, const kgma_genome *genome, int64_t n_a, const int32_t *contig, const int64_t *lo,
                  const int64_t *hi, Queries &Q)
{
    if (!contig || !lo || !hi) return failf(ctx, KGMA_E_ARG, "%s: null ranges", fn);
    Q.source = 0;
    Q.g = genome_text(genome);
    Q.contig = contig;
    Q.pos.resize((size_t)n_a);
    Q.n.resize((size_t)n_a);
    for (int64_t i = 0; i < n_a; i++) {
        if (contig[i] < 0 || contig[i] >= Q.g.n_contigs) return failf(ctx, KGMA_E_ARG, "%s: range %lld: no record %d", fn, (long long)i, contig[i]);
        const int64_t L = Q.g.cd[contig[i]].len, n = hi[i] - lo[i] + 1;
        if (lo[i] < 1 || hi[i] > L || n < 0)
            return failf(ctx, KGMA_E_ARG, "%s: range %lld: %lld:%lld outside record %d of %lld residues", fn, (long long)i, (long long)lo[i],
                         (long long)hi[i], contig[i], (long long)L);
        if (n > KGMA_KMAT_MAX_LEN)
            return failf(ctx, KGMA_E_UNSUPPORTED, "%s: range %lld has %lld residues (max %d)", fn, (long long)i, (long long)n, KGMA_KMAT_MAX_LEN);
        Q.pos[(size_t)i] = lo[i];
        Q.n[(size_t)i] = (int32_t)n;
    }
    return KGMA_OK;
}

// The common body of the four entry points.  genome: the A side is ranges (contig, lo, hi), otherwise sequences (a, a_off).
int entry(kgma_ctx *ctx, const char *fn, const kgma_genome *genome, bool ranges, int32_t k, const uint8_t *a, const int64_t *a_off,
          int64_t n_a, const int32_t *contig, const int64_t *lo, const int64_t *hi, const uint8_t *b, const int64_t *b_off, int32_t n_b,
          bool nearest, int32_t n_near, int32_t *D, double *dist, int32_t *index, int32_t *D_near)
{
    if (!ctx) return KGMA_E_ARG;
    *ctx_kmat_stats(ctx) = kgma_kmat_stats{};
    if (ranges && !genome) return failf(ctx, KGMA_E_ARG, "%s: null genome", fn);
    const bool symmetric = !ranges && !b;                      // B = A
    if (ranges && !b) return failf(ctx, KGMA_E_ARG, "%s: null B", fn);
    bool empty = false;
    int rc = check_scalars(ctx, fn, k, n_a, symmetric ? std::max<int64_t>(n_a, 1) : n_b, nearest, n_near, &empty);
    if (rc || empty) return rc;
    if (!symmetric && !b_off) return failf(ctx, KGMA_E_ARG, "%s: null B offsets", fn);
    Queries Q;
    std::vector<int64_t> a_rel, b_rel;
    if (ranges) {
        if ((rc = a_from_ranges(ctx, fn, genome, n_a, contig, lo, hi, Q))) return rc;
    } else {
        if (!a || !a_off) return failf(ctx, KGMA_E_ARG, "%s: null A", fn);
        if ((rc = check_offsets(ctx, fn, "A", "a_off", a_off, n_a, a_rel))) return rc;
        Q.source = 1;
        Q.text = a + a_off[0];
        Q.bytes = a_rel[(size_t)n_a];
        Q.pos.assign(a_rel.begin(), a_rel.end() - 1);
        Q.n.resize((size_t)n_a);
        for (int64_t i = 0; i < n_a; i++) Q.n[(size_t)i] = (int32_t)(a_rel[(size_t)i + 1] - a_rel[(size_t)i]);
    }
    if (symmetric) return kmat_run(ctx, fn, k, Q, "A sequence", Q.text, a_rel.data(), (int32_t)n_a, "A sequence", n_near, D, dist, index, D_near);
    if ((rc = check_offsets(ctx, fn, "B", "b_off", b_off, n_b, b_rel))) return rc;
    return kmat_run(ctx, fn, k, Q, ranges ? "range" : "A sequence", b + b_off[0], b_rel.data(), n_b, "B sequence", n_near, D, dist, index, D_near);
}

}  // namespace

namespace kgma {

int kmat_run(kgma_ctx *ctx, const char *fn, int32_t k, const Queries &A, const char *a_name, const uint8_t *b, const int64_t *b_off,
             int32_t n_b, const char *b_name, int32_t n_near, int32_t *D, double *dist, int32_t *index, int32_t *D_near)
{
    *ctx_kmat_stats(ctx) = kgma_kmat_stats{};
    const int64_t n_a = (int64_t)A.n.size();
    int device = 0;
    hipStream_t st = nullptr;
    ctx_device(ctx, &device, &st);
    (void)hipSetDevice(device);
    DeviceHold hold;

    // geometry: tiles of T sequences of B along x; chunks of rows of A along y, as many as fill the device while a chunk keeps
    // KGMA_KMAT_MIN_ROWS rows (the tile's build is paid once per chunk)
    const int T = kmat_tile(k), n_cus = std::max(1, ctx_n_cus(ctx));
    const int64_t n_tiles = ((int64_t)n_b + T - 1) / T;
    const int64_t max_chunks = std::min<int64_t>(65535, (n_a + KGMA_KMAT_MIN_ROWS - 1) / KGMA_KMAT_MIN_ROWS);
    int64_t gx, chunks, norm_grid;
    if (k <= 7) {
        gx = std::min<int64_t>(n_tiles, (int64_t)1 << 20);
        chunks = std::min<int64_t>(max_chunks, std::max<int64_t>(1, (4 * (int64_t)n_cus + gx - 1) / gx));
        norm_grid = std::min<int64_t>(n_a, 8 * (int64_t)n_cus);
    } else {
        const int64_t rows = kmat_scratch_rows(k);
        gx = std::min<int64_t>(n_tiles, rows);
        chunks = std::min<int64_t>(max_chunks, std::max<int64_t>(1, rows / gx));
        norm_grid = std::min<int64_t>(n_a, rows);
    }
    const int64_t rows_per_chunk = (n_a + chunks - 1) / chunks;
    chunks = (n_a + rows_per_chunk - 1) / rows_per_chunk;

    KmatArgs a;
    memset(&a, 0, sizeof a);
    uint8_t *d_text = nullptr, *d_b = nullptr;
    int64_t *d_pos = nullptr, *d_boff = nullptr;
    int32_t *d_n = nullptr, *d_contig = nullptr, *d_D = nullptr, *d_idx = nullptr, *d_Dn = nullptr;
    uint32_t *d_na = nullptr, *d_scratch = nullptr;
    double *d_dist = nullptr;
    unsigned long long *d_bad = nullptr;
    K_TRY(hold.upload(d_b, b, (size_t)b_off[n_b], st));
    K_TRY(hold.upload(d_boff, b_off, (size_t)n_b + 1, st));
    K_TRY(hold.upload(d_pos, A.pos.data(), (size_t)n_a, st));
    K_TRY(hold.upload(d_n, A.n.data(), (size_t)n_a, st));
    if (A.source == 0) {
        K_TRY(hold.upload(d_contig, A.contig, (size_t)n_a, st));
        a.text = A.g.d_ascii; a.cd = A.g.d_cd; a.q_contig = d_contig;
    } else {
        K_TRY(hold.upload(d_text, A.text, (size_t)A.bytes, st));
        a.text = d_text;
    }
    K_TRY(hold.alloc(d_na, (size_t)n_a));
    K_TRY(hold.alloc(d_D, (size_t)(n_a * n_b)));
    if (n_near == 0 && dist) K_TRY(hold.alloc(d_dist, (size_t)(n_a * n_b)));
    K_TRY(hold.alloc(d_bad, 2));
    K_TRY(hipMemsetAsync(d_bad, 0xFF, 2 * sizeof(unsigned long long), st));
    if (k > 7) {
        const size_t words = (size_t)std::max(norm_grid, gx * chunks) << (2 * k);
        K_TRY(hold.alloc(d_scratch, words));
        K_TRY(hipMemsetAsync(d_scratch, 0, words * sizeof(uint32_t), st));
    }
    if (n_near > 0) {
        K_TRY(hold.alloc(d_idx, (size_t)(n_a * n_near)));
        K_TRY(hold.alloc(d_Dn, (size_t)(n_a * n_near)));
    }
    for (int e = 0; e < 3; e++) K_TRY(hipEventCreate(&hold.ev[e]));
    a.q_pos = d_pos; a.q_n = d_n; a.b_text = d_b; a.b_off = d_boff; a.n_a = n_a; a.n_b = n_b; a.k = k;
    a.rows_per_chunk = rows_per_chunk; a.na = d_na; a.scratch = d_scratch; a.D = d_D; a.dist = d_dist;
    a.half_inv_k = 1.0 / (double)(2 * k);
    a.bad = d_bad; a.n_near = n_near; a.near_index = d_idx; a.near_D = d_Dn;

    kgma_kmat_stats S{};
    K_TRY(hipEventRecord(hold.ev[0], st));
    K_TRY(launch_kmat_norm(a, A.source, (int)norm_grid, st));
    K_TRY(launch_kmat(a, A.source, (int)gx, (int)chunks, st));
    K_TRY(hipEventRecord(hold.ev[1], st));
    S.n_launches = 2;
    if (n_near > 0) {
        K_TRY(launch_kmat_select(a, st));
        S.n_launches++;
    }
    K_TRY(hipEventRecord(hold.ev[2], st));
    unsigned long long bad[2] = {NO_BAD, NO_BAD};
    K_TRY(hipMemcpyAsync(bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, st));
    K_TRY(hipStreamSynchronize(st));
    for (int side = 0; side < 2; side++) {
        if (bad[side] == NO_BAD) continue;
        const long long seq = (long long)(bad[side] >> 16), pos = (long long)(bad[side] & 0xFFFF);
        if (side == 0 && A.source == 0)
            return failf(ctx, KGMA_E_BADBASE, "%s: %s %lld: record %d position %lld: residue is not one of A/C/G/T/N (KeyError, Consts.jl:22-28)", fn,
                         a_name, seq, A.contig[seq], (long long)A.pos[(size_t)seq] + pos);
        return failf(ctx, KGMA_E_BADBASE, "%s: %s %lld position %lld: residue is not one of A/C/G/T/N (KeyError, Consts.jl:22-28)", fn,
                     side == 0 ? a_name : b_name, seq, pos + 1);
    }
    if (n_near == 0) {
        if (D) K_TRY(hipMemcpyAsync(D, d_D, (size_t)(n_a * n_b) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (dist) K_TRY(hipMemcpyAsync(dist, d_dist, (size_t)(n_a * n_b) * sizeof(double), hipMemcpyDeviceToHost, st));
    } else {
        if (index) K_TRY(hipMemcpyAsync(index, d_idx, (size_t)(n_a * n_near) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (D_near) K_TRY(hipMemcpyAsync(D_near, d_Dn, (size_t)(n_a * n_near) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    K_TRY(hipStreamSynchronize(st));
    float ms = 0;
    K_TRY(hipEventElapsedTime(&ms, hold.ev[0], hold.ev[1]));
    S.kmat_ms = ms;
    if (n_near > 0) {
        K_TRY(hipEventElapsedTime(&ms, hold.ev[1], hold.ev[2]));
        S.select_ms = ms;
    }
    S.n_pairs = n_a * n_b;
    S.form = k <= 7 ? 0 : 1;
    S.tile = T;
    S.chunks = (int32_t)chunks;
    *ctx_kmat_stats(ctx) = S;
    return KGMA_OK;
}

}  // namespace kgma

extern "C" {

int kgma_kmer_dist_matrix(kgma_ctx *ctx, int32_t k, const uint8_t *a, const int64_t *a_off, int64_t n_a, const uint8_t *b,
                          const int64_t *b_off, int32_t n_b, int32_t *D, double *dist)
{
    return entry(ctx, "kgma_kmer_dist_matrix", nullptr, false, k, a, a_off, n_a, nullptr, nullptr, nullptr, b, b_off, n_b, false, 0, D, dist,
                 nullptr, nullptr);
}

int kgma_kmer_dist_matrix_ranges(kgma_ctx *ctx, const kgma_genome *genome, int32_t k, int64_t n_a, const int32_t *contig, const int64_t *lo,
                                 const int64_t *hi, const uint8_t *b, const int64_t *b_off, int32_t n_b, int32_t *D, double *dist)
{
    return entry(ctx, "kgma_kmer_dist_matrix_ranges", genome, true, k, nullptr, nullptr, n_a, contig, lo, hi, b, b_off, n_b, false, 0, D, dist,
                 nullptr, nullptr);
}

int kgma_kmer_nearest(kgma_ctx *ctx, int32_t k, const uint8_t *a, const int64_t *a_off, int64_t n_a, const uint8_t *b, const int64_t *b_off,
                      int32_t n_b, int32_t n_near, int32_t *index, int32_t *D_near)
{
    return entry(ctx, "kgma_kmer_nearest", nullptr, false, k, a, a_off, n_a, nullptr, nullptr, nullptr, b, b_off, n_b, true, n_near, nullptr,
                 nullptr, index, D_near);
}

int kgma_kmer_nearest_ranges(kgma_ctx *ctx, const kgma_genome *genome, int32_t k, int64_t n_a, const int32_t *contig, const int64_t *lo,
                             const int64_t *hi, const uint8_t *b, const int64_t *b_off, int32_t n_b, int32_t n_near, int32_t *index,
                             int32_t *D_near)
{
    return entry(ctx, "kgma_kmer_nearest_ranges", genome, true, k, nullptr, nullptr, n_a, contig, lo, hi, b, b_off, n_b, true, n_near, nullptr,
                 nullptr, index, D_near);
}

int kgma_get_kmat_stats(kgma_ctx *ctx, kgma_kmat_stats *out)
{
    if (!ctx || !out) return KGMA_E_ARG;
    *out = *ctx_kmat_stats(ctx);
    return KGMA_OK;
}

}  // extern "C"
