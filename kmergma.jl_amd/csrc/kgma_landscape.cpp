// kgma_landscape.cpp -- host side of the distance landscape (kgma_dist_layout, kgma_dist_bins, kgma_dist_sweep; kernels:
// kgma_landscape.hip).
//
// The calls read the distances the last scan kept on the device.  One call: check the arguments, derive the layout of the vector
// from the records' window counts, upload the table of the records that have values, run the kernel(s) and bring the result down.
// Every device buffer belongs to the call and is freed before it returns.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kgma_landscape.h"

using namespace kgma;

namespace {

constexpr int64_t MAX_VALUES = (int64_t)1 << 40;      // a workgroup's 32-bit counters and the grids hold far more than any device does

#define L_TRY(expr)                                                                                          \
    do {                                                                                                     \
        const hipError_t e__ = (expr);                                                                       \
        if (e__ != hipSuccess) return failf(ctx, KGMA_E_HIP, "%s: %s failed: %s", fn, #expr, hipGetErrorString(e__)); \
    } while (0)

// values per record: nwin - 1 where the record was evaluated
inline int64_t record_values(int64_t nwin) { return nwin > 0 ? nwin - 1 : 0; }

// the records that have values: their value offsets (and a closing n)
void value_table(const std::vector<int64_t> &nwin, std::vector<int64_t> &voff, std::vector<int64_t> &rec)
{
    voff.clear(); rec.clear();
    int64_t at = 0;
    for (size_t c = 0; c < nwin.size(); c++) {
        const int64_t nv = record_values(nwin[c]);
        if (nv == 0) continue;
        voff.push_back(at);
        rec.push_back((int64_t)c);
        at += nv;
    }
    voff.push_back(at);
}

}  // namespace

extern "C" {

int kgma_dist_layout(kgma_ctx *ctx, int64_t *offset, int64_t cap, int64_t *n)
{
    if (!ctx || !n) return KGMA_E_ARG;
    DistView v;
    const int rc = ctx_dist_view(ctx, "kgma_dist_layout", 1, false, &v);
    if (rc) return rc;
    *n = (int64_t)v.nwin->size() + 1;
    if (!offset) return KGMA_OK;
    if (cap < *n) return failf(ctx, KGMA_E_ARG, "kgma_dist_layout: capacity %lld < %lld", (long long)cap, (long long)*n);
    int64_t at = 0;
    for (size_t c = 0; c < v.nwin->size(); c++) {
        offset[c] = at;
        at += record_values((*v.nwin)[c]);
    }
    offset[v.nwin->size()] = at;
    return KGMA_OK;
}

int kgma_dist_bins(kgma_ctx *ctx, int32_t kfv, int64_t bin, double *bin_min, int64_t *bin_argmin, int64_t *bin_offset, int64_t cap,
                   int64_t *n_bins)
{
    const char *fn = "kgma_dist_bins";
    if (!ctx || !n_bins) return KGMA_E_ARG;
    DistView v;
    const int rc = ctx_dist_view(ctx, fn, kfv, true, &v);
    if (rc) return rc;
    if (bin < 1) return failf(ctx, KGMA_E_ARG, "%s: bin = %lld", fn, (long long)bin);
    if (v.n >= MAX_VALUES) return failf(ctx, KGMA_E_UNSUPPORTED, "%s: %lld values", fn, (long long)v.n);
    bin = std::min(bin, std::max<int64_t>(v.n, 1));            // (no record is longer: the same bins)
    const size_t nc = v.nwin->size();
    std::vector<int64_t> voff, rec, boff;
    value_table(*v.nwin, voff, rec);
    int64_t total = 0;
    for (size_t r = 0; r < rec.size(); r++) {
        boff.push_back(total);
        total += (voff[r + 1] - voff[r] + bin - 1) / bin;
    }
    boff.push_back(total);
    *n_bins = total;
    if (bin_offset) {
        size_t r = 0;
        for (size_t c = 0; c < nc; c++) {
            bin_offset[c] = boff[r];
            if (r < rec.size() && rec[r] == (int64_t)c) r++;
        }
        bin_offset[nc] = total;
    }
    if (!bin_min && !bin_argmin) return KGMA_OK;
    if (!bin_min || !bin_argmin) return failf(ctx, KGMA_E_ARG, "%s: bin_min and bin_argmin come together", fn);
    if (cap < total) return failf(ctx, KGMA_E_ARG, "%s: capacity %lld < %lld", fn, (long long)cap, (long long)total);
    kgma_landscape_stats *S = ctx_landscape_stats(ctx);
    S->bins_ms = S->combine_ms = 0; S->n_values = v.n; S->n_bins = total; S->n_launches = 0;
    if (total == 0) return KGMA_OK;

    int device = 0;
    hipStream_t st = nullptr;
    ctx_device(ctx, &device, &st);
    (void)hipSetDevice(device);
    DeviceHold hold;
    const int64_t n_wg = (v.n + LS_WG_VALUES - 1) / LS_WG_VALUES;
    LandscapeBinsArgs a;
    memset(&a, 0, sizeof a);
    int64_t *d_voff = nullptr, *d_boff = nullptr;
    L_TRY(hold.upload(d_voff, voff.data(), voff.size(), st));
    L_TRY(hold.upload(d_boff, boff.data(), boff.size(), st));
    L_TRY(hold.alloc(a.bin_min, (size_t)total));
    L_TRY(hold.alloc(a.bin_argmin, (size_t)total));
    L_TRY(hold.alloc(a.part_val, (size_t)(2 * n_wg)));
    L_TRY(hold.alloc(a.part_idx, (size_t)(2 * n_wg)));
    L_TRY(hold.alloc(a.part_bin, (size_t)(2 * n_wg)));
    for (int e = 0; e < 3; e++) L_TRY(hipEventCreate(&hold.ev[e]));
    a.dist = v.d_dist; a.n = v.n; a.voff = d_voff; a.boff = d_boff; a.n_rec = (int32_t)rec.size(); a.bin = bin;
    L_TRY(hipEventRecord(hold.ev[0], st));
    L_TRY(launch_landscape_bins(a, n_wg, st));
    L_TRY(hipEventRecord(hold.ev[1], st));
    L_TRY(launch_landscape_combine(a, n_wg, st));
    L_TRY(hipEventRecord(hold.ev[2], st));
    L_TRY(hipMemcpyAsync(bin_min, a.bin_min, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, st));
    L_TRY(hipMemcpyAsync(bin_argmin, a.bin_argmin, (size_t)total * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    L_TRY(hipStreamSynchronize(st));
    float ms = 0;
    L_TRY(hipEventElapsedTime(&ms, hold.ev[0], hold.ev[1]));
    S->bins_ms = ms;
    L_TRY(hipEventElapsedTime(&ms, hold.ev[1], hold.ev[2]));
    S->combine_ms = ms;
    S->n_launches = 2;
    return KGMA_OK;
}

int kgma_dist_sweep(kgma_ctx *ctx, int32_t kfv, const double *thr, int64_t n_thr, int64_t *windows_below, int64_t *dips_below)
{
    const char *fn = "kgma_dist_sweep";
    if (!ctx) return KGMA_E_ARG;
    DistView v;
    const int rc = ctx_dist_view(ctx, fn, kfv, true, &v);
    if (rc) return rc;
    if (n_thr < 1 || n_thr > KGMA_SWEEP_MAX_THRESHOLDS)
        return failf(ctx, KGMA_E_ARG, "%s: n_thr = %lld is not one of 1 .. %d", fn, (long long)n_thr, KGMA_SWEEP_MAX_THRESHOLDS);
    if (!thr || !windows_below || !dips_below) return failf(ctx, KGMA_E_ARG, "%s: null argument", fn);
    for (int64_t j = 0; j < n_thr; j++) {
        if (!std::isfinite(thr[j])) return failf(ctx, KGMA_E_ARG, "%s: threshold %lld is not finite", fn, (long long)j);
        if (j && !(thr[j - 1] < thr[j])) return failf(ctx, KGMA_E_ARG, "%s: thresholds are not strictly increasing at %lld", fn, (long long)j);
    }
    if (v.n >= MAX_VALUES) return failf(ctx, KGMA_E_UNSUPPORTED, "%s: %lld values", fn, (long long)v.n);
    kgma_landscape_stats *S = ctx_landscape_stats(ctx);
    S->sweep_ms = 0; S->n_values = v.n; S->n_launches = 0; S->sweep_slots = landscape_sweep_slots((int32_t)n_thr);
    for (int64_t j = 0; j < n_thr; j++) windows_below[j] = dips_below[j] = 0;
    if (v.n == 0) return KGMA_OK;

    int device = 0;
    hipStream_t st = nullptr;
    ctx_device(ctx, &device, &st);
    (void)hipSetDevice(device);
    DeviceHold hold;
    std::vector<int64_t> voff, rec;
    value_table(*v.nwin, voff, rec);
    LandscapeSweepArgs a;
    memset(&a, 0, sizeof a);
    int64_t *d_voff = nullptr;
    double *d_thr = nullptr;
    unsigned long long *d_acc = nullptr;
    L_TRY(hold.upload(d_voff, voff.data(), voff.size(), st));
    L_TRY(hold.upload(d_thr, thr, (size_t)n_thr, st));
    L_TRY(hold.alloc(d_acc, (size_t)(2 * n_thr)));
    L_TRY(hipMemsetAsync(d_acc, 0, (size_t)(2 * n_thr) * sizeof(unsigned long long), st));
    for (int e = 0; e < 2; e++) L_TRY(hipEventCreate(&hold.ev[e]));
    a.dist = v.d_dist; a.n = v.n; a.voff = d_voff; a.n_rec = (int32_t)rec.size(); a.thr = d_thr; a.n_thr = (int32_t)n_thr;
    a.hist = d_acc; a.diff = d_acc + n_thr;
    const int grid = (int)std::min<int64_t>((v.n + LSW_WG_VALUES - 1) / LSW_WG_VALUES, LSW_MAX_GRID);
    L_TRY(hipEventRecord(hold.ev[0], st));
    L_TRY(launch_landscape_sweep(a, grid, st));
    L_TRY(hipEventRecord(hold.ev[1], st));
    std::vector<unsigned long long> acc((size_t)(2 * n_thr));
    L_TRY(hipMemcpyAsync(acc.data(), d_acc, acc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    L_TRY(hipStreamSynchronize(st));
    int64_t below = 0, runs = 0;
    for (int64_t j = 0; j < n_thr; j++) {
        below += (int64_t)acc[(size_t)j];
        runs += (int64_t)acc[(size_t)(n_thr + j)];
        windows_below[j] = below;
        dips_below[j] = runs;
    }
    float ms = 0;
    L_TRY(hipEventElapsedTime(&ms, hold.ev[0], hold.ev[1]));
    S->sweep_ms = ms;
    S->n_launches = 1;
    return KGMA_OK;
}

int kgma_get_landscape_stats(kgma_ctx *ctx, kgma_landscape_stats *out)
{
    if (!ctx || !out) return KGMA_E_ARG;
    *out = *ctx_landscape_stats(ctx);
    return KGMA_OK;
}

}  // extern "C"
