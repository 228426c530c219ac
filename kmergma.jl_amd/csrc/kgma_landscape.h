// kgma_landscape.h -- what kgma_landscape.cpp (host) and kgma_landscape.hip (kernels) share, and the view the host file has of a
// context's kept distances (defined in kgma_api.cpp, which owns the struct).
#ifndef KGMA_LANDSCAPE_H
#define KGMA_LANDSCAPE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "kgma_assign.h"

namespace kgma {

// A workgroup of landscape_bins_kernel reduces LS_WG_VALUES consecutive values: LS_WAVES waves of LS_WAVE_ITERS stretches of
// LS_STRETCH values (two per lane, one 16-byte load).  A bin that reaches beyond its workgroup's values leaves a partial result;
// landscape_combine_kernel folds the partial results of every such bin.
constexpr int LS_THREADS = 256;
constexpr int LS_WAVES = LS_THREADS / 64;
constexpr int LS_STRETCH = 128;
constexpr int LS_WAVE_ITERS = 4;
constexpr int LS_WAVE_VALUES = LS_STRETCH * LS_WAVE_ITERS;
constexpr int LS_WG_VALUES = LS_WAVES * LS_WAVE_VALUES;

// landscape_sweep_kernel: a wave takes LSW_WAVE_ITERS stretches in a row, a workgroup LSW_WG_VALUES values per round
constexpr int LSW_WAVE_ITERS = 16;
constexpr int LSW_WAVE_VALUES = LS_STRETCH * LSW_WAVE_ITERS;
constexpr int LSW_WG_VALUES = LS_WAVES * LSW_WAVE_VALUES;
constexpr int LSW_MAX_GRID = 2048;

// The records that have values, as the kernels see them: record r holds values voff[r] .. voff[r + 1] (strictly increasing,
// voff[n_rec] = n) and, in landscape_bins_kernel, bins boff[r] .. boff[r + 1].
struct LandscapeBinsArgs {
    const double *dist;
    int64_t n;
    const int64_t *voff, *boff;
    int32_t n_rec;
    int64_t bin;                       // 1 .. max(n, 1)
    double *bin_min;
    int64_t *bin_argmin;               // window start within the record (1-based)
    // two slots per workgroup (its first and its last bin, where they reach beyond it): part_bin < 0 marks an unused slot
    unsigned long long *part_val;
    int64_t *part_idx, *part_bin;
};

struct LandscapeSweepArgs {
    const double *dist;
    int64_t n;
    const int64_t *voff;
    int32_t n_rec;
    const double *thr;
    int32_t n_thr;
    unsigned long long *hist, *diff;   // [n_thr] each, zeroed; diff holds signed sums
};

hipError_t launch_landscape_bins(const LandscapeBinsArgs &a, int64_t n_wg, hipStream_t st);
hipError_t launch_landscape_combine(const LandscapeBinsArgs &a, int64_t n_wg, hipStream_t st);
int landscape_sweep_slots(int32_t n_thr);                    // threshold slots of the kernel form that serves n_thr
hipError_t launch_landscape_sweep(const LandscapeSweepArgs &a, int grid, hipStream_t st);

// kgma_api.cpp: the distances the last scan kept for KFV `kfv` (device pointer, valid until the next scan) and the evaluated
// windows per record.  need_dists == false asks for the layout alone.  Returns KGMA_OK or the status the landscape calls document,
// with kgma_last_error set; `fn` names the caller there.
struct DistView {
    const double *d_dist = nullptr;
    int64_t n = 0;
    const std::vector<int64_t> *nwin = nullptr;
};
int ctx_dist_view(kgma_ctx *ctx, const char *fn, int32_t kfv, bool need_dists, DistView *view);
kgma_landscape_stats *ctx_landscape_stats(kgma_ctx *ctx);

}  // namespace kgma

#endif
