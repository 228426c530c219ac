// kgma_landscape.hip -- reductions over the per-window distances a scan kept on the device.
//
// Both kernels read the Float64 vector of kgma_get_dists as it is: record after record, nwin - 1 values per record.  The records that
// have values come as a table voff[0 .. n_rec] of strictly increasing value offsets (voff[n_rec] = n), so a value's record is a
// binary search and a walk from one record to the next always advances.
//
// landscape_bins_kernel: minimum and first window attaining it per bin of `bin` consecutive values of a record.  A workgroup takes
//   LS_WG_VALUES consecutive values, a wave LS_WAVE_VALUES of them in stretches of LS_STRETCH (one 16-byte load per lane, all of a
//   wave's loads issued before the first is used).  The bins a workgroup touches are consecutive, so they index a table in LDS.
//   Minima are compared as 64-bit patterns (the distances are non-negative, so that is their order, and the result is the stored
//   double bit for bit; the integer forms cannot write a negative one, and gen_kernel's Float64 form writes 0.0 for a value its
//   rounding took below zero -- kgma_generic.hip).  Phase 0 folds the values into the table's minima, phase 1 the local index of every value that equals its
//   bin's minimum into the table's index (the smallest wins: the first window).  A stretch inside one record with bin >= LS_STRETCH
//   holds at most two bins, known to the whole wave: one butterfly per bin and one LDS atomic per wave in phase 0, two ballots in
//   phase 1.  Every other stretch (short bins, record boundaries) goes lane by lane with one LDS atomic per value.
//   A bin that reaches beyond the workgroup's values is left as a partial result (at most the first and the last bin of a
//   workgroup); landscape_combine_kernel folds the partial results of each such bin in order of position.
//
// landscape_sweep_kernel<NT>: for n_thr <= NT strictly increasing thresholds in LDS, r(d) = number of thresholds <= d by
//   comparisons alone.  hist[r] counts values (only r < n_thr is kept: windows_below[j] = sum hist[0 .. j]); a value with r(d) <
//   r(predecessor) starts a run for the thresholds r(d) <= j < r(predecessor): +1 at r(d), -1 at r(predecessor) (dropped at
//   n_thr, which no prefix sum reads).  A record's first value has no predecessor (rank n_thr); the predecessor of a wave's first
//   value is read from global memory.  Both arrays live in LDS per workgroup and are flushed once with 64-bit global atomic adds.
//   A stretch whose values all lie at or above the largest threshold (most of a genome) skips the searches and the atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kgma_landscape.h"

namespace kgma {

namespace {

constexpr unsigned long long LS_NONE = ~0ull;     // above every distance's bit pattern

// the record of value g (0 <= g < voff[n_rec]): the r with voff[r] <= g < voff[r + 1]
__device__ __forceinline__ int ls_rec_of(const int64_t *__restrict__ voff, int n_rec, int64_t g)
{
    int lo = 0, hi = n_rec;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (voff[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// a / b for a >= 0, b >= 1: the 32-bit division where both fit
__device__ __forceinline__ int64_t ls_div(int64_t a, int64_t b)
{
    return ((uint64_t)(a | b) >> 32) == 0 ? (int64_t)((uint32_t)a / (uint32_t)b) : a / b;
}

__device__ __forceinline__ unsigned long long ls_shfl_xor(unsigned long long v, int mask)
{
    const unsigned int lo = (unsigned int)__shfl_xor((int)(unsigned int)v, mask, 64);
    const unsigned int hi = (unsigned int)__shfl_xor((int)(unsigned int)(v >> 32), mask, 64);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long ls_wave_min(unsigned long long v)
{
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long t = ls_shfl_xor(v, m);
        v = t < v ? t : v;
    }
    return v;
}

// phase 1 of a bin the whole wave knows: e0 / e1 say whether the lane's first / second value equals the bin's minimum
__device__ __forceinline__ void ls_first_equal(bool e0, bool e1, int lane, unsigned int stretch_local, int j, int rec, unsigned int *s_idx,
                                               int *s_rec)
{
    const unsigned long long b0 = __ballot(e0), b1 = __ballot(e1);
    if ((b0 | b1) == 0) return;
    unsigned int first = 2 * LS_STRETCH;
    if (b0) first = 2u * (unsigned int)__builtin_ctzll(b0);
    if (b1) first = min(first, 2u * (unsigned int)__builtin_ctzll(b1) + 1u);
    if (lane == 0) {
        atomicMin(&s_idx[j], stretch_local + first);
        s_rec[j] = rec;
    }
}

}  // namespace

__global__ __launch_bounds__(LS_THREADS) void landscape_bins_kernel(LandscapeBinsArgs a)
{
    __shared__ unsigned long long s_min[LS_WG_VALUES];
    __shared__ unsigned int s_idx[LS_WG_VALUES];      // index of the first value at the minimum, from the workgroup's first value
    __shared__ int s_rec[LS_WG_VALUES];               // ... and its record
    __shared__ int64_t s_edge[4];                     // first bin, last bin, first bin lies inside the workgroup, last bin does
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t wg0 = (int64_t)blockIdx.x * LS_WG_VALUES;
    const int64_t wg1 = min(wg0 + (int64_t)LS_WG_VALUES, a.n);
    const int64_t gw = wg0 + (int64_t)w * LS_WAVE_VALUES;

    unsigned long long v[LS_WAVE_ITERS][2];
#pragma unroll
    for (int it = 0; it < LS_WAVE_ITERS; it++) {
        const int64_t g = gw + it * LS_STRETCH + 2 * lane;
        v[it][0] = v[it][1] = LS_NONE;
        if (g + 1 < wg1) {
            const ulonglong2 t = *reinterpret_cast<const ulonglong2 *>(a.dist + g);     // g is even: 16-byte aligned
            v[it][0] = t.x; v[it][1] = t.y;
        } else if (g < wg1) {
            v[it][0] = *reinterpret_cast<const unsigned long long *>(a.dist + g);
        }
    }
    for (int i = tid; i < LS_WG_VALUES; i += LS_THREADS) { s_min[i] = LS_NONE; s_idx[i] = ~0u; }
    if (tid == 0) {
        int c = ls_rec_of(a.voff, a.n_rec, wg0);
        int64_t q = ls_div(wg0 - a.voff[c], a.bin);
        s_edge[0] = a.boff[c] + q;
        s_edge[2] = a.voff[c] + q * a.bin == wg0 && min(wg0 + a.bin, a.voff[c + 1]) <= wg1;
        c = ls_rec_of(a.voff, a.n_rec, wg1 - 1);
        q = ls_div(wg1 - 1 - a.voff[c], a.bin);
        const int64_t bs = a.voff[c] + q * a.bin;
        s_edge[1] = a.boff[c] + q;
        s_edge[3] = bs >= wg0 && min(bs + a.bin, a.voff[c + 1]) <= wg1;
    }
    __syncthreads();
    const int64_t first_bin = s_edge[0];

    for (int phase = 0; phase < 2; phase++) {
        // wave state: record c = values [.., rend), current bin qb = values [.., be)
        int c = 0;
        int64_t rend = -1, be = 0, qb = 0;
#pragma unroll
        for (int it = 0; it < LS_WAVE_ITERS; it++) {
            const int64_t g0 = gw + it * LS_STRETCH;
            if (g0 >= wg1) break;
            const int64_t g1 = min(g0 + (int64_t)LS_STRETCH, wg1);
            if (g0 >= rend) {
                c = ls_rec_of(a.voff, a.n_rec, g0);
                const int64_t rbeg = a.voff[c];
                rend = a.voff[c + 1];
                const int64_t q = ls_div(g0 - rbeg, a.bin);
                be = min(rbeg + (q + 1) * a.bin, rend);
                qb = a.boff[c] + q;
            } else {
                while (g0 >= be) { be = min(be + a.bin, rend); qb++; }
            }
            const int64_t g = g0 + 2 * lane;
            const unsigned long long v0 = v[it][0], v1 = v[it][1];
            const unsigned int sl = (unsigned int)(g0 - wg0);
            if (a.bin >= LS_STRETCH && g1 <= rend) {
                // one record, bins qb = [.., be) and, where be < g1, qb + 1
                const int ja = (int)(qb - first_bin);
                const bool in_a0 = g < be, in_a1 = g + 1 < be, two = be < g1;
                if (phase == 0) {
                    const unsigned long long x0 = in_a0 ? v0 : LS_NONE, x1 = in_a1 ? v1 : LS_NONE;
                    const unsigned long long ma = ls_wave_min(x0 < x1 ? x0 : x1);
                    if (lane == 0) atomicMin(&s_min[ja], ma);
                    if (two) {
                        const unsigned long long y0 = in_a0 ? LS_NONE : v0, y1 = in_a1 ? LS_NONE : v1;
                        const unsigned long long mb = ls_wave_min(y0 < y1 ? y0 : y1);
                        if (lane == 0) atomicMin(&s_min[ja + 1], mb);
                    }
                } else {
                    const bool ok0 = g < g1, ok1 = g + 1 < g1;
                    const unsigned long long ma = s_min[ja];
                    ls_first_equal(ok0 && in_a0 && v0 == ma, ok1 && in_a1 && v1 == ma, lane, sl, ja, c, s_idx, s_rec);
                    if (two) {
                        const unsigned long long mb = s_min[ja + 1];
                        ls_first_equal(ok0 && !in_a0 && v0 == mb, ok1 && !in_a1 && v1 == mb, lane, sl, ja + 1, c, s_idx, s_rec);
                    }
                }
            } else {
                int cc = c;
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    const int64_t gi = g + e;
                    if (gi >= g1) continue;
                    while (a.voff[cc + 1] <= gi) cc++;
                    const int j = (int)(a.boff[cc] + ls_div(gi - a.voff[cc], a.bin) - first_bin);
                    const unsigned long long x = e ? v1 : v0;
                    if (phase == 0) {
                        atomicMin(&s_min[j], x);
                    } else if (x == s_min[j]) {
                        atomicMin(&s_idx[j], (unsigned int)(gi - wg0));
                        s_rec[j] = cc;
                    }
                }
            }
        }
        __syncthreads();
    }

    const int n_local = (int)(s_edge[1] - first_bin) + 1;
    const bool first_in = s_edge[2] != 0, last_in = s_edge[3] != 0;
    for (int j = tid; j < n_local; j += LS_THREADS) {
        const bool whole = (j > 0 || first_in) && (j < n_local - 1 || last_in);
        const unsigned long long m = s_min[j];
        const int64_t gi = wg0 + s_idx[j];
        if (whole) {
            a.bin_min[first_bin + j] = __longlong_as_double((long long)m);
            a.bin_argmin[first_bin + j] = gi - a.voff[s_rec[j]] + 2;
        } else {
            const int64_t slot = 2 * (int64_t)blockIdx.x + (j == 0 ? 0 : 1);
            a.part_val[slot] = m;
            a.part_idx[slot] = gi;
            a.part_bin[slot] = first_bin + j;
        }
    }
    if (tid == 0) {
        const bool slot0 = !(first_in && (n_local > 1 || last_in));
        const bool slot1 = n_local > 1 && !last_in;
        if (!slot0) a.part_bin[2 * (int64_t)blockIdx.x] = -1;
        if (!slot1) a.part_bin[2 * (int64_t)blockIdx.x + 1] = -1;
    }
}

// One thread per slot.  The slots of a bin follow each other in order of position, with unused slots between them; the thread of a
// bin's first slot folds the others (a later slot wins only with a smaller minimum, so the first window at the minimum stays).
__global__ __launch_bounds__(LS_THREADS) void landscape_combine_kernel(LandscapeBinsArgs a, int64_t n_slots)
{
    const int64_t i = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    if (i >= n_slots) return;
    const int64_t b = a.part_bin[i];
    if (b < 0) return;
    // (the workgroup before holds the same bin in one of its two slots if it holds it at all)
    for (int64_t k = i - 1; k >= 0 && k >= i - 2; k--) {
        const int64_t pb = a.part_bin[k];
        if (pb < 0) continue;
        if (pb == b) return;
        break;
    }
    unsigned long long m = a.part_val[i];
    int64_t gi = a.part_idx[i];
    for (int64_t k = i + 1; k < n_slots; k++) {
        const int64_t pb = a.part_bin[k];
        if (pb < 0) continue;
        if (pb != b) break;
        const unsigned long long x = a.part_val[k];
        if (x < m) { m = x; gi = a.part_idx[k]; }
    }
    a.bin_min[b] = __longlong_as_double((long long)m);
    a.bin_argmin[b] = gi - a.voff[ls_rec_of(a.voff, a.n_rec, gi)] + 2;
}

template <int NT>
__global__ __launch_bounds__(LS_THREADS) void landscape_sweep_kernel(LandscapeSweepArgs a)
{
    extern __shared__ double lsw_lds[];
    double *thr = lsw_lds;
    unsigned int *hist = reinterpret_cast<unsigned int *>(thr + NT);
    int *diff = reinterpret_cast<int *>(hist + NT);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_thr = a.n_thr;
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    for (int i = tid; i < NT; i += LS_THREADS) {
        thr[i] = i < n_thr ? a.thr[i] : inf;
        hist[i] = 0;
        diff[i] = 0;
    }
    __syncthreads();
    const double top = thr[n_thr - 1];
    // thresholds <= d: comparisons only
    auto rank = [&](double d) {
        int lo = 0;
#pragma unroll
        for (int step = NT / 2; step >= 1; step >>= 1)
            if (thr[lo + step - 1] <= d) lo += step;
        if (thr[lo] <= d) lo++;
        return min(lo, n_thr);
    };

    for (int64_t base = (int64_t)blockIdx.x * LSW_WG_VALUES; base < a.n; base += (int64_t)gridDim.x * LSW_WG_VALUES) {
        const int64_t gw = base + (int64_t)w * LSW_WAVE_VALUES;
        if (gw >= a.n) continue;
        const int64_t ge = min(gw + (int64_t)LSW_WAVE_VALUES, a.n);
        int cn = ls_rec_of(a.voff, a.n_rec, gw);                 // the next record start at or after the stretch in hand
        if (a.voff[cn] < gw) cn++;
        int carry = n_thr;                                       // rank of the value before the stretch in hand
        if (a.voff[cn] != gw) {
            const double p = a.dist[gw - 1];
            carry = p < top ? rank(p) : n_thr;
        }
        for (int it = 0; it < LSW_WAVE_ITERS; it++) {
            const int64_t g0 = gw + (int64_t)it * LS_STRETCH;
            if (g0 >= ge) break;
            const int64_t g1 = min(g0 + (int64_t)LS_STRETCH, ge);
            const int64_t g = g0 + 2 * lane;
            double d0 = inf, d1 = inf;
            if (g + 1 < g1) {
                const double2 t = *reinterpret_cast<const double2 *>(a.dist + g);
                d0 = t.x; d1 = t.y;
            } else if (g < g1) {
                d0 = a.dist[g];
            }
            bool st0 = false, st1 = false;                       // the value is the first of its record
            while (a.voff[cn] < g1) {
                const int64_t off = a.voff[cn] - g0;
                if ((off >> 1) == lane) { if (off & 1) st1 = true; else st0 = true; }
                cn++;
            }
            if (!__any(d0 < top || d1 < top)) { carry = n_thr; continue; }
            const int r0 = d0 < top ? rank(d0) : n_thr, r1 = d1 < top ? rank(d1) : n_thr;
            int p0 = __shfl_up(r1, 1, 64);
            if (lane == 0) p0 = carry;
            if (st0) p0 = n_thr;
            const int p1 = st1 ? n_thr : r0;
            carry = __shfl(r1, 63, 64);
            if (r0 < n_thr) {
                atomicAdd(&hist[r0], 1u);
                if (r0 < p0) {
                    atomicAdd(&diff[r0], 1);
                    if (p0 < n_thr) atomicSub(&diff[p0], 1);
                }
            }
            if (r1 < n_thr) {
                atomicAdd(&hist[r1], 1u);
                if (r1 < p1) {
                    atomicAdd(&diff[r1], 1);
                    if (p1 < n_thr) atomicSub(&diff[p1], 1);
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n_thr; i += LS_THREADS) {
        if (hist[i]) atomicAdd(&a.hist[i], (unsigned long long)hist[i]);
        if (diff[i]) atomicAdd(&a.diff[i], (unsigned long long)(long long)diff[i]);
    }
}

hipError_t launch_landscape_bins(const LandscapeBinsArgs &a, int64_t n_wg, hipStream_t st)
{
    if (n_wg <= 0) return hipSuccess;
    hipLaunchKernelGGL(landscape_bins_kernel, dim3((unsigned)n_wg), dim3(LS_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_landscape_combine(const LandscapeBinsArgs &a, int64_t n_wg, hipStream_t st)
{
    if (n_wg <= 0) return hipSuccess;
    const int64_t n_slots = 2 * n_wg;
    hipLaunchKernelGGL(landscape_combine_kernel, dim3((unsigned)((n_slots + LS_THREADS - 1) / LS_THREADS)), dim3(LS_THREADS), 0, st, a, n_slots);
    return hipGetLastError();
}

int landscape_sweep_slots(int32_t n_thr) { return n_thr <= 64 ? 64 : n_thr <= 512 ? 512 : 4096; }

hipError_t launch_landscape_sweep(const LandscapeSweepArgs &a, int grid, hipStream_t st)
{
    if (a.n <= 0 || grid <= 0) return hipSuccess;
    const int slots = landscape_sweep_slots(a.n_thr);
    auto fn = slots == 64 ? &landscape_sweep_kernel<64> : slots == 512 ? &landscape_sweep_kernel<512> : &landscape_sweep_kernel<4096>;
    const size_t lds = (size_t)slots * (sizeof(double) + sizeof(unsigned int) + sizeof(int));
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(LS_THREADS), lds, st, a);
    return hipGetLastError();
}

}  // namespace kgma
