// kgma_calib.hip -- distance of chosen windows of a resident genome (kgma_window_dists) and of mutated copies of host
// sequences that are never materialised (kgma_mutation_dists): the device half of threshold calibration, the working
// form of src/DistanceTesting.jl (estimate_optimal_threshold with the genome's own windows, mutate_seq, gen_sub_vs_ref).
//
// One ITEM is one run of residues: a window of W residues of a record, or one (sequence, rate, trial) copy of a host
// sequence whose residue j is substituted by a counter-based hash (below), so the copy exists only as the codes a lane
// forms in its registers.  One counting-and-distance body serves both, templated on where the residues come from.
// A workgroup takes an item at a time, persistent over a grid-stride loop.  The 4^k 32-bit counters live in LDS for
// k <= 7 and in a per-workgroup global table for k = 8 ... 10, kept all-zero between items as kdist_kernel keeps its
// scratch (agent-scope atomics; what is counted is cleared before the next item).
//
// Integer form (S/N KFV): D = sum_x (S[x] - N c[x])^2 = sumS2 - 2 N sum_j S[x_j] + N^2 sum_j c[x_j], j over the item's
//   k-mer positions (sum_j c[x_j] = sum_x c[x]^2, sum_j S[x_j] = sum_x S[x] c[x]).  Three passes over the POSITIONS,
//   none over the 4^k bins: count (one atomic add per k-mer), sum, clear.  Exact int64 (kgma_set_refs guarantees
//   sumS2 + N^2 n^2 < 2^61, which bounds every term: 2 N S c <= S^2 + N^2 c^2).  dist = (double)D / scale.
// Float64 form (any KFV): dist = (1 / 2k) * sum_x (ref[x] - c[x])^2 by a dense pass over the bins as kdist_kernel
//   MODE 0, in ONE fixed order: lane t of the 256 sums the bins t, t + 256, ... of the DEVICE index order (first base
//   least significant) in increasing order, the 64 lanes of a wave are combined by a shuffle tree (distances 32, 16,
//   ... 1), the four waves in wave order, and the total is multiplied by RN(1 / 2k).  The pass clears what it reads.
// Strobemer form (strobe_calib_kernel, below calib_kernel): the integer form over randstrobe bins, for the strobemer engine's
//   reference (kgma_strobe_window_dists, kgma_strobe_mutation_dists).
//
// Mutation rule (kgma.h, kgma_mutation_dists): mix64 is the splitmix64 finaliser, G = 0x9E3779B97F4A7C15,
//   K = mix64(mix64(mix64(seed + G (i + 1)) + G (r + 1)) + G (t + 1)) for sequence i, rate r, trial t;
//   z = mix64(K + G (j + 1)) for residue j (0-based); substituted iff (z >> 11) < P[r] = floor(rate 2^53);
//   new base = MUT[b][((z & 0x7FF) * 3) >> 11], MUT in the order of mutation_dict (src/DistanceTesting.jl:38-42).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "kgma_device.h"
#include "kgma_strobe_bin.h"

namespace kgma {

namespace {

constexpr int CB_THREADS = 256;
constexpr uint64_t CB_G = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// a window of a resident genome: residues through the reference's code table (Consts.jl:22-28: A0 C1 G2 T3 N3, either case)
struct WindowSource {
    const uint8_t *p;
    int64_t len;
    int64_t bad_base;                             // what first_bad reports for residue 0: its byte offset in the residue text
    __device__ __forceinline__ WindowSource(const CalibArgs &a, int64_t item)
    {
        const int64_t o = a.item_off[item];
        p = a.text + o; len = a.W; bad_base = o;
    }
    __device__ __forceinline__ int code(int64_t j) const
    {
        const uint32_t c = p[j] & 0xDFu;
        return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : (c == 'T' || c == 'N') ? 3 : -1;
    }
};

// trial t at rate r of host sequence i, item = (i * n_rates + r) * n_trials + t: A/C/G/T only (mutation_dict has no other key)
struct MutationSource {
    const uint8_t *p;
    int64_t len;
    int64_t bad_base;                             // byte offset of residue 0 in the uploaded sequences
    uint64_t K, P;
    __device__ __forceinline__ MutationSource(const CalibArgs &a, int64_t item)
    {
        const int64_t t = item % a.n_trials, ir = item / a.n_trials;
        const int64_t r = ir % a.n_rates, i = ir / a.n_rates;
        const int64_t o = a.item_off[i];
        p = a.text + o; len = a.item_off[i + 1] - o; bad_base = o;
        K = mix64(mix64(mix64(a.seed + CB_G * (uint64_t)(i + 1)) + CB_G * (uint64_t)(r + 1)) + CB_G * (uint64_t)(t + 1));
        P = a.P[r];
    }
    __device__ __forceinline__ int code(int64_t j) const
    {
        const uint32_t c = p[j] & 0xDFu;
        const int b = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
        if (b < 0) return -1;
        const uint64_t z = mix64(K + CB_G * (uint64_t)(j + 1));
        if ((z >> 11) >= P) return b;
        // A -> C G T, C -> A G T, G -> C A T, T -> C G A as 2-bit codes, three per byte-wide row
        const uint32_t row = b == 0 ? 0x39u : b == 1 ? 0x38u : b == 2 ? 0x31u : 0x09u;
        return (int)((row >> (2 * (uint32_t)(((z & 0x7FFull) * 3) >> 11))) & 3u);
    }
};

__device__ __forceinline__ double wave_sum(double v)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

__device__ __forceinline__ int64_t wave_sum(int64_t v)
{
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)v, d, 64);
        const uint32_t hi = (uint32_t)__shfl_down((int)(uint32_t)((uint64_t)v >> 32), d, 64);
        v += (int64_t)(((uint64_t)hi << 32) | lo);
    }
    return v;
}

// index of the k-mer at position j in the device index order (first base least significant); a residue outside the table counts as T
template <class SRC>
__device__ __forceinline__ uint32_t kmer_at(const SRC &src, int64_t j, int k)
{
    uint32_t v = 0;
    for (int t = 0; t < k; t++) {
        const int c = src.code(j + t);
        v |= (uint32_t)(c < 0 ? 3 : c) << (2 * t);
    }
    return v;
}

}  // namespace

template <class SRC, bool LDS_TABLE, bool FP>
__global__ __launch_bounds__(CB_THREADS) void calib_kernel(const CalibArgs a)
{
    extern __shared__ uint32_t cb_lds[];
    __shared__ double wave_f[CB_THREADS / 64];
    __shared__ int64_t wave_s[CB_THREADS / 64], wave_c[CB_THREADS / 64];
    const int tid = threadIdx.x, k = a.k;
    const uint32_t nb = 1u << (2 * k);
    uint32_t *cnt = LDS_TABLE ? cb_lds : a.scratch + (size_t)blockIdx.x * nb;
    if (LDS_TABLE) {
        for (uint32_t x = tid; x < nb; x += CB_THREADS) cnt[x] = 0;
        __syncthreads();
    }
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const SRC src(a, item);
        const int64_t nk = src.len - k + 1;       // k-mer positions (<= 0: nothing is counted)
        // every residue is looked up (kmer_count runs Nt_bits over the whole sequence, also below k residues)
        for (int64_t i = tid; i < src.len; i += CB_THREADS)
            if (src.code(i) < 0) atomicMin(a.first_bad, (unsigned long long)(src.bad_base + i));
        for (int64_t j = tid; j < nk; j += CB_THREADS) {
            const uint32_t v = kmer_at(src, j, k);
            if (LDS_TABLE) atomicAdd(&cnt[v], 1u);
            else __hip_atomic_fetch_add(&cnt[v], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        if (FP) {
            const double *ref = a.R;
            double acc = 0.0;
            for (uint32_t x = tid; x < nb; x += CB_THREADS) {
                // the global table is written by atomics (at the L2): read it there too
                const uint32_t c = LDS_TABLE ? cnt[x] : __hip_atomic_load(&cnt[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const double d = ref[x] - (double)c;
                acc += d * d;
                if (LDS_TABLE) cnt[x] = 0;
                else if (c) __hip_atomic_store(&cnt[x], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            acc = wave_sum(acc);
            if ((tid & 63) == 0) wave_f[tid >> 6] = acc;
            __syncthreads();
            if (tid == 0) {
                double tot = 0.0;
                for (int w = 0; w < CB_THREADS / 64; w++) tot += wave_f[w];
                a.dist_out[item] = a.half_inv_k * tot;
            }
        } else {
            const int32_t *S = a.S;
            int64_t sS = 0, sC = 0;
            for (int64_t j = tid; j < nk; j += CB_THREADS) {
                const uint32_t v = kmer_at(src, j, k);
                const uint32_t c = LDS_TABLE ? cnt[v] : __hip_atomic_load(&cnt[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                sS += S[v];
                sC += c;
            }
            sS = wave_sum(sS); sC = wave_sum(sC);
            if ((tid & 63) == 0) { wave_s[tid >> 6] = sS; wave_c[tid >> 6] = sC; }
            __syncthreads();                      // every count has been read: the positions may be cleared
            for (int64_t j = tid; j < nk; j += CB_THREADS) {
                const uint32_t v = kmer_at(src, j, k);
                if (LDS_TABLE) cnt[v] = 0;
                else __hip_atomic_store(&cnt[v], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (tid == 0) {
                int64_t tS = 0, tC = 0;
                for (int w = 0; w < CB_THREADS / 64; w++) { tS += wave_s[w]; tC += wave_c[w]; }
                const int64_t D = a.sumS2 - 2 * a.N * tS + a.N * a.N * tC;
                a.D_out[item] = D;
                a.dist_out[item] = (double)D / a.scale;
            }
        }
        __syncthreads();                          // counters cleared (and the wave partials free) before the next item
    }
}

// The strobemer form (kgma_strobe_window_dists, kgma_strobe_mutation_dists): the integer form above with the randstrobe bin of the
// k = w_max + s - 1 residues at a position (strobe_bin, the rule strobe_kernel scans with) in the place of the k-mer, and the
// 4^(2s) 32-bit counters in LDS.  What the reference's count vector holds, read literally (kgma_strobe.hip): an item has
// n = len - k + 1 strobemers, the n - 1 at residues 0 .. n - 2 and a LAST one at residue `last` -- n - 1 for a mutated copy (all
// of the sequence's strobemers), and for a window the strobemer at residue W - k of the window's RECORD: its permanent item,
// which is the window's own last strobemer only for the record's first window.  The residues looked up are those the items read.
template <class SRC, int SS>
__global__ __launch_bounds__(CB_THREADS) void strobe_calib_kernel(const StrobeCalibArgs a)
{
    constexpr uint32_t NB = 1u << (4 * SS);
    constexpr bool WINDOW = std::is_same<SRC, WindowSource>::value;
    __shared__ uint32_t cnt[NB];
    __shared__ int64_t wave_s[CB_THREADS / 64], wave_c[CB_THREADS / 64];
    const int tid = threadIdx.x, k = a.c.k;
    const int w_min = a.w_min, w_max = a.w_max;
    const uint32_t z0 = a.zero[0], z1 = a.zero[1], z2 = a.zero[2], z3 = a.zero[3];
    for (uint32_t x = tid; x < NB; x += CB_THREADS) cnt[x] = 0;
    __syncthreads();
    for (int64_t item = blockIdx.x; item < a.c.n_items; item += gridDim.x) {
        const SRC src(a.c, item);
        const int64_t n = src.len - k + 1;        // strobemers (<= 0: nothing is counted)
        const int64_t last = WINDOW ? a.rec_off[item] + (src.len - k) - src.bad_base : n - 1;
        auto bin_at = [&](int64_t p) {
            return strobe_bin<SS>(kmer_at(src, p < n - 1 ? p : last, k), w_min, w_max, z0, z1, z2, z3);
        };
        // a mutated copy: every residue is looked up, as in calib_kernel; a window: residues 0 .. W - 2 and the permanent item's k
        for (int64_t i = tid; i < (WINDOW ? src.len - 1 : src.len); i += CB_THREADS)
            if (src.code(i) < 0) atomicMin(a.c.first_bad, (unsigned long long)(src.bad_base + i));
        if (WINDOW && tid < k && src.code(last + tid) < 0) atomicMin(a.c.first_bad, (unsigned long long)(src.bad_base + last + tid));
        for (int64_t p = tid; p < n; p += CB_THREADS) atomicAdd(&cnt[bin_at(p)], 1u);
        __syncthreads();
        const int32_t *S = a.c.S;
        int64_t sS = 0, sC = 0;
        for (int64_t p = tid; p < n; p += CB_THREADS) {
            const uint32_t v = bin_at(p);
            sS += S[v];
            sC += cnt[v];
        }
        sS = wave_sum(sS); sC = wave_sum(sC);
        if ((tid & 63) == 0) { wave_s[tid >> 6] = sS; wave_c[tid >> 6] = sC; }
        __syncthreads();                          // every count has been read: the positions may be cleared
        for (int64_t p = tid; p < n; p += CB_THREADS) cnt[bin_at(p)] = 0;
        if (tid == 0) {
            int64_t tS = 0, tC = 0;
            for (int w = 0; w < CB_THREADS / 64; w++) { tS += wave_s[w]; tC += wave_c[w]; }
            const int64_t D = a.c.sumS2 - 2 * a.c.N * tS + a.c.N * a.c.N * tC;
            a.c.D_out[item] = D;
            a.c.dist_out[item] = (double)D / a.c.scale;
        }
        __syncthreads();                          // counters cleared (and the wave partials free) before the next item
    }
}

template <class SRC>
static hipError_t launch_strobe_calib_src(const StrobeCalibArgs &a, int grid, hipStream_t st)
{
    auto fn = a.s == 1 ? &strobe_calib_kernel<SRC, 1> : a.s == 2 ? &strobe_calib_kernel<SRC, 2> : &strobe_calib_kernel<SRC, 3>;
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(CB_THREADS), 0, st, a);
    return hipGetLastError();
}

// source 0: genome windows, 1: mutated copies.  `grid` = calib_grid(1, ...): the counters are in LDS.
hipError_t launch_strobe_calib(const StrobeCalibArgs &a, int source, int grid, hipStream_t st)
{
    if (a.c.n_items <= 0) return hipSuccess;
    if (a.s < 1 || a.s > KGMA_STROBE_MAX_S || a.w_min < 1 || a.w_min > a.w_max || a.c.k != a.w_max + a.s - 1 || a.c.k > KGMA_STROBE_MAX_K ||
        grid < 1 || (source == 0 && (a.rec_off == nullptr || a.c.W <= a.c.k)))
        return hipErrorInvalidConfiguration;
    return source == 0 ? launch_strobe_calib_src<WindowSource>(a, grid, st) : launch_strobe_calib_src<MutationSource>(a, grid, st);
}

// workgroups of a launch (= rows of the global counter table when k > 7: at most 64 MiB of it)
int calib_grid(int k, int64_t n_items, int n_cus)
{
    const int64_t cap = k <= 7 ? (int64_t)n_cus * 8 : k == 8 ? 256 : k == 9 ? 64 : 16;
    return (int)(n_items < cap ? (n_items < 1 ? 1 : n_items) : cap);
}

template <class SRC>
static hipError_t launch_calib_src(const CalibArgs &a, int grid, hipStream_t st)
{
    if (a.k <= 7) {
        const size_t lds = (size_t)4 << (2 * a.k);
        auto fn = a.fp ? &calib_kernel<SRC, true, true> : &calib_kernel<SRC, true, false>;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(CB_THREADS), lds, st, a);
    } else {
        auto fn = a.fp ? &calib_kernel<SRC, false, true> : &calib_kernel<SRC, false, false>;
        hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(CB_THREADS), 0, st, a);
    }
    return hipGetLastError();
}

// source 0: genome windows, 1: mutated copies.  `grid` = calib_grid(...) (the caller sized a.scratch for it).
hipError_t launch_calib(const CalibArgs &a, int source, int grid, hipStream_t st)
{
    if (a.n_items <= 0) return hipSuccess;
    return source == 0 ? launch_calib_src<WindowSource>(a, grid, st) : launch_calib_src<MutationSource>(a, grid, st);
}

}  // namespace kgma
