// kgma_kmat.hip -- all-pairs k-mer distances (kgma_kmer_dist_matrix, kgma_kmer_nearest and their _ranges forms).
//
// D(a, b) = sum_x (c_a[x] - c_b[x])^2 with c_s = kmer_count(s, k) (src/Kmers.jl:14-28), an exact integer; dist = RN(1/2k) * D is
// kmer_dist(a, b, k) (src/Kmers.jl:54-56) bit for bit.  The kernels rest on
//     D = |c_a|^2 + |c_b|^2 - 2 * sum_p c_b[x_p],        p over the k-mer positions of a, x_p the k-mer at p:
// the dot product is a sum of table lookups along a, and so is |c_s|^2 = sum_p c_s[x_p] along s itself.  No count vector is ever
// walked bin by bin.
//
//   kmat_norm_kernel<SRC, LDS_TABLE>      na[a] = |c_a|^2: one workgroup per sequence of A in turn builds its table, sums its own
//                                         lookups and clears the table by walking the k-mers again.  It is also where every
//                                         residue of A is looked up (bad[0]).
//   kmat_kernel<SRC, LDS_TABLE, T>        a workgroup builds the tables of a tile of T sequences of B (every residue of B is
//                                         looked up there: bad[1]), sums |c_b|^2 the same way, and its waves then take the rows of
//                                         its chunk of A in turn: a lane forms the k-mer of positions lane, lane + 64, ... once and
//                                         looks it up in all T tables; T accumulators, one wave reduction, T consecutive int32 out.
//   kmat_select_kernel                    one wave per row: n_near rounds of a wave-wide minimum over the keys D << 32 | index
//                                         above the previous round's key.  Deterministic, no sorting.
// LDS_TABLE (k <= 7): 16-bit counters, two to a dword, incremented by a 32-bit LDS atomic of 1 << 16 * (x & 1) -- a sequence has
// at most 32767 k-mers, so no carry crosses the halves.  Otherwise (k = 8, 9, 10) T = 1 and the table is 4^k 32-bit counters of a
// per-workgroup global scratch, written and read at agent scope and left all-zero, after kdist_kernel<false>.
// SRC says where A's residues lie, as in kgma_assign.hip: a range of a record of the resident text, or a run of an uploaded buffer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kgma_device.h"

namespace kgma {

namespace {

constexpr int KM_THREADS = KGMA_KMAT_THREADS;
constexpr int KM_WAVES = KM_THREADS / 64;

__device__ __forceinline__ int km_code(uint32_t c)
{
    c &= 0xDFu;                                   // fold case
    return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : (c == 'T' || c == 'N') ? 3 : -1;
}

struct RangeSource {      // sequence i of A: residues lo .. lo + n - 1 (1-based) of record contig[i] of the resident text
    static __device__ __forceinline__ const uint8_t *text(const KmatArgs &a, int64_t i)
    {
        return a.text + a.cd[a.q_contig[i]].ascii_off + (a.q_pos[i] - 1);
    }
};
struct SeqSource {        // sequence i of A: n bytes at offset q_pos[i] of the uploaded sequences
    static __device__ __forceinline__ const uint8_t *text(const KmatArgs &a, int64_t i) { return a.text + a.q_pos[i]; }
};

// One sequence's counters.  LDS: counter x is half (x & 1) of dword x >> 1; global: dword x, always touched at agent scope.
template <bool LDS_TABLE>
struct Table {
    uint32_t *t;
    __device__ __forceinline__ void add(uint32_t x) const
    {
        if (LDS_TABLE) atomicAdd(&t[x >> 1], 1u << (16 * (x & 1)));
        else __hip_atomic_fetch_add(&t[x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ uint32_t get(uint32_t x) const
    {
        if (LDS_TABLE) return (t[x >> 1] >> (16 * (x & 1))) & 0xFFFFu;
        return __hip_atomic_load(&t[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void clear(uint32_t x) const
    {
        if (LDS_TABLE) t[x >> 1] = 0;             // (both halves: every k-mer of the sequence is walked, so both get there anyway)
        else __hip_atomic_store(&t[x], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
template <bool LDS_TABLE>
__device__ __forceinline__ uint32_t table_words(int k) { return LDS_TABLE ? 1u << (2 * k - 1) : 1u << (2 * k); }

// The k-mer at residues pos .. pos + k - 1, first base most significant; a bad residue (reported elsewhere) counts as T
__device__ __forceinline__ uint32_t kmer_at(const uint8_t *__restrict__ p, int pos, int k)
{
    uint32_t v = 0;
    for (int t = 0; t < k; t++) {
        const int c = km_code(p[pos + t]);
        v = (v << 2) | (uint32_t)(c < 0 ? 3 : c);
    }
    return v;
}

// every residue is looked up (kmer_count runs Nt_bits over eachindex(str), also below k residues)
__device__ __forceinline__ void check_residues(const uint8_t *__restrict__ p, int n, int tid, unsigned long long *slot, int64_t seq)
{
    for (int i = tid; i < n; i += KM_THREADS)
        if (km_code(p[i]) < 0) atomicMin(slot, ((unsigned long long)seq << 16) | (unsigned long long)i);
}

template <bool LDS_TABLE>
__device__ __forceinline__ void count_kmers(const Table<LDS_TABLE> tab, const uint8_t *__restrict__ p, int n, int k, int tid)
{
    for (int pos = tid; pos + k <= n; pos += KM_THREADS) tab.add(kmer_at(p, pos, k));
}
template <bool LDS_TABLE>
__device__ __forceinline__ void clear_kmers(const Table<LDS_TABLE> tab, const uint8_t *__restrict__ p, int n, int k, int tid)
{
    for (int pos = tid; pos + k <= n; pos += KM_THREADS) tab.clear(kmer_at(p, pos, k));
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

// The wave's totals of T accumulators: every step halves the accumulators a lane still carries (the half it keeps is chosen by
// one bit of its lane number, the other half goes to its partner), so T - 1 shuffles do the work of 6 T.  Returns in every lane
// the total of accumulator lane / (64 / T).
template <int T>
__device__ __forceinline__ uint32_t reduce_tile(uint32_t (&acc)[T], int lane)
{
    int d = 32;
#pragma unroll
    for (int n = T; n > 1; n >>= 1, d >>= 1) {
        const bool up = (lane & d) != 0;
#pragma unroll
        for (int i = 0; i < n / 2; i++) {
            const uint32_t send = up ? acc[i] : acc[i + n / 2], keep = up ? acc[i + n / 2] : acc[i];
            acc[i] = keep + (uint32_t)__shfl_xor((int)send, d, 64);
        }
    }
    uint32_t v = acc[0];
#pragma unroll
    for (; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

}  // namespace

template <class SRC, bool LDS_TABLE>
__global__ __launch_bounds__(KM_THREADS) void kmat_norm_kernel(const KmatArgs a)
{
    extern __shared__ uint32_t km_lds[];
    __shared__ uint32_t part[KM_WAVES];
    const int tid = threadIdx.x, k = a.k;
    const uint32_t tw = table_words<LDS_TABLE>(k);
    const Table<LDS_TABLE> tab{LDS_TABLE ? km_lds : a.scratch + (size_t)blockIdx.x * tw};
    if (LDS_TABLE) {
        for (uint32_t x = tid; x < tw; x += KM_THREADS) tab.t[x] = 0;
        __syncthreads();
    }
    for (int64_t s = blockIdx.x; s < a.n_a; s += gridDim.x) {
        const uint8_t *p = SRC::text(a, s);
        const int n = a.q_n[s];
        check_residues(p, n, tid, a.bad + 0, s);
        count_kmers(tab, p, n, k, tid);
        __syncthreads();
        uint32_t acc = 0;                         // the whole sum is at most 32767^2 < 2^30
        for (int pos = tid; pos + k <= n; pos += KM_THREADS) acc += tab.get(kmer_at(p, pos, k));
        acc = wave_sum(acc);
        if ((tid & 63) == 0) part[tid >> 6] = acc;
        __syncthreads();                          // every lookup is done: the table may be cleared
        if (tid == 0) {
            uint32_t tot = 0;
            for (int w = 0; w < KM_WAVES; w++) tot += part[w];
            a.na[s] = tot;
        }
        clear_kmers(tab, p, n, k, tid);
        __syncthreads();                          // table all-zero (and `part` free) before the next sequence
    }
}

// grid: x -- tiles of T sequences of B, taken in turn; y -- chunks of rows_per_chunk rows of A
template <class SRC, bool LDS_TABLE, int T>
__global__ __launch_bounds__(KM_THREADS) void kmat_kernel(const KmatArgs a)
{
    static_assert(LDS_TABLE || T == 1, "the global form holds one table per workgroup");
    extern __shared__ uint32_t km_lds[];
    __shared__ uint32_t nb2[T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = a.k;
    const uint32_t tw = table_words<LDS_TABLE>(k);
    uint32_t *const base = LDS_TABLE ? km_lds : a.scratch + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * tw;
    const int64_t row0 = (int64_t)blockIdx.y * a.rows_per_chunk;
    const int64_t row1 = row0 + a.rows_per_chunk < a.n_a ? row0 + a.rows_per_chunk : a.n_a;
    const int n_tiles = (a.n_b + T - 1) / T;
    if (LDS_TABLE) {
        for (uint32_t x = tid; x < T * tw; x += KM_THREADS) base[x] = 0;
        __syncthreads();
    }
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int b0 = tile * T, nt = a.n_b - b0 < T ? a.n_b - b0 : T;
        for (int t = 0; t < nt; t++) {
            const int64_t o = a.b_off[b0 + t];
            const int n = (int)(a.b_off[b0 + t + 1] - o);
            if (blockIdx.y == 0) check_residues(a.b_text + o, n, tid, a.bad + 1, b0 + t);
            count_kmers(Table<LDS_TABLE>{base + t * tw}, a.b_text + o, n, k, tid);
        }
        __syncthreads();
        for (int t = wave; t < nt; t += KM_WAVES) {               // |c_b|^2, a wave per sequence of the tile
            const int64_t o = a.b_off[b0 + t];
            const int n = (int)(a.b_off[b0 + t + 1] - o);
            const Table<LDS_TABLE> tab{base + t * tw};
            uint32_t acc = 0;
            for (int pos = lane; pos + k <= n; pos += 64) acc += tab.get(kmer_at(a.b_text + o, pos, k));
            acc = wave_sum(acc);
            if (lane == 0) nb2[t] = acc;
        }
        __syncthreads();
        for (int64_t row = row0 + wave; row < row1; row += KM_WAVES) {
            const uint8_t *p = SRC::text(a, row);
            const int n = a.q_n[row];
            uint32_t acc[T];
#pragma unroll
            for (int t = 0; t < T; t++) acc[t] = 0;
            for (int pos = lane; pos + k <= n; pos += 64) {
                const uint32_t x = kmer_at(p, pos, k);
#pragma unroll
                for (int t = 0; t < T; t++) acc[t] += Table<LDS_TABLE>{base + t * tw}.get(x);   // (tables past nt are all-zero)
            }
            const uint32_t dot = reduce_tile<T>(acc, lane);
            const int t = lane / (64 / T);
            if (lane % (64 / T) == 0 && t < nt) {
                const int64_t D = (int64_t)a.na[row] + (int64_t)nb2[t] - 2 * (int64_t)dot;
                const int64_t at = row * a.n_b + b0 + t;
                a.D[at] = (int32_t)D;
                if (a.dist) a.dist[at] = a.half_inv_k * (double)D;
            }
        }
        __syncthreads();                          // every row is done: the tables may be cleared
        for (int t = 0; t < nt; t++) {
            const int64_t o = a.b_off[b0 + t];
            clear_kmers(Table<LDS_TABLE>{base + t * tw}, a.b_text + o, (int)(a.b_off[b0 + t + 1] - o), k, tid);
        }
        __syncthreads();                          // tables all-zero (and nb2 free) before the next tile
    }
}

__global__ __launch_bounds__(KM_THREADS) void kmat_select_kernel(const KmatArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * KM_WAVES + (threadIdx.x >> 6);
    if (row >= a.n_a) return;
    const int32_t *__restrict__ d = a.D + row * a.n_b;
    long long prev = -1;                          // keys are not negative: 0 <= D < 2^31
    for (int r = 0; r < a.n_near; r++) {          // n_near <= n_b: every round finds a key
        long long best = 0x7FFFFFFFFFFFFFFFll;
        for (int j = lane; j < a.n_b; j += 64) {
            const long long key = ((long long)d[j] << 32) | (long long)j;
            if (key > prev && key < best) best = key;
        }
        for (int s = 32; s >= 1; s >>= 1) {
            const long long o = __shfl_xor(best, s, 64);
            best = o < best ? o : best;
        }
        if (lane == 0) {
            if (a.near_index) a.near_index[row * a.n_near + r] = (int32_t)(best & 0xFFFFFFFFll);
            if (a.near_D) a.near_D[row * a.n_near + r] = (int32_t)(best >> 32);
        }
        prev = best;
    }
}

// k >= 8: workgroups of a launch at most (= rows of the scratch, <= 512 MiB as kdist_grid's)
int kmat_scratch_rows(int k) { return k <= 7 ? 0 : k == 8 ? 512 : k == 9 ? 256 : 128; }

template <class K>
static hipError_t launch_with_lds(K kern, dim3 grid, size_t lds, hipStream_t st, const KmatArgs &a)
{
    if (lds) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, grid, dim3(KM_THREADS), lds, st, a);
    return hipGetLastError();
}

template <class SRC>
static hipError_t launch_kmat_norm_src(const KmatArgs &a, int grid, hipStream_t st)
{
    if (a.k <= 7) return launch_with_lds(&kmat_norm_kernel<SRC, true>, dim3((unsigned)grid), (size_t)2 << (2 * a.k), st, a);
    return launch_with_lds(&kmat_norm_kernel<SRC, false>, dim3((unsigned)grid), 0, st, a);
}

hipError_t launch_kmat_norm(const KmatArgs &a, int source, int grid, hipStream_t st)
{
    if (grid <= 0) return hipSuccess;
    return source == 0 ? launch_kmat_norm_src<RangeSource>(a, grid, st) : launch_kmat_norm_src<SeqSource>(a, grid, st);
}

template <class SRC>
static hipError_t launch_kmat_src(const KmatArgs &a, dim3 grid, hipStream_t st)
{
    const size_t lds = ((size_t)2 << (2 * a.k)) * (size_t)kmat_tile(a.k);
    switch (kmat_tile(a.k)) {
    case 16: return launch_with_lds(&kmat_kernel<SRC, true, 16>, grid, lds, st, a);
    case 8: return launch_with_lds(&kmat_kernel<SRC, true, 8>, grid, lds, st, a);
    case 4: return launch_with_lds(&kmat_kernel<SRC, true, 4>, grid, lds, st, a);
    default: return launch_with_lds(&kmat_kernel<SRC, false, 1>, grid, 0, st, a);
    }
}

hipError_t launch_kmat(const KmatArgs &a, int source, int grid_x, int grid_y, hipStream_t st)
{
    if (grid_x <= 0 || grid_y <= 0) return hipSuccess;
    const dim3 grid((unsigned)grid_x, (unsigned)grid_y);
    return source == 0 ? launch_kmat_src<RangeSource>(a, grid, st) : launch_kmat_src<SeqSource>(a, grid, st);
}

hipError_t launch_kmat_select(const KmatArgs &a, hipStream_t st)
{
    if (a.n_a <= 0) return hipSuccess;
    hipLaunchKernelGGL(kmat_select_kernel, dim3((unsigned)((a.n_a + KM_WAVES - 1) / KM_WAVES)), dim3(KM_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace kgma
