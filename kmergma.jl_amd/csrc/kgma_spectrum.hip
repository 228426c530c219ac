// kgma_spectrum.hip -- k-mer counts of ranges of the resident genome (kgma_genome_kmer_count; semantics: include/kgma.h).
//
// The work is cut into units: `span` consecutive considered starts of one range (no unit spans two ranges; per-range prefix of
// unit counts, binary search per group, as kgma_pwm.hip).  A group -- a workgroup, or a wave in the `wave` form -- walks a
// contiguous chunk of units.  Per unit it loads the residues of its starts and the k - 1 behind them from the residue text (1 byte
// per base: N and case are there, which the 2-bit copies have lost) with 16-byte loads contiguous over the lanes, aligned down to
// 16 bytes (a record's slot is 32-aligned and padded: such a load stays inside it; the bytes in front of the range and behind what
// it covers are masked), and keeps them in LDS as CLASSES: base code, N, other, and a bit for lower case.  The lanes of a wave then
// take consecutive starts, read their k classes and form the k-mer value (first base most significant).
//
//   spectrum_kernel<GROUP, true>    `wg` (GROUP 256, k <= 7) and `wave` (GROUP 64, k <= 4): 4^k 32-bit counters per group in LDS,
//                                   kept while the range stays the same; when it changes and at the end of the chunk the
//                                   non-zero counters go to the range's row with no-return 64-bit atomic adds.
//   spectrum_kernel<256, false>     `global` (k >= 8; any k when forced): every start adds to the row directly.
//
// In every form a wave whose counted lanes all hold the same k-mer adds once, the lane count (ballot against the first counted
// lane's value): a homopolymer or an assembly gap is otherwise 64 serialised atomics on one address.  Skipped starts are counted by
// ballot and reach n_skipped with one atomic per wave per unit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kgma_spectrum.h"

namespace kgma {

namespace {

// range of unit u: the r with prefix[r] <= u < prefix[r + 1] (ranges without units share their prefix with the next one)
__device__ __forceinline__ int64_t unit_range(const int64_t *__restrict__ prefix, int64_t n, int64_t u)
{
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= u) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// class of one residue byte: A0 C1 G2 T3 in either case, N -> 3 | SP_N, anything else 3 | SP_OTHER; lower case adds SP_MASKED
__device__ __forceinline__ uint32_t residue_class(uint32_t b)
{
    const uint32_t lower = (b - 'a') < 26u ? 1u : 0u;
    const uint32_t i = (b & ~(lower << 5)) - 'A';                              // letter index of the folded byte
    constexpr uint32_t LETTERS = (1u << 0) | (1u << 2) | (1u << 6) | (1u << 13) | (1u << 19);   // A C G N T
    const bool known = i < 26u && ((LETTERS >> i) & 1u);
    const uint32_t c = ((i + 1) >> 1) & 3u;                                    // A 0, C 1, G 3, T 2
    uint32_t cls = c ^ (c >> 1);
    if (i == 13u) cls = 3u | SP_N;
    if (!known) cls = 3u | SP_OTHER;
    return cls | (lower ? SP_MASKED : 0u);
}

__device__ __forceinline__ int64_t imin(int64_t x, int64_t y) { return x < y ? x : y; }

template <int GROUP>
__device__ __forceinline__ void group_sync()
{
    if (GROUP == SP_THREADS) {
        __syncthreads();
    } else {                                                                   // a wave: its LDS traffic is ordered, nothing waits
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}

}  // namespace

template <int GROUP, bool TABLE>
__global__ __launch_bounds__(SP_THREADS) void spectrum_kernel(const SpectrumArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sp_lds[];
    constexpr int GROUPS = SP_THREADS / GROUP;
    const int k = a.k, span = a.span;
    const int tab_words = TABLE ? 1 << (2 * k) : 0;
    const int cls_words = (span + 32) >> 2;
    const int in_wg = (int)threadIdx.x / GROUP, tid = (int)threadIdx.x % GROUP, lane = tid & 63, wave = tid >> 6;
    uint32_t *__restrict__ tab = sp_lds + (size_t)in_wg * (size_t)(tab_words + cls_words);
    uint32_t *__restrict__ cls = tab + tab_words;
    const uint8_t *__restrict__ cls8 = reinterpret_cast<const uint8_t *>(cls);

    const int64_t group = (int64_t)blockIdx.x * GROUPS + in_wg;
    int64_t u = group * a.units_per_group;
    const int64_t u_end = imin(a.n_units, u + a.units_per_group);
    if (u >= u_end) return;                                                    // (group-uniform; a wave group meets no barrier)
    if (TABLE) {
        for (int i = tid; i < tab_words; i += GROUP) tab[i] = 0;
    }
    int64_t r = unit_range(a.unit_prefix, a.n_ranges, u);
    unsigned long long bad = ~0ull;

    while (u < u_end) {
        // ---- the units of range r that lie in the chunk ---------------------------------------------------------------------
        const int64_t first_unit = a.unit_prefix[r], r_end = imin(u_end, a.unit_prefix[r + 1]);
        const int64_t n_starts = a.r_starts[r], n_cover = a.r_cover[r], lo0 = a.r_lo[r] - 1;    // lo0: 0-based in the record
        const int32_t contig = a.r_contig[r];
        const uint8_t *__restrict__ text = a.text + a.cd[contig].ascii_off;
        unsigned long long *__restrict__ row = a.counts + ((unsigned long long)r << (2 * k));
        for (; u < r_end; u++) {
            const int64_t s0 = (u - first_unit) * (int64_t)span;               // first start of the unit, from lo
            const int n_here = (int)imin(span, n_starts - s0);        // (0: a range shorter than k)
            const int n_res = (int)imin(n_cover - s0, (int64_t)span + k - 1);
            const int64_t r0 = lo0 + s0;
            const int lead = (int)(r0 & 15);
            const uint8_t *__restrict__ src = text + (r0 - lead);
            const int n_chunks = (lead + n_res + 15) >> 4;                    // <= (15 + span + 9 + 15) / 16 <= (span + 32) / 16
            group_sync<GROUP>();                                               // (the last unit's classes have been read)
            for (int i = tid; i < n_chunks; i += GROUP) {
                const uint4 v = *reinterpret_cast<const uint4 *>(src + 16 * i);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                uint32_t o[4];
#pragma unroll
                for (int d = 0; d < 4; d++) {
                    uint32_t packed = 0;
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        const int j = 16 * i + 4 * d + b - lead;               // residue of the unit
                        uint32_t c = residue_class((w[d] >> (8 * b)) & 0xFFu);
                        if (j < 0 || j >= n_res) c = 0;
                        if (a.check_bad && (c & SP_OTHER)) {
                            const unsigned long long key = ((unsigned long long)(uint32_t)contig << SP_POS_BITS) | (unsigned long long)(r0 + j + 1);
                            bad = key < bad ? key : bad;
                        }
                        packed |= c << (8 * b);
                    }
                    o[d] = packed;
                }
                *reinterpret_cast<uint4 *>(cls + 4 * i) = make_uint4(o[0], o[1], o[2], o[3]);
            }
            group_sync<GROUP>();
            // ---- count: the lanes of a wave take consecutive starts -----------------------------------------------------------
            unsigned n_skip = 0;                                               // (wave-uniform)
            for (int base = 64 * wave; base < n_here; base += GROUP) {
                const int s = base + lane;
                const bool active = s < n_here;
                uint32_t kmer = 0, seen = 0;
                if (active) {
                    const uint8_t *__restrict__ p = cls8 + lead + s;
                    for (int i = 0; i < k; i++) {
                        const uint32_t c = p[i];
                        kmer = (kmer << 2) | (c & SP_CODE);
                        seen |= c;
                    }
                }
                const bool skip = active && (seen & a.skip_mask) != 0;
                const bool count = active && !skip;
                n_skip += (unsigned)__builtin_popcountll(__ballot(skip));
                const uint64_t B = __ballot(count);
                if (B == 0) continue;
                const int leader = __builtin_amdgcn_readfirstlane(__builtin_ctzll(B));
                const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)kmer, leader);
                const bool uniform = __ballot(count && kmer == first) == B;
                const uint32_t add = uniform ? (uint32_t)__builtin_popcountll(B) : 1u;
                if (uniform ? lane == leader : count) {
                    if (TABLE) atomicAdd(&tab[kmer], add);
                    else atomicAdd(&row[kmer], (unsigned long long)add);
                }
            }
            if (n_skip && lane == 0) atomicAdd(&a.skipped[r], (unsigned long long)n_skip);
        }
        // ---- the range ends here, or the chunk does: flush the table ----------------------------------------------------------
        if (TABLE) {
            group_sync<GROUP>();
            for (int i = tid; i < tab_words; i += GROUP) {
                const uint32_t c = tab[i];
                if (c) {
                    atomicAdd(&row[i], (unsigned long long)c);
                    tab[i] = 0;
                }
            }
            // (the next unit's first group_sync orders these stores before its adds)
        }
        while (r + 1 < a.n_ranges && a.unit_prefix[r + 1] <= u) r++;
    }
    if (bad != ~0ull) atomicMin(a.bad, bad);
}

hipError_t launch_spectrum(const SpectrumArgs &a, int form, int64_t n_workgroups, size_t lds_bytes, hipStream_t st)
{
    if (n_workgroups < 1) return hipSuccess;
    if (n_workgroups > 0x7FFFFFFFll) return hipErrorInvalidValue;
    auto fn = form == SP_FORM_WG ? &spectrum_kernel<SP_THREADS, true> : form == SP_FORM_WAVE ? &spectrum_kernel<64, true> : &spectrum_kernel<SP_THREADS, false>;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fn, dim3((unsigned)n_workgroups), dim3(SP_THREADS), lds_bytes, st, a);
    return hipGetLastError();
}

}  // namespace kgma
