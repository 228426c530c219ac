// kgma_pwm.hip -- position-weight-matrix search over the resident genome (pwmMatch; semantics: include/kgma.h): every start s of
// every record at which score(s) = sum_i W[i][t[s + i]] reaches the matrix's threshold, a genome N scoring its row's minimum.
//
//   pwm_kernel   a workgroup owns PW_WG_STARTS consecutive starts of one record; no workgroup spans two records (per-record
//                prefix of workgroup counts, binary search per workgroup, as kgma_approx.hip).  It loads the residues of its
//                starts and the PW_TAIL behind them from the residue text (1 byte per base, N kept) with 16-byte loads,
//                contiguous over the lanes, and keeps them in LDS as PAIR CODES: byte r holds class(t[r]) + 8 * class(t[r + 1]),
//                the index of a pair table.  Then it loops over the matrices of the batch with the text in LDS.  The host has
//                taken the constant rows out and folded every other row with the row behind it into a table of 64 sums
//                (kgma_pwm.h), which the workgroup copies to LDS; a start's score is n_pairs times one byte read (the pair
//                code at s + col[p]) and one table read.  The lanes of a wave take consecutive starts, so the byte reads of a
//                wave fall into 16 or 17 consecutive dwords (no bank conflict), and the table reads go to the at most 25 entries
//                two residues can select, the 16 of two bases in 16 different banks.  A wave scores PW_GROUP starts per lane with
//                the pair loop outside: a pair's column is fetched once, the reads of the group differ by constant offsets.
//                Starts behind the record's last possible one (s + m - 1 > L) are scored on whatever the tail holds and dropped.
//
// Emission is that of the other searches: ballot, wave prefix, one atomicAdd per wave on a cursor that keeps counting past the
// buffer's capacity (the host regrows and runs again).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kgma_pwm.h"

namespace kgma {

namespace {

constexpr int TEXT_BYTES = PW_WG_STARTS + PW_TAIL;
constexpr int TEXT_DWORDS = TEXT_BYTES / 4;
constexpr int N_CHUNKS = TEXT_BYTES / 16;
constexpr int PW_GROUP = 16;                                       // starts a lane scores at once
constexpr int GROUP_STARTS = 64 * PW_GROUP;
constexpr uint32_t NO_RESIDUE4 = 0x01010101u * AP_NO_RESIDUE;
static_assert(PW_WAVE_STARTS % GROUP_STARTS == 0, "whole groups");

// record of workgroup w: the c with prefix[c] <= w < prefix[c + 1]
__device__ __forceinline__ int wg_record(const int64_t *__restrict__ prefix, int n, int64_t w)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= w) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// four residues -> four classes: (b >> 1) & 7
__device__ __forceinline__ uint32_t classes(uint32_t x) { return (x >> 1) & 0x07070707u; }

// the lanes with `ok` append one hit each: one atomicAdd per wave
__device__ __forceinline__ void emit(bool ok, const PwmArgs &a, int matrix, int contig, int64_t start1, int score)
{
    const uint64_t B = __ballot(ok);
    if (B == 0) return;
    const int lane = (int)(threadIdx.x & 63u);
    const int leader = __builtin_ctzll(B);
    const unsigned rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(B >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)B, 0u));
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(&a.ctl[0], (unsigned long long)__builtin_popcountll(B));
    const uint32_t blo = (uint32_t)__shfl((int)(uint32_t)base, leader), bhi = (uint32_t)__shfl((int)(uint32_t)(base >> 32), leader);
    const unsigned long long slot = (((unsigned long long)bhi << 32) | blo) + rank;
    if (ok && slot < a.cap) {
        PwmHit h;
        h.matrix = matrix; h.contig = contig; h.start = start1; h.score = score; h.reserved = 0;
        a.out[slot] = h;
    }
}

}  // namespace

__global__ __launch_bounds__(PW_THREADS) void pwm_kernel(const PwmArgs a)
{
    __shared__ uint32_t s_cls[TEXT_DWORDS + 1];                                // classes, then one dword for the look-ahead
    __shared__ uint32_t s_code[TEXT_DWORDS];                                   // pair codes
    __shared__ int32_t s_tab[PW_MAX_PAIRS * PW_PAIR_ENTRIES];
    __shared__ int s_col[PW_MAX_PAIRS + 1];                                    // the first row of each pair, then 0
    const int tid = (int)threadIdx.x;
    const int64_t wg = (int64_t)blockIdx.x;
    const int c = wg_record(a.wg_prefix, a.n_contigs, wg);
    const ContigDesc d = a.cd[c];
    const int64_t wg_first = (wg - a.wg_prefix[c]) * (int64_t)PW_WG_STARTS;    // 0-based in the record
    const uint8_t *__restrict__ text = a.ascii + d.ascii_off;

    // ---- the text of the workgroup: residues wg_first .. wg_first + TEXT_BYTES - 1 as classes, then as pair codes -------------
    // (a record's slot of the text is 32-aligned and ends >= 32 bytes behind its last residue: a 16-byte load that begins on a
    //  residue stays inside it; what it brings from behind the last residue is 3 bits like any class and no valid start reads it)
    for (int i = tid; i < N_CHUNKS; i += PW_THREADS) {
        const int64_t r = wg_first + 16ll * i;
        uint4 v = make_uint4(NO_RESIDUE4, NO_RESIDUE4, NO_RESIDUE4, NO_RESIDUE4);
        if (r < d.len) v = *reinterpret_cast<const uint4 *>(text + r);
        uint32_t *dst = s_cls + 4 * i;
        dst[0] = classes(v.x); dst[1] = classes(v.y); dst[2] = classes(v.z); dst[3] = classes(v.w);
    }
    if (tid == 0) s_cls[TEXT_DWORDS] = 0;
    __syncthreads();
    for (int i = tid; i < TEXT_DWORDS; i += PW_THREADS) {
        const uint32_t x = s_cls[i], y = s_cls[i + 1];
        s_code[i] = x | (((x >> 8) | (y << 24)) << 3);                         // (classes are < 8: no carry between the bytes)
    }

    const int wave = tid >> 6, lane = tid & 63;
    const uint8_t *__restrict__ code = reinterpret_cast<const uint8_t *>(s_code) + lane;

    for (int qi = 0; qi < a.n_matrices; qi++) {
        const PwmMatrix *__restrict__ M = a.matrices + qi;
        const int n_pairs = min(__builtin_amdgcn_readfirstlane(M->n_pairs), PW_MAX_PAIRS), thr = __builtin_amdgcn_readfirstlane(M->thr);
        const int konst = __builtin_amdgcn_readfirstlane(M->konst), id = __builtin_amdgcn_readfirstlane(M->id);
        // starts 0 .. n_valid - 1 of the record exist; n_here of them are the workgroup's
        const int64_t n_valid = d.len - __builtin_amdgcn_readfirstlane(M->rows) + 1 - wg_first;
        const int n_here = n_valid <= 0 ? 0 : n_valid >= PW_WG_STARTS ? PW_WG_STARTS : (int)n_valid;
        __syncthreads();                                                       // (the codes are there; the last matrix's table is read)
        for (int i = tid; i < n_pairs * PW_PAIR_ENTRIES; i += PW_THREADS) s_tab[i] = a.tables[M->tab_off + i];
        if (tid <= PW_MAX_PAIRS) s_col[tid] = tid < n_pairs ? (int)M->col[tid] & (PW_MAX_ROWS - 1) : 0;
        __syncthreads();
#pragma unroll 1
        for (int g = 0; g < PW_WAVE_STARTS / GROUP_STARTS; g++) {
            const int group_first = wave * PW_WAVE_STARTS + g * GROUP_STARTS;  // in the workgroup
            if (group_first >= n_here) break;                                  // (wave-uniform)
            const uint8_t *__restrict__ mine = code + group_first;
            int acc[PW_GROUP];
#pragma unroll
            for (int j = 0; j < PW_GROUP; j++) acc[j] = 0;
            int col = __builtin_amdgcn_readfirstlane(s_col[0]);
            for (int p = 0; p < n_pairs; p++) {
                const uint8_t *__restrict__ at = mine + col;
                const int32_t *__restrict__ tab = s_tab + p * PW_PAIR_ENTRIES;
                const int next = s_col[p + 1];                                 // (read ahead: its latency hides behind this pair's reads)
                uint32_t e[PW_GROUP];
                int v[PW_GROUP];
#pragma unroll
                for (int j = 0; j < PW_GROUP; j++) e[j] = at[64 * j];
#pragma unroll
                for (int j = 0; j < PW_GROUP; j++) v[j] = tab[e[j]];
#pragma unroll
                for (int j = 0; j < PW_GROUP; j++) acc[j] += v[j];
                col = __builtin_amdgcn_readfirstlane(next);
            }
            const int lane_first = group_first + lane;
            bool any = false;
#pragma unroll
            for (int j = 0; j < PW_GROUP; j++) any |= acc[j] >= thr && lane_first + 64 * j < n_here;
            if (__ballot(any) == 0) continue;
            // ---- some lane of the wave has a hit among these -----------------------------------------------------------------
#pragma unroll
            for (int j = 0; j < PW_GROUP; j++)
                emit(acc[j] >= thr && lane_first + 64 * j < n_here, a, id, c, wg_first + (lane_first + 64 * j) + 1, acc[j] + konst);
        }
    }
}

hipError_t launch_pwm(const PwmArgs &a, int64_t n_wg, hipStream_t st)
{
    if (n_wg < 1) return hipSuccess;
    if (n_wg > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pwm_kernel, dim3((unsigned)n_wg), dim3(PW_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace kgma
