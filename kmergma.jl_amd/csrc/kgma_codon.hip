// kgma_codon.hip -- codon-weight-matrix search over the resident genome (protMatch; semantics: include/kgma.h): every nucleotide
// start s of every record at which score(s) = sum_i row_i[codon(t[s + 3i], t[s + 3i + 1], t[s + 3i + 2])] reaches the matrix's
// threshold, all three reading frames in one pass.  The kernel knows nothing of genetic codes or strands: both are in the matrix.
//
//   codon_kernel a workgroup owns CD_WG_STARTS consecutive starts of one record; no workgroup spans two records (per-record
//                prefix of workgroup counts, binary search per workgroup, as kgma_pwm.hip).  It loads the residues of its
//                starts and the CD_TAIL behind them from the residue text (1 byte per base, N kept) with 16-byte loads,
//                contiguous over the lanes, and keeps them in LDS as CODON CODES, one byte per residue position: byte r holds
//                16 b(t[r]) + 4 b(t[r + 1]) + b(t[r + 2]) (A 0, C 1, G 2, T 3), or 64 when one of the three is no base (N, or
//                behind the record's end).  Then it loops over the matrices of the batch with the codes in LDS.  The host has
//                taken the constant rows out (kgma_codon.h); the workgroup copies the tables of the others to LDS, 65 int16_t
//                entries and one of padding each, and a start's score is n_rows times one byte read (the code at s + 3 col[p])
//                and one 2-byte table read.  The lanes of a wave take consecutive starts, so the byte reads of a wave fall into
//                16 or 17 consecutive dwords (no bank conflict); the 64 codons of a table lie in 32 consecutive dwords, one
//                bank each, so lanes that read different codons read different banks or the same dword; only the ambiguous
//                entry shares codon 0's bank.  A wave scores CD_GROUP starts per lane with the row loop outside: a row's column
//                is fetched once, the reads of the group differ by constant offsets.
//                Starts behind the record's last possible one (s + 3m - 1 > L) are scored on whatever the tail holds and dropped.
//
// Emission is that of the other searches: ballot, wave prefix, one atomicAdd per wave on a cursor that keeps counting past the
// buffer's capacity (the host regrows and runs again).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kgma_codon.h"

namespace kgma {

namespace {

constexpr int TEXT_BYTES = CD_WG_STARTS + CD_TAIL;
constexpr int TEXT_DWORDS = TEXT_BYTES / 4;
constexpr int N_CHUNKS = TEXT_BYTES / 16;
constexpr int TAB_DWORDS = CD_TAB_STRIDE / 2;
constexpr int CD_GROUP = 16;                                       // starts a lane scores at once
constexpr int GROUP_STARTS = 64 * CD_GROUP;
constexpr uint32_t NO_RESIDUE4 = 0x01010101u * AP_NO_RESIDUE;
constexpr uint32_t NO_CLASS4 = 0x01010101u * ((AP_NO_RESIDUE >> 1) & 7);
static_assert(CD_WAVE_STARTS % GROUP_STARTS == 0, "whole groups");
// the last code byte a start of the workgroup reads, and the last residue that code is made of, are staged
static_assert(CD_WG_STARTS - 1 + 3 * (CD_MAX_ROWS - 1) + 2 < TEXT_BYTES, "the staged text holds every codon of the longest matrix");

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

// four residues -> four classes: (b >> 1) & 7 (A 0, C 1, T 2, G 3, N 7, no residue 4)
__device__ __forceinline__ uint32_t classes(uint32_t x) { return (x >> 1) & 0x07070707u; }
// four classes -> four base codes A 0, C 1, G 2, T 3 (meaningless where the class is no base)
__device__ __forceinline__ uint32_t bases(uint32_t c) { return (c ^ (c >> 1)) & 0x03030303u; }

// the lanes with `ok` append one hit each: one atomicAdd per wave
__device__ __forceinline__ void emit(bool ok, const CodonArgs &a, int matrix, int contig, int64_t start1, int score)
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
        CodonHit h;
        h.matrix = matrix; h.contig = contig; h.start = start1; h.score = score; h.reserved = 0;
        a.out[slot] = h;
    }
}

}  // namespace

__global__ __launch_bounds__(CD_THREADS) void codon_kernel(const CodonArgs a)
{
    __shared__ uint32_t s_code[TEXT_DWORDS];                                   // codon codes
    __shared__ uint32_t s_tab32[CD_MAX_ROWS * TAB_DWORDS];                     // the tables: int16_t entries, copied as dwords
    const int16_t *s_tab = reinterpret_cast<const int16_t *>(s_tab32);
    // the classes, then one dword for the look-ahead: they live where the tables will (the barrier in front of the first
    // matrix's copy lies behind their last read)
    uint32_t *s_cls = s_tab32;
    static_assert(TEXT_DWORDS + 1 <= CD_MAX_ROWS * TAB_DWORDS, "the classes fit the tables' room");
    __shared__ int s_col[CD_MAX_ROWS + 1];                                     // the row of each table, then 0
    const int tid = (int)threadIdx.x;
    const int64_t wg = (int64_t)blockIdx.x;
    const int c = wg_record(a.wg_prefix, a.n_contigs, wg);
    const ContigDesc d = a.cd[c];
    const int64_t wg_first = (wg - a.wg_prefix[c]) * (int64_t)CD_WG_STARTS;    // 0-based in the record
    const uint8_t *__restrict__ text = a.ascii + d.ascii_off;

    // ---- the text of the workgroup: residues wg_first .. wg_first + TEXT_BYTES - 1 as classes, then as codon codes ------------
    // (a record's slot of the text is 32-aligned and ends >= 32 bytes behind its last residue: a 16-byte load that begins on a
    //  residue stays inside it; what it brings from behind the last residue is 3 bits like any class and no valid start reads it)
    for (int i = tid; i < N_CHUNKS; i += CD_THREADS) {
        const int64_t r = wg_first + 16ll * i;
        uint4 v = make_uint4(NO_RESIDUE4, NO_RESIDUE4, NO_RESIDUE4, NO_RESIDUE4);
        if (r < d.len) v = *reinterpret_cast<const uint4 *>(text + r);
        uint32_t *dst = s_cls + 4 * i;
        dst[0] = classes(v.x); dst[1] = classes(v.y); dst[2] = classes(v.z); dst[3] = classes(v.w);
    }
    if (tid == 0) s_cls[TEXT_DWORDS] = NO_CLASS4;
    __syncthreads();
    for (int i = tid; i < TEXT_DWORDS; i += CD_THREADS) {
        const uint32_t x = s_cls[i], y = s_cls[i + 1];
        const uint32_t x1 = (x >> 8) | (y << 24), x2 = (x >> 16) | (y << 16);  // the classes one and two residues on
        const uint32_t code = (bases(x) << 4) | (bases(x1) << 2) | bases(x2);  // (< 64 in every byte: no carry between them)
        const uint32_t bad = ((x | x1 | x2) >> 2) & 0x01010101u;               // classes 4 ... 7 are no base
        s_code[i] = (code & ~(bad * 0xFFu)) | (bad << 6);
    }

    const int wave = tid >> 6, lane = tid & 63;
    const uint8_t *__restrict__ code = reinterpret_cast<const uint8_t *>(s_code) + lane;

    for (int qi = 0; qi < a.n_matrices; qi++) {
        const CodonMatrix *__restrict__ M = a.matrices + qi;
        const int n_rows = min(__builtin_amdgcn_readfirstlane(M->n_rows), CD_MAX_ROWS), thr = __builtin_amdgcn_readfirstlane(M->thr);
        const int konst = __builtin_amdgcn_readfirstlane(M->konst), id = __builtin_amdgcn_readfirstlane(M->id);
        // starts 0 .. n_valid - 1 of the record exist; n_here of them are the workgroup's
        const int64_t n_valid = d.len - 3 * (int64_t)__builtin_amdgcn_readfirstlane(M->rows) + 1 - wg_first;
        const int n_here = n_valid <= 0 ? 0 : n_valid >= CD_WG_STARTS ? CD_WG_STARTS : (int)n_valid;
        __syncthreads();                                                       // (the codes are there; the last matrix's tables are read)
        const uint32_t *__restrict__ src = reinterpret_cast<const uint32_t *>(a.tables + M->tab_off);
        for (int i = tid; i < n_rows * TAB_DWORDS; i += CD_THREADS) s_tab32[i] = src[i];
        if (tid <= CD_MAX_ROWS) s_col[tid] = tid < n_rows ? 3 * ((int)M->col[tid] & (CD_MAX_ROWS - 1)) : 0;   // in residues
        __syncthreads();
#pragma unroll 1
        for (int g = 0; g < CD_WAVE_STARTS / GROUP_STARTS; g++) {
            const int group_first = wave * CD_WAVE_STARTS + g * GROUP_STARTS;  // in the workgroup
            if (group_first >= n_here) break;                                  // (wave-uniform)
            const uint8_t *__restrict__ mine = code + group_first;
            int acc[CD_GROUP];
#pragma unroll
            for (int j = 0; j < CD_GROUP; j++) acc[j] = 0;
            int col = __builtin_amdgcn_readfirstlane(s_col[0]);
            for (int p = 0; p < n_rows; p++) {
                const uint8_t *__restrict__ at = mine + col;
                const int16_t *__restrict__ tab = s_tab + p * CD_TAB_STRIDE;
                const int next = s_col[p + 1];                                 // (read ahead: its latency hides behind this row's reads)
                uint32_t e[CD_GROUP];
                int v[CD_GROUP];
#pragma unroll
                for (int j = 0; j < CD_GROUP; j++) e[j] = at[64 * j];
#pragma unroll
                for (int j = 0; j < CD_GROUP; j++) v[j] = tab[e[j]];
#pragma unroll
                for (int j = 0; j < CD_GROUP; j++) acc[j] += v[j];
                col = __builtin_amdgcn_readfirstlane(next);
            }
            const int lane_first = group_first + lane;
            bool any = false;
#pragma unroll
            for (int j = 0; j < CD_GROUP; j++) any |= acc[j] >= thr && lane_first + 64 * j < n_here;
            if (__ballot(any) == 0) continue;
            // ---- some lane of the wave has a hit among these -----------------------------------------------------------------
#pragma unroll
            for (int j = 0; j < CD_GROUP; j++)
                emit(acc[j] >= thr && lane_first + 64 * j < n_here, a, id, c, wg_first + (lane_first + 64 * j) + 1, acc[j] + konst);
        }
    }
}

hipError_t launch_codon(const CodonArgs &a, int64_t n_wg, hipStream_t st)
{
    if (n_wg < 1) return hipSuccess;
    if (n_wg > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(codon_kernel, dim3((unsigned)n_wg), dim3(CD_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace kgma
