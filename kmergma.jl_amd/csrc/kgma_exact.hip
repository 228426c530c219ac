// kgma_exact.hip -- exact sequence search over the resident genome (exactMatch, src/ExactMatch.jl:89-121): every start
// position of every record at which a query occurs, symbol for symbol after case folding (BioSequences' ExactSearchQuery with
// isequal on DNAAlphabet{4}: N matches only N, an IUPAC code only itself).
//
// Both kernels walk the genome ONCE for a whole batch of queries.  A record is cut into tiles (no tile spans two records); a
// workgroup takes one tile, a lane KGMA_EXACT_ITERS runs of consecutive start positions.  For a run the lane loads the residues
// its starts can see into registers, forms the leading window of every start once, and then loops over the queries: per query
// and start one masked compare of the window against the query's leading symbols (scalar operands), folded into a running minimum.
// Only a wave in which some lane's minimum is zero -- some start matches a query's leading symbols -- enters the slow path: it
// verifies the rest of the query against the residue text and emits (query, record, start) through ballot + wave prefix + one
// atomicAdd per wave on a global cursor, which keeps counting past the buffer's capacity (the host regrows and runs again).
//
//   exact_ascii_kernel   reads the case-preserving residue text, 1 byte per base: 16 starts per run, the first min(m, 8) symbols
//                        in the window.  Serves every query.  CHECK: every residue is also tested against the 16-symbol alphabet
//                        (launched only for genomes the pack kernel found a residue outside A/C/G/T/N in).
//   exact_2bit_kernel    reads the 2-bit interleaved copy, 0.25 byte per base: 32 starts per run, the first min(m, 16) symbols cut
//                        out with one funnel shift per start, as the scan kernels cut k-mers.  Queries of A/C/G/T only; the copy
//                        stores N as T, so every survivor is verified against the residue text from its first symbol on.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kgma_device.h"

namespace kgma {

namespace {

constexpr uint32_t FOLD4 = 0xDFDFDFDFu;
// letters of the alphabet by (ch | 0x20) - 'a': a b c d g h k m n r s t v w y
constexpr uint32_t DNA_LETTERS = (1u << 0) | (1u << 1) | (1u << 2) | (1u << 3) | (1u << 6) | (1u << 7) | (1u << 10) | (1u << 12) | (1u << 13) |
                                 (1u << 17) | (1u << 18) | (1u << 19) | (1u << 21) | (1u << 22) | (1u << 24);

__device__ __forceinline__ bool dna_symbol(uint32_t ch)
{
    const uint32_t l = (ch | 0x20u) - 'a';
    return (l < 26u && ((DNA_LETTERS >> l) & 1u)) || ch == '-';
}

// record of tile t: the c with tile_prefix[c] <= t < tile_prefix[c + 1]
__device__ __forceinline__ int tile_record(const int64_t *__restrict__ prefix, int n, int64_t t)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// query text [from, m) against the residues at p, case folded; eight bytes at a time
__device__ __forceinline__ bool same_text(const uint8_t *__restrict__ p, const uint8_t *__restrict__ t, int64_t from, int64_t m)
{
    int64_t i = from;
    for (; i + 8 <= m; i += 8) {
        uint64_t a, b;
        __builtin_memcpy(&a, p + i, 8);
        __builtin_memcpy(&b, t + i, 8);
        if ((a & 0xDFDFDFDFDFDFDFDFull) != b) return false;
    }
    for (; i < m; i++)
        if ((p[i] & 0xDFu) != t[i]) return false;
    return true;
}

// The query descriptors are the same for every lane and constant for the launch: read through the constant address space they
// come in by scalar loads (the scalar cache), one query ahead of the compares that use them.
typedef const ExactQuery __attribute__((address_space(4))) *QueryTable;
__device__ __forceinline__ QueryTable query_table(const ExactArgs &a) { return (QueryTable)(uintptr_t)a.queries; }
__device__ __forceinline__ ExactQuery load_query(QueryTable t, int i)
{
    ExactQuery Q;
    Q.text_off = t[i].text_off; Q.len = t[i].len;
    Q.pat[0] = t[i].pat[0]; Q.pat[1] = t[i].pat[1]; Q.mask[0] = t[i].mask[0]; Q.mask[1] = t[i].mask[1];
    Q.id = t[i].id; Q.pad = 0;
    return Q;
}

// the lanes with `ok` append one match each: one atomicAdd per wave
__device__ __forceinline__ void emit(bool ok, const ExactArgs &a, int query, int contig, int64_t start1)
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
        ExactMatch mt;
        mt.query = query; mt.contig = contig; mt.start = start1;
        a.out[slot] = mt;
    }
}

}  // namespace

template <bool CHECK>
__global__ __launch_bounds__(KGMA_EXACT_THREADS) void exact_ascii_kernel(const ExactArgs a)
{
    constexpr int RUN = KGMA_EXACT_RUN_ASCII;
    const int64_t tile = (int64_t)blockIdx.x;
    const int c = tile_record(a.tile_prefix, a.n_contigs, tile);
    const ContigDesc d = a.cd[c];
    const int64_t tile_off = (tile - a.tile_prefix[c]) * (int64_t)(KGMA_EXACT_THREADS * KGMA_EXACT_ITERS * RUN);
    const uint8_t *__restrict__ text = a.ascii + d.ascii_off;
    const QueryTable qt_all = query_table(a);
    for (int it = 0; it < KGMA_EXACT_ITERS; it++) {
        const int64_t it_off = tile_off + (int64_t)it * (KGMA_EXACT_THREADS * RUN);
        if (it_off >= d.len) break;                                     // (workgroup-uniform)
        const int64_t off = it_off + (int64_t)threadIdx.x * RUN;      // the lane's first start, 0-based in the record
        const bool live = off < d.len;
        // residues off .. off + 23 (a record's slot in the text ends >= 32 bytes behind its last residue: kgma_api.cpp, genome_layout)
        uint32_t x[6] = {0u, 0u, 0u, 0u, 0u, 0u};
        if (live) {
            const uint4 v = *reinterpret_cast<const uint4 *>(text + off);
            const uint2 u = *reinterpret_cast<const uint2 *>(text + off + 16);
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; x[4] = u.x; x[5] = u.y;
        }
        if (CHECK && live) {
            int bad = -1;
#pragma unroll
            for (int i = RUN - 1; i >= 0; i--)
                if (off + i < d.len && !dna_symbol((x[i >> 2] >> (8 * (i & 3))) & 0xFFu)) bad = i;
            if (bad >= 0) atomicMin(&a.ctl[1], ((unsigned long long)c << 40) | (unsigned long long)(off + bad));
        }
#pragma unroll
        for (int i = 0; i < 6; i++) x[i] &= FOLD4;
        // w[j]: the four folded bytes from offset j on; start j's window is (w[j], w[j + 4])
        uint32_t w[RUN + 4];
#pragma unroll
        for (int j = 0; j < RUN + 4; j++)
            w[j] = (j & 3) == 0 ? x[j >> 2] : __builtin_amdgcn_alignbyte(x[(j >> 2) + 1], x[j >> 2], (uint32_t)(j & 3));
        ExactQuery Qnext = load_query(qt_all, 0);
        for (int qi = 0; qi < a.n_queries; qi++) {
            const ExactQuery Q = Qnext;
            Qnext = load_query(qt_all, qi + 1 < a.n_queries ? qi + 1 : qi);
            uint32_t mn = 0xFFFFFFFFu;
#pragma unroll
            for (int j = 0; j < RUN; j++) {
                const uint32_t df = ((w[j] ^ Q.pat[0]) & Q.mask[0]) | ((w[j + 4] ^ Q.pat[1]) & Q.mask[1]);
                mn = df < mn ? df : mn;
            }
            if (__ballot(live && mn == 0u) == 0) continue;
            // ---- some start of this wave matches the query's leading symbols ---------------------------------------------
            uint32_t hit = 0;
#pragma unroll
            for (int j = 0; j < RUN; j++) {
                const uint32_t df = ((w[j] ^ Q.pat[0]) & Q.mask[0]) | ((w[j + 4] ^ Q.pat[1]) & Q.mask[1]);
                hit |= (df == 0u ? 1u : 0u) << j;
            }
            const uint8_t *__restrict__ qt = a.qtext + Q.text_off;
            for (int j = 0; j < RUN; j++) {
                bool ok = live && ((hit >> j) & 1u) && off + j + Q.len <= d.len;
                if (__ballot(ok) == 0) continue;
                if (ok && Q.len > 8) ok = same_text(text + off + j, qt, 8, Q.len);
                emit(ok, a, Q.id, c, off + j + 1);
            }
        }
    }
}

__global__ __launch_bounds__(KGMA_EXACT_THREADS) void exact_2bit_kernel(const ExactArgs a)
{
    constexpr int RUN = KGMA_EXACT_RUN_2BIT;
    const int64_t tile = (int64_t)blockIdx.x;
    const int c = tile_record(a.tile_prefix, a.n_contigs, tile);
    const ContigDesc d = a.cd[c];
    const int64_t tile_off = (tile - a.tile_prefix[c]) * (int64_t)(KGMA_EXACT_THREADS * KGMA_EXACT_ITERS * RUN);
    const uint8_t *__restrict__ text = a.ascii + d.ascii_off;
    const QueryTable qt_all = query_table(a);
    const uint32_t *__restrict__ codes = a.inter + 2 * d.word_off;     // base b of the record: dword b / 16, bits 2 (b % 16)
    for (int it = 0; it < KGMA_EXACT_ITERS; it++) {
        const int64_t it_off = tile_off + (int64_t)it * (KGMA_EXACT_THREADS * RUN);
        if (it_off >= d.len) break;
        const int64_t off = it_off + (int64_t)threadIdx.x * RUN;
        const bool live = off < d.len;
        // bases off .. off + 47 (a record is followed by 32 words of padding in the copy)
        uint32_t x0 = 0u, x1 = 0u, x2 = 0u;
        if (live) {
            const uint2 v = *reinterpret_cast<const uint2 *>(codes + (off >> 4));
            x0 = v.x; x1 = v.y; x2 = codes[(off >> 4) + 2];
        }
        uint32_t w[RUN];
#pragma unroll
        for (int j = 0; j < RUN; j++)
            w[j] = j < 16 ? __builtin_amdgcn_alignbit(x1, x0, 2u * (uint32_t)(j & 15)) : __builtin_amdgcn_alignbit(x2, x1, 2u * (uint32_t)(j & 15));
        ExactQuery Qnext = load_query(qt_all, 0);
        for (int qi = 0; qi < a.n_queries; qi++) {
            const ExactQuery Q = Qnext;
            Qnext = load_query(qt_all, qi + 1 < a.n_queries ? qi + 1 : qi);
            uint32_t mn = 0xFFFFFFFFu;
#pragma unroll
            for (int j = 0; j < RUN; j++) {
                const uint32_t df = (w[j] ^ Q.pat[0]) & Q.mask[0];
                mn = df < mn ? df : mn;
            }
            if (__ballot(live && mn == 0u) == 0) continue;
            uint32_t hit = 0;
#pragma unroll
            for (int j = 0; j < RUN; j++) hit |= (((w[j] ^ Q.pat[0]) & Q.mask[0]) == 0u ? 1u : 0u) << j;
            const uint8_t *__restrict__ qt = a.qtext + Q.text_off;
            for (int j = 0; j < RUN; j++) {
                bool ok = live && ((hit >> j) & 1u) && off + j + Q.len <= d.len;
                if (__ballot(ok) == 0) continue;
                if (ok) ok = same_text(text + off + j, qt, 0, Q.len);   // (also what tells a genome N from the query's T)
                emit(ok, a, Q.id, c, off + j + 1);
            }
        }
    }
}

// start positions per tile of the two kernels (the host builds ExactArgs::tile_prefix with it)
int64_t exact_tile_starts(bool two_bit)
{
    return (int64_t)KGMA_EXACT_THREADS * KGMA_EXACT_ITERS * (two_bit ? KGMA_EXACT_RUN_2BIT : KGMA_EXACT_RUN_ASCII);
}

// kind: 0 = residue text, 1 = residue text with the alphabet check, 2 = 2-bit copy
hipError_t launch_exact(const ExactArgs &a, int kind, int64_t n_tiles, hipStream_t st)
{
    if (n_tiles < 1) return hipSuccess;
    if (n_tiles > 0x7FFFFFFFll) return hipErrorInvalidValue;
    const dim3 grid((unsigned)n_tiles), block(KGMA_EXACT_THREADS);
    if (kind == 2) hipLaunchKernelGGL(exact_2bit_kernel, grid, block, 0, st, a);
    else if (kind == 1) hipLaunchKernelGGL(exact_ascii_kernel<true>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(exact_ascii_kernel<false>, grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace kgma
