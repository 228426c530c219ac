// kgma_twobit.hip -- .2bit ingest (kgma_genome_from_2bit_file): the packed bases of a UCSC .2bit file and its N / soft-mask block
// lists -> the resident residue text, in ONE pass: 0.25 byte read and 1 byte written per base, plus the block tables.  There is no
// second pass that paints the blocks (a mammalian assembly is half soft-masked, in millions of blocks: painting would write half
// the text twice).
//
// Tiling as kgma_revcomp.hip: a record's slot in the text (its residues rounded up to 32 bytes plus 32 bytes of padding) is cut
// into tiles (no tile spans two records: TwobitArgs::tile_prefix, binary-searched per workgroup); a workgroup takes one tile, a
// lane KGMA_TWOBIT_ITERS chunks of 16 text bytes, each written with ONE aligned 16-byte non-temporal store.  The 16 bases of a
// chunk are one dword of packed bytes: the host stages every record's packed bytes at a 16-byte aligned offset (in the file they
// start at any byte), so the dword of chunk i lies at packed_off + i / 4, aligned, and a wave's loads are one 256-byte run.
//
// Decoding.  Packed byte p holds four bases, the FIRST in its two most significant bits.  Its four 2-bit fields are spread to
// the low bits of four bytes, first base in byte 0 -- ((p >> 6) | (p << 4) | (p << 14) | (p << 24)) & 0x03030303 -- and that dword
// is the selector of one v_perm_b32 against the constant "TCAG" (code 0 = T, 1 = C, 2 = A, 3 = G).
//
// Blocks.  Per record the N blocks and the mask blocks are disjoint, increasing and not adjacent (the host normalises them), so
// at most 8 blocks of a list meet a 16-base chunk.  The blocks that meet the TILE are found once per workgroup (two binary
// searches per list over the record's blocks, on workgroup-uniform values) and, when there are at most KGMA_TWOBIT_LDS_BLOCKS of
// them, copied to LDS; a lane then finds the first block that ends behind its chunk's start by a binary search inside that range
// and walks on while blocks start inside the chunk, building a 16-bit set per list.  A set is applied per output dword: its four
// bits are spread to the low bits of four bytes (nib * 0x00204081 & 0x01010101: bit k lands at 8k, no carries), times 0xFF a
// byte select for 'N', shifted left by 5 the 0x20 that lower-cases.  An N inside a mask block is 'n', as twoBitToFa writes it.
//
// Outside the residues.  Bytes of the slot behind the record's last residue are written as zeros -- the last chunk through a third
// set (the positions below the record's length), so neither the 2 padding bits of a record's last byte nor the bytes that pad the
// staged record to 16 ever surface -- the 64 bytes behind the last slot are the host's (one memset): the text needs no clearing
// pass.  No address outside [packed_off, packed_off + packed bytes rounded up to 4) is formed: only chunks that start below the
// record's length load.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kgma_device.h"

namespace kgma {

namespace {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

constexpr int KGMA_TWOBIT_LDS_BLOCKS = 1024;                           // blocks of one list a tile keeps in LDS (8 KiB per list)
constexpr uint32_t TCAG = 'T' | ('C' << 8) | ('A' << 16) | ((uint32_t)'G' << 24);

// record of tile t: the c with tile_prefix[c] <= t < tile_prefix[c + 1] (as kgma_revcomp.hip)
__device__ __forceinline__ int tile_record(const int64_t *__restrict__ prefix, int n, int64_t t)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// first j in [lo, hi) whose block ends behind residue x (hi: none)
__device__ __forceinline__ int64_t first_end_behind(const TwobitBlock *__restrict__ blk, int64_t lo, int64_t hi, int64_t x)
{
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)blk[mid].end > x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// first j in [lo, hi) whose block starts at or behind residue x (hi: none)
__device__ __forceinline__ int64_t first_start_from(const TwobitBlock *__restrict__ blk, int64_t lo, int64_t hi, int64_t x)
{
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)blk[mid].start >= x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// bit j set: residue i + j lies in one of the blocks pb[0 .. cnt) (the tile's)
template <class P>
__device__ __forceinline__ uint32_t chunk_bits(P pb, int cnt, int64_t i)
{
    int lo = 0, hi = cnt;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)pb[mid].end > i) hi = mid; else lo = mid + 1;
    }
    uint32_t bits = 0;
    for (; lo < cnt; lo++) {
        const int64_t s = pb[lo].start, e = pb[lo].end;
        if (s >= i + 16) break;
        const uint32_t from = (uint32_t)((s > i ? s : i) - i), to = (uint32_t)((e < i + 16 ? e : i + 16) - i);   // 0 <= from < to <= 16
        bits |= ((1u << to) - 1u) & ~((1u << from) - 1u);
    }
    return bits;
}

// the four bits of nib in the low bits of four bytes (bit k -> bit 8 k)
__device__ __forceinline__ uint32_t spread4(uint32_t nib) { return (nib * 0x00204081u) & 0x01010101u; }

// four residues from packed byte p: 'N' where nb is set, lower case where mb is set, zero where kb is clear
__device__ __forceinline__ uint32_t unpack4(uint32_t p, uint32_t nb, uint32_t mb, uint32_t kb)
{
    const uint32_t sel = ((p >> 6) | (p << 4) | (p << 14) | (p << 24)) & 0x03030303u;
    const uint32_t letters = __builtin_amdgcn_perm(TCAG, TCAG, sel);  // (selector bytes 0 ... 3: either operand holds the table)
    const uint32_t n = spread4(nb) * 0xFFu;
    const uint32_t r = (letters & ~n) | (0x4E4E4E4Eu & n) | (spread4(mb) << 5);
    return r & (spread4(kb) * 0xFFu);
}

}  // namespace

__global__ __launch_bounds__(KGMA_TWOBIT_THREADS) void twobit_unpack_kernel(const TwobitArgs a)
{
    constexpr int64_t PASS = (int64_t)KGMA_TWOBIT_THREADS * 16;
    constexpr int64_t TILE = PASS * KGMA_TWOBIT_ITERS;
    __shared__ TwobitBlock s_blk[2][KGMA_TWOBIT_LDS_BLOCKS];
    const int64_t tile = (int64_t)blockIdx.x;
    const int c = tile_record(a.tile_prefix, a.n_contigs, tile);
    const ContigDesc d = a.cd[c];
    const int64_t L = d.len;
    const int64_t slot = ((L + 31) & ~31ll) + 32;                     // the record's bytes of the text, padding included
    const int64_t tile_off = (tile - a.tile_prefix[c]) * TILE;
    const TwobitBlock *__restrict__ blk = a.blk;
    const uint8_t *__restrict__ src = a.packed + a.packed_off[c];
    uint8_t *__restrict__ dst = a.dst + d.ascii_off;
    // the blocks of either list that meet the tile (workgroup-uniform)
    int64_t first[2];
    int cnt[2];
    for (int l = 0; l < 2; l++) {
        const int64_t *__restrict__ prefix = l == 0 ? a.n_prefix : a.m_prefix;
        const int64_t rb = prefix[c], re = prefix[c + 1];
        first[l] = first_end_behind(blk, rb, re, tile_off);
        cnt[l] = (int)(first_start_from(blk, first[l], re, tile_off + TILE) - first[l]);   // (at most TILE / 2 + 1)
        if (cnt[l] <= KGMA_TWOBIT_LDS_BLOCKS)
            for (int j = (int)threadIdx.x; j < cnt[l]; j += KGMA_TWOBIT_THREADS) s_blk[l][j] = blk[first[l] + j];
    }
    __syncthreads();
    for (int it = 0; it < KGMA_TWOBIT_ITERS; it++) {
        const int64_t it_off = tile_off + (int64_t)it * PASS;
        if (it_off >= slot) break;                                    // (workgroup-uniform)
        const int64_t i = it_off + (int64_t)threadIdx.x * 16;         // the lane's chunk: bytes i .. i + 15 of the record's slot
        if (i >= slot) continue;
        u32x4_t out = {0u, 0u, 0u, 0u};
        if (i < L) {                                                  // (the chunks behind it are padding: zeros)
            const uint32_t w = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(src + (i >> 2)));
            uint32_t nb = 0u, mb = 0u;
            if (cnt[0] > 0) nb = cnt[0] <= KGMA_TWOBIT_LDS_BLOCKS ? chunk_bits(&s_blk[0][0], cnt[0], i) : chunk_bits(blk + first[0], cnt[0], i);
            if (cnt[1] > 0) mb = cnt[1] <= KGMA_TWOBIT_LDS_BLOCKS ? chunk_bits(&s_blk[1][0], cnt[1], i) : chunk_bits(blk + first[1], cnt[1], i);
            const uint32_t kb = L - i >= 16 ? 0xFFFFu : (1u << (uint32_t)(L - i)) - 1u;   // residues of the chunk
            out.x = unpack4(w & 0xFFu, nb & 15u, mb & 15u, kb & 15u);
            out.y = unpack4((w >> 8) & 0xFFu, (nb >> 4) & 15u, (mb >> 4) & 15u, (kb >> 4) & 15u);
            out.z = unpack4((w >> 16) & 0xFFu, (nb >> 8) & 15u, (mb >> 8) & 15u, (kb >> 8) & 15u);
            out.w = unpack4(w >> 24, nb >> 12, mb >> 12, kb >> 12);
        }
        __builtin_nontemporal_store(out, reinterpret_cast<u32x4_t *>(dst + i));
    }
}

// bytes of a record's slot one tile covers (the host builds TwobitArgs::tile_prefix with it)
int64_t twobit_tile_bytes() { return (int64_t)KGMA_TWOBIT_THREADS * KGMA_TWOBIT_ITERS * 16; }

hipError_t launch_twobit_unpack(const TwobitArgs &a, int64_t n_tiles, hipStream_t st)
{
    if (n_tiles < 1) return hipSuccess;
    if (n_tiles > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(twobit_unpack_kernel, dim3((unsigned)n_tiles), dim3(KGMA_TWOBIT_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace kgma
