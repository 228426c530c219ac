// kgma_revcomp.hip -- reverse complement of the resident residue text (kgma_genome_revcomp): record c of the destination is
// record c of the source read backwards through the complement map, dst[off + i] = comp(src[off + L - 1 - i]).  Source and
// destination share one layout (genome_layout from the same record lengths), so every ContigDesc serves both.
//
// The kernel is memory-bound: 1 byte read and 1 byte written per base.  A record's slot in the text (its residues rounded up to
// 32 bytes plus 32 bytes of padding) is cut into tiles (no tile spans two records: RevcompArgs::tile_prefix); a workgroup takes
// one tile, a lane RC_ITERS chunks of 16 destination bytes, each written with ONE aligned 16-byte non-temporal store.  The 16
// source bytes of a chunk end where the chunk's mirror image ends: they start at byte off + L - 16 - i, which is 16-byte aligned
// only when L is a multiple of 16.  The misalignment is L % 16 for EVERY chunk of the record (off and i are multiples of 16), so
// it is uniform over the workgroup: a chunk's bytes lie in two aligned 16-byte blocks, and one v_perm per dword with a
// workgroup-uniform selector shifts and byte-reverses them in registers -- no byte loads.  A lane loads the lower block (one
// non-temporal 16-byte load: the text is read once); the upper block is the lower block of the lane before and comes from there
// by a wave shuffle (a wave's first lane loads it), so every block is fetched once, as in a copy.  When L % 16 == 0 there is no
// upper block.
//
// Tail.  The last chunk of a record (i + 16 > L) mirrors bytes that would lie below the record's first residue.  A block that
// starts below the record is not loaded: it counts as zeros, comp(0) = 0, and so the chunk's bytes behind the record's end come
// out zero without a store mask -- and no address below byte 0 of the buffer is ever formed (record 0 starts at offset 0).
// Chunks that lie wholly in the slot's padding store zeros: the kernel writes every byte of every slot, the 64 bytes behind the
// last slot are the host's (one memset), and the destination buffer needs no clearing pass (which would be a third byte per base).
//
// comp.  A<->T C<->G M<->K R<->Y V<->B H<->D in either case, every other byte unchanged (W S N '-' are their own complements; a
// byte outside the alphabet is copied, so that the pack kernel reports it at its mirrored position).  For a letter the map only
// touches the low five bits: comp(b) = b ^ delta[b & 31].  The 32-entry delta table is eight dword constants looked up in
// registers, four bytes per instruction: v_perm_b32 is an 8-entry byte table, four of them cover the 32 entries (selector = low
// three bits of each byte) and two more levels of v_perm pick among them by bits 3 and 4; a byte mask keeps the delta of letters
// (bit 6 set, bit 7 clear) only.  About 25 VALU instructions per dword, no LDS, no table fill and no barrier per workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kgma_device.h"

namespace kgma {

namespace {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// b ^ comp(b) of the letter with (b & 31) == idx
constexpr uint32_t rc_delta(int idx)
{
    return idx == 1 || idx == 20 ? 0x15u     // A T
         : idx == 3 || idx == 7 ? 0x04u      // C G
         : idx == 13 || idx == 11 ? 0x06u    // M K
         : idx == 18 || idx == 25 ? 0x0Bu    // R Y
         : idx == 22 || idx == 2 ? 0x14u     // V B
         : idx == 8 || idx == 4 ? 0x0Cu      // H D
         : 0u;
}
constexpr uint32_t rc_word(int first)
{
    return rc_delta(first) | (rc_delta(first + 1) << 8) | (rc_delta(first + 2) << 16) | (rc_delta(first + 3) << 24);
}

// comp of four bytes
__device__ __forceinline__ uint32_t comp4(uint32_t x)
{
    const uint32_t sel = x & 0x07070707u;
    const uint32_t t0 = __builtin_amdgcn_perm(rc_word(4), rc_word(0), sel);
    const uint32_t t1 = __builtin_amdgcn_perm(rc_word(12), rc_word(8), sel);
    const uint32_t t2 = __builtin_amdgcn_perm(rc_word(20), rc_word(16), sel);
    const uint32_t t3 = __builtin_amdgcn_perm(rc_word(28), rc_word(24), sel);
    // byte j of the result: byte j of the low operand, or of the high one (selector j + 4) where the index bit is set
    const uint32_t s3 = ((x >> 1) & 0x04040404u) | 0x03020100u;
    const uint32_t s4 = ((x >> 2) & 0x04040404u) | 0x03020100u;
    const uint32_t lo = __builtin_amdgcn_perm(t1, t0, s3), hi = __builtin_amdgcn_perm(t3, t2, s3);
    const uint32_t delta = __builtin_amdgcn_perm(hi, lo, s4);
    // 0xFF in the bytes that hold a letter: 0x80 - {0, 1} = 0x80, 0x7F per byte (no borrow leaves a byte), then flip bit 7
    const uint32_t letter = (x >> 6) & ~(x >> 7) & 0x01010101u;
    return x ^ (delta & ((0x80808080u - letter) ^ 0x80808080u));
}

// One chunk from the two 16-byte blocks w[0..7] that cover its source bytes sh .. sh + 15, D = sh / 4: destination dword q is the
// source dword 3 - q byte-reversed (`rev` also shifts by sh % 4 bytes) and complemented.
template <int D>
__device__ __forceinline__ u32x4_t revcomp_chunk(const uint32_t (&w)[8], uint32_t rev)
{
    u32x4_t out;
    out.x = comp4(__builtin_amdgcn_perm(w[D + 4], w[D + 3], rev));
    out.y = comp4(__builtin_amdgcn_perm(w[D + 3], w[D + 2], rev));
    out.z = comp4(__builtin_amdgcn_perm(w[D + 2], w[D + 1], rev));
    out.w = comp4(__builtin_amdgcn_perm(w[D + 1], w[D], rev));
    return out;
}

// record of tile t: the c with tile_prefix[c] <= t < tile_prefix[c + 1] (as kgma_exact.hip)
__device__ __forceinline__ int tile_record(const int64_t *__restrict__ prefix, int n, int64_t t)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace

__global__ __launch_bounds__(KGMA_REVCOMP_THREADS) void revcomp_kernel(const RevcompArgs a)
{
    constexpr int64_t PASS = (int64_t)KGMA_REVCOMP_THREADS * 16;
    const int64_t tile = (int64_t)blockIdx.x;
    const int c = tile_record(a.tile_prefix, a.n_contigs, tile);
    const ContigDesc d = a.cd[c];
    const int64_t L = d.len;
    const int64_t slot = ((L + 31) & ~31ll) + 32;                     // the record's bytes of the text, padding included
    const int64_t tile_off = (tile - a.tile_prefix[c]) * (PASS * KGMA_REVCOMP_ITERS);
    const uint32_t sh = (uint32_t)L & 15u;                            // misalignment of every chunk's source bytes
    const uint32_t rev = 0x00010203u + (sh & 3u) * 0x01010101u;       // bytes sh % 4 + 3 ... sh % 4 of a dword pair
    const uint8_t *__restrict__ src = a.src + d.ascii_off;
    uint8_t *__restrict__ dst = a.dst + d.ascii_off;
    for (int it = 0; it < KGMA_REVCOMP_ITERS; it++) {
        const int64_t it_off = tile_off + (int64_t)it * PASS;
        if (it_off >= slot) break;                                    // (workgroup-uniform)
        const int64_t i = it_off + (int64_t)threadIdx.x * 16;         // the lane's chunk: destination bytes i .. i + 15 of the record
        if (i >= slot) continue;
        const bool live = i < L;                                      // (the chunks behind it are padding: zeros)
        // source bytes L - 16 - i .. L - 1 - i of the record = bytes sh .. sh + 15 of the two 16-byte blocks at b0
        const int64_t b0 = L - 16 - i - (int64_t)sh;                  // multiple of 16; -16 in the record's last chunk when sh != 0
        u32x4_t lo = {0u, 0u, 0u, 0u}, hi = {0u, 0u, 0u, 0u};
        if (live && b0 >= 0) lo = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t *>(src + b0));
        if (sh != 0u) {                                               // (workgroup-uniform)
            // the upper block is the lower block of the lane before (its chunk is the one before: it is live if this one is);
            // a wave's first lane loads it (b0 + 16 >= 0, and the block ends inside the slot)
            hi.x = __shfl_up(lo.x, 1); hi.y = __shfl_up(lo.y, 1); hi.z = __shfl_up(lo.z, 1); hi.w = __shfl_up(lo.w, 1);
            if (live && (threadIdx.x & 63u) == 0u) hi = *reinterpret_cast<const u32x4_t *>(src + b0 + 16);
        }
        u32x4_t out = {0u, 0u, 0u, 0u};
        if (live) {
            const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            switch (sh >> 2) {                                        // (workgroup-uniform)
            case 0: out = revcomp_chunk<0>(w, rev); break;
            case 1: out = revcomp_chunk<1>(w, rev); break;
            case 2: out = revcomp_chunk<2>(w, rev); break;
            default: out = revcomp_chunk<3>(w, rev); break;
            }
        }
        __builtin_nontemporal_store(out, reinterpret_cast<u32x4_t *>(dst + i));
    }
}

// bytes of a record's slot one tile covers (the host builds RevcompArgs::tile_prefix with it)
int64_t revcomp_tile_bytes() { return (int64_t)KGMA_REVCOMP_THREADS * KGMA_REVCOMP_ITERS * 16; }

hipError_t launch_revcomp(const RevcompArgs &a, int64_t n_tiles, hipStream_t st)
{
    if (n_tiles < 1) return hipSuccess;
    if (n_tiles > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(revcomp_kernel, dim3((unsigned)n_tiles), dim3(KGMA_REVCOMP_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace kgma
