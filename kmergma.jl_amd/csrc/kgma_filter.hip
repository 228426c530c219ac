// kgma_filter.hip -- exact lower bound on the window distance: which windows the count-table scan has to look at (k = 5, 6).
//
// With c[x] the copies of k-mer x among the n k-mers of window s and sumS(s) = sum over the window's k-mer positions p of S[K_p]
// (= sum_x S[x] c[x]):
//     D_s = sum_x (S[x] - N c[x])^2 = sumS2 - 2N sumS(s) + N^2 sum_x c[x]^2  >=  sumS2 - 2N sumS(s) + N^2 n
// because c^2 >= c and sum_x c[x] = n.  So D_s <= Dmax needs sumS(s) >= U = ceil((sumS2 + N^2 n - Dmax) / 2N): an integer test on a
// sliding sum of table lookups -- no count table, no atomics.  S >= 0 (sums of counts), so the sum over any SUPERSET of a window's
// positions still bounds sumS from above: the test is made per GRANULE of 16 window starts, on the sum over every position one of
// the granule's windows uses (FilterArgs::nblk blocks of 16 positions).
//
// One wave walks one stream of the scan's regular stream table, 64 blocks (1024 positions) per iteration: lane = block = one dword
// of the 2-bit genome copy plus its successor; 16 k-mers cut out like stream8_kernel's, 16 lookups in the S table staged in LDS,
// one block sum; a DPP prefix sum over the lanes plus the carry; the granule's sum is the difference of two prefix values nblk
// lanes apart (the previous iteration's prefixes stay in a register).  Positions behind the record's last k-mer count as 0 (no
// window of the record uses them), so the candidate set is a function of the records alone.
// The S table is kept as 32 interleaved copies where they fit the LDS (4^k bytes or int16 each): lane l reads copy l % 32, which
// lives in bank l % 32, so the 64 random reads of a wave never collide (2 LDS cycles instead of ~7 for one copy).
// Output: per wave iteration with a candidate, ONE entry {record, granule of bit 0, 64-bit mask} appended with one atomic.
// In a step (kgma_repack_scan_hits) whose S entries are bytes the block sums come from the step's pack instead: pack_sums_kernel
// (below) writes them beside the 2-bit copy, and filter_sums_kernel walks the streams on those sums, four blocks per lane.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "kgma_device.h"
#include "kgma_pack.h"

namespace kgma {

namespace {

__device__ __forceinline__ uint32_t f_incl_scan(uint32_t x)
{
    int32_t v = (int32_t)x;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);   // row_bcast:15 -> rows 1,3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);   // row_bcast:31 -> rows 2,3
    return (uint32_t)v;
}

}  // namespace

// The S table in LDS: dword (x / EPD) of copy c is LDS dword (x / EPD) * COPIES + c (EPD = 4 / ES entries per dword)
template <int K, int ES, int COPIES>
__device__ __forceinline__ void f_stage_table(uint32_t *fsm, const int32_t *S)
{
    constexpr int NB = 1 << (2 * K);
    constexpr int EPD = 4 / ES;
    for (int t = (int)threadIdx.x; t < NB / EPD * COPIES; t += (int)blockDim.x) {
        const int d = t / COPIES;
        uint32_t v = 0;
#pragma unroll
        for (int e = 0; e < EPD; e++) v |= (uint32_t)S[d * EPD + e] << (8 * ES * e);
        fsm[t] = v;
    }
    __syncthreads();
}

// ES: bytes per S entry (1: every S < 256, 2: < 65536); COPIES: 32 bank-interleaved copies, or 1
template <int K, int ES, int COPIES>
__global__ __launch_bounds__(1024) void filter_kernel(FilterArgs a)
{
    constexpr int NB = 1 << (2 * K);
    constexpr uint32_t KM = (uint32_t)NB - 1u;
    constexpr int EPD = 4 / ES;                                        // entries per dword
    extern __shared__ uint32_t fsm[];
    f_stage_table<K, ES, COPIES>(fsm, a.S);
    const uint8_t *tab = reinterpret_cast<const uint8_t *>(fsm);
    const int lane = (int)(threadIdx.x & 63);
    const uint32_t coff = COPIES > 1 ? 4u * (uint32_t)(lane & (COPIES - 1)) : 0u;
    auto lookup = [&](const uint32_t x) -> uint32_t {
        const uint32_t off = (x / EPD) * (4u * COPIES) + coff + (x % EPD) * ES;
        if constexpr (ES == 1) return tab[off];
        else return *reinterpret_cast<const uint16_t *>(tab + off);
    };
    const int waves_per_wg = (int)(blockDim.x >> 6);
    const int wave0 = (int)blockIdx.x * waves_per_wg + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n_waves = (int)gridDim.x * waves_per_wg;
    const int nblk = a.nblk;
    const int lo_idx = ((lane - nblk) & 63) << 2;                      // (bpermute takes byte addresses)

    for (int t = wave0; t < a.n_tiles; t += n_waves) {
        const TileDesc td = a.tiles[t];
        const int64_t g0 = (td.win0 - 1) >> 4;                         // first granule of the stream (streams start on 64-window boundaries)
        const int ng = (td.n_valid + 15) >> 4;
        const int nb = ng + nblk - 1;                                  // blocks the stream's granules use
        // k-mer positions of the record from the stream's first block on (the record's last k-mer is at len - K), clamped to int32
        const int64_t rem64 = a.cd[td.contig].len - K - (g0 << 4);
        const int rem = __builtin_amdgcn_readfirstlane((int)(rem64 < -1 ? -1 : (rem64 > 0x3FFFFFFF ? 0x3FFFFFFF : rem64)));
        const int64_t dw0 = 2 * td.word_base;
        const int iters = (nb + 63) >> 6;
        auto load = [&](const int it, uint32_t &d0, uint32_t &d1) {
            const int64_t j = dw0 + ((int64_t)it << 6) + lane;
            d0 = j < a.n_dwords ? a.inter[j] : 0u;
            d1 = j + 1 < a.n_dwords ? a.inter[j + 1] : 0u;
        };
        uint32_t carry = 0, prevI = 0, n0, n1;
        load(0, n0, n1);
        for (int it = 0; it < iters; it++) {
            const uint32_t d0 = n0, d1 = n1;
            if (it + 1 < iters) load(it + 1, n0, n1);
            const int jb = (it << 6) + lane;                           // block, local to the stream
            uint32_t sum = 0;
            if (rem - (((it << 6) + 63) << 4) >= 15) {                 // (wave-uniform) every position of the iteration is a k-mer of the record
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const uint32_t x = (i == 0 ? d0 : __builtin_amdgcn_alignbit(d1, d0, 2 * i)) & KM;
                    sum += lookup(x);
                }
            } else {                                                   // the record's end: positions 0 ... lim of the lane's block count
                const int lim = rem - (jb << 4);
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const uint32_t x = (i == 0 ? d0 : __builtin_amdgcn_alignbit(d1, d0, 2 * i)) & KM;
                    const uint32_t v = lookup(x);
                    sum += i <= lim ? v : 0u;
                }
            }
            const uint32_t I = f_incl_scan(sum) + carry;               // (mod 2^32: only differences nblk blocks apart are used)
            carry = (uint32_t)__builtin_amdgcn_readlane((int)I, 63);
            const uint32_t lo_cur = (uint32_t)__builtin_amdgcn_ds_bpermute(lo_idx, (int)I);
            const uint32_t lo_prev = (uint32_t)__builtin_amdgcn_ds_bpermute(lo_idx, (int)prevI);
            const uint32_t bound = I - (lane >= nblk ? lo_cur : lo_prev);
            prevI = I;
            const int gl = jb - (nblk - 1);                            // the granule whose last block this lane holds
            const uint64_t m = __ballot(gl >= 0 && gl < ng && bound >= a.U);
            if (m != 0 && lane == 0) {
                const unsigned int idx = atomicAdd(a.ctl, 1u);
                if (idx < a.cap) {
                    FilterEntry e;
                    e.contig = td.contig;
                    e.gbase = (int32_t)(g0 + (it << 6) - (nblk - 1));
                    e.mask = m;
                    a.list[idx] = e;
                }
            }
        }
    }
}

// The form on the block sums a.bsum that pack_sums_kernel wrote in this step (kgma_filter_stats::form bit 16): no k-mers, no S
// table.  A wave iteration covers 256 blocks, lane l the blocks 4l ... 4l + 3 -- one 8-byte load (bsum + 2 * word_base is 4-byte
// aligned whatever the record's word offset, and an 8-byte global load needs no more) -- so that the DPP scan, the carry, the loop
// and the ballots' bookkeeping run once per 256 blocks: a serial prefix over the lane's four sums, one scan over the lane totals.
// With nblk = 4 qa + QB the lower end of element q of lane l is element (q - QB) & 3 of lane l - qa - [q < QB], of this iteration
// or, for the first lanes, of the one before.  Every source lane is read by exactly one destination per q, so the SOURCE chooses
// which iteration's value it offers: one ds_bpermute per element.
// The list keeps its format (64 consecutive granules per entry): the four ballots hold block 4l + q at bit l and are transposed,
// with four more ballots, only when one of them is non-zero.
// QB: nblk % 4 (which element of the source lane an element reads is then fixed at compile time)
template <int QB>
__global__ __launch_bounds__(1024) void filter_sums_kernel(FilterArgs a, int K)
{
    const int lane = (int)(threadIdx.x & 63);
    const int waves_per_wg = (int)(blockDim.x >> 6);
    const int wave0 = (int)blockIdx.x * waves_per_wg + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n_waves = (int)gridDim.x * waves_per_wg;
    const int nblk = a.nblk;
    const int qa = nblk >> 2;
    int lo_idx[4];                                                     // (bpermute takes byte addresses)
    bool offer_cur[4];                                                 // the lane's reader is in this iteration (else in the next)
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int back = qa + (q < QB ? 1 : 0);
        lo_idx[q] = ((lane - back) & 63) << 2;
        offer_cur[q] = lane + back < 64;
    }
    const uint32_t *pairs = reinterpret_cast<const uint32_t *>(a.bsum);   // a plane word's two sums
    const int64_t n_pairs = a.n_dwords >> 1;

    for (int t = wave0; t < a.n_tiles; t += n_waves) {
        const TileDesc td = a.tiles[t];
        const int64_t g0 = (td.win0 - 1) >> 4;                         // first granule of the stream (streams start on 64-window boundaries)
        const int ng = (td.n_valid + 15) >> 4;
        const int nb = ng + nblk - 1;                                  // blocks the stream's granules use
        // blocks of the stream that hold a k-mer of the record (its last k-mer is at len - K): the partial last one is masked in
        // bsum, a block behind it may belong to the next record
        const int64_t rem64 = a.cd[td.contig].len - K - (g0 << 4);
        const int nvb = __builtin_amdgcn_readfirstlane(rem64 < 0 ? 0 : (int)((rem64 > 0x3FFFFFFF ? 0x3FFFFFFF : rem64) >> 4) + 1);
        const int iters = (nb + 255) >> 8;
        auto load = [&](const int it, uint32_t &x, uint32_t &y) {
            const int64_t j = td.word_base + ((int64_t)it << 7) + 2 * lane;
            x = 0u; y = 0u;
            if (j + 1 < n_pairs) {
                u32x2_t v;
                __builtin_memcpy(&v, pairs + j, 8);
                x = v.x; y = v.y;
            } else if (j < n_pairs) {
                x = pairs[j];
            }
        };
        uint32_t carry = 0, prevR[4] = {0u, 0u, 0u, 0u}, nx, ny;
        load(0, nx, ny);
        for (int it = 0; it < iters; it++) {
            const uint32_t x = nx, y = ny;
            if (it + 1 < iters) load(it + 1, nx, ny);
            const int jb = (it << 8) + 4 * lane;                       // the lane's first block, local to the stream
            uint32_t s[4] = {x & 0xFFFFu, x >> 16, y & 0xFFFFu, y >> 16};
            if ((it << 8) + 256 > nvb) {                               // (wave-uniform) the record ends in this iteration
#pragma unroll
                for (int q = 0; q < 4; q++) s[q] = jb + q < nvb ? s[q] : 0u;
            }
            uint32_t I[4], R[4];
            const uint32_t p1 = s[0] + s[1], p2 = p1 + s[2], p3 = p2 + s[3];
            I[3] = f_incl_scan(p3) + carry;                            // (mod 2^32: only differences nblk blocks apart are used)
            carry = (uint32_t)__builtin_amdgcn_readlane((int)I[3], 63);
            const uint32_t base = I[3] - p3;
            I[0] = base + s[0]; I[1] = base + p1; I[2] = base + p2;
#pragma unroll
            for (int q = 0; q < 4; q++) R[q] = I[(q - QB) & 3];
            uint64_t m[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(lo_idx[q], (int)(offer_cur[q] ? R[q] : prevR[q]));
                prevR[q] = R[q];
                const int gl = jb + q - (nblk - 1);                    // the granule whose last block this is
                m[q] = __ballot(((uint32_t)gl < (uint32_t)ng) & (I[q] - lo >= a.U));
            }
            if ((m[0] | m[1] | m[2] | m[3]) != 0) {                    // rare: entry e holds the blocks 64 e ... 64 e + 63 of the iteration
                const uint64_t mine = (lane & 3) == 0 ? m[0] : (lane & 3) == 1 ? m[1] : (lane & 3) == 2 ? m[2] : m[3];
#pragma unroll 1
                for (int e = 0; e < 4; e++) {
                    const uint64_t me = __ballot(((mine >> (16 * e + (lane >> 2))) & 1u) != 0);
                    if (me != 0 && lane == 0) {
                        const unsigned int idx = atomicAdd(a.ctl, 1u);
                        if (idx < a.cap) {
                            FilterEntry fe;
                            fe.contig = td.contig;
                            fe.gbase = (int32_t)(g0 + (it << 8) + 64 * e - (nblk - 1));
                            fe.mask = me;
                            a.list[idx] = fe;
                        }
                    }
                }
            }
        }
    }
}

// ---- the step's pack with the block sums -------------------------------------------------------------------------------------
// pack_sums_kernel writes what pack_kernel writes (kgma_kernels.hip: planes, interleaved copy, first_bad) and, per dword J of the
// interleaved copy, bsum[J] = the sum of S over the k-mers that start in the dword and are k-mers of its record (position <= len - K);
// 0 for padding.  filter_sums_kernel then loads one sum where filter_kernel cuts and looks up 16 k-mers: the codes are in
// registers here anyway, and the pack waits for HBM while the filter waits for the vector unit.
// Persistent waves.  In LDS: the PAIR table P[y] = S[y & KM] + S[(y >> 2) & KM] over the (K + 1)-mers y (uint16: every S < 256, so
// P <= 510 and a block sum <= 4080), one copy, and behind it S itself as bytes.  On the fast path a dword's sum is eight reads of
// P at the even positions -- the address is the (K + 1)-mer cut out one bit low, i.e. already times two: a shift or v_alignbit and
// one AND per two positions; the word-by-word path looks single positions up in the byte table.  A wave takes UNITS of 128 consecutive plane words (two
// chunks of 64: lane l packs words l and 64 + l) and has the next unit's four 16-byte loads per lane in flight while it encodes the
// current one (64 KiB per CU at 16 waves).  A word's second dword needs the first dword of the next word: lane l + 1's, the other
// chunk's lane 0 for lane 63 of the first chunk, and for the unit's last word K - 1 residues encoded by lane 0 on the side.
// Fast path: the unit lies in one record, every word is full and of accepted letters, and K - 1 residues of the record follow it --
// no position needs the mask.  Everything else (record ends, partial words, padding, several records in a unit, a residue to
// report) goes word by word like pack_kernel's slow path, with the mask; keeping pack_word's one-residue-at-a-time branch out of
// the fast path is also what keeps the kernel inside the 128 VGPRs of a 16-wave workgroup (121, no scratch).
constexpr int PS_UNIT = 128;

__device__ __forceinline__ uint32_t ps_code(uint32_t ch)               // the code pack_word gives a residue (one it reports: 0)
{
    ch &= 0xDFu;
    return (ch == 'C' ? 1u : 0u) | (ch == 'G' ? 2u : 0u) | ((ch == 'T' || ch == 'N') ? 3u : 0u);
}
__device__ __forceinline__ int64_t ps_uniform(const int64_t x)         // a wave-uniform value, to scalar registers
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(x >> 32));
    return (int64_t)((uint64_t)hi << 32 | lo);
}
template <int K>
__device__ __forceinline__ uint32_t ps_halo(const uint2 b)             // 2-bit codes of the first K - 1 of 8 residues
{
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < K - 1; i++) r |= ps_code(((i < 4 ? b.x : b.y) >> (8 * (i & 3))) & 0xFFu) << (2 * i);
    return r;
}
// the same of residues that are all accepted letters, in either case (a unit with another one is reported and its sums are void)
template <int K>
__device__ __forceinline__ uint32_t ps_halo_clean(const uint2 b)
{
    const uint32_t c0 = __builtin_amdgcn_perm(0x03000000u, 0x02030100u, (b.x >> 1) & 0x07070707u);   // (as pack_word_2bit)
    uint32_t r = __builtin_amdgcn_udot4(c0, 0x40100401u, 0u, false);
    if (K > 5) {
        const uint32_t c1 = __builtin_amdgcn_perm(0x03000000u, 0x02030100u, (b.y >> 1) & 0x07070707u);
        r = __builtin_amdgcn_udot4(c1, 0x40100401u, 0u, false) << 8 | r;
    }
    return r & ((1u << (2 * (K - 1))) - 1u);
}
// sum of S over the first nv of the 16 k-mers that start in d0 (d1: the dword behind it); tab: S as bytes
template <int K>
__device__ __forceinline__ uint32_t ps_sum16_masked(const uint32_t d0, const uint32_t d1, const uint8_t *tab, const int nv)
{
    constexpr uint32_t KM = (1u << (2 * K)) - 1u;
    uint32_t sum = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t v = tab[(i == 0 ? d0 : __builtin_amdgcn_alignbit(d1, d0, 2 * i)) & KM];
        sum += i < nv ? v : 0u;
    }
    return sum;
}
// sum of S over all 16 k-mers that start in d0: eight pair sums.  ptab: the pair table; the byte offset of the pair at positions
// i, i + 1 is the (K + 1)-mer at i times 2.  A pair that lies inside d0 takes a plain shift (two-operand forms issue at twice
// v_alignbit's rate, profiles/r01_valu_issue_rates.txt)
template <int K>
__device__ __forceinline__ uint32_t ps_sum16_pairs(const uint32_t d0, const uint32_t d1, const uint8_t *ptab)
{
    constexpr uint32_t M2 = ((1u << (2 * (K + 1))) - 1u) << 1;
    uint32_t sum = 0;
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
        const uint32_t y2 = i == 0 ? d0 << 1 : 2 * i + 2 * (K + 1) <= 32 ? d0 >> (2 * i - 1) : __builtin_amdgcn_alignbit(d1, d0, 2 * i - 1);
        sum += *reinterpret_cast<const uint16_t *>(ptab + (y2 & M2));
    }
    return sum;
}
// the pair table (4^(K+1) uint16) at fsm, S as bytes (4^K) behind it
template <int K>
__device__ __forceinline__ void ps_stage_tables(uint32_t *fsm, const int32_t *S)
{
    constexpr int NB = 1 << (2 * K), NP = 4 * NB;
    constexpr uint32_t KM = (uint32_t)NB - 1u;
    uint32_t *bytes = fsm + NP / 2;
    for (int t = (int)threadIdx.x; t < NB / 4; t += (int)blockDim.x)
        bytes[t] = (uint32_t)S[4 * t] | (uint32_t)S[4 * t + 1] << 8 | (uint32_t)S[4 * t + 2] << 16 | (uint32_t)S[4 * t + 3] << 24;
    __syncthreads();
    const uint8_t *tab = reinterpret_cast<const uint8_t *>(bytes);
    for (int t = (int)threadIdx.x; t < NP / 2; t += (int)blockDim.x) {
        const uint32_t y = 2u * (uint32_t)t, hi = tab[(y >> 2) & KM];    // (y and y + 1 share their second k-mer)
        fsm[t] = ((uint32_t)tab[y & KM] + hi) | ((uint32_t)tab[(y + 1u) & KM] + hi) << 16;
    }
    __syncthreads();
}

// COPY = false, the sums-only form of a sparse step: the same encoding, sums and first_bad, but no word of
// the 2-bit copy is stored (nor a plane: the form is only chosen for genomes without planes) -- the step packs the blocks it reads
// with pack_kernel afterwards.  A fast unit then issues two stores per lane, not four, and the kernel moves 1.125 B per base.
//
// TEST = true (only with COPY = false), the form that makes the prefilter's granule test itself and stores nothing in its steady
// loop.  bsum is ONE array over all blocks of the genome, 0 in the padding, and records lie 2 *
// CONTIG_PAD_WORDS = 64 zero blocks apart while nblk - 1 <= 62: the sum of the nblk blocks from a granule's first block on never
// reaches the next record, so the candidate set is a prefix-sum difference over the GLOBAL block array, and only the label
// (record, granule) and the test 0 <= granule < ceil(nwin / 16) are per record.  A chunk (64 plane words = 128 blocks, two per
// lane, the sums of the storing form's layout) is one iteration of filter_sums_kernel's scheme with two blocks per lane.  The carry
// wants consecutive units: a wave takes RUNS of a.run units, the runs dealt round-robin over the waves, and PRIMES a run with the
// second chunk of the unit in front of it (128 blocks >= nblk - 1), of which nothing is emitted.  In a clean fast unit the
// record is the wave's (scalar registers); elsewhere each candidate lane looks its block's record up and appends one granule.
template <int K, bool COPY, bool TEST = false>
__global__ __launch_bounds__(1024) void pack_sums_kernel(PackSumsArgs a)
{
    static_assert(!TEST || !COPY, "the testing form stores nothing");
    extern __shared__ uint32_t fsm[];
    ps_stage_tables<K>(fsm, a.S);
    const int lane = (int)(threadIdx.x & 63);
    const uint8_t *ptab = reinterpret_cast<const uint8_t *>(fsm);      // pair sums
    const uint8_t *tab = ptab + (8u << (2 * K));                       // S as bytes
    const int waves_per_wg = (int)(blockDim.x >> 6);
    const int64_t wave0 = (int64_t)blockIdx.x * waves_per_wg + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t n_waves = (int64_t)gridDim.x * waves_per_wg;
    const int64_t n_units = (a.total_words + PS_UNIT - 1) / PS_UNIT;
    const int next_idx = ((lane + 1) & 63) << 2;                       // (bpermute takes byte addresses)
    uint2 *out = reinterpret_cast<uint2 *>(a.planes);
    uint2 *out2 = reinterpret_cast<uint2 *>(a.inter);
    uint32_t *outs = reinterpret_cast<uint32_t *>(a.bsum);             // one dword per plane word: its two sums

    // a unit's record and path (wave-uniform), and on the fast path its loads
    // (TEST: u, the unit; rel: the unit's first block in the record's numbering; ng: the record's granules, or -1 in a PRIMING
    //  visit: only the unit's second chunk is wanted, and nothing emitted)
    struct Unit { int c; bool fast; u32x4_t v[4]; uint2 halo; int u, rel, ng; __device__ bool prime() const { return ng < 0; } };
    // The record of the wave's latest unit, in scalar registers: c = the last record that starts at or before the unit's first word
    // (record 0 in the lead padding), and `next`, the word at which record c + 1 starts (INT64_MAX behind the last).  A wave's units
    // only move forward, so the record stands until a unit starts at or past `next`; only then it is looked up again, from the
    // block's entry on -- once in about 60 units on a genome of 100 records.  A unit inside its record touches no memory for it.
    int rc = 0;
    int64_t r_word_off = 0, r_len = 0, r_ascii_off = 0, r_next = 0;    // (r_next = 0: the wave's first unit looks its record up)
    auto prepare = [&](const int64_t u, Unit &n) {
        const int64_t g0 = u * PS_UNIT;
        if (TEST ? __builtin_expect(g0 >= r_next, 0) : g0 >= r_next) {
            int c = a.block_contig[g0 >> a.block_shift];
            while (c + 1 < a.n_contigs && a.cd[c + 1].word_off <= g0) c++;
            const ContigDesc d = a.cd[c];
            // (the addresses are wave-uniform and the loads vector loads all the same: the kernel writes global memory)
            rc = __builtin_amdgcn_readfirstlane(c);
            r_word_off = ps_uniform(d.word_off); r_len = ps_uniform(d.len); r_ascii_off = ps_uniform(d.ascii_off);
            r_next = c + 1 < a.n_contigs ? ps_uniform(a.cd[c + 1].word_off) : INT64_MAX;
        }
        const int64_t w0 = g0 - r_word_off;
        n.c = rc;
        if constexpr (TEST) {
            const int64_t nwin = r_len - (a.nk + K - 1) + 1, ng = nwin > 0 ? (nwin + 15) >> 4 : 0;
            n.rel = (int)(2 * w0);
            if (!n.prime()) n.ng = (int)(ng > 0x7FFFFFFF ? 0x7FFFFFFF : ng);
        }
        n.fast = w0 >= 0 && g0 + PS_UNIT <= a.total_words && (w0 + PS_UNIT) * 32 + (K - 1) <= r_len;
        if (n.fast) {
            const uint8_t *base = a.ascii + r_ascii_off + w0 * 32;
            const u32x4_t *p = reinterpret_cast<const u32x4_t *>(base) + 2 * lane;
            if (!TEST || !n.prime()) {
                n.v[0] = __builtin_nontemporal_load(p);
                n.v[1] = __builtin_nontemporal_load(p + 1);
            }
            n.v[2] = __builtin_nontemporal_load(p + 128);
            n.v[3] = __builtin_nontemporal_load(p + 129);
            n.halo = make_uint2(0u, 0u);
            if (lane == 0) n.halo = *reinterpret_cast<const uint2 *>(base + PS_UNIT * 32);
        }
    };
    // (gb: a wave-uniform word index, so that the addresses are a scalar base plus the lane's offset)
    auto store = [&](const int64_t gb, const int l, const uint2 r, const uint2 iw, const uint32_t s01) {
        if constexpr (COPY) {
            if (a.planes != nullptr) {
                u32x2_t rv; rv.x = r.x; rv.y = r.y;
                __builtin_nontemporal_store(rv, reinterpret_cast<u32x2_t *>(out + gb) + l);
            }
            u32x2_t iv; iv.x = iw.x; iv.y = iw.y;
            __builtin_nontemporal_store(iv, reinterpret_cast<u32x2_t *>(out2 + gb) + l);
        }
        __builtin_nontemporal_store(s01, outs + gb + l);
    };

    // A unit's work comes in two parts, so that the loop can take the next unit's loads over and issue the one after's between
    // them: encode() leaves what a clean fast unit stores in registers (planes, 2-bit words, the four sums as two dwords), and
    // the loop stores it; any other unit goes word by word (by_word) before the loop takes the next one over.
    struct Enc { uint2 r0, r1, i0, i1; uint32_t s0, s1; };
    auto encode = [&](const Unit &cu, Enc &e) -> bool {
        bool clean = false;
        uint2 r0 = make_uint2(0u, 0u), r1 = r0, i0 = r0, i1 = r0;
        e.s0 = e.s1 = 0u;
        if (cu.fast) {
            uint32_t bad0, bad1;
            const uint4 a0 = make_uint4(cu.v[0].x, cu.v[0].y, cu.v[0].z, cu.v[0].w), b0 = make_uint4(cu.v[1].x, cu.v[1].y, cu.v[1].z, cu.v[1].w);
            const uint4 a1 = make_uint4(cu.v[2].x, cu.v[2].y, cu.v[2].z, cu.v[2].w), b1 = make_uint4(cu.v[3].x, cu.v[3].y, cu.v[3].z, cu.v[3].w);
            if (TEST && cu.prime()) {
                bad0 = 0u;
                i1 = pack_word_2bit(a1, b1, &bad1);
            } else if (!COPY || a.planes == nullptr) {                 // (no planes kept: straight to the 2-bit codes)
                i0 = pack_word_2bit(a0, b0, &bad0);
                i1 = pack_word_2bit(a1, b1, &bad1);
            } else {
                r0 = pack_word<true>(a0, b0, 32, &bad0);
                r1 = pack_word<true>(a1, b1, 32, &bad1);
                i0 = interleave_word(r0); i1 = interleave_word(r1);
            }
            clean = __ballot((bad0 | bad1) != 0) == 0;                 // (a residue to report: the unit goes word by word)
        }
        if (clean) {
            // the first dword of the next word: lane l + 1's; lane 63 reads lane 0, which offers the other chunk's / the halo's
            const uint32_t h = ps_halo_clean<K>(cu.halo);
            uint32_t n0 = 0u;                                          // (a priming visit has no first chunk)
            if (!TEST || !cu.prime()) n0 = (uint32_t)__builtin_amdgcn_ds_bpermute(next_idx, (int)(lane == 0 ? i1.x : i0.x));
            const uint32_t n1 = (uint32_t)__builtin_amdgcn_ds_bpermute(next_idx, (int)(lane == 0 ? h : i1.x));
            // (one sum's 16 lookups at a time: the other waves of the SIMD cover their latency, interleaving all 64 only costs registers)
            uint32_t s00 = 0u, s01 = 0u;
            __builtin_amdgcn_sched_barrier(0);
            if (!TEST || !cu.prime()) {
                s00 = ps_sum16_pairs<K>(i0.x, i0.y, ptab);
                __builtin_amdgcn_sched_barrier(0);
                s01 = ps_sum16_pairs<K>(i0.y, n0, ptab);
                __builtin_amdgcn_sched_barrier(0);
            }
            const uint32_t s10 = ps_sum16_pairs<K>(i1.x, i1.y, ptab);
            __builtin_amdgcn_sched_barrier(0);
            const uint32_t s11 = ps_sum16_pairs<K>(i1.y, n1, ptab);
            e.s0 = s00 | (s01 << 16);
            e.s1 = s10 | (s11 << 16);
        }
        e.r0 = r0; e.r1 = r1; e.i0 = i0; e.i1 = i1;
        return clean;
    };
    // (TEST: nothing is stored; the chunks' sums go to e.s0, e.s1, 0 for a word outside the genome; from chunk q0 on)
    auto by_word = [&](const int64_t u, const int c0, Enc &e, const int q0) {
        const int64_t g0 = u * PS_UNIT;
        if constexpr (TEST) e.s0 = e.s1 = 0u;
#pragma unroll 1
        for (int q = q0; q < PS_UNIT / 64; q++) {
            const int64_t g = g0 + q * 64 + lane;
            if (g >= a.total_words) continue;
            int c = c0;
            while (c + 1 < a.n_contigs && a.cd[c + 1].word_off <= g) c++;
            const ContigDesc d = a.cd[c];
            const int64_t w = g - d.word_off, L = d.len, base0 = w * 32;
            uint2 r = make_uint2(0u, 0u), iw = make_uint2(0u, 0u);
            uint32_t s0 = 0, s1 = 0;
            if (w >= 0 && base0 < L) {
                const uint8_t *src = a.ascii + d.ascii_off + base0;
                const uint4 *p = reinterpret_cast<const uint4 *>(src);
                const int nvalid = (L - base0) < 32 ? (int)(L - base0) : 32;
                uint32_t bad;
                r = pack_word(p[0], p[1], nvalid, &bad);
                if (bad) atomicMin(&a.first_bad[c], (unsigned long long)(base0 + __builtin_ctz(bad) + 1));
                iw = interleave_word(r);
                // (a k-mer that reaches into the next word lies in the record: so does what it reads of that word)
                const uint32_t h = base0 + 32 < L ? ps_halo<K>(*reinterpret_cast<const uint2 *>(src + 32)) : 0u;
                const int64_t nk = L - K + 1 - base0;                  // k-mers of the record from the word's first position on
                const int nv0 = nk < 0 ? 0 : nk > 16 ? 16 : (int)nk, nv1 = nk < 16 ? 0 : nk > 32 ? 16 : (int)(nk - 16);
                s0 = ps_sum16_masked<K>(iw.x, iw.y, tab, nv0);
                s1 = ps_sum16_masked<K>(iw.y, h, tab, nv1);
            }
            if constexpr (TEST) (q == 0 ? e.s0 : e.s1) = s0 | (s1 << 16);
            else store(g0 + q * 64, lane, r, iw, s0 | (s1 << 16));
        }
    };

    // The steady loop, per unit u of the wave (cu: u's loads, taken over; nx: those of the wave's next unit, in flight):
    //   encode u -- wait for nx and take it over -- issue the loads of the unit after -- store u.
    // Loads and stores count on one counter (vmcnt), in order: where the loop waits for nx, the only stores not yet acknowledged
    // are those of the unit before u, a whole encode old, and u's own go out behind the new loads with nothing waiting on them.
    // (Taking nx over behind u's stores, as `cu = nx` at the loop's head did, made every unit wait for its predecessor's stores to
    // drain with no load in flight: EXPERIMENTS.md section 16.)  A record lookup, where one runs, waits at the same place.
    if constexpr (TEST) {
        // The same loop over the wave's VISITS: the units of its runs, each run behind its priming visit.  Nothing is stored; a
        // chunk's sums go through the scan, the two lower ends and the test where the storing form stores them.
        // (the host launches this form with fewer than 2^30 units: units, runs and the visit cursor are 32-bit scalars)
        const int R = a.run, nu = (int)n_units, nw = (int)n_waves;
        if (wave0 * R >= n_units) return;
        const int nblk = a.nblk, hb = nblk & 1;                        // nblk = 2 ha + hb
        int lo_idx[2];                                                 // (bpermute takes byte addresses)
        int offer_cur[2];                                              // lanes below it have their reader in this chunk (else in the next)
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int back = (nblk >> 1) + (q < hb ? 1 : 0);
            lo_idx[q] = ((lane - back) & 63) << 2;
            offer_cur[q] = 64 - back;                                  // (a scalar and a compare per use: a lane mask held across the loop costs two)
        }
        uint32_t carry = 0, prevR[2] = {0u, 0u};                       // (block 0 of the genome has nothing in front: 0)
        unsigned int n_primed = 0;
        int v_u0 = (int)wave0 * R, v_i = wave0 == 0 ? 0 : -1;          // the next visit: unit v_u0 + v_i of the run from v_u0 (-1: the priming one)
        auto next = [&](Unit &n) {
            if (v_u0 >= nu) { n.u = -1; n.fast = false; n.ng = 0; return; }
            n.u = v_u0 + v_i;
            n.ng = v_i < 0 ? -1 : 0;
            prepare(n.u, n);
            v_i++;
            if (v_i == R || v_u0 + v_i >= nu) { v_u0 += nw * R; v_i = -1; }
        };
        auto append = [&](const int32_t c, const int32_t gbase, const uint64_t mask) {
            const unsigned int idx = atomicAdd(a.ctl, 1u);
            if (idx < a.cap) {
                FilterEntry fe;
                fe.contig = c; fe.gbase = gbase; fe.mask = mask;
                a.list[idx] = fe;
            }
        };
        // chunk q of the unit: s01 = the lane's two block sums; own: the unit lies in the record the unit names
        auto test = [&](const Unit &un, const bool own, const uint32_t s01, const int q) {
            const uint32_t s1 = s01 >> 16;
            const uint32_t I1 = f_incl_scan((s01 & 0xFFFFu) + s1) + carry;   // (mod 2^32: only differences nblk blocks apart are used)
            carry = (uint32_t)__builtin_amdgcn_readlane((int)I1, 63);
            const uint32_t I[2] = {I1 - s1, I1};
            const uint32_t Rq[2] = {hb ? I[1] : I[0], hb ? I[0] : I[1]};     // the lower end of element q is element (q - hb) & 1 of its source lane
            bool cand[2];
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(lo_idx[e], (int)(lane < offer_cur[e] ? Rq[e] : prevR[e]));
                prevR[e] = Rq[e];
                cand[e] = I[e] - lo >= a.U;
            }
            if (un.prime()) return;
            const int back = q * 128 - (nblk - 1);                     // from the unit's first block to the granule of lane 0's element 0
            if (own) {
                const int gl = un.rel + back + 2 * lane;
                const uint64_t m0 = __ballot(cand[0] & ((uint32_t)gl < (uint32_t)un.ng));
                const uint64_t m1 = __ballot(cand[1] & ((uint32_t)(gl + 1) < (uint32_t)un.ng));
                if (__builtin_expect((m0 | m1) != 0, 0)) {             // rare: entry e holds the blocks 64 e ... 64 e + 63 of the chunk
                    const uint64_t mine = (lane & 1) ? m1 : m0;
#pragma unroll 1
                    for (int e = 0; e < 2; e++) {
                        const uint64_t me = __ballot(((mine >> (32 * e + (lane >> 1))) & 1u) != 0);
                        if (me != 0 && lane == 0) append(un.c, un.rel + back + 64 * e, me);
                    }
                }
            } else if (__builtin_expect(cand[0] | cand[1], 0)) {       // rare: every candidate lane finds its block's record
#pragma unroll 1
                for (int e = 0; e < 2; e++) {
                    const int64_t B = (int64_t)un.u * (2 * PS_UNIT) + back + 2 * lane + e, w = B >> 1;
                    if (!cand[e] || B < 0 || w >= a.total_words) continue;
                    int c = a.block_contig[w >> a.block_shift];
                    while (c + 1 < a.n_contigs && a.cd[c + 1].word_off <= w) c++;
                    const ContigDesc d = a.cd[c];
                    const int64_t g = B - 2 * d.word_off, nwin = d.len - (a.nk + K - 1) + 1;
                    if (g >= 0 && nwin > 0 && g < ((nwin + 15) >> 4)) append(c, (int32_t)g, 1u);
                }
            }
        };
        Unit cu, nx;
        cu.c = nx.c = 0; cu.fast = nx.fast = false; cu.u = nx.u = -1; cu.rel = nx.rel = cu.ng = nx.ng = 0;
        nx.halo = cu.halo = make_uint2(0u, 0u);
#pragma unroll
        for (int i = 0; i < 4; i++) nx.v[i] = cu.v[i] = u32x4_t{0u, 0u, 0u, 0u};
        next(cu);
        next(nx);
#pragma unroll
        for (int i = 0; i < 4; i++) asm volatile("" : "+v"(cu.v[i]));
        asm volatile("" : "+v"(cu.halo.x), "+v"(cu.halo.y));
        while (cu.u >= 0) {
            Enc e;
            const bool clean = encode(cu, e);
            if (__builtin_expect(!clean, 0)) {
                by_word(cu.u, cu.c, e, cu.prime() ? 1 : 0);
                if (!cu.prime() && lane == 0) atomicAdd(a.ctl + 1, 1u);  // units that went word by word (kgma_get_pack_test_stats)
            }
            if (!cu.prime()) test(cu, clean, e.s0, 0);
            else n_primed++;
            test(cu, clean, e.s1, 1);
            __builtin_amdgcn_sched_barrier(0);
            cu = nx;
#pragma unroll
            for (int i = 0; i < 4; i++) asm volatile("" : "+v"(cu.v[i]));
            asm volatile("" : "+v"(cu.halo.x), "+v"(cu.halo.y));
            next(nx);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (lane == 0 && n_primed != 0) atomicAdd(a.ctl + 2, n_primed);   // chunks primed (kgma_get_pack_test_stats)
        return;
    }
    if (wave0 >= n_units) return;
    Unit cu, nx;
    nx.c = 0; nx.fast = false; nx.halo = cu.halo = make_uint2(0u, 0u);
#pragma unroll
    for (int i = 0; i < 4; i++) nx.v[i] = cu.v[i] = u32x4_t{0u, 0u, 0u, 0u};
    prepare(wave0, cu);
    if (wave0 + n_waves < n_units) prepare(wave0 + n_waves, nx);
    // (the first unit's loads are waited for here: a wait for them at the loop's head would stand in every iteration, behind the
    //  stores and the new loads)
#pragma unroll
    for (int i = 0; i < 4; i++) asm volatile("" : "+v"(cu.v[i]));
    asm volatile("" : "+v"(cu.halo.x), "+v"(cu.halo.y));
    for (int64_t u = wave0; u < n_units; u += n_waves) {
        Enc e;
        const int c0 = cu.c;
        const bool clean = encode(cu, e);
        if (!clean) by_word(u, c0, e, 0);                              // (with its own loads and stores, and one buffer less alive)
        __builtin_amdgcn_sched_barrier(0);
        cu = nx;
        // (the copy is pinned here: left to the compiler it sinks to the back-edge, behind the stores)
#pragma unroll
        for (int i = 0; i < 4; i++) asm volatile("" : "+v"(cu.v[i]));
        asm volatile("" : "+v"(cu.halo.x), "+v"(cu.halo.y));
        if (u + 2 * n_waves < n_units) prepare(u + 2 * n_waves, nx);
        __builtin_amdgcn_sched_barrier(0);
        if (clean) {
            store(u * PS_UNIT, lane, e.r0, e.i0, e.s0);
            store(u * PS_UNIT + 64, lane, e.r1, e.i1, e.s1);
        }
    }
}

// count of entries (it keeps counting past the capacity) to the pinned mirror; the device counter is left at zero for the next scan
__global__ void filter_publish_kernel(unsigned int *ctl, unsigned int *host)
{
    if (threadIdx.x == 0) {
        host[0] = __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(ctl, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the testing pack's three counters (entries, units that went word by word, chunks primed) to the pinned mirror, and back to zero
__global__ void pack_test_publish_kernel(unsigned int *ctl, unsigned int *host)
{
    if (threadIdx.x < 3) {
        host[threadIdx.x] = __hip_atomic_load(ctl + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(ctl + threadIdx.x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

bool filter_applies(int k, int64_t s_max) { return (k == 5 || k == 6) && s_max >= 0 && s_max <= 65535; }

static int64_t filter_grid(const FilterArgs &a, int n_cus, int per_cu)
{
    int64_t grid = (int64_t)n_cus * per_cu;
    const int64_t need = ((int64_t)a.n_tiles + 15) / 16;
    if (grid > need) grid = need;
    return grid < 1 ? 1 : grid;
}

template <int K, int ES, int COPIES>
static hipError_t filter_launch(const FilterArgs &a, int n_cus, hipStream_t st)
{
    constexpr size_t lds = ((size_t)1 << (2 * K)) * ES * COPIES;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&filter_kernel<K, ES, COPIES>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    // persistent waves: every CU's wave slots once (one 16-wave workgroup where the copies fill the LDS, else two)
    hipLaunchKernelGGL((filter_kernel<K, ES, COPIES>), dim3((unsigned)filter_grid(a, n_cus, lds > (64u << 10) ? 1 : 2)), dim3(1024), lds, st, a);
    return hipGetLastError();
}

static hipError_t filter_sums_launch(const FilterArgs &a, int k, int n_cus, hipStream_t st)
{
    int per_cu = 2;
    if (const char *w = getenv("KGMA_FILTER_WGS")) per_cu = atoi(w) == 1 ? 1 : 2;       // experiments (EXPERIMENTS.md section 14)
    const dim3 grid((unsigned)filter_grid(a, n_cus, per_cu));
    switch (a.nblk & 3) {
    case 0: hipLaunchKernelGGL(filter_sums_kernel<0>, grid, dim3(1024), 0, st, a, k); break;
    case 1: hipLaunchKernelGGL(filter_sums_kernel<1>, grid, dim3(1024), 0, st, a, k); break;
    case 2: hipLaunchKernelGGL(filter_sums_kernel<2>, grid, dim3(1024), 0, st, a, k); break;
    default: hipLaunchKernelGGL(filter_sums_kernel<3>, grid, dim3(1024), 0, st, a, k); break;
    }
    return hipGetLastError();
}

bool pack_sums_applies(int k, int64_t s_max) { return (k == 5 || k == 6) && s_max >= 0 && s_max < 256; }

template <int K, bool COPY, bool TEST = false>
static hipError_t pack_sums_launch(const PackSumsArgs &a, int n_cus, hipStream_t st)
{
    constexpr size_t lds = ((size_t)1 << (2 * K)) * 9;                 // 4^(K+1) uint16 + 4^K bytes
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&pack_sums_kernel<K, COPY, TEST>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    // persistent waves: one 16-wave workgroup per CU (at up to 128 VGPRs a second one would not be resident beside it)
    int64_t grid = n_cus;
    if (const char *w = getenv("KGMA_PACK_WGS")) {                     // tests and experiments: at most so many workgroups, 1 ... CUs
        const int64_t n = atoll(w);
        grid = n < 1 ? 1 : n < n_cus ? n : n_cus;
    }
    const int64_t units = (a.total_words + PS_UNIT - 1) / PS_UNIT;
    const int64_t need = ((TEST ? (units + a.run - 1) / a.run : units) + 15) / 16;     // (TEST: a wave takes whole runs)
    if (grid > need) grid = need;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL((pack_sums_kernel<K, COPY, TEST>), dim3((unsigned)grid), dim3(1024), lds, st, a);
    return hipGetLastError();
}

// waves the sums-only pack runs on a device of n_cus CUs (the in-pack test's size gate counts runs per wave)
int64_t pack_sums_waves(int n_cus)
{
    int64_t grid = n_cus;
    if (const char *w = getenv("KGMA_PACK_WGS")) {
        const int64_t n = atoll(w);
        grid = n < 1 ? 1 : n < n_cus ? n : n_cus;
    }
    return 16 * grid;
}

// sums_only: the form that stores no word of the 2-bit copy (a genome that keeps planes has no such form: they are written with it)
hipError_t launch_pack_sums(const PackSumsArgs &a, int k, int64_t s_max, int n_cus, bool sums_only, hipStream_t st, unsigned int *host_count)
{
    if (!pack_sums_applies(k, s_max) || a.total_words <= 0 || a.block_shift < 0 || ((int64_t)1 << a.block_shift) % PS_UNIT != 0) return hipErrorInvalidValue;
    if (sums_only && a.planes != nullptr) return hipErrorInvalidValue;
    if (a.list != nullptr) {                                           // the testing form: host_count gets its four counters
        const int64_t units = (a.total_words + PS_UNIT - 1) / PS_UNIT;
        if (units + (int64_t)n_cus * 16 * a.run >= ((int64_t)1 << 30)) return hipErrorInvalidValue;
        if (!sums_only || a.nblk < 1 || a.nblk > 63 || a.run < 1 || a.nk < 1 || a.ctl == nullptr || host_count == nullptr) return hipErrorInvalidValue;
        const hipError_t e = k == 5 ? pack_sums_launch<5, false, true>(a, n_cus, st) : pack_sums_launch<6, false, true>(a, n_cus, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(pack_test_publish_kernel, dim3(1), dim3(64), 0, st, a.ctl, host_count);
        return hipGetLastError();
    }
    if (sums_only) return k == 5 ? pack_sums_launch<5, false>(a, n_cus, st) : pack_sums_launch<6, false>(a, n_cus, st);
    return k == 5 ? pack_sums_launch<5, true>(a, n_cus, st) : pack_sums_launch<6, true>(a, n_cus, st);
}

// *form: the instantiation launched, S entry bytes | table copies << 8 (kgma_filter_stats::form); bit 16: filter_sums_kernel, on the
// block sums a.bsum that pack_sums_kernel wrote (byte entries only)
hipError_t launch_filter(const FilterArgs &a, int k, int64_t s_max, int n_cus, unsigned int *host_count, int32_t *form, hipStream_t st)
{
    if (!filter_applies(k, s_max) || a.nblk < 1 || a.nblk > 63) return hipErrorInvalidValue;
    const int es = s_max < 256 ? 1 : 2, copies = k == 6 && es == 2 ? 1 : 32;
    const bool presummed = a.bsum != nullptr;
    if (presummed && es != 1) return hipErrorInvalidValue;
    hipError_t e;
    if (presummed) e = filter_sums_launch(a, k, n_cus, st);
    else if (k == 5) e = es == 1 ? filter_launch<5, 1, 32>(a, n_cus, st) : filter_launch<5, 2, 32>(a, n_cus, st);
    else e = es == 1 ? filter_launch<6, 1, 32>(a, n_cus, st) : filter_launch<6, 2, 1>(a, n_cus, st);
    if (e != hipSuccess) return e;
    *form = es | (copies << 8) | (presummed ? 1 << 16 : 0);
    hipLaunchKernelGGL(filter_publish_kernel, dim3(1), dim3(64), 0, st, a.ctl, host_count);
    return hipGetLastError();
}

}  // namespace kgma
