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

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kgma_device.h"

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

// ES: bytes per S entry (1: every S < 256, 2: < 65536); COPIES: 32 bank-interleaved copies, or 1
template <int K, int ES, int COPIES>
__global__ __launch_bounds__(1024) void filter_kernel(FilterArgs a)
{
    constexpr int NB = 1 << (2 * K);
    constexpr uint32_t KM = (uint32_t)NB - 1u;
    constexpr int EPD = 4 / ES;                                        // entries per dword
    extern __shared__ uint32_t fsm[];
    // dword (x / EPD) of copy c is LDS dword (x / EPD) * COPIES + c
    for (int t = (int)threadIdx.x; t < NB / EPD * COPIES; t += (int)blockDim.x) {
        const int d = t / COPIES;
        uint32_t v = 0;
#pragma unroll
        for (int e = 0; e < EPD; e++) v |= (uint32_t)a.S[d * EPD + e] << (8 * ES * e);
        fsm[t] = v;
    }
    __syncthreads();
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

// count of entries (it keeps counting past the capacity) to the pinned mirror; the device counter is left at zero for the next scan
__global__ void filter_publish_kernel(unsigned int *ctl, unsigned int *host)
{
    if (threadIdx.x == 0) {
        host[0] = __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(ctl, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

bool filter_applies(int k, int64_t s_max) { return (k == 5 || k == 6) && s_max >= 0 && s_max <= 65535; }

template <int K, int ES, int COPIES>
static hipError_t filter_launch(const FilterArgs &a, int n_cus, hipStream_t st)
{
    constexpr size_t lds = ((size_t)1 << (2 * K)) * ES * COPIES;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&filter_kernel<K, ES, COPIES>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    // persistent waves: every CU's wave slots once (one 16-wave workgroup where the copies fill the LDS, else two)
    const int per_cu = lds > (64u << 10) ? 1 : 2;
    int64_t grid = (int64_t)n_cus * per_cu;
    const int64_t need = ((int64_t)a.n_tiles + 15) / 16;
    if (grid > need) grid = need;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL((filter_kernel<K, ES, COPIES>), dim3((unsigned)grid), dim3(1024), lds, st, a);
    return hipGetLastError();
}

// *form: the instantiation launched, S entry bytes | table copies << 8 (kgma_filter_stats::form)
hipError_t launch_filter(const FilterArgs &a, int k, int64_t s_max, int n_cus, unsigned int *host_count, int32_t *form, hipStream_t st)
{
    if (!filter_applies(k, s_max) || a.nblk < 1 || a.nblk > 63) return hipErrorInvalidValue;
    const int es = s_max < 256 ? 1 : 2, copies = k == 6 && es == 2 ? 1 : 32;
    hipError_t e;
    if (k == 5) e = es == 1 ? filter_launch<5, 1, 32>(a, n_cus, st) : filter_launch<5, 2, 32>(a, n_cus, st);
    else e = es == 1 ? filter_launch<6, 1, 32>(a, n_cus, st) : filter_launch<6, 2, 1>(a, n_cus, st);
    if (e != hipSuccess) return e;
    *form = es | (copies << 8);
    hipLaunchKernelGGL(filter_publish_kernel, dim3(1), dim3(64), 0, st, a.ctl, host_count);
    return hipGetLastError();
}

}  // namespace kgma
