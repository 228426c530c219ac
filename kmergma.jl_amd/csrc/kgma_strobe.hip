// kgma_strobe.hip -- the strobemer engine (StrobeGMA!, src/StrobemerGMA/StrobeGenomeMiner.jl:5-95) as a count-table stream walk:
// the integer form of gen_kernel (kgma_generic.hip) with counters in LDS, a randstrobe bin in the place of the k-mer.
//
// What the reference computes per record (read literally).  A randstrobe of the k = w_max + s - 1 residues at a position
// (Strobemers.jl:45-65): `first` is the s-mer at offset 1; because `min_score::Int = 2 << 63` is 0 and the test is `<=`, the second
// s-mer is the one at the LAST offset i in w_min..w_max with (as_UInt(first) + as_UInt(s-mer at i)) % q == 0, at w_min if there is
// none; the bin is first * 4^s + second (natural values).  The scan (StrobeGenomeMiner.jl:48-67) removes the strobemer starting at
// i and "enters" the one read from view(seq, i+W-k : i+W), which starts at i + W - k: the LAST strobemer of the window before it.
// So after step i the count vector holds the W - k strobemers starting at i+1 .. i+W-k plus one copy of the record's strobemer
// W-k+1 that never leaves: a sliding scan of nk = W - k items over the strobemer stream, window start q = i + 1 for
// q = 1 .. L - W (q = 1 is the first window, never tested), over counts that carry one permanent extra item per record.
//
// ONE WAVE owns a stream (a run of consecutive window starts of one record), keeps the 4^(2s) 16-bit counts of its window in LDS
// and advances 64 windows per step (lane = window); the counts of bins that several lanes of a step touch are corrected with
// ballots of the lower lanes' transitions, exactly as in gen_kernel.  The permanent item is the first one inserted in every
// stream's warm-up (its position follows from the stream descriptor: the record starts win0 - 1 residues before the stream), so
// the first-window identity D0 = sum S^2 - 2N sum_p S[x_p] + N^2 (n + 2 pairs) holds with n = nk + 1 items.
//   e = S[l] - S[r] - N (c[l] - 1 - c[r]),  E = (D - D0) / 2N as an int64 prefix, compared with (T - D0) / 2N.
// Records are REC_WIDE (int64 E), D0out and the distance array as gen_kernel writes them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#include "kgma_device.h"
#include "kgma_strobe_bin.h"

namespace kgma {

namespace {

__device__ __forceinline__ int s_uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ int64_t s_uni64(int64_t v)
{
    return (int64_t)(((uint64_t)(uint32_t)s_uni((int)(uint32_t)((uint64_t)v >> 32)) << 32) | (uint32_t)s_uni((int)(uint32_t)v));
}
__device__ __forceinline__ int64_t s_shfl_xor64(int64_t v, int d)
{
    const int lo = __shfl_xor((int)(uint32_t)v, d), hi = __shfl_xor((int)(uint32_t)((uint64_t)v >> 32), d);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ int64_t s_readlane64(int64_t v, int l)
{
    const int lo = __builtin_amdgcn_readlane((int)(uint32_t)v, l), hi = __builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), l);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
template <int CTRL, int ROWS>
__device__ __forceinline__ int64_t s_dpp64(int64_t v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, ROWS, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)((uint64_t)v >> 32), CTRL, ROWS, 0xF, false);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
// wave-wide inclusive prefix sum on the DPP network
__device__ __forceinline__ int64_t s_scan(int64_t v)
{
    v += s_dpp64<0x111, 0xF>(v);      // row_shr:1
    v += s_dpp64<0x112, 0xF>(v);      // row_shr:2
    v += s_dpp64<0x114, 0xF>(v);      // row_shr:4
    v += s_dpp64<0x118, 0xF>(v);      // row_shr:8
    v += s_dpp64<0x142, 0xA>(v);      // row_bcast:15 -> rows 1, 3
    v += s_dpp64<0x143, 0xC>(v);      // row_bcast:31 -> rows 2, 3
    return v;
}
__device__ __forceinline__ int64_t s_sum(int64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += s_shfl_xor64(v, d);
    return v;
}
__device__ __forceinline__ int64_t s_min(int64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const int64_t o = s_shfl_xor64(v, d); v = o < v ? o : v; }
    return v;
}

// (the randstrobe bin of 16 packed residues, strobe_bin<SS>: kgma_strobe_bin.h)

}  // namespace

template <int SS>
__global__ __launch_bounds__(1024) void strobe_kernel(ScanArgs a, StrobeParams g)
{
    constexpr int NB = 1 << (4 * SS);                                 // bins
    constexpr int CW = NB / 2;                                        // dwords of a wave's count table (two 16-bit counters each)
    extern __shared__ __attribute__((aligned(16))) uint32_t ssmem[];  // [S table: NB int32][count tables of the waves]
    const int lane = threadIdx.x & 63;
    const int wave = s_uni((int)(threadIdx.x >> 6));
    const int nw = (int)(blockDim.x >> 6);
    const int slot = (int)blockIdx.x * nw + wave;
    const int nk = g.nk;
    const int w_min = g.w_min, w_max = g.w_max;
    const uint32_t z0 = g.zero[0], z1 = g.zero[1], z2 = g.zero[2], z3 = g.zero[3];
    uint32_t *const C = ssmem + NB + (size_t)wave * (size_t)CW;
    for (int i = threadIdx.x; i < NB; i += blockDim.x) reinterpret_cast<int32_t *>(ssmem)[i] = g.S[i];
    __syncthreads();                                                  // (the only workgroup barrier: every wave reaches it)
    const int32_t *St = reinterpret_cast<const int32_t *>(ssmem);
    const int kid = g.kfv_id;
    const int64_t Nn = g.N, twoN = 2 * (int64_t)g.N;
    double *dist = a.dist[0];

    for (int tile = slot; tile < a.n_tiles; tile += g.n_slots) {
        for (int i = lane; i < CW; i += 64) C[i] = 0;
        const TileDesc td = a.tiles[tile];
        const int n_valid = td.n_valid, first_test = td.first_test;
        const uint32_t *gi = a.inter + 2 * td.word_base;              // 2-bit codes, 16 residues per dword, first residue = bits 0-1
        const int n_pos = n_valid + nk - 1;
        const int n_blocks = (n_pos + 63) >> 6;
        // the record's permanent item: its strobemer at 0-based position nk.  Streams start on 64-window boundaries, so the record
        // starts a whole number of dwords ((win0 - 1) / 16) before the stream.
        int64_t wsum;
        {
            const uint32_t *gr = gi - ((td.win0 - 1) >> 4);
            const uint32_t xw = __builtin_amdgcn_alignbit(gr[(nk >> 4) + 1], gr[nk >> 4], 2u * (uint32_t)(nk & 15));
            const uint32_t xb = (uint32_t)s_uni((int)strobe_bin<SS>(xw, w_min, w_max, z0, z1, z2, z3));
            if (lane == 0) atomicAdd(&C[xb >> 1], 1u << (16u * (xb & 1u)));   // (LDS operations of a wave complete in order: after the clear)
            wsum = St[xb];
        }
        int64_t pairs = 0;
        int64_t D0 = 0;                                               // exact D of the stream's first window
        int64_t TE = 0, TEhi = 0;                                     // E < TE below thr; TE <= E < TEhi at threshold
        int64_t carry = 0;
        // dip under construction (wave-uniform)
        int in_run = 0, run_start = 0, argf = 0, argl = 0, nmin = 0;
        int64_t minV = 0;

        // genome words of a step: the dword pair holding the 16 residues at position 64 b + lane (the entering strobemer) and the
        // pair of the leaving one (nk positions back; none yet in the warm-up).  Reads run up to a step past the stream's end: the
        // genome buffer is padded by more than that.
        auto load_words = [&](const int bb, uint32_t &e0, uint32_t &e1, uint32_t &l0, uint32_t &l1) {
            const int pp = (bb << 6) + lane;
            const int ie = pp >> 4, il = (pp >= nk ? pp - nk : 0) >> 4;
            e0 = gi[ie]; e1 = gi[ie + 1]; l0 = gi[il]; l1 = gi[il + 1];
        };
        uint32_t pe0, pe1, pl0, pl1;
        load_words(0, pe0, pe1, pl0, pl1);
        for (int b = 0; b < n_blocks; b++) {
            const int p = (b << 6) + lane;
            const bool haveL = p >= nk;
            const uint32_t kp = strobe_bin<SS>(__builtin_amdgcn_alignbit(pe1, pe0, 2u * (uint32_t)(p & 15)), w_min, w_max, z0, z1, z2, z3);
            uint32_t ks;
            {
                const int pl = haveL ? p - nk : 0;
                ks = strobe_bin<SS>(__builtin_amdgcn_alignbit(pl1, pl0, 2u * (uint32_t)(pl & 15)), w_min, w_max, z0, z1, z2, z3);
                ks = haveL ? ks : kp;
            }
            const int64_t tab_p = St[kp], tab_l = St[ks];
            load_words(b + 1, pe0, pe1, pl0, pl1);                    // the next step's genome words, one step ahead
            const bool differ = kp != ks;                             // StrobeGenomeMiner.jl:59: nothing happens if left == right
            const bool actE = differ || !haveL, actL = differ && haveL;
            // start-of-step counts, this lane's transition applied, and the counts the returning operations saw
            uint32_t cp, cs, oldp, olds;
            {
                const uint32_t shp = 16u * (kp & 1u), shs = 16u * (ks & 1u);
                uint32_t wop = 0, wos = 0;
                const uint32_t wcp = C[kp >> 1];                      // (LDS operations of a wave complete in order)
                const uint32_t wcs = C[ks >> 1];
                if (actE) wop = atomicAdd(&C[kp >> 1], 1u << shp);
                if (actL) wos = atomicSub(&C[ks >> 1], 1u << shs);
                cp = (wcp >> shp) & 0xFFFFu; cs = (wcs >> shs) & 0xFFFFu;
                oldp = (wop >> shp) & 0xFFFFu; olds = (wos >> shs) & 0xFFFFu;
            }
            // exact counts of the entering / leaving bin in THIS lane's window: the value read, corrected by the transitions of the
            // lower lanes wherever another lane of the step touched the bin (windows shorter than a step can enter and leave a bin
            // inside one step, whose transient counts could hide that: there every acting lane takes the correction rounds)
            int32_t cP, cS;
            {
                const bool all = nk < 64;
                uint64_t pendE = __ballot(actE && (all || oldp != cp)), pendL = __ballot(actL && (all || olds != cs));
                int32_t corrP = 0, corrS = 0;
                if (pendE | pendL) {
                    const uint64_t AE = __ballot(actE), AL = __ballot(actL);
                    while ((pendE | pendL) != 0) {
                        uint32_t x0;
                        if (pendE) x0 = (uint32_t)__builtin_amdgcn_readlane((int)kp, __builtin_ctzll(pendE));
                        else x0 = (uint32_t)__builtin_amdgcn_readlane((int)ks, __builtin_ctzll(pendL));
                        const uint64_t eqP = __ballot(kp == x0), eqS = __ballot(ks == x0);
                        const uint64_t ME = eqP & AE, ML = eqS & AL;
                        const int32_t ne = (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(ME >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ME, 0u));
                        const int32_t nl = (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(ML >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ML, 0u));
                        corrP = kp == x0 ? ne - nl : corrP;
                        corrS = ks == x0 ? ne - nl : corrS;
                        pendE &= ~eqP;
                        pendL &= ~eqS;
                    }
                }
                cP = (int32_t)cp + corrP;
                cS = (int32_t)cs + corrS;
            }
            int64_t e = 0;
            if (actL) e = tab_l - tab_p - Nn * (int64_t)(cS - 1 - cP);
            if ((b << 6) < nk) {                                      // warm-up steps: the stream's first window
                const bool wu = p < nk;
                wsum += s_sum(wu ? tab_p : 0);
                pairs += s_sum(wu ? (int64_t)cP : 0);
                if (nk - 1 < (b << 6) + 64) {
                    // sum (S - N c)^2 = sum S^2 - 2N sum_p S[x_p] + N^2 (n + 2 pairs) over the n = nk + 1 items of the window
                    D0 = s_uni64(g.sumS2 - twoN * wsum + Nn * Nn * ((int64_t)nk + 1 + 2 * pairs));
                    if (lane == 0) a.D0out[(size_t)(kid - 1) * a.n_tiles + tile] = D0;
                    // E < TE  <=>  D0 + 2N E < T;  TE <= E < TEhi  <=>  T <= D <= T_hi
                    const int64_t num = g.T - D0;
                    TE = num > 0 ? (num + twoN - 1) / twoN : -((-num) / twoN);
                    const int64_t numh = g.T_hi - D0;
                    const int64_t TH = numh >= 0 ? numh / twoN : -((-numh + twoN - 1) / twoN);
                    TEhi = g.T_hi >= g.T && TH + 1 > TE ? TH + 1 : TE;
                    TE = s_uni64(TE); TEhi = s_uni64(TEhi);
                }
            }
            const int64_t val = carry + s_scan(e);                    // E of the window this lane's transition leads to
            carry = s_readlane64(val, 63);
            const int q = p - nk + 1;                                 // window start (local)
            const bool tested = q >= first_test && q < n_valid;
            const bool under = tested && val < TE;
            const bool att = tested && !under && val < TEhi;
            if (dist != nullptr && tested) dist[td.dist_base + q] = (double)(D0 + twoN * val) / g.inv_scale;
            const uint64_t U = __ballot(under), A = __ballot(att);
            if ((U | A) == 0 && !in_run) continue;

            // ---- a dip touches this step -------------------------------------------------------------------------------
            const int q0 = (b << 6) - nk + 1;
            if (att) {
                DevRecord rec;
                rec.tile = tile; rec.kind_kfv = REC_ATT | REC_WIDE | (kid << 8);
                rec.start = q; rec.end = q; rec.argf = rec.argl = q; rec.nmin = 0; rec.has_exit = 0;
                rec.minE = rec.exitE = (int32_t)(uint32_t)val; rec.minE_hi = rec.exitE_hi = (int32_t)(uint32_t)((uint64_t)val >> 32);
                const unsigned int idx = atomicAdd(a.rec_count, 1u);
                if (idx < a.rec_cap) a.recs[idx] = rec;
                atomicAdd(a.n_att, 1ull);
            }
            int cursor = 0;
            while (cursor < 64) {
                const uint64_t rem = ~(uint64_t)0 << cursor;
                if (in_run) {
                    const uint64_t nz = ~U & rem;
                    const int end_lane = nz ? __builtin_ctzll(nz) : 64;
                    if (end_lane > cursor) {
                        const bool inseg = lane >= cursor && lane < end_lane;
                        const int64_t segmin = s_min(inseg ? val : INT64_MAX);
                        const uint64_t eq = __ballot(inseg && val == segmin);
                        const int fl = __builtin_ctzll(eq);
                        const int ll2 = 63 - __builtin_clzll(eq), pc = __builtin_popcountll(eq);
                        if (nmin == 0 || segmin < minV) { minV = segmin; argf = q0 + fl; argl = q0 + ll2; nmin = pc; }
                        else if (segmin == minV) { argl = q0 + ll2; nmin += pc; }
                    }
                    if (end_lane < 64) {
                        const int qe = q0 + end_lane;
                        const int64_t exitV = s_readlane64(val, end_lane);
                        if (lane == 0) {
                            DevRecord rec;
                            rec.tile = tile; rec.kind_kfv = REC_RUN | REC_WIDE | (kid << 8);
                            rec.start = run_start; rec.end = qe - 1; rec.argf = argf; rec.argl = argl; rec.nmin = nmin;
                            rec.has_exit = qe < n_valid ? 1 : 0;
                            rec.minE = (int32_t)(uint32_t)minV; rec.minE_hi = (int32_t)(uint32_t)((uint64_t)minV >> 32);
                            rec.exitE = (int32_t)(uint32_t)exitV; rec.exitE_hi = (int32_t)(uint32_t)((uint64_t)exitV >> 32);
                            const unsigned int idx = atomicAdd(a.rec_count, 1u);
                            if (idx < a.rec_cap) a.recs[idx] = rec;
                        }
                        in_run = 0;
                        cursor = end_lane;
                    } else {
                        cursor = 64;
                    }
                } else {
                    const uint64_t nu = U & rem;
                    if (!nu) break;
                    cursor = __builtin_ctzll(nu);
                    in_run = 1; run_start = q0 + cursor; nmin = 0; minV = 0; argf = argl = run_start;
                }
            }
        }
        // a run still open at the end of the stream (the host joins it with the next stream's)
        if (in_run && lane == 0) {
            DevRecord rec;
            rec.tile = tile; rec.kind_kfv = REC_RUN | REC_WIDE | (kid << 8);
            rec.start = run_start; rec.end = n_valid - 1; rec.argf = argf; rec.argl = argl; rec.nmin = nmin;
            rec.has_exit = 0;
            rec.minE = (int32_t)(uint32_t)minV; rec.minE_hi = (int32_t)(uint32_t)((uint64_t)minV >> 32);
            rec.exitE = 0; rec.exitE_hi = 0;
            const unsigned int idx = atomicAdd(a.rec_count, 1u);
            if (idx < a.rec_cap) a.recs[idx] = rec;
        }
    }
}

// ---- geometry + launch ----------------------------------------------------------------------------------------------
namespace {

const void *strobe_fn(int s)
{
    if (s == 1) return reinterpret_cast<const void *>(&strobe_kernel<1>);
    if (s == 2) return reinterpret_cast<const void *>(&strobe_kernel<2>);
    return reinterpret_cast<const void *>(&strobe_kernel<3>);
}
// sixteen waves per workgroup: [S table 4 * 4^(2s) bytes | 16 count tables of 2 * 4^(2s) bytes] = 144 KiB at s = 3, 9 KiB at s = 2
constexpr int STROBE_NW = 16;
size_t strobe_lds(int s) { return ((size_t)4 << (4 * s)) + (size_t)STROBE_NW * ((size_t)2 << (4 * s)); }

}  // namespace

// streams resident per CU (what the host sizes the stream table for)
int strobe_slots_per_cu(int s)
{
    if (s < 1 || s > KGMA_STROBE_MAX_S) return 0;
    const void *fn = strobe_fn(s);
    int blocks = 0;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)strobe_lds(s)) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, 64 * STROBE_NW, strobe_lds(s)) != hipSuccess || blocks < 1) {
        (void)hipGetLastError();
        blocks = 1;
    }
    if (blocks * STROBE_NW > 32) blocks = 32 / STROBE_NW;
    return STROBE_NW * blocks;
}

hipError_t launch_strobe(const ScanArgs &a, const StrobeParams &g, hipStream_t st)
{
    if (a.n_tiles <= 0) return hipSuccess;
    if (g.s < 1 || g.s > KGMA_STROBE_MAX_S || g.w_min < 1 || g.w_min > g.w_max || g.w_max + g.s - 1 > KGMA_STROBE_MAX_K || g.nk < 1 ||
        g.nk + 1 > KGMA_MAX_NK_WIDE || g.S == nullptr || g.n_slots < STROBE_NW || g.n_slots % STROBE_NW != 0)
        return hipErrorInvalidConfiguration;
    const void *fn = strobe_fn(g.s);
    const size_t lds = strobe_lds(g.s);
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    ScanArgs a_copy = a;
    StrobeParams g_copy = g;
    void *args[2] = {&a_copy, &g_copy};
    return hipLaunchKernel(fn, dim3((unsigned)(g.n_slots / STROBE_NW)), dim3(64u * (unsigned)STROBE_NW), args, lds, st);
}

}  // namespace kgma
