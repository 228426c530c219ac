// kgma_approx.hip -- semi-global edit-distance search over the resident genome (approxMatch; semantics: include/kgma.h): every
// end position j of every record at which score(j) = min_s ed(query, t[s..j]) is at most the query's max_edits, and for each
// reported end the start of the shortest substring that attains the score.  Myers' bit-vector algorithm (J. ACM 46(3), 1999) in
// Hyyro's formulation: the column of the dynamic programme is held as vertical delta vectors Pv / Mv, one bit per query symbol.
//
//   approx_kernel<WORDS>   a lane owns AP_TILE consecutive end positions of one record, a workgroup AP_WG_BASES; no workgroup spans
//                          two records (per-record prefix of workgroup counts, binary search per workgroup, as kgma_exact.hip does
//                          with its tiles).  The workgroup loads its residues and the AP_LEAD before them from the residue text
//                          (1 byte per base, N kept: the 2-bit copies store N as T) with 16-byte loads, contiguous over the
//                          lanes, and keeps them in LDS as residue classes; a lane's tile is AP_TILE / 4 dwords of it, and a pad
//                          dword per tile puts the lanes of a wave on 32 different banks.  Then it loops over the queries of the
//                          batch with the text in LDS.  Per query a lane starts from the fresh state (Pv = ones, Mv = 0,
//                          score = m) m + max_edits columns before its first end, rounded up to whole dwords -- a substring
//                          within e edits of the query is at most m + e long, so the restarted state is >= the true one
//                          everywhere and equal to it wherever the true one is <= e -- and reports only the ends it owns.
//                          Where there is no residue (before a record's first) the text holds a class no symbol matches, which
//                          leaves a fresh state fresh.  The query sits at the TOP of the vectors (its last symbol is the top bit):
//                          the score's delta is the bit a shift by one pushes out, whatever m is, and the bits below the query
//                          stay Pv = 1, Mv = 0 and never carry into it.  Peq of the current query, one mask per class, is a 64-byte
//                          table in LDS: a column's lookup is one read at few distinct addresses (broadcast).
//                          WORDS = 2: m <= 64 in a 64-bit vector (32-bit add plus carry); WORDS = 1: m <= 32 in the upper word.
//   approx_start_kernel    a lane per reported end: the anchored form of the recurrence (the horizontal delta of row 0 is +1) on
//                          the reversed query against t[j], t[j-1], ...; the first column c >= 1 whose score equals the end's
//                          edits gives start = j - c + 1.  It exists within m + edits columns and inside the record.
//
// Emission is that of the other searches: ballot, wave prefix, one atomicAdd per wave on a cursor that keeps counting past the
// buffer's capacity (the host regrows and runs again).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kgma_approx.h"

namespace kgma {

namespace {

constexpr int TILE_DWORDS = AP_TILE / 4;
constexpr int LANE_STRIDE = TILE_DWORDS + 1;                       // dwords: odd, so 32 lanes hit 32 banks
constexpr int TEXT_DWORDS = (AP_THREADS + 1) * LANE_STRIDE;        // block 0 holds the lead (its last AP_LEAD bytes)
constexpr int N_CHUNKS = (AP_LEAD + AP_WG_BASES) / 16;
constexpr uint32_t NO_RESIDUE4 = 0x01010101u * AP_NO_RESIDUE;

template <int WORDS> struct Bits;
template <> struct Bits<1> { typedef uint32_t type; };
template <> struct Bits<2> { typedef uint64_t type; };

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

// four residues -> four classes, each times 8 (the byte offset of its Peq entry): ((b >> 1) & 7) << 3
__device__ __forceinline__ uint32_t class_offsets(uint32_t x) { return (x << 2) & 0x38383838u; }

// the lanes with `ok` append one hit each: one atomicAdd per wave
__device__ __forceinline__ void emit(bool ok, const ApproxArgs &a, int query, int contig, int64_t end1, int edits)
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
        ApproxHit h;
        h.query = query; h.contig = contig; h.start = 0; h.end = end1; h.edits = edits; h.reserved = 0;
        a.out[slot] = h;
    }
}

// One column of the search form, the query at the top of the vectors.  off: the residue's class times 8.
template <int WORDS>
__device__ __forceinline__ void column(const uint64_t *peq, uint32_t off, typename Bits<WORDS>::type &Pv, typename Bits<WORDS>::type &Mv,
                                       int &score)
{
    typedef typename Bits<WORDS>::type V;
    constexpr int TOP = 32 * WORDS - 1;
    const char *entry = reinterpret_cast<const char *>(peq) + off;
    const V Eq = WORDS == 2 ? (V)*reinterpret_cast<const uint64_t *>(entry) : (V)*reinterpret_cast<const uint32_t *>(entry + 4);
    const V Xv = Eq | Mv;
    const V Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
    V Ph = Mv | ~(Xh | Pv);
    V Mh = Pv & Xh;
    score += (int)(Ph >> TOP) - (int)(Mh >> TOP);
    Ph <<= 1;
    Mh <<= 1;
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
}

}  // namespace

template <int WORDS>
__global__ __launch_bounds__(AP_THREADS) void approx_kernel(const ApproxArgs a)
{
    typedef typename Bits<WORDS>::type V;
    __shared__ uint32_t s_text[TEXT_DWORDS];
    __shared__ uint64_t s_peq[AP_CLASSES];
    const int tid = (int)threadIdx.x;
    const int64_t wg = (int64_t)blockIdx.x;
    const int c = wg_record(a.wg_prefix, a.n_contigs, wg);
    const ContigDesc d = a.cd[c];
    const int64_t wg_first = (wg - a.wg_prefix[c]) * (int64_t)AP_WG_BASES;     // 0-based in the record
    const uint8_t *__restrict__ text = a.ascii + d.ascii_off;

    // ---- the text of the workgroup: residues wg_first - AP_LEAD .. wg_first + AP_WG_BASES - 1, as classes ----------------------
    // (a record's slot of the text is 32-aligned and ends >= 32 bytes behind its last residue: a 16-byte load that begins on a
    //  residue stays inside it)
    for (int i = tid; i < N_CHUNKS; i += AP_THREADS) {
        const int64_t r = wg_first - AP_LEAD + 16ll * i;
        uint4 v = make_uint4(NO_RESIDUE4, NO_RESIDUE4, NO_RESIDUE4, NO_RESIDUE4);
        if (r >= 0 && r < d.len) v = *reinterpret_cast<const uint4 *>(text + r);
        const int q = 16 * i + (AP_TILE - AP_LEAD);                            // byte in block space: the lead ends block 0
        uint32_t *dst = s_text + (q >> 2) + q / AP_TILE;                       // (+ one pad dword per block before it)
        dst[0] = class_offsets(v.x); dst[1] = class_offsets(v.y); dst[2] = class_offsets(v.z); dst[3] = class_offsets(v.w);
    }

    const int64_t lane_first = wg_first + (int64_t)tid * AP_TILE;
    const int64_t left = d.len - lane_first;
    const int rem = left <= 0 ? 0 : left >= AP_TILE ? AP_TILE : (int)left;     // ends the lane owns that exist
    // a wave whose first lane owns nothing has nothing to do; one whose first lane owns the record's last ends needs only those
    const int rem0 = __builtin_amdgcn_readfirstlane(rem);
    const int n_main = (rem0 + 3) >> 2;
    const uint32_t *__restrict__ mine = s_text + (tid + 1) * LANE_STRIDE;      // the lane's tile; the columns before it end block tid
    const uint32_t *__restrict__ before = s_text + tid * LANE_STRIDE + TILE_DWORDS;

    for (int qi = 0; qi < a.n_queries; qi++) {
        __syncthreads();                                                       // (the text is there; the last query's table is read)
        if (tid < AP_CLASSES) s_peq[tid] = a.queries[qi].peq[tid];
        __syncthreads();
        if (rem0 == 0) continue;                                               // (wave-uniform)
        const int m = a.queries[qi].len, e = a.queries[qi].max_edits, id = a.queries[qi].id;
        const int warm = (m + e + 3) >> 2;                                     // dwords
        V Pv = ~(V)0, Mv = 0;
        int score = m;
        for (int w = -warm; w < 0; w++) {
            const uint32_t x = before[w];
            column<WORDS>(s_peq, x & 0xFFu, Pv, Mv, score);
            column<WORDS>(s_peq, (x >> 8) & 0xFFu, Pv, Mv, score);
            column<WORDS>(s_peq, (x >> 16) & 0xFFu, Pv, Mv, score);
            column<WORDS>(s_peq, x >> 24, Pv, Mv, score);
        }
        for (int dd = 0; dd < n_main; dd++) {
            const uint32_t x = mine[dd];
            int s[4];
            column<WORDS>(s_peq, x & 0xFFu, Pv, Mv, score); s[0] = score;
            column<WORDS>(s_peq, (x >> 8) & 0xFFu, Pv, Mv, score); s[1] = score;
            column<WORDS>(s_peq, (x >> 16) & 0xFFu, Pv, Mv, score); s[2] = score;
            column<WORDS>(s_peq, x >> 24, Pv, Mv, score); s[3] = score;
            const int lo01 = s[0] < s[1] ? s[0] : s[1], lo23 = s[2] < s[3] ? s[2] : s[3];
            const int lo = lo01 < lo23 ? lo01 : lo23;
            if (__ballot(lo <= e && 4 * dd < rem) == 0) continue;
            // ---- some lane of the wave has a matching end among these four -------------------------------------------------
#pragma unroll
            for (int i = 0; i < 4; i++) emit(s[i] <= e && 4 * dd + i < rem, a, id, c, lane_first + 4 * dd + i + 1, s[i]);
        }
    }
}

__global__ __launch_bounds__(256) void approx_start_kernel(const ApproxArgs a)
{
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= a.n_hits) return;
    const ApproxHit hit = a.out[h];
    const ApproxQuery *__restrict__ Q = a.queries + hit.query;
    const uint8_t *__restrict__ text = a.ascii + a.cd[hit.contig].ascii_off;
    const int m = Q->len;
    const int64_t most = hit.end < (int64_t)(m + hit.edits) ? hit.end : (int64_t)(m + hit.edits);
    uint64_t Pv = ~0ull, Mv = 0;
    int score = m;
    int64_t start = 0;                                                         // (0: no column attains the score -- the host refuses it)
    for (int64_t col = 1; col <= most; col++) {
        const uint64_t Eq = Q->rev[(text[hit.end - col] >> 1) & 7u];
        const uint64_t Xv = Eq | Mv;
        const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
        uint64_t Ph = Mv | ~(Xh | Pv);
        uint64_t Mh = Pv & Xh;
        score += (int)((Ph >> (m - 1)) & 1u) - (int)((Mh >> (m - 1)) & 1u);
        Ph = (Ph << 1) | 1u;
        Mh <<= 1;
        Pv = Mh | ~(Xv | Ph);
        Mv = Ph & Xv;
        if (score == hit.edits) { start = hit.end - col + 1; break; }
    }
    a.out[h].start = start;
}

// words: 1 or 2, the 32-bit words of the bit vectors (1 serves queries of at most 32 symbols)
hipError_t launch_approx(const ApproxArgs &a, int words, int64_t n_wg, hipStream_t st)
{
    if (n_wg < 1) return hipSuccess;
    if (n_wg > 0x7FFFFFFFll) return hipErrorInvalidValue;
    const dim3 grid((unsigned)n_wg), block(AP_THREADS);
    if (words == 1) hipLaunchKernelGGL(approx_kernel<1>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(approx_kernel<2>, grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_approx_starts(const ApproxArgs &a, hipStream_t st)
{
    if (a.n_hits < 1) return hipSuccess;
    const int64_t n_wg = (a.n_hits + 255) / 256;
    if (n_wg > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(approx_start_kernel, dim3((unsigned)n_wg), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace kgma
