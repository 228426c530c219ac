// kgma_assign.hip -- gene assignment (kgma_assign_seqs / kgma_assign_ranges): every query (a hit) against every reference gene.
//
// The model is the hit aligner's (kgma_align.hip, tests/align_ref.py): Gotoh affine-gap DP, the reference global, leading and
// trailing gaps in the reference free (the query's overhang), a gap of length L scoring gap_open + L * gap_extend, EDNAFULL
// restricted to A/C/G/T/N.  Reference rows go to lanes in strips of 64 and a strip sweeps the query's columns as an anti-diagonal
// wavefront, exactly as there: lane r is at column t - r + 1 in step t, takes H / I of the row above from lane r - 1 (DPP
// wave_shr:1; lane 0 from the previous strip's last row, kept in LDS) and the diagonal from what it fetched one step earlier.
//
//   assign_score_kernel<SRC>   one wave per (query, reference) pair, the score only: no trace, no traceback, one int32 written.
//                              LDS per wave: the strip-boundary rows H / I (int32 per column) and the query's residue codes.
//   assign_trace_kernel<SRC>   one wave per (query, chosen reference): the same sweep with one trace byte per cell (wavefront-
//                              major, as align_kernel), then lane 0 walks the traceback -- match, then deletion, then insertion,
//                              a gap extended where extending and opening tie -- and COUNTS the alignment's columns.
// SRC says where a query's residues lie: RangeSource -- a range of a record of the resident genome's residue text;
// SeqSource -- a run of an uploaded buffer of host sequences (strobe_calib_kernel<SRC, s> in kgma_calib.hip is the precedent).
// The sweep itself is one function, sweep<TRACE>, so both kernels are the same recurrence by construction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kgma_device.h"

namespace kgma {

namespace {

constexpr int32_t A_NEG = -(1 << 29);          // "no alignment ends here" (kgma_align.hip, kgma_align_host.cpp)
enum : uint32_t { T_M = 1, T_D = 2, T_I = 4, T_DEXT = 8, T_IEXT = 16 };

__device__ __forceinline__ int base_code(uint32_t c)
{
    c &= 0xDFu;
    return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;   // N and everything else
}

// EDNAFULL (NUC.4.4) restricted to A,C,G,T,N
__device__ __forceinline__ int32_t edna(int x, int y)
{
    if (x < 4 && y < 4) return x == y ? 5 : -4;
    return (x == 4 && y == 4) ? -1 : -2;
}

// A row's substitution scores against the five codes, + 4, one nibble per code: the cell step is a bit-field extract
__device__ __forceinline__ uint32_t edna_profile(int x)
{
    uint32_t p = 0;
    for (int y = 0; y < 5; y++) p |= (uint32_t)(edna(x, y) + 4) << (4 * y);
    return p;
}

__device__ __forceinline__ int32_t shr1(int32_t x, int32_t carry_in)
{
    return __builtin_amdgcn_update_dpp(carry_in, x, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
}

struct RangeSource {      // query q: residues lo .. lo + n - 1 (1-based) of record contig[q] of the resident text
    static __device__ __forceinline__ const uint8_t *text(const AssignArgs &a, int q)
    {
        return a.text + a.cd[a.q_contig[q]].ascii_off + (a.q_pos[q] - 1);
    }
};
struct SeqSource {        // query q: n bytes at offset q_pos[q] of the uploaded sequences
    static __device__ __forceinline__ const uint8_t *text(const AssignArgs &a, int q) { return a.text + a.q_pos[q]; }
};

// The wave's LDS: rowH[0 .. max_n], rowI[0 .. max_n], then one byte per column: 4 * the residue code of columns 1 .. n
struct WaveLds {
    int32_t *rowH, *rowI;
    uint8_t *bc;
};
__device__ __forceinline__ WaveLds wave_lds(int32_t *sh, int max_n)
{
    WaveLds w;
    w.rowH = sh;
    w.rowI = sh + (max_n + 1);
    w.bc = reinterpret_cast<uint8_t *>(w.rowI + (max_n + 1));
    return w;
}

// Row 0 (an unaligned prefix of the query is free) and the query's codes
__device__ __forceinline__ void load_query(const WaveLds &w, const uint8_t *b, int n, int lane)
{
    for (int j = lane; j <= n; j += 64) {
        w.rowH[j] = 0;
        w.rowI[j] = A_NEG;
        w.bc[j] = j ? (uint8_t)(4 * base_code(b[j - 1])) : 16;
    }
}

// All strips of reference `ref` (m residues) against the query in `w` (n residues).  Returns H(m, n) in every lane.
// TRACE: one byte per cell at tr[(strip * steps + t) * 64 + lane], steps = n + 63 (align_kernel's layout).
template <bool TRACE>
__device__ __forceinline__ int32_t sweep(const WaveLds &w, const uint8_t *__restrict__ ref, int m, int n, int go, int ge, int lane,
                                         uint8_t *__restrict__ tr)
{
    const int goe = go + ge;
    int32_t score = 0;
    const int n_strips = (m + 63) >> 6;
    for (int s = 0; s < n_strips; s++) {
        const int i = 64 * s + lane + 1;        // this lane's row (reference position, 1-based)
        const bool row_ok = i <= m;
        const uint32_t prof = edna_profile(row_ok ? base_code(ref[i - 1]) : 4);
        // deletions on the last row are trailing gaps of the reference: free
        const int32_t dgoe = i == m ? 0 : goe, dge = i == m ? 0 : ge;
        const int32_t col0_up = i - 1 == 0 ? 0 : -(go + ge * (i - 1));      // H(i-1, 0)
        int32_t Hleft = -(go + ge * i), Dleft = A_NEG;                       // H(i,0), D(i,0)
        int32_t outH = 0, outI = A_NEG;         // H / I of this lane's cell of the previous step (for the lane below)
        int32_t uH_prev = 0;                    // H(i-1, j-1) as fetched one step earlier
        const bool feeds = s + 1 < n_strips;    // the strip's last row is the next strip's row above
        // the score pass stops a strip when its last occupied lane has left the query; the trace layout keeps n + 63 steps
        const int rows = m - 64 * s < 64 ? m - 64 * s : 64;
        const int steps = TRACE ? n + 63 : n + rows - 1;
        for (int t = 0; t < steps; t++) {
            const int j = t - lane + 1;         // this lane's column in this step
            // the row above at column j: lane-1's cell of the previous step; lane 0 reads the previous strip's row
            const int jl0 = t + 1;
            const int32_t c0H = jl0 <= n ? w.rowH[jl0] : 0, c0I = jl0 <= n ? w.rowI[jl0] : A_NEG;
            const int32_t uH = shr1(outH, c0H), uI = shr1(outI, c0I);
            const bool ok = row_ok && j >= 1 && j <= n;
            uint32_t tb = 0;
            int32_t h = 0, ins = A_NEG;
            if (ok) {
                const int32_t diag = j == 1 ? col0_up : uH_prev;
                const int32_t dopen = Hleft - dgoe, dext = Dleft - dge;
                const int32_t d = dopen > dext ? dopen : dext;
                const int32_t iopen = uH - goe, iext = uI - ge;
                ins = iopen > iext ? iopen : iext;
                const int32_t mt = diag + (int32_t)((prof >> w.bc[j]) & 15u) - 4;
                h = mt > d ? mt : d;
                h = h > ins ? h : ins;
                if (TRACE) {
                    if (dext >= dopen) tb |= T_DEXT;
                    if (iext >= iopen) tb |= T_IEXT;
                    if (mt == h) tb |= T_M;
                    if (d == h) tb |= T_D;
                    if (ins == h) tb |= T_I;
                }
                Hleft = h; Dleft = d;
                if (i == m && j == n) score = h;
            }
            if (TRACE) tr[((int64_t)s * steps + t) * 64 + lane] = (uint8_t)tb;   // wavefront-major: one 64-byte row per step
            uH_prev = uH;
            outH = h; outI = ins;
            // the strip's last row feeds lane 0 of the next strip (63 columns behind lane 0's reads: in place)
            if (feeds && lane == 63 && ok) { w.rowH[j] = h; w.rowI[j] = ins; }
        }
    }
    return __builtin_amdgcn_readlane(score, (m - 1) & 63);   // the score lives in the lane that owns row m
}

}  // namespace

// Pair p of the launch: query items[p / n_cols], column p % n_cols; the column is the reference itself, or -- a screened call --
// names it through the candidate table.  scores[query * n_cols + column] = H(m, n).
template <class SRC>
__global__ __launch_bounds__(64) void assign_score_kernel(const AssignArgs a)
{
    extern __shared__ int32_t sh[];
    const WaveLds w = wave_lds(sh, a.max_n);
    const int lane = threadIdx.x;
    const int64_t p = a.first + blockIdx.x;
    const int q = a.items[p / a.n_cols], col = (int)(p % a.n_cols);
    const int r = a.cand ? a.cand[(int64_t)q * a.n_cols + col] : col;
    const int n = a.q_n[q];
    load_query(w, SRC::text(a, q), n, lane);
    const int64_t r0 = a.ref_off[r];
    const int32_t score = sweep<false>(w, a.refs + r0, (int)(a.ref_off[r + 1] - r0), n, a.go, a.ge, lane, nullptr);
    if (lane == 0) a.scores[(int64_t)q * a.n_cols + col] = score;
}

// Job b of the launch: query job_q[first + b] against reference job_r[first + b].  out[job] = its kgma_assignment (8 int32).
template <class SRC>
__global__ __launch_bounds__(64) void assign_trace_kernel(const AssignArgs a)
{
    extern __shared__ int32_t sh[];
    const WaveLds w = wave_lds(sh, a.max_n);
    const int lane = threadIdx.x;
    const int64_t job = a.first + blockIdx.x;
    const int q = a.job_q[job], r = a.job_r[job];
    const int n = a.q_n[q];
    load_query(w, SRC::text(a, q), n, lane);
    const int64_t r0 = a.ref_off[r];
    const uint8_t *ref = a.refs + r0;
    const int m = (int)(a.ref_off[r + 1] - r0);
    uint8_t *tr = a.trace + (int64_t)blockIdx.x * a.trace_stride;
    const int32_t score = sweep<true>(w, ref, m, n, a.go, a.ge, lane, tr);
    __threadfence();                            // the trace bytes of all lanes are read back by lane 0
    if (lane != 0) return;

    // ---- traceback from (m, n): match > delete > insert (kgma_align_host.cpp), counting columns ------------------
    const int steps = n + 63;
    auto trace_at = [&](int i, int j) -> uint32_t {
        if (i == 0) return j ? (T_D | T_DEXT) : 0u;
        if (j == 0) return T_I | (i > 1 ? T_IEXT : 0u);
        const int s = (i - 1) >> 6, l = (i - 1) & 63, t = j - 1 + l;
        return tr[((int64_t)s * steps + t) * 64 + l];
    };
    int i = m, j = n, state = 0;               // 0 = H, 1 = in a deletion run, 2 = in an insertion run
    int32_t n_eq = 0, n_x = 0, n_ins = 0, n_d = 0;
    int32_t d_run = 0;                          // length of the D run the walk is in (0: the last column was not a D)
    int32_t trail = -1;                         // D columns before the first other column of the walk = the CIGAR's trailing D run
    auto other = [&]() { if (trail < 0) trail = d_run; d_run = 0; };
    while (i > 0 || j > 0) {
        const uint32_t t = trace_at(i, j);
        if (state == 1) {
            n_d++; d_run++;
            const bool ext = (t & T_DEXT) != 0 && j > 1;
            j--;
            state = ext ? 1 : 0;
            if (i == 0) state = j > 0 ? 1 : 0;
            continue;
        }
        if (state == 2) {
            other(); n_ins++;
            i--;
            state = (t & T_IEXT) ? 2 : 0;
            if (j == 0) state = i > 0 ? 2 : 0;
            continue;
        }
        if (i > 0 && j > 0 && (t & T_M)) {
            const int x = base_code(ref[i - 1]), y = w.bc[j] >> 2;
            other();
            if (x == y && x < 4) n_eq++; else n_x++;
            i--; j--;
        } else if (j > 0 && (i == 0 || (t & T_D))) {
            state = 1;
        } else {
            state = 2;
        }
    }
    // the walk ran back to front: the D run it ends in is the CIGAR's leading one (m >= 1: the two end runs are never one run)
    if (trail < 0) trail = 0;
    const int32_t lead = d_run;
    int32_t *o = a.out + 8 * job;
    o[0] = r; o[1] = score; o[2] = n_eq; o[3] = n_x; o[4] = n_ins; o[5] = n_d - lead - trail;
    o[6] = lead + 1; o[7] = n - trail;
}

int64_t assign_trace_bytes(int m, int n) { return (int64_t)((m + 63) >> 6) * (n + 63) * 64; }
size_t assign_lds_bytes(int max_n) { return (size_t)(max_n + 1) * 8 + (size_t)(max_n + 1) + 16; }

template <class SRC>
static hipError_t launch_assign_src(const AssignArgs &a, bool trace, int grid, hipStream_t st)
{
    const size_t lds = assign_lds_bytes(a.max_n);
    auto kern = trace ? &assign_trace_kernel<SRC> : &assign_score_kernel<SRC>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_assign(const AssignArgs &a, int source, bool trace, int grid, hipStream_t st)
{
    if (grid <= 0) return hipSuccess;
    return source == 0 ? launch_assign_src<RangeSource>(a, trace, grid, st) : launch_assign_src<SeqSource>(a, trace, grid, st);
}

}  // namespace kgma
