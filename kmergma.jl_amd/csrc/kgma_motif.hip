// kgma_motif.hip -- IUPAC motif search with mismatches over the resident genome (kgma_motif_match; the working form of the
// reference's src/RSS.jl): every start position of every record at which a motif of 1 ... 64 IUPAC symbols lies with at most
// max_mismatch non-matching positions.  A genome base matches a motif symbol when it is in the symbol's set; a genome N matches
// only a motif N.
//
// The kernel is bit-sliced over the bit-plane copy of the genome (one {hi, lo} word pair per 32 bases, N stored as T) and walks
// the genome ONCE for a whole batch of motifs.  A record is cut into tiles (no tile spans two records); a workgroup takes one
// tile, a lane KGMA_MOTIF_ITERS plane words, all held at once.  For a word the lane owns its 32 start positions: it loads the word pair and the
// next two (96 bases: a start at bit 31 sees 64 more) and then loops over the motifs, and per motif over its INFORMATIVE positions
// only (the host compacts them; an N costs nothing).  Per position with offset o and base set S:
//     H, L   = the two planes shifted by o (one funnel shift each; the word pair changes at o = 32, hence two loops)
//     x      = H ? (L ? nT : nG) : (L ? nC : nA)        nX = all ones when X is NOT in S: wave-uniform, so the select is
//                                                       nA ^ L c1 ^ H c2 ^ HL c3 with scalar coefficients (five operations)
//     count += x                                        a bit-sliced ripple-carry counter with a sticky overflow word
// so that one 32-bit operation serves 32 starts.  The counter has P planes, P the smallest with 2^P - 1 >= max_mismatch, and starts
// at 2^P - 1 - max_mismatch: it overflows exactly when the count exceeds max_mismatch, and the survivors are the starts whose
// overflow bit is still clear.  The kernel is instantiated per P (0 ... 4); a batch with different max_mismatch values runs with
// the largest P any of its motifs needs, each motif starting its counter at its own 2^P - 1 - max_mismatch.
//
// The planes store N as T, so the plane-level count is a LOWER bound on the mismatches: no false negative, and every survivor is
// verified against the residue text (case folded), where its exact count is taken -- that is what rejects a genome N under a
// motif T.  The verified ones are appended as {motif, record, start, mismatches} through ballot + wave prefix + one atomicAdd per
// wave on a cursor that keeps counting past the buffer's capacity (the host regrows and runs again).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kgma_device.h"

namespace kgma {

namespace {

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

// The motif descriptors and their position lists are the same for every lane and constant for the launch: read through the
// constant address space they come in by scalar loads (the scalar cache).
typedef const MotifDesc __attribute__((address_space(4))) *MotifTable;
typedef const uint32_t __attribute__((address_space(4))) *InfoTable;

// base set (bit 0 A, 1 C, 2 G, 3 T) of a case-folded residue; N = all four, anything else = all four as well (the host has
// refused genomes with such residues)
__device__ __forceinline__ uint32_t residue_set(uint32_t ch)
{
    return ch == 'A' ? 1u : ch == 'C' ? 2u : ch == 'G' ? 4u : ch == 'T' ? 8u : 15u;
}

// the lanes with `ok` append one hit each: one atomicAdd per wave
__device__ __forceinline__ void emit(bool ok, const MotifArgs &a, int motif, int contig, int64_t start1, int mism)
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
        MotifHit h;
        h.motif = motif; h.contig = contig; h.start = start1; h.mismatches = mism; h.reserved = 0;
        a.out[slot] = h;
    }
}

// One informative position, decoded once for all the words a lane holds: the shift and the coefficients of the mismatch word.
// nX is all ones when base X is NOT in the set; the mismatch word H ? (L ? nT : nG) : (L ? nC : nA) is, as a polynomial over
// GF(2) in H and L, nA ^ L c1 ^ H c2 ^ HL c3 with wave-uniform coefficients: one scalar operand per vector operation.
struct Position { uint32_t o, nA, c1, c2, c3; };
__device__ __forceinline__ Position decode_position(uint32_t e)
{
    const uint32_t set = e >> 8;
    const uint32_t nA = (set & 1u) - 1u, nC = ((set >> 1) & 1u) - 1u, nG = ((set >> 2) & 1u) - 1u, nT = ((set >> 3) & 1u) - 1u;
    Position q;
    q.o = e & 31u; q.nA = nA; q.c1 = nA ^ nC; q.c2 = nA ^ nG; q.c3 = q.c1 ^ nG ^ nT;
    return q;
}

// the mismatch word of 32 starts at one position, added into the counter
template <int P>
__device__ __forceinline__ void count_position(const Position &q, uint32_t hA, uint32_t hB, uint32_t lA, uint32_t lB, uint32_t (&cnt)[P > 0 ? P : 1],
                                               uint32_t &ov)
{
    const uint32_t H = __builtin_amdgcn_alignbit(hB, hA, q.o), L = __builtin_amdgcn_alignbit(lB, lA, q.o);
    uint32_t carry = q.nA ^ (L & q.c1) ^ (H & q.c2) ^ (H & L & q.c3);
#pragma unroll
    for (int p = 0; p < P; p++) {
        const uint32_t t = cnt[p] & carry;
        cnt[p] ^= carry;
        carry = t;
    }
    ov |= carry;
}

}  // namespace

template <int P>
__global__ __launch_bounds__(KGMA_MOTIF_THREADS) void motif_kernel(const MotifArgs a)
{
    constexpr int IT = KGMA_MOTIF_ITERS, PP = P > 0 ? P : 1;
    const int64_t tile = (int64_t)blockIdx.x;
    const int c = tile_record(a.tile_prefix, a.n_contigs, tile);
    const ContigDesc d = a.cd[c];
    const int64_t tile_off = (tile - a.tile_prefix[c]) * (int64_t)(KGMA_MOTIF_THREADS * IT * 32);
    const uint8_t *__restrict__ text = a.ascii + d.ascii_off;
    const uint2 *__restrict__ planes = reinterpret_cast<const uint2 *>(a.planes) + d.word_off;   // base b of the record: word b / 32, bit b % 32
    const MotifTable mt = (MotifTable)(uintptr_t)a.motifs;
    const InfoTable info = (InfoTable)(uintptr_t)a.info;
    // The lane's IT words, all held at once: a position's shift and coefficients (scalar work, and the wait for the scalar load
    // that brings them) are then paid once per IT words, and the IT counter chains are independent of each other.
    // Word `it` covers bases off .. off + 95 of the record (a record is followed by 32 words of padding in the plane copy:
    // kgma_api.cpp, genome_layout); words that begin behind the record's end are not loaded and have no start.
    const int64_t off0 = tile_off + (int64_t)threadIdx.x * 32;        // the lane's first start, 0-based in the record
    uint32_t h[IT][3], l[IT][3];
#pragma unroll
    for (int it = 0; it < IT; it++) {
        const int64_t off = off0 + (int64_t)it * (KGMA_MOTIF_THREADS * 32);
#pragma unroll
        for (int j = 0; j < 3; j++) {
            uint2 v = make_uint2(0u, 0u);
            if (off < d.len) v = planes[(off >> 5) + j];
            h[it][j] = v.x; l[it][j] = v.y;
        }
    }
    for (int mi = 0; mi < a.n_motifs; mi++) {
        const int info_off = mt[mi].info_off, n_lo = mt[mi].n_lo, n_hi = mt[mi].n_hi, len = mt[mi].len, max_mm = mt[mi].max_mm, id = mt[mi].id;
        const uint32_t init = ((1u << P) - 1u) - (uint32_t)max_mm;
        uint32_t cnt[IT][PP], ov[IT];
#pragma unroll
        for (int it = 0; it < IT; it++) {
            ov[it] = 0u;
#pragma unroll
            for (int p = 0; p < PP; p++) cnt[it][p] = ((init >> p) & 1u) ? ~0u : 0u;
        }
        const InfoTable ip = info + info_off;
        uint32_t e_next = ip[0];
        for (int i = 0; i < n_lo; i++) {
            const Position q = decode_position(e_next);
            e_next = ip[i + 1];
#pragma unroll
            for (int it = 0; it < IT; it++) count_position<P>(q, h[it][0], h[it][1], l[it][0], l[it][1], cnt[it], ov[it]);
        }
        for (int i = n_lo; i < n_lo + n_hi; i++) {
            const Position q = decode_position(e_next);
            e_next = ip[i + 1];
#pragma unroll
            for (int it = 0; it < IT; it++) count_position<P>(q, h[it][1], h[it][2], l[it][1], l[it][2], cnt[it], ov[it]);
        }
#pragma unroll
        for (int it = 0; it < IT; it++) {
            const int64_t off = off0 + (int64_t)it * (KGMA_MOTIF_THREADS * 32);
            // starts of this word at which the whole motif lies inside the record
            const int64_t room = d.len - (int64_t)len - off + 1;
            const uint32_t inside = room <= 0 ? 0u : room >= 32 ? ~0u : (1u << (uint32_t)room) - 1u;
            uint32_t surv = ~ov[it] & inside;
            // ---- verification on the residue text: every lane takes its survivors one at a time (wave-uniform trip count) ----
            while (__ballot(surv != 0u) != 0) {
                bool ok = surv != 0u;
                const int j = ok ? __builtin_ctz(surv) : 0;
                surv &= surv - 1u;
                int mism = 0;
                if (ok) {
                    const uint8_t *__restrict__ p = text + off + j;
                    for (int i = 0; i < n_lo + n_hi; i++) {
                        const uint32_t e = ip[i];
                        const uint32_t rs = residue_set((uint32_t)p[e & 63u] & 0xDFu);
                        mism += (rs & ~(e >> 8)) != 0u ? 1 : 0;
                    }
                    ok = mism <= max_mm;
                }
                emit(ok, a, id, c, off + j + 1, mism);
            }
        }
    }
}

// start positions per tile (the host builds MotifArgs::tile_prefix with it)
int64_t motif_tile_starts() { return (int64_t)KGMA_MOTIF_THREADS * KGMA_MOTIF_ITERS * 32; }

// counter planes a motif with `max_mm` allowed mismatches needs: the smallest P with 2^P - 1 >= max_mm
int motif_planes(int max_mm)
{
    int p = 0;
    while ((1 << p) - 1 < max_mm) p++;
    return p;
}

// P: counter planes of the launch, >= motif_planes of every motif in it
hipError_t launch_motif(const MotifArgs &a, int P, int64_t n_tiles, hipStream_t st)
{
    if (n_tiles < 1 || a.n_motifs < 1) return hipSuccess;
    if (n_tiles > 0x7FFFFFFFll || P < 0 || P > 4) return hipErrorInvalidValue;
    const dim3 grid((unsigned)n_tiles), block(KGMA_MOTIF_THREADS);
    switch (P) {
    case 0: hipLaunchKernelGGL(motif_kernel<0>, grid, block, 0, st, a); break;
    case 1: hipLaunchKernelGGL(motif_kernel<1>, grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL(motif_kernel<2>, grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL(motif_kernel<3>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(motif_kernel<4>, grid, block, 0, st, a); break;
    }
    return hipGetLastError();
}

}  // namespace kgma
