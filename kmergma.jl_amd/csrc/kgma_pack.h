// kgma_pack.h -- ASCII residues -> bit planes -> 2-bit interleaved codes, one plane word (32 residues) per lane: the device
// functions shared by pack_kernel (kgma_kernels.hip) and pack_sums_kernel (kgma_filter.hip).  Include after hip_runtime.h.
#pragma once
#include <stdint.h>

namespace kgma {

// (the types the non-temporal load / store builtins take)
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

// One lane packs 32 residues (two 16-byte loads) into one {hi,lo} word pair.
// CLEAN_ONLY: the caller takes only full words of accepted letters -- *bad_out is non-zero when the word is not one (the result is
// then void, and the caller packs the word again with the full form, which does one residue at a time).
template <bool CLEAN_ONLY = false>
__device__ __forceinline__ uint2 pack_word(const uint4 a, const uint4 b, const int nvalid, uint32_t *bad_out)
{
    uint32_t h = 0, l = 0, bad = 0;
    const uint32_t x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    // Four residues per 32-bit word at a time.  After folding case, (ch >> 1) & 7 is distinct for the five
    // accepted letters (A 0, C 1, T 2, G 3, N 7): v_perm_b32 uses it as an index into two 8-byte tables,
    // one giving the letter back (any difference = a residue outside A/C/G/T/N) and one giving the code
    // as 0x00 / 0x0F / 0xF0 / 0xFF (low nibble = code bit 0, high nibble = code bit 1; N -> T's code 3).
    // ANDing with one bit per byte and summing the bytes (v_sad_u8) collects four residues' plane bits.
    uint32_t diff = 0, hw[8], lw[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t v = x[j] & 0xDFDFDFDFu;                       // fold case
        const uint32_t sel = (v >> 1) & 0x07070707u;
        const uint32_t letter = __builtin_amdgcn_perm(0x4E000000u, 0x47544341u, sel);   // idx 7 'N' | 3 'G' 2 'T' 1 'C' 0 'A'
        const uint32_t code = __builtin_amdgcn_perm(0xFF000000u, 0xF0FF0F00u, sel);     // idx 7 -> 3 | G 2, T 3, C 1, A 0
        diff |= v ^ letter;
        // residue t of word j goes to bit 4*(j&1)+t of the plane byte: pick that bit out of the nibble that
        // carries the plane's indicator
        if (j & 1) {
            lw[j] = (code << 4) & 0x80402010u;
            hw[j] = code & 0x80402010u;
        } else {
            lw[j] = code & 0x08040201u;
            hw[j] = (code >> 4) & 0x08040201u;
        }
    }
    if (CLEAN_ONLY || (diff == 0 && nvalid == 32)) {
#pragma unroll
        for (int q = 0; q < 4; q++) {                                // 8 residues -> one byte of each plane
            const uint32_t lb = __builtin_amdgcn_sad_u8(lw[2 * q + 1], 0u, __builtin_amdgcn_sad_u8(lw[2 * q], 0u, 0u));
            const uint32_t hb = __builtin_amdgcn_sad_u8(hw[2 * q + 1], 0u, __builtin_amdgcn_sad_u8(hw[2 * q], 0u, 0u));
            l |= lb << (8 * q);
            h |= hb << (8 * q);
        }
        if (CLEAN_ONLY) bad = diff;
    } else {
        // a record's last (partial) word, or a residue to report: one residue at a time
#pragma unroll
        for (int i = 0; i < 32; i++) {
            const uint32_t ch = ((x[i >> 2] >> (8 * (i & 3))) & 0xFFu) & 0xDFu;  // fold case
            const uint32_t isA = ch == 'A', isC = ch == 'C', isG = ch == 'G';
            const uint32_t isT = (ch == 'T') | (ch == 'N');
            const uint32_t in = i < nvalid;
            h |= ((isG | isT) & in) << i;
            l |= ((isC | isT) & in) << i;
            bad |= ((1u ^ (isA | isC | isG | isT)) & in) << i;
        }
    }
    *bad_out = bad;
    return make_uint2(h, l);
}

// 32 residues straight to the two dwords of the 2-bit interleaved copy (what interleave_word makes of pack_word's planes), for
// callers that keep no planes and take only full words of accepted letters: *bad_out is non-zero when the word is not one (the
// result is then void).  Per dword of four residues one v_perm gives the codes 0 ... 3 in the bytes and one dot product with
// {1, 4, 16, 64} puts them side by side in a byte, first residue lowest; the four bytes of a dword of the copy are chained through
// the dot product's addend, shifted with a two-operand shift.  (x >> 1) & 7 needs no case fold first -- bit 5 is not among bits
// 1 ... 3 -- so the fold is one AND of the differences per word: ~60 VALU against ~95 with shift-or steps and a byte gather.
__device__ __forceinline__ uint2 pack_word_2bit(const uint4 a, const uint4 b, uint32_t *bad_out)
{
    const uint32_t x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t diff = 0, code[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t sel = (x[j] >> 1) & 0x07070707u;
        const uint32_t letter = __builtin_amdgcn_perm(0x4E000000u, 0x47544341u, sel);   // (as pack_word)
        code[j] = __builtin_amdgcn_perm(0x03000000u, 0x02030100u, sel);                 // idx 7 -> 3 | G 2, T 3, C 1, A 0
        diff |= x[j] ^ letter;
    }
    *bad_out = diff & 0xDFDFDFDFu;                                   // (either case)
    uint32_t w[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        uint32_t r = __builtin_amdgcn_udot4(code[4 * h + 3], 0x40100401u, 0u, false);
#pragma unroll
        for (int j = 2; j >= 0; j--) r = __builtin_amdgcn_udot4(code[4 * h + j], 0x40100401u, r << 8, false);
        w[h] = r;
    }
    return make_uint2(w[0], w[1]);
}

// 2-bit interleaved copy of a plane word pair (stream8_kernel cuts a k-mer out of it with ONE funnel shift):
// base t of the word -> bits 2t (code bit 0 = lo plane) and 2t+1 (code bit 1 = hi plane) of a 64-bit value.
__device__ __forceinline__ uint32_t spread16(uint32_t x)             // bit j of the low half -> bit 2j
{
    x &= 0xFFFFu;
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}
__device__ __forceinline__ uint2 interleave_word(const uint2 hl)     // hl = {hi plane, lo plane}
{
    const uint32_t i0 = spread16(hl.y & 0xFFFFu) | (spread16(hl.x & 0xFFFFu) << 1);
    const uint32_t i1 = spread16(hl.y >> 16) | (spread16(hl.x >> 16) << 1);
    return make_uint2(i0, i1);
}

}  // namespace kgma
