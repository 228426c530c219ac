// kgma_strobe_bin.h -- the randstrobe bin rule (Strobemers.jl:45-65), the ONE definition the device code has: strobe_kernel
// (kgma_strobe.hip) and strobe_calib_kernel (kgma_calib.hip) include it.  The host half of the rule, the zero-score mask, is
// strobe_zero_mask in kgma_device.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kgma {

// The bin of the randstrobe whose first residue is the low 2 bits of x (16 residues, first residue least significant: the packed
// genome's order).  The score is formed from NATURAL values (first residue most significant), so the 2-bit groups of x are
// reversed once: residue j then sits at bits 31-2j .. 30-2j and the s-mer at 0-based offset o is a plain bit field.  The modulus
// is a lookup: the sum of two s-mer values is below 2 * 4^s <= 128, and `zero` has bit v set where v % q == 0.
// Only the first k = w_max + s - 1 residues of x are read.
template <int SS>
__device__ __forceinline__ uint32_t strobe_bin(const uint32_t x, const int w_min, const int w_max, const uint32_t z0, const uint32_t z1,
                                               const uint32_t z2, const uint32_t z3)
{
    constexpr uint32_t M = (1u << (2 * SS)) - 1u;
    const uint32_t r = __brev(x);
    const uint32_t R = ((r & 0x55555555u) << 1) | ((r >> 1) & 0x55555555u);
    const uint32_t first = R >> (32 - 2 * SS);
    uint32_t second = (R >> (32 - 2 * (w_min - 1 + SS))) & M;
    for (int o = w_min - 1; o < w_max; o++) {                         // (wave-uniform bounds; ascending: the last offset of score 0 wins)
        const uint32_t c = (R >> (32 - 2 * (o + SS))) & M;
        const uint32_t sum = first + c;
        uint32_t zw;
        if constexpr (SS <= 2) zw = z0;                               // sums below 32
        else { zw = sum < 64u ? (sum < 32u ? z0 : z1) : (sum < 96u ? z2 : z3); }
        second = ((zw >> (sum & 31u)) & 1u) ? c : second;
    }
    return (first << (2 * SS)) | second;
}

}  // namespace kgma
