// kgma_codon.h -- what kgma_codon.cpp (host) and kgma_codon.hip (kernel) share, and what the context keeps for the search.
#ifndef KGMA_CODON_H
#define KGMA_CODON_H

#include "kgma_approx.h"   // (the residue classes of the text)

namespace kgma {

// codon_kernel: a workgroup owns CD_WG_STARTS consecutive nucleotide starts of one record (all three frames), each of its waves
// CD_WAVE_STARTS of them, and the lanes of a wave take consecutive starts (lane l the starts l, l + 64, ... of the wave's).  The
// workgroup stages the residues of its starts and the CD_TAIL behind them in LDS: the longest matrix reads the codon at
// s + 3 * 63, whose last residue is s + 191 (>= 3 * 64 residues behind the last start's first; a multiple of 16).
constexpr int CD_THREADS = 256;
constexpr int CD_LANE_STARTS = 1;
constexpr int CD_WAVE_STARTS = 2048;
constexpr int CD_WG_STARTS = (CD_THREADS / 64) * CD_WAVE_STARTS;
constexpr int CD_TAIL = 208;
constexpr int CD_MAX_ROWS = 64;
constexpr int CD_ENTRIES = 65;                    // 64 codons (16 b0 + 4 b1 + b2; A 0, C 1, G 2, T 3) and the ambiguous one
constexpr int CD_AMBIGUOUS = 64;
// A table as the kernel reads it: the 65 weights as int16_t and one of padding, 33 dwords.  A 4-byte LDS read is banked by
// (address / 4) mod 32, so 65 int32 entries would put the codons c and c + 32 on one bank; as int16_t the 64 codons of a table
// lie in 32 consecutive dwords, one bank each (two codons of one dword are one address), and only the ambiguous entry shares a bank.
constexpr int CD_TAB_STRIDE = 66;
static_assert(CD_TAB_STRIDE >= CD_ENTRIES && CD_TAB_STRIDE % 2 == 0, "whole dwords");
static_assert(CD_TAIL >= 3 * CD_MAX_ROWS && CD_TAIL % 16 == 0 && CD_WAVE_STARTS % 128 == 0, "the tail holds the longest matrix");

// A matrix as the kernel sees it.  The host has taken the rows of 65 equal weights out (their weight is in `konst`); row
// col[p] of the matrix is table p: tables[tab_off + CD_TAB_STRIDE * p ...], indexed by the codon code of the three residues at
// s + 3 * col[p].  A start is a hit iff the sum of its n_rows entries is >= thr (the caller's threshold less konst); the
// reported score is that sum plus konst.
struct CodonMatrix {
    int32_t rows;         // m, 1 ... 64 (codons: the site covers 3 m residues)
    int32_t n_rows;       // rows with a table, 1 ... 64
    int32_t thr, konst;
    int32_t id;           // 0-based matrix index reported in the hits
    int32_t tab_off;      // in entries
    int32_t pad[2];
    uint8_t col[CD_MAX_ROWS];    // the row of table p
};
struct CodonHit {         // = kgma_codon_hit
    int32_t matrix, contig;
    int64_t start;        // 1-based
    int32_t score, reserved;
};
static_assert(sizeof(CodonHit) == 24, "codon hits are 24 bytes");

struct CodonArgs {
    const uint8_t *ascii;
    const ContigDesc *cd;
    const int64_t *wg_prefix;     // [n_contigs + 1]: workgroups of the records before record c (none spans two records)
    int32_t n_contigs, n_matrices;
    const CodonMatrix *matrices;
    const int16_t *tables;        // (tab_off is a multiple of CD_TAB_STRIDE: every table begins on a dword)
    CodonHit *out;
    unsigned long long *ctl;      // [0]: hits counted (also past cap)
    unsigned long long cap;
};

hipError_t launch_codon(const CodonArgs &a, int64_t n_wg, hipStream_t st);

// What the context keeps for kgma_codon_match: the device buffer of the hits (kept between calls), the hits and the stats of
// the last call
struct CodonState {
    HitBuffer<CodonHit> out;
    std::vector<kgma_codon_hit> hits;
    kgma_codon_stats stats{};
    void release() { out.release(); }
};

// kgma_api.cpp: the state above (released by kgma_destroy)
CodonState *ctx_codon(kgma_ctx *ctx);

}  // namespace kgma

#endif
