// kgma_pwm.h -- what kgma_pwm.cpp (host) and kgma_pwm.hip (kernel) share, and what the context keeps for the search.
#ifndef KGMA_PWM_H
#define KGMA_PWM_H

#include "kgma_approx.h"   // (the residue classes of the text)

namespace kgma {

// pwm_kernel: a workgroup owns PW_WG_STARTS consecutive starts of one record, each of its waves PW_WAVE_STARTS of them, and the
// lanes of a wave take consecutive starts (lane l the starts l, l + 64, ... of the wave's).  The workgroup stages the residues of
// its starts and the PW_TAIL behind them (>= the 63 further residues the longest matrix reads, plus the one a pair code looks
// ahead, a multiple of 16) in LDS.
constexpr int PW_THREADS = 256;
constexpr int PW_LANE_STARTS = 1;
constexpr int PW_WAVE_STARTS = 2048;
constexpr int PW_WG_STARTS = (PW_THREADS / 64) * PW_WAVE_STARTS;
constexpr int PW_TAIL = 80;
constexpr int PW_MAX_ROWS = 64;
constexpr int PW_MAX_PAIRS = PW_MAX_ROWS / 2;
constexpr int PW_PAIR_ENTRIES = 64;               // two residue classes of 3 bits each (kgma_approx.h: A 0, C 1, T 2, G 3, N 7)
static_assert(PW_TAIL >= PW_MAX_ROWS && PW_TAIL % 16 == 0 && PW_WAVE_STARTS % 128 == 0, "the tail holds the longest matrix");

// A matrix as the kernel sees it.  The host has taken the rows of four equal weights out (their weight is in `konst`) and
// folded each remaining row with the row behind it into a table of PW_PAIR_ENTRIES sums indexed by class(t[s + col]) +
// 8 * class(t[s + col + 1]): tables[tab_off + 64 * p ...] is pair p's.  A start is a hit iff the sum of its n_pairs entries is
// >= thr (the caller's threshold less konst); the reported score is that sum plus konst.
struct PwmMatrix {
    int32_t rows;         // m, 1 ... 64
    int32_t n_pairs;      // 1 ... 32
    int32_t thr, konst;
    int32_t id;           // 0-based matrix index reported in the hits
    int32_t tab_off;      // in entries
    int32_t pad[2];
    uint8_t col[PW_MAX_PAIRS];   // the first row of pair p
};
struct PwmHit {           // = kgma_pwm_hit
    int32_t matrix, contig;
    int64_t start;        // 1-based
    int32_t score, reserved;
};
static_assert(sizeof(PwmHit) == 24, "pwm hits are 24 bytes");

struct PwmArgs {
    const uint8_t *ascii;
    const ContigDesc *cd;
    const int64_t *wg_prefix;     // [n_contigs + 1]: workgroups of the records before record c (none spans two records)
    int32_t n_contigs, n_matrices;
    const PwmMatrix *matrices;
    const int32_t *tables;
    PwmHit *out;
    unsigned long long *ctl;      // [0]: hits counted (also past cap)
    unsigned long long cap;
};

hipError_t launch_pwm(const PwmArgs &a, int64_t n_wg, hipStream_t st);

// What the context keeps for kgma_pwm_match: the device buffer of the hits (kept between calls), the hits and the stats of the
// last call
struct PwmState {
    HitBuffer<PwmHit> out;
    std::vector<kgma_pwm_hit> hits;
    kgma_pwm_stats stats{};
    void release() { out.release(); }
};

// kgma_api.cpp: the state above (released by kgma_destroy)
PwmState *ctx_pwm(kgma_ctx *ctx);

}  // namespace kgma

#endif
