// kgma_exact.h -- what kgma_exact.cpp (host) needs of kgma_exact.hip (kernels; the records they share are in kgma_device.h) and
// what the context keeps for it.
#ifndef KGMA_EXACT_H
#define KGMA_EXACT_H

#include "kgma_search.h"

namespace kgma {

int64_t exact_tile_starts(bool two_bit);
hipError_t launch_exact(const ExactArgs &a, int kind, int64_t n_tiles, hipStream_t st);

// What the context keeps for kgma_exact_match: the device buffers (kept between calls) and the matches of the last call
struct ExactState {
    Kept<ExactQuery> q;
    Kept<uint8_t> text;
    Kept<int64_t> prefix;
    Kept<unsigned long long> ctl;
    HitBuffer<ExactMatch> out;
    std::vector<kgma_match> matches;
    void release() { q.release(); text.release(); prefix.release(); ctl.release(); out.release(); }
};

// kgma_api.cpp: the state above (released by kgma_destroy)
ExactState *ctx_exact(kgma_ctx *ctx);

}  // namespace kgma

#endif
