// kgma_motif.h -- what kgma_motif.cpp (host) needs of kgma_motif.hip (kernel; the records they share are in kgma_device.h) and
// what the context keeps for it.
#ifndef KGMA_MOTIF_H
#define KGMA_MOTIF_H

#include "kgma_search.h"

namespace kgma {

int64_t motif_tile_starts();
int motif_planes(int max_mm);
hipError_t launch_motif(const MotifArgs &a, int P, int64_t n_tiles, hipStream_t st);

// What the context keeps for kgma_motif_match: the device buffers (kept between calls) and the hits of the last call
struct MotifState {
    Kept<MotifDesc> q;
    Kept<uint32_t> info;
    Kept<int64_t> prefix;
    Kept<unsigned long long> ctl;
    HitBuffer<MotifHit> out;
    std::vector<kgma_motif_hit> hits;
    void release() { q.release(); info.release(); prefix.release(); ctl.release(); out.release(); }
};

// kgma_api.cpp: the state above (released by kgma_destroy)
MotifState *ctx_motif(kgma_ctx *ctx);

}  // namespace kgma

#endif
