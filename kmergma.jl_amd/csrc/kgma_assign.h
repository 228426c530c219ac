// kgma_assign.h -- what kgma_assign.cpp needs of a context and a genome.  Their structs are kgma_api.cpp's; these four functions
// (defined there) are all of them that the assignment's host code sees.
#ifndef KGMA_ASSIGN_H
#define KGMA_ASSIGN_H

#include <hip/hip_runtime.h>

#include "../../include/kgma.h"
#include "kgma_device.h"

namespace kgma {

struct GenomeText {
    const uint8_t *d_ascii;       // residue text on the device
    const ContigDesc *d_cd;       // record table on the device ...
    const ContigDesc *cd;         // ... and on the host
    int64_t n_contigs;
};

int ctx_fail(kgma_ctx *ctx, int code, const char *message);   // sets kgma_last_error; returns code
void ctx_device(const kgma_ctx *ctx, int *device, hipStream_t *stream);
kgma_assign_stats *ctx_assign_stats(kgma_ctx *ctx);
GenomeText genome_text(const kgma_genome *g);

}  // namespace kgma

#endif
