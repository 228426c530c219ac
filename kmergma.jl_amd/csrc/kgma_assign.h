// kgma_assign.h -- what kgma_assign.cpp and kgma_kmat.cpp share, and what the two need of a context beyond kgma_search.h.
#ifndef KGMA_ASSIGN_H
#define KGMA_ASSIGN_H

#include "kgma_search.h"

namespace kgma {

int ctx_n_cus(const kgma_ctx *ctx);
kgma_assign_stats *ctx_assign_stats(kgma_ctx *ctx);
kgma_kmat_stats *ctx_kmat_stats(kgma_ctx *ctx);

struct Queries {                      // the queries of an assignment / the A side of a distance matrix: either source, validated
    int source = 1;                   // 0: genome ranges, 1: uploaded sequences
    GenomeText g{};                   // source 0
    const int32_t *contig = nullptr;  // source 0
    const uint8_t *text = nullptr;    // source 1: the bytes [base, base + bytes)
    int64_t bytes = 0;
    std::vector<int64_t> pos;         // source 0: first residue (1-based); source 1: offset in `text`
    std::vector<int32_t> n;
};

// kgma_kmat.cpp: the distance matrix of A (validated, at least one sequence) against the n_b >= 1 sequences b[b_off[i] .. b_off[i + 1])
// (b_off[0] == 0, lengths validated), k in 1 .. 10, at most 2^30 pairs.  n_near == 0: D and / or dist ([n_a][n_b]) come down;
// n_near >= 1: the matrix stays on the device and index and / or D_near ([n_a][n_near]) come down.  Sets the context's kmat stats
// (zero on any failure); `fn` names the caller in errors, a_name / b_name what a sequence of either side is called there.
int kmat_run(kgma_ctx *ctx, const char *fn, int32_t k, const Queries &A, const char *a_name, const uint8_t *b, const int64_t *b_off,
             int32_t n_b, const char *b_name, int32_t n_near, int32_t *D, double *dist, int32_t *index, int32_t *D_near);

}  // namespace kgma

#endif
