// kgma_assign.h -- what kgma_assign.cpp and kgma_kmat.cpp need of a context and a genome, and what the two share.  The structs of
// a context and a genome are kgma_api.cpp's; the functions below (defined there) are all of them that these host files see.
#ifndef KGMA_ASSIGN_H
#define KGMA_ASSIGN_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

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
int ctx_n_cus(const kgma_ctx *ctx);
kgma_assign_stats *ctx_assign_stats(kgma_ctx *ctx);
kgma_kmat_stats *ctx_kmat_stats(kgma_ctx *ctx);
GenomeText genome_text(const kgma_genome *g);

// Everything a call holds on the device, released by the destructor on every path out
struct DeviceHold {
    std::vector<void *> mem;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    template <class T>
    hipError_t alloc(T *&p, size_t count)
    {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, std::max<size_t>(1, count) * sizeof(T));
        if (e == hipSuccess) mem.push_back(q);
        p = static_cast<T *>(q);
        return e;
    }
    template <class T>
    hipError_t upload(T *&p, const T *src, size_t count, hipStream_t st)
    {
        hipError_t e = alloc(p, count);
        if (e == hipSuccess && count) e = hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, st);
        return e;
    }
    ~DeviceHold()
    {
        for (void *q : mem) (void)hipFree(q);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

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
