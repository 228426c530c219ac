// kgma_motif.cpp -- host side of the IUPAC motif search with mismatches (kgma_motif_match, kgma_get_motif_matches; the working
// form of src/RSS.jl; kernel: kgma_motif.hip).
//
// One call: check the motifs and list each one's informative positions, make the genome's plane copy and residue check current,
// run the kernel over the whole batch by the protocol of kgma_search.h and sort the hits by (motif, contig, start).  Every device
// buffer belongs to the context and is kept between calls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "kgma_motif.h"

using namespace kgma;

static_assert(sizeof(kgma_motif_hit) == sizeof(MotifHit), "kgma_motif_hit is the device record");

extern "C" {

int kgma_motif_match(kgma_ctx *ctx, const kgma_genome *gc, const uint8_t *motifs, const int64_t *offsets, int32_t n_motifs,
                     const int32_t *max_mismatch)
{
    const char *fn = "kgma_motif_match";
    if (!ctx || !gc) return KGMA_E_ARG;
    MotifState *S = ctx_motif(ctx);
    S->hits.clear();                                   // (whatever happens below: a failed call leaves no hits of an earlier one behind)
    if (n_motifs < 0 || (n_motifs > 0 && (!motifs || !offsets || !max_mismatch))) return failf(ctx, KGMA_E_ARG, "kgma_motif_match: no motifs");
    std::vector<MotifDesc> descs;
    std::vector<uint32_t> info;
    int P = 0;
    for (int32_t i = 0; i < n_motifs; i++) {
        const int64_t b = offsets[i], m = offsets[i + 1] - b;
        if (m < 1 || m > 64) return failf(ctx, KGMA_E_ARG, "kgma_motif_match: motif %d has %lld symbols (1 ... 64)", i, (long long)m);
        const int32_t d = max_mismatch[i];
        if (d < 0 || d > 15) return failf(ctx, KGMA_E_ARG, "kgma_motif_match: motif %d: max_mismatch %d (0 ... 15)", i, d);
        MotifDesc M{};
        M.info_off = (int32_t)info.size(); M.len = (int32_t)m; M.max_mm = d; M.id = i;
        for (int64_t j = 0; j < m; j++) {
            const uint32_t set = iupac_set(motifs[b + j]);
            if (!set) return failf(ctx, KGMA_E_ARG, "kgma_motif_match: motif %d, symbol %lld (0x%02x) is not an IUPAC nucleotide code", i, (long long)j + 1, motifs[b + j]);
            if (set == 15u) continue;
            info.push_back((uint32_t)j | (set << 8));          // (offsets ascend: those below 32 come first)
            if (j < 32) M.n_lo++; else M.n_hi++;
        }
        if (d >= M.n_lo + M.n_hi)
            return failf(ctx, KGMA_E_ARG, "kgma_motif_match: motif %d: max_mismatch %d is not smaller than its %d informative (non-N) positions: every start would match",
                         i, d, M.n_lo + M.n_hi);
        info.push_back(0x0F00u);                               // the spare entry the kernel's read-ahead touches
        P = std::max(P, motif_planes(d));
        descs.push_back(M);
    }
    int rc = genome_searchable(ctx, gc, PackedCopy::Planes);
    if (rc) return rc;
    const GenomeText g = genome_text(gc);
    const int64_t nc = g.n_contigs;
    const std::vector<int64_t> prefix = tile_prefix(nc, motif_tile_starts(), false, [&](int64_t c) { return g.cd[c].len; });
    const int64_t n_tiles = prefix[(size_t)nc];
    if ((rc = one_launch(ctx, fn, n_tiles, "tiles"))) return rc;
    std::vector<kgma_motif_hit> found;
    if (n_motifs > 0 && n_tiles > 0) {
        int device = 0;
        hipStream_t st = nullptr;
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        ctx_device(ctx, &device, &st);
        ctx_events(ctx, &ev0, &ev1);
        if ((rc = S->q.reserve(ctx, (int64_t)descs.size()))) return rc;
        if ((rc = S->info.reserve(ctx, (int64_t)info.size()))) return rc;
        if ((rc = S->prefix.reserve(ctx, nc + 1))) return rc;
        if ((rc = S->ctl.reserve(ctx, 2))) return rc;
        if ((rc = S->out.reserve(ctx, fn))) return rc;
        KGMA_TRY(hipMemcpyAsync(S->q.d, descs.data(), descs.size() * sizeof(MotifDesc), hipMemcpyHostToDevice, st));
        KGMA_TRY(hipMemcpyAsync(S->info.d, info.data(), info.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        KGMA_TRY(hipMemcpyAsync(S->prefix.d, prefix.data(), prefix.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
        KGMA_TRY(hipEventRecord(ev0, st));
        MotifArgs a{};
        a.planes = g.d_planes; a.ascii = g.d_ascii; a.cd = g.d_cd; a.tile_prefix = S->prefix.d;
        a.n_contigs = (int32_t)nc; a.n_motifs = (int32_t)descs.size();
        a.motifs = S->q.d; a.info = S->info.d;
        unsigned long long ctl[2] = {0, 0};
        int n_launches = 0;
        rc = S->out.fill(ctx, fn, "hits", st, S->ctl.d, ctl, [&](MotifHit *out, unsigned long long cap, unsigned long long *d_ctl) {
            a.out = out; a.cap = cap; a.ctl = d_ctl;
            return launch_motif(a, P, n_tiles, st);
        }, &n_launches);
        if (rc) return rc;
        KGMA_TRY(hipEventRecord(ev1, st));
        KGMA_TRY(hipEventSynchronize(ev1));
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ev0, ev1);
        kgma_stats *stats = ctx_stats(ctx);
        stats->scan_ms = ms;
        stats->n_launches = n_launches;
        if ((rc = S->out.fetch(ctx, fn, ctl[0], found))) return rc;
        std::sort(found.begin(), found.end(), [](const kgma_motif_hit &x, const kgma_motif_hit &y) {
            return x.motif != y.motif ? x.motif < y.motif : x.contig != y.contig ? x.contig < y.contig : x.start < y.start;
        });
    }
    S->hits.swap(found);
    return KGMA_OK;
}

int kgma_get_motif_matches(kgma_ctx *ctx, kgma_motif_hit *out, int64_t cap, int64_t *n)
{
    return ctx ? copy_out(ctx, "kgma_get_motif_matches", ctx_motif(ctx)->hits, out, cap, n) : KGMA_E_ARG;
}

}  // extern "C"
