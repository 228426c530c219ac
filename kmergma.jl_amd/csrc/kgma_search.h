// kgma_search.h -- what the host files beside kgma_api.cpp share (host side only): the view they have of a context and a genome,
// whose structs are kgma_api.cpp's (the functions declared below are defined there and are all of the two that these files see),
// and the protocol of the five sequence searches (kgma_exact.cpp, kgma_motif.cpp, kgma_approx.cpp, kgma_pwm.cpp, kgma_codon.cpp):
//
//   a per-record prefix of workgroup counts (tile_prefix) that must fit one launch (one_launch); a genome whose packed copy and
//   residue check are current (genome_searchable); a buffer of hit records kept on the context (HitBuffer): 65,536 records at
//   first, filled by one launch that counts every hit, also those that do not fit, and, when they did not fit, regrown once to
//   exactly the counted size and filled by a second launch; the hits brought down and sorted by (pattern, record, position); and a
//   getter the caller asks twice, for the number and for the records (copy_out).
#ifndef KGMA_SEARCH_H
#define KGMA_SEARCH_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/kgma.h"
#include "kgma_device.h"

namespace kgma {

// ---- the view of a context and a genome (kgma_api.cpp) ---------------------------------------------------------------------------
struct GenomeText {
    const uint8_t *d_ascii;       // residue text on the device
    const ContigDesc *d_cd;       // record table on the device ...
    const ContigDesc *cd;         // ... and on the host
    int64_t n_contigs;
    const uint32_t *d_planes;     // the bit planes (made on demand: current after genome_searchable(..., PackedCopy::Planes))
    const uint32_t *d_inter;      // the 2-bit interleaved copy (current after genome_searchable(..., PackedCopy::Inter))
};
enum class PackedCopy { Inter, Planes };

int ctx_fail(kgma_ctx *ctx, int code, const char *message);   // sets kgma_last_error; returns code
void ctx_device(const kgma_ctx *ctx, int *device, hipStream_t *stream);
void ctx_events(const kgma_ctx *ctx, hipEvent_t *ev0, hipEvent_t *ev1);   // the context's pair of timing events
kgma_stats *ctx_stats(kgma_ctx *ctx);
int64_t *ctx_device_bytes(kgma_ctx *ctx);                     // the context's account of its device memory
kgma_spectrum_stats *ctx_spectrum_stats(kgma_ctx *ctx);       // the last kgma_genome_kmer_count (kgma_spectrum.cpp)
void ctx_set_kernel_name(kgma_ctx *ctx, const char *name);    // what kgma_scan_kernel_name answers
GenomeText genome_text(const kgma_genome *g);
// What a search does before it launches: the device is made current, the pack's residue check and the packed copy the kernel reads
// are made current, bases_scanned is set and scan_ms / n_launches are zeroed in kgma_stats.  clean == nullptr: a residue outside
// A/C/G/T/N in any record is KGMA_E_BADBASE; else *clean says whether there is none, and the caller deals with the others.
int genome_searchable(kgma_ctx *ctx, const kgma_genome *g, PackedCopy copy = PackedCopy::Inter, bool *clean = nullptr);

inline int failf(kgma_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return ctx_fail(ctx, code, buf);
}

// (where `ctx` is the context and `fn` the name of the entry point)
#define KGMA_TRY(expr)                                                                                       \
    do {                                                                                                     \
        const hipError_t e__ = (expr);                                                                       \
        if (e__ != hipSuccess) return kgma::failf(ctx, KGMA_E_HIP, "%s: %s failed: %s", fn, #expr, hipGetErrorString(e__)); \
    } while (0)

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

// A device buffer the context keeps between calls and accounts in device_bytes: at least `need` elements after the call (what it
// held is not kept when it grows)
template <class T>
int dev_reserve(kgma_ctx *ctx, T *&ptr, int64_t &cap, int64_t need)
{
    if (need <= cap && ptr) return KGMA_OK;
    int64_t &device_bytes = *ctx_device_bytes(ctx);
    if (ptr) { (void)hipFree(ptr); device_bytes -= cap * (int64_t)sizeof(T); ptr = nullptr; cap = 0; }
    const int64_t n = std::max<int64_t>(need, 16);
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&ptr), (size_t)n * sizeof(T));
    if (e != hipSuccess) return failf(ctx, KGMA_E_HIP, "hipMalloc of %lld bytes failed: %s", (long long)n * (long long)sizeof(T), hipGetErrorString(e));
    cap = n;
    device_bytes += n * (int64_t)sizeof(T);
    return KGMA_OK;
}
template <class T>
struct Kept {
    T *d = nullptr;
    int64_t cap = 0;
    int reserve(kgma_ctx *ctx, int64_t need) { return dev_reserve(ctx, d, cap, need); }
    void release() { if (d) (void)hipFree(d); d = nullptr; cap = 0; }
};

// ---- what the searches share ---------------------------------------------------------------------------------------------------
// base set of an IUPAC symbol (bit 0 A, 1 C, 2 G, 3 T), either case; 0: not one of the 15 symbols
inline uint32_t iupac_set(uint8_t ch)
{
    switch (ch & 0xDFu) {
    case 'A': return 1;  case 'C': return 2;  case 'G': return 4;  case 'T': return 8;
    case 'R': return 5;  case 'Y': return 10; case 'S': return 6;  case 'W': return 9;
    case 'K': return 12; case 'M': return 3;  case 'B': return 14; case 'D': return 13;
    case 'H': return 11; case 'V': return 7;  case 'N': return 15;
    default: return 0;
    }
}

// a record's slot in the residue text: its residues rounded up to 32 bytes, and 32 more
inline int64_t record_slot_bytes(int64_t len) { return ((len + 31) & ~31ll) + 32; }

// tiles of `per_tile` units over n records of len_of(c) residues, one record after the other: prefix[c] tiles lie before record c,
// prefix[n] is their number.  by_slot: a record counts its whole slot of the text, else the starts a pattern of min_len residues
// has in it (min_len 1: its residues)
template <class LenOf>
std::vector<int64_t> tile_prefix(int64_t n, int64_t per_tile, bool by_slot, LenOf len_of, int64_t min_len = 1)
{
    std::vector<int64_t> prefix((size_t)n + 1, 0);
    for (int64_t c = 0; c < n; c++) {
        const int64_t units = by_slot ? record_slot_bytes(len_of(c)) : std::max<int64_t>(0, len_of(c) - min_len + 1);
        prefix[(size_t)c + 1] = prefix[(size_t)c] + (units + per_tile - 1) / per_tile;
    }
    return prefix;
}

// a launch's grid holds at most 2^31 - 1 workgroups (`unit`: what the caller calls them)
inline int one_launch(kgma_ctx *ctx, const char *fn, int64_t n_groups, const char *unit)
{
    if (n_groups > 0x7FFFFFFFll) return failf(ctx, KGMA_E_UNSUPPORTED, "%s: %lld %s exceed one launch", fn, (long long)n_groups, unit);
    return KGMA_OK;
}

// The buffer of hit records a search keeps on the context.  `fn` names the entry point and `noun` its records in the messages.
template <class Rec>
struct HitBuffer {
    static constexpr int64_t FIRST_CAP = (int64_t)1 << 16;
    Rec *d = nullptr;
    int64_t cap = 0;

    int reserve(kgma_ctx *ctx, const char *fn)       // the first capacity, once
    {
        if (d) return KGMA_OK;
        if (hipMalloc(reinterpret_cast<void **>(&d), (size_t)FIRST_CAP * sizeof(Rec)) != hipSuccess) {
            (void)hipGetLastError();
            d = nullptr;
            return failf(ctx, KGMA_E_NOMEM, "%s: no device memory for the hit buffer", fn);
        }
        cap = FIRST_CAP;
        *ctx_device_bytes(ctx) += FIRST_CAP * (int64_t)sizeof(Rec);
        return KGMA_OK;
    }
    void release() { if (d) (void)hipFree(d); d = nullptr; cap = 0; }

    // launch(out, cap, d_ctl) fills the reserved buffer: it writes the hits that fit and counts every hit in d_ctl[0].  ctl: the
    // values the two control words have in front of a launch, and after the call what the last launch left in them -- ctl[0] hits
    // are in the buffer.  A count beyond the capacity: the buffer is regrown to exactly that count (the larger one is taken before
    // the old one is given up: without room for it the context stays as it was) and the launch repeated, once.  The second word
    // is the kernel's to report trouble in: a launch that changes it ends the call there, and the caller looks at it.
    template <class Launch>
    int fill(kgma_ctx *ctx, const char *fn, const char *noun, hipStream_t st, unsigned long long *d_ctl, unsigned long long (&ctl)[2],
             Launch launch, int *n_launches)
    {
        const unsigned long long init[2] = {ctl[0], ctl[1]};
        for (int attempt = 0;; attempt++) {
            // (zeros are set on the device, other values copied there)
            if (init[0] || init[1]) KGMA_TRY(hipMemcpyAsync(d_ctl, init, sizeof init, hipMemcpyHostToDevice, st));
            else KGMA_TRY(hipMemsetAsync(d_ctl, 0, sizeof init, st));
            KGMA_TRY(launch(d, (unsigned long long)cap, d_ctl));
            ++*n_launches;
            KGMA_TRY(hipMemcpyAsync(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
            KGMA_TRY(hipStreamSynchronize(st));
            if (ctl[1] != init[1] || ctl[0] <= (unsigned long long)cap) return KGMA_OK;
            if (attempt == 1) return failf(ctx, KGMA_E_OVERFLOW, "%s: %llu %s overflowed the regrown buffer", fn, ctl[0], noun);
            Rec *fresh = nullptr;
            if (ctl[0] > (1ull << 40) || hipMalloc(reinterpret_cast<void **>(&fresh), (size_t)ctl[0] * sizeof(Rec)) != hipSuccess) {
                (void)hipGetLastError();
                return failf(ctx, KGMA_E_NOMEM, "%s: no device memory for %llu %s", fn, ctl[0], noun);
            }
            (void)hipFree(d);
            *ctx_device_bytes(ctx) += ((int64_t)ctl[0] - cap) * (int64_t)sizeof(Rec);
            d = fresh; cap = (int64_t)ctl[0];
        }
    }

    // the first n records of the buffer (fill has waited for them), appended to `found` (Host: the record as include/kgma.h
    // declares it)
    template <class Host>
    int fetch(kgma_ctx *ctx, const char *fn, unsigned long long n, std::vector<Host> &found) const
    {
        const size_t n0 = found.size();
        found.resize(n0 + (size_t)n);
        if (n) KGMA_TRY(hipMemcpy(found.data() + n0, d, (size_t)n * sizeof(Rec), hipMemcpyDeviceToHost));
        return KGMA_OK;
    }
};

// The getters' two calls: out == nullptr asks for the number, else `v` is copied to out[0, cap)
template <class T>
int copy_out(kgma_ctx *ctx, const char *fn, const std::vector<T> &v, T *out, int64_t cap, int64_t *n)
{
    if (!n) return KGMA_E_ARG;
    *n = (int64_t)v.size();
    if (!out) return KGMA_OK;
    if (cap < *n) return failf(ctx, KGMA_E_ARG, "%s: capacity %lld < %lld", fn, (long long)cap, (long long)*n);
    if (*n) memcpy(out, v.data(), (size_t)*n * sizeof(T));
    return KGMA_OK;
}

}  // namespace kgma

#endif
