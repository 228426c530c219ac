// kgma_stage_fill.h -- what the bytes of one window of a staged upload are.  An upload is a byte range of device memory given as
// a sorted list of segments, each backed by host memory or by a stretch of a file, with a gap byte everywhere between them.
// stage_fill is a pure host function (no HIP, no context; files are read with pread on a descriptor), so that it links alone:
// tools/stage_fill_main.cpp checks it against a byte-by-byte model.
#ifndef KGMA_STAGE_FILL_H
#define KGMA_STAGE_FILL_H

#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#pragma GCC visibility push(hidden)   // (internal to libkgma: not part of its dynamic symbol table)
namespace kgma {

// fd < 0: `host` is memory.  fd >= 0, no host: bytes of that file from file_off on.  Both: host is a mapping of the file from file_off
// on -- a stretch is populated (MADV_POPULATE_READ) before it is copied, and read through the descriptor where the kernel refuses
struct StageSeg { int64_t dev_off, len; const uint8_t *host; int fd; int64_t file_off; };

// Writes bytes [b0, e0) of the staging buffer that holds the window starting at device byte w0, and nothing else.  segs: sorted by
// dev_off, not overlapping.  false: a read failed or came up short -- the rest of the range is the gap byte then.
inline bool stage_fill(uint8_t *stage, int64_t w0, int64_t b0, int64_t e0, const StageSeg *segs, size_t n_segs, uint8_t gap)
{
    int64_t at = w0 + b0;
    const int64_t end = w0 + e0;
    size_t si = (size_t)(std::upper_bound(segs, segs + n_segs, at, [](int64_t x, const StageSeg &S) { return x < S.dev_off + S.len; }) - segs);
    while (at < end) {
        if (si == n_segs || segs[si].dev_off >= end) { memset(stage + (at - w0), gap, (size_t)(end - at)); break; }
        const StageSeg &S = segs[si];
        if (S.dev_off > at) { memset(stage + (at - w0), gap, (size_t)(S.dev_off - at)); at = S.dev_off; }
        const int64_t n = std::min<int64_t>(end, S.dev_off + S.len) - at, rel = at - S.dev_off;
        uint8_t *dst = stage + (at - w0);
        bool from_memory = S.host != nullptr;
#ifdef MADV_POPULATE_READ
        if (from_memory && S.fd >= 0 && n > 0) {
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(S.host + rel) & ~(uintptr_t)4095;
            const uintptr_t a1 = reinterpret_cast<uintptr_t>(S.host + rel + n);
            from_memory = madvise(reinterpret_cast<void *>(a0), (size_t)(a1 - a0), MADV_POPULATE_READ) == 0;
        }
#endif
        if (from_memory) {
            memcpy(dst, S.host + rel, (size_t)n);
        } else {
            for (int64_t done = 0; done < n;) {
                const ssize_t got = pread(S.fd, dst + done, (size_t)(n - done), (off_t)(S.file_off + rel + done));
                if (got <= 0) { memset(dst + done, gap, (size_t)(end - at - done)); return false; }
                done += got;
            }
        }
        at += n;
        if (at == S.dev_off + S.len) si++;
    }
    return true;
}

}  // namespace kgma
#pragma GCC visibility pop

#endif
