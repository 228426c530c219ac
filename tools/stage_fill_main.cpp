// stage_fill_main.cpp -- checks the window filler of the staged upload (kmergma.jl_amd/csrc/kgma_stage_fill.h) against a
// byte-by-byte model, on the CPU and alone (the header needs neither HIP nor a context):
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o stage_fill tools/stage_fill_main.cpp
//   ./stage_fill
// A few hundred seeded random uploads: 0-6 segments of 0-40 bytes with gaps of 0-20 between them, backed by memory or by a
// temporary file the program writes, gap bytes 0 and '\n', windows of 1, 2, 7, 16 and 64 bytes, every window filled in 1-4
// ranges.  Every range is filled into a buffer with guard bytes around it: nothing outside [b0, e0) may change.  Then a file
// that is shorter than a segment claims: the filler must report the failed read and leave the rest of the range as the gap byte.
// Exit status: 0 when everything agrees, 1 with a message otherwise.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../kmergma.jl_amd/csrc/kgma_stage_fill.h"

using kgma::StageSeg;

static int failures = 0;
#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            if (failures++ < 20) { printf(__VA_ARGS__); printf("\n"); } \
        }                                                         \
    } while (0)

constexpr uint8_t GUARD = 0xA5;
constexpr int64_t PAD = 8;

// One range of one window, filled into a guarded buffer; returns the filler's verdict and the bytes of the range
static bool fill_range(const std::vector<StageSeg> &segs, uint8_t gap, int64_t w0, int64_t window, int64_t b0, int64_t e0,
                       std::vector<uint8_t> &got, const char *what)
{
    std::vector<uint8_t> buf((size_t)(window + 2 * PAD), GUARD);
    const bool ok = kgma::stage_fill(buf.data() + PAD, w0, b0, e0, segs.data(), segs.size(), gap);
    for (int64_t i = -PAD; i < window + PAD; i++)
        if (i < b0 || i >= e0) CHECK(buf[(size_t)(i + PAD)] == GUARD, "%s: byte %lld outside [%lld, %lld) of the window at %lld was written", what, (long long)i, (long long)b0, (long long)e0, (long long)w0);
    got.assign(buf.begin() + PAD + b0, buf.begin() + PAD + e0);
    return ok;
}

int main()
{
    char path[] = "/tmp/stage_fill_XXXXXX";
    const int fd = mkstemp(path);
    if (fd < 0) { printf("cannot create a temporary file\n"); return 1; }
    std::mt19937_64 rng(20240607);
    auto pick = [&](int64_t lo, int64_t hi) { return (int64_t)(rng() % (uint64_t)(hi - lo + 1)) + lo; };
    const int64_t windows[] = {1, 2, 7, 16, 64};
    int64_t file_len = 0;
    for (int trial = 0; trial < 400; trial++) {
        const uint8_t gap = trial & 1 ? '\n' : 0;
        // the segments, their backing bytes, and the model: the whole upload byte by byte
        const int n_segs = (int)pick(0, 6);
        std::vector<std::vector<uint8_t>> mem((size_t)n_segs);
        std::vector<StageSeg> segs;
        std::vector<uint8_t> model;
        for (int s = 0; s < n_segs; s++) {
            model.insert(model.end(), (size_t)pick(0, 20), gap);
            const int64_t len = pick(0, 40);
            std::vector<uint8_t> &bytes = mem[(size_t)s];
            for (int64_t i = 0; i < len; i++) bytes.push_back((uint8_t)pick(1, 255));
            if (pick(0, 1)) {
                segs.push_back(StageSeg{(int64_t)model.size(), len, bytes.data(), -1, 0});
            } else {                                             // in the file, behind what earlier trials wrote
                if (len && pwrite(fd, bytes.data(), (size_t)len, (off_t)file_len) != (ssize_t)len) { printf("cannot write the temporary file\n"); return 1; }
                segs.push_back(StageSeg{(int64_t)model.size(), len, nullptr, fd, file_len});
                file_len += len;
            }
            model.insert(model.end(), bytes.begin(), bytes.end());
        }
        model.insert(model.end(), (size_t)pick(0, 20), gap);
        const int64_t total = (int64_t)model.size();
        for (const int64_t window : windows)
            for (int64_t w0 = 0; w0 < total; w0 += window) {
                const int64_t len = std::min(window, total - w0);
                const int64_t T = pick(1, 4), per = (len + T - 1) / T;   // (parallel_ranges' cut)
                for (int64_t t = 0; t < T; t++) {
                    const int64_t b0 = std::min(len, t * per), e0 = std::min(len, (t + 1) * per);
                    std::vector<uint8_t> got;
                    CHECK(fill_range(segs, gap, w0, window, b0, e0, got, "random upload"), "trial %d: a read failed", trial);
                    for (int64_t i = b0; i < e0; i++)
                        CHECK(got[(size_t)(i - b0)] == model[(size_t)(w0 + i)], "trial %d, window %lld at %lld: byte %lld is 0x%02x, the model has 0x%02x", trial,
                              (long long)window, (long long)w0, (long long)i, got[(size_t)(i - b0)], model[(size_t)(w0 + i)]);
                }
            }
    }
    // a file shorter than a segment claims: 10 bytes are there, the segment says 30
    {
        const std::vector<uint8_t> bytes(10, 'G');
        if (pwrite(fd, bytes.data(), bytes.size(), (off_t)file_len) != (ssize_t)bytes.size()) { printf("cannot write the temporary file\n"); return 1; }
        const std::vector<StageSeg> segs{StageSeg{4, 30, nullptr, fd, file_len}};
        for (const uint8_t gap : {(uint8_t)0, (uint8_t)'\n'}) {
            std::vector<uint8_t> got;
            CHECK(!fill_range(segs, gap, 0, 64, 0, 40, got, "short file"), "short file: the failed read was not reported");
            for (int64_t i = 0; i < 40; i++) {
                const uint8_t want = i >= 4 && i < 14 ? 'G' : gap;
                CHECK(got[(size_t)i] == want, "short file: byte %lld is 0x%02x, expected 0x%02x", (long long)i, got[(size_t)i], want);
            }
            CHECK(fill_range(segs, gap, 0, 64, 0, 14, got, "short file"), "short file: a range that ends with the file reported a failure");
        }
    }
    close(fd);
    unlink(path);
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("stage_fill: ok\n");
    return 0;
}
