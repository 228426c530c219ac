// spectrum_plan_main.cpp -- checks the plan of kgma_genome_kmer_count (kmergma.jl_amd/csrc/kgma_spectrum.h: argument checks,
// considered starts, covered residues, unit prefix, form and geometry) on the CPU and alone -- the header needs neither HIP nor a
// context:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o spectrum_plan tools/spectrum_plan_main.cpp
//   ./spectrum_plan
// Seeded random range lists over random records, every k, every flag set, every forced form and workgroup cap, against a model
// that counts the considered starts one by one; then every argument error of include/kgma.h with its status.
// Exit status: 0 when everything agrees, 1 with a message otherwise.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../kmergma.jl_amd/csrc/kgma_spectrum.h"

using namespace kgma;

static int failures = 0;
#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            if (failures++ < 20) { printf(__VA_ARGS__); printf("\n"); } \
        }                                                         \
    } while (0)

static void random_lists(uint64_t seed)
{
    std::mt19937_64 rng(seed);
    auto upto = [&](int64_t n) { return (int64_t)(rng() % (uint64_t)(n + 1)); };
    const int64_t n_records = 1 + upto(4);
    std::vector<int64_t> len((size_t)n_records);
    for (auto &L : len) L = upto(3) == 0 ? upto(12) : upto(40000);
    const int32_t k = (int32_t)(1 + upto(9));
    const uint32_t flags = (uint32_t)upto(7);
    const int64_t n_ranges = 1 + upto(30);
    std::vector<int32_t> contig((size_t)n_ranges);
    std::vector<int64_t> lo((size_t)n_ranges), hi((size_t)n_ranges);
    for (int64_t r = 0; r < n_ranges; r++) {
        contig[(size_t)r] = (int32_t)upto(n_records - 1);
        const int64_t L = len[(size_t)contig[(size_t)r]];
        lo[(size_t)r] = 1 + upto(L);                                // 1 .. L + 1
        hi[(size_t)r] = lo[(size_t)r] - 1 + upto(L - lo[(size_t)r] + 1);
    }
    const int forced = (int)upto(3) - 1, wgs = upto(2) == 0 ? (int)(1 + upto(3)) : 0;
    SpectrumPlan P;
    std::string err;
    bool empty = true;
    const int rc = spectrum_plan("t", len.data(), n_records, k, flags, n_ranges, contig.data(), lo.data(), hi.data(), true, forced, wgs, 256, P,
                                 err, &empty);
    CHECK(rc == KGMA_OK && !empty, "seed %llu: rc %d (%s)", (unsigned long long)seed, rc, err.c_str());
    if (rc) return;
    int64_t total = 0;
    for (int64_t r = 0; r < n_ranges; r++) {
        const int64_t L = len[(size_t)contig[(size_t)r]];
        int64_t starts = 0, last = lo[(size_t)r] - 1;
        for (int64_t p = lo[(size_t)r]; p <= hi[(size_t)r]; p++) {
            const bool considered = (flags & KGMA_COUNT_BY_START) ? p + k - 1 <= L : p + k - 1 <= hi[(size_t)r];
            starts += considered;
            last = (flags & KGMA_COUNT_BY_START) ? std::min<int64_t>(hi[(size_t)r] + k - 1, L) : hi[(size_t)r];
        }
        CHECK(P.starts[(size_t)r] == starts, "seed %llu range %lld: %lld starts, model %lld", (unsigned long long)seed, (long long)r,
              (long long)P.starts[(size_t)r], (long long)starts);
        CHECK(P.cover[(size_t)r] == last - lo[(size_t)r] + 1, "seed %llu range %lld: cover %lld", (unsigned long long)seed, (long long)r,
              (long long)P.cover[(size_t)r]);
        CHECK(starts == 0 || P.cover[(size_t)r] == starts + k - 1, "seed %llu range %lld: cover is not starts + k - 1", (unsigned long long)seed, (long long)r);
        CHECK(lo[(size_t)r] - 1 + P.cover[(size_t)r] <= L, "seed %llu range %lld: covers past the record", (unsigned long long)seed, (long long)r);
        const int64_t units = P.prefix[(size_t)r + 1] - P.prefix[(size_t)r];
        CHECK(units == (starts ? (starts + P.span - 1) / P.span : P.cover[(size_t)r] ? 1 : 0), "seed %llu range %lld: %lld units", (unsigned long long)seed,
              (long long)r, (long long)units);
        total += starts;
    }
    CHECK(P.n_positions == total && P.n_units == P.prefix[(size_t)n_ranges], "seed %llu: totals", (unsigned long long)seed);
    const bool allowed = forced == SP_FORM_GLOBAL || (forced == SP_FORM_WG && k <= 7) || (forced == SP_FORM_WAVE && k <= 4);
    if (allowed) CHECK(P.form == forced, "seed %llu: form %d, forced %d", (unsigned long long)seed, P.form, forced);
    else CHECK(P.form == (k > 7 ? SP_FORM_GLOBAL : (k <= 4 && total < n_ranges * (int64_t)SP_WG_SPAN) ? SP_FORM_WAVE : SP_FORM_WG), "seed %llu: form %d", (unsigned long long)seed, P.form);
    CHECK(P.span == (P.form == SP_FORM_WAVE ? SP_WAVE_SPAN : SP_WG_SPAN) && P.span % 64 == 0, "seed %llu: span", (unsigned long long)seed);
    CHECK(P.lds_bytes == sp_lds_bytes(P.form, k, P.span) && P.lds_bytes <= 160 * 1024, "seed %llu: %zu bytes of LDS", (unsigned long long)seed, P.lds_bytes);
    if (P.n_units) {
        CHECK(P.units_per_group >= 1 && P.units_per_group * (int64_t)P.span <= SP_TABLE_MAX, "seed %llu: chunk", (unsigned long long)seed);
        CHECK(P.n_groups * P.units_per_group >= P.n_units && (P.n_groups - 1) * P.units_per_group < P.n_units, "seed %llu: groups", (unsigned long long)seed);
        CHECK(P.n_workgroups * sp_groups_per_wg(P.form) >= P.n_groups && P.n_workgroups >= 1, "seed %llu: workgroups", (unsigned long long)seed);
        if (wgs) CHECK(P.n_workgroups <= wgs, "seed %llu: %lld workgroups, cap %d", (unsigned long long)seed, (long long)P.n_workgroups, wgs);
    }
}

static int plan_rc(int32_t k, uint32_t flags, int64_t n, const int32_t *c, const int64_t *lo, const int64_t *hi, bool counts, std::string &err,
                   bool *empty)
{
    static const int64_t len[2] = {10, 4};
    SpectrumPlan P;
    return spectrum_plan("t", len, 2, k, flags, n, c, lo, hi, counts, -1, 0, 256, P, err, empty);
}

static void argument_errors()
{
    const int32_t c0[1] = {0}, c2[1] = {2}, cneg[1] = {-1}, c1[1] = {1};
    const int64_t one[1] = {1}, four[1] = {4}, zero[1] = {0}, five[1] = {5}, three[1] = {3}, eleven[1] = {11};
    std::string err;
    bool empty = false;
    CHECK(plan_rc(2, 0, 1, c0, one, four, true, err, &empty) == KGMA_OK && !empty, "a good call");
    CHECK(plan_rc(2, 0, 0, nullptr, nullptr, nullptr, false, err, &empty) == KGMA_OK && empty, "no ranges");
    CHECK(plan_rc(0, 0, 1, c0, one, four, true, err, &empty) == KGMA_E_ARG, "k = 0");
    CHECK(plan_rc(11, 0, 1, c0, one, four, true, err, &empty) == KGMA_E_UNSUPPORTED, "k = 11");
    CHECK(plan_rc(2, 8, 1, c0, one, four, true, err, &empty) == KGMA_E_ARG, "flag 8");
    CHECK(plan_rc(2, 0, -1, c0, one, four, true, err, &empty) == KGMA_E_ARG, "n = -1");
    CHECK(plan_rc(2, 0, 1, nullptr, one, four, true, err, &empty) == KGMA_E_ARG, "null contig");
    CHECK(plan_rc(2, 0, 1, c0, nullptr, four, true, err, &empty) == KGMA_E_ARG, "null lo");
    CHECK(plan_rc(2, 0, 1, c0, one, nullptr, true, err, &empty) == KGMA_E_ARG, "null hi");
    CHECK(plan_rc(2, 0, 1, c0, one, four, false, err, &empty) == KGMA_E_ARG, "null counts");
    CHECK(plan_rc(2, 0, 1, c2, one, four, true, err, &empty) == KGMA_E_ARG && err.find("no record 2") != std::string::npos, "record 2");
    CHECK(plan_rc(2, 0, 1, cneg, one, four, true, err, &empty) == KGMA_E_ARG, "record -1");
    CHECK(plan_rc(2, 0, 1, c0, zero, four, true, err, &empty) == KGMA_E_ARG && err.find("range 0: 0:4") != std::string::npos, "lo = 0");
    CHECK(plan_rc(2, 0, 1, c1, one, five, true, err, &empty) == KGMA_E_ARG, "hi > L");
    CHECK(plan_rc(2, 0, 1, c0, five, three, true, err, &empty) == KGMA_E_ARG, "hi < lo - 1");
    CHECK(plan_rc(2, 0, 1, c0, five, four, true, err, &empty) == KGMA_OK, "hi = lo - 1");
    CHECK(plan_rc(2, 0, 1, c0, eleven, eleven, true, err, &empty) == KGMA_E_ARG, "lo = L + 1 with hi = lo");
    CHECK(plan_rc(10, 0, 257, c0, one, four, true, err, &empty) == KGMA_E_UNSUPPORTED && err.find("2^28") != std::string::npos, "2^28 counts");   // (refused before a range is read)
}

int main()
{
    for (uint64_t seed = 1; seed <= 600; seed++) random_lists(seed);
    argument_errors();
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("spectrum plan ok\n");
    return 0;
}
