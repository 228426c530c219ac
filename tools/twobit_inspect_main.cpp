// twobit_inspect_main.cpp -- prints what the host parser of kgma_genome_from_2bit_file (kmergma.jl_amd/csrc/kgma_twobit.cpp)
// makes of .2bit files: per file the status and, for a file it accepts, the record table.  Links the parser alone, no HIP:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
//       -o twobit_inspect tools/twobit_inspect_main.cpp kmergma.jl_amd/csrc/kgma_twobit.cpp
//   ./twobit_inspect file.2bit ...
// (the stand-alone program under which the parser is run with the sanitizers over good and malformed files).
// Exit status: 0 when every file was parsed or refused with a status and a message, 2 when a refusal came without a message.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <string>

#include "../include/kgma.h"
#include "../kmergma.jl_amd/csrc/kgma_twobit.h"

int main(int argc, char **argv)
{
    int bad = 0;
    for (int i = 1; i < argc; i++) {
        const int fd = open(argv[i], O_RDONLY);
        struct stat sb;
        if (fd < 0 || fstat(fd, &sb) != 0) {
            printf("%s: cannot open\n", argv[i]);
            if (fd >= 0) close(fd);
            continue;
        }
        kgma::TwoBitFile f;
        std::string err;
        const int rc = kgma::twobit_parse(fd, (int64_t)sb.st_size, kgma::TWOBIT_MAX_RECORDS, f, err);
        close(fd);
        if (rc != KGMA_OK) {
            printf("%s: status %d: %s\n", argv[i], rc, err.c_str());
            if (err.empty()) bad = 2;
            continue;
        }
        printf("%s: version %u, %zu records, %lld bases, %zu N blocks, %zu mask blocks, %lld packed bytes\n", argv[i], f.version,
               f.recs.size(), (long long)f.total_bases, f.n_blocks.size(), f.m_blocks.size(), (long long)f.packed_bytes);
        for (size_t r = 0; r < f.recs.size(); r++) {
            const kgma::TwoBitRecord &R = f.recs[r];
            printf("  %zu '%s': dnaSize %lld, packedDna at %lld (%lld bytes), N blocks", r, R.name.c_str(), (long long)R.dna_size,
                   (long long)R.packed_off, (long long)R.packed_bytes);
            for (int64_t j = R.n_begin; j < R.n_end && j < R.n_begin + 8; j++) printf(" [%u,%u)", f.n_blocks[(size_t)j].start, f.n_blocks[(size_t)j].end);
            printf(" (%lld), mask blocks", (long long)(R.n_end - R.n_begin));
            for (int64_t j = R.m_begin; j < R.m_end && j < R.m_begin + 8; j++) printf(" [%u,%u)", f.m_blocks[(size_t)j].start, f.m_blocks[(size_t)j].end);
            printf(" (%lld)\n", (long long)(R.m_end - R.m_begin));
        }
    }
    return bad;
}
