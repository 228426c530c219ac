// kgma_twobit.h -- host parser of UCSC .2bit files (kgma_twobit.cpp).  No HIP header: a plain C++ compiler builds both files.
//
// The file (all integers 32-bit, in the file's byte order):
//   header   signature 0x1A412743 (0x4327411A: byte-swapped file), version (0: 32-bit record offsets, 1: 64-bit), sequenceCount,
//            reserved
//   index    sequenceCount x { nameSize (1 byte), name, offset of the record from the start of the file }
//   record   dnaSize, nBlockCount, nBlockStarts[], nBlockSizes[], maskBlockCount, maskBlockStarts[], maskBlockSizes[], reserved,
//            packedDna: ceil(dnaSize / 4) bytes, four bases per byte, first base in the two most significant bits,
//            T = 0, C = 1, A = 2, G = 3, last byte zero-padded
// Residue i is N inside an N block, else the letter of its code; then lower-cased inside a mask block.
#ifndef KGMA_TWOBIT_H
#define KGMA_TWOBIT_H

#include <stdint.h>

#include <string>
#include <vector>

namespace kgma {

constexpr int64_t TWOBIT_MAX_RECORDS = 0x7FFFFFF0ll;   // what a genome holds (kgma_genome_from_host)

struct TwoBitBlock {
    uint32_t start, end;          // residues start .. end - 1 (0-based), start < end <= dnaSize
};

struct TwoBitRecord {
    std::string name;
    int64_t dna_size = 0;
    int64_t packed_off = 0;       // file offset of packedDna
    int64_t packed_bytes = 0;     // ceil(dna_size / 4)
    int64_t n_begin = 0, n_end = 0;   // the record's N blocks: TwoBitFile::n_blocks[n_begin .. n_end)
    int64_t m_begin = 0, m_end = 0;   // its mask blocks: TwoBitFile::m_blocks[m_begin .. m_end)
};

// Block lists are NORMALISED: empty blocks dropped, sorted by start, overlapping or adjacent blocks merged -- so the blocks of a
// record are disjoint, increasing and separated by at least one residue (files written by faToTwoBit are in that form already).
struct TwoBitFile {
    uint32_t version = 0;
    int64_t total_bases = 0;
    int64_t packed_bytes = 0;     // sum over the records
    std::vector<TwoBitRecord> recs;
    std::vector<TwoBitBlock> n_blocks, m_blocks;
};

// Reads header, index and the per-record tables of the open file `fd` (file_size bytes) with pread and validates ALL of it: every
// offset, table and packedDna range lies inside the file, every block inside its record, no sum leaves 64 bits, at most
// max_records records.  Returns a KGMA_* status (include/kgma.h): KGMA_E_UNSUPPORTED for a byte-swapped file or version > 1,
// KGMA_E_ARG for everything else that is wrong; `err` then names the record and the field.
int twobit_parse(int fd, int64_t file_size, int64_t max_records, TwoBitFile &out, std::string &err);

}  // namespace kgma

#endif
