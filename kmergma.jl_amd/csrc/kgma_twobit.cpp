// kgma_twobit.cpp -- host parser of UCSC .2bit files: header, index and per-record tables (format: kgma_twobit.h).  Everything a
// kernel will later index with -- record sizes, block lists, the place of the packed bases -- is validated here, before any
// device work: a bad file ends in a status code.  No HIP header is included; the file also builds with a plain C++ compiler
// (tools/twobit_inspect_main.cpp links it alone).
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "../../include/kgma.h"
#include "kgma_twobit.h"

namespace kgma {

namespace {

constexpr uint32_t TWOBIT_SIG = 0x1A412743u, TWOBIT_SIG_SWAPPED = 0x4327411Au;

int bad(std::string &err, int code, const char *fmt, ...)
{
    char buf[384];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}

// pread of exactly n bytes at `off`; false when the range leaves the file or the read fails
bool read_at(int fd, int64_t file_size, int64_t off, void *dst, int64_t n)
{
    if (off < 0 || n < 0 || off > file_size || n > file_size - off) return false;
    uint8_t *p = static_cast<uint8_t *>(dst);
    while (n > 0) {
        const ssize_t got = pread(fd, p, (size_t)n, (off_t)off);
        if (got <= 0) return false;
        p += got; off += got; n -= got;
    }
    return true;
}

// index and record tables are read front to back in small fields: one pread per 64 KiB instead of one per field (a file of
// many short records would otherwise cost nine system calls per record)
struct Cursor {
    int fd;
    int64_t file_size, pos;
    std::vector<uint8_t> buf;
    int64_t buf_off = 0;
    Cursor(int fd_, int64_t size_, int64_t pos_) : fd(fd_), file_size(size_), pos(pos_) {}
    bool get_at(int64_t off, void *dst, int64_t n)
    {
        if (off < 0 || off > file_size) return false;
        pos = off;
        return get(dst, n);
    }
    bool get(void *dst, int64_t n)
    {
        if (n > file_size - pos) return false;
        if (n == 0) return true;
        if (pos < buf_off || pos + n > buf_off + (int64_t)buf.size()) {
            const int64_t want = std::min<int64_t>(std::max<int64_t>(n, 65536), file_size - pos);
            buf.resize((size_t)want);
            if (!read_at(fd, file_size, pos, buf.data(), want)) return false;
            buf_off = pos;
        }
        memcpy(dst, buf.data() + (pos - buf_off), (size_t)n);
        pos += n;
        return true;
    }
};

// One block list of record `rec` (`what`: "nBlock" / "maskBlock") whose count field lies at `off`: reads count, starts[] and
// sizes[], checks every block against dna_size, appends the normalised list to `out` and moves `off` behind the table.
int read_blocks(Cursor &cur, int64_t rec, const char *what, int64_t dna_size, int64_t &off, std::vector<TwoBitBlock> &out,
                std::vector<uint32_t> &tmp, std::string &err)
{
    const int64_t file_size = cur.file_size;
    uint32_t count = 0;
    if (!cur.get_at(off, &count, 4))
        return bad(err, KGMA_E_ARG, "record %lld: %sCount at offset %lld lies past the end of the file", (long long)rec, what, (long long)off);
    off += 4;
    const int64_t bytes = (int64_t)count * 8;                          // (count < 2^32: no overflow)
    if (bytes > file_size - off)
        return bad(err, KGMA_E_ARG, "record %lld: %sStarts / %sSizes (%u blocks at offset %lld) run past the end of the file", (long long)rec,
                   what, what, count, (long long)off);
    tmp.resize((size_t)count * 2);
    if (count > 0 && !(bytes <= 4096 ? cur.get_at(off, tmp.data(), bytes) : read_at(cur.fd, file_size, off, tmp.data(), bytes)))
        return bad(err, KGMA_E_ARG, "record %lld: cannot read %sStarts / %sSizes", (long long)rec, what, what);
    off += bytes;
    const size_t first = out.size();
    bool ordered = true;                                               // disjoint, increasing and not adjacent: nothing to merge
    for (uint32_t i = 0; i < count; i++) {
        const uint64_t s = tmp[i], n = tmp[(size_t)count + i];
        if (s + n > (uint64_t)dna_size)
            return bad(err, KGMA_E_ARG, "record %lld: %s %u (start %llu, size %llu) ends behind dnaSize %lld", (long long)rec, what, i,
                       (unsigned long long)s, (unsigned long long)n, (long long)dna_size);
        if (n == 0) continue;
        if (out.size() > first && s <= out.back().end) ordered = false;
        out.push_back(TwoBitBlock{(uint32_t)s, (uint32_t)(s + n)});
    }
    if (!ordered) {
        std::sort(out.begin() + (std::ptrdiff_t)first, out.end(), [](const TwoBitBlock &a, const TwoBitBlock &b) { return a.start < b.start; });
        size_t w = first;
        for (size_t r = first + 1; r < out.size(); r++) {
            if (out[r].start <= out[w].end) out[w].end = std::max(out[w].end, out[r].end);
            else out[++w] = out[r];
        }
        out.resize(w + 1);
    }
    return KGMA_OK;
}

}  // namespace

int twobit_parse(int fd, int64_t file_size, int64_t max_records, TwoBitFile &out, std::string &err)
{
    out = TwoBitFile();
    uint32_t hdr[4] = {0, 0, 0, 0};
    if (!read_at(fd, file_size, 0, hdr, 4)) return bad(err, KGMA_E_ARG, "header: the file is shorter than its signature field");
    if (hdr[0] == TWOBIT_SIG_SWAPPED)
        return bad(err, KGMA_E_UNSUPPORTED, "header: signature 0x%08X is that of a byte-swapped .2bit file (not read)", hdr[0]);
    if (hdr[0] != TWOBIT_SIG) return bad(err, KGMA_E_ARG, "header: signature 0x%08X is not 0x%08X: not a .2bit file", hdr[0], TWOBIT_SIG);
    if (!read_at(fd, file_size, 0, hdr, 16)) return bad(err, KGMA_E_ARG, "header: the file ends inside its 16-byte header");
    if (hdr[1] > 1) return bad(err, KGMA_E_UNSUPPORTED, "header: version %u (0 and 1 are read)", hdr[1]);
    out.version = hdr[1];
    const int64_t n_rec = hdr[2];
    if (n_rec > max_records) return bad(err, KGMA_E_ARG, "header: sequenceCount %lld exceeds the %lld records a genome holds", (long long)n_rec, (long long)max_records);
    // an index entry takes at least 1 + 4 bytes: a count the file cannot hold is refused before anything is sized by it
    const int64_t off_bytes = out.version == 1 ? 8 : 4;
    if (n_rec > (file_size - 16) / (1 + off_bytes))
        return bad(err, KGMA_E_ARG, "header: an index of sequenceCount %lld entries runs past the end of the file", (long long)n_rec);
    out.recs.resize((size_t)n_rec);
    std::vector<int64_t> rec_off((size_t)n_rec);
    Cursor cur(fd, file_size, 16);
    for (int64_t r = 0; r < n_rec; r++) {
        uint8_t name_size = 0;
        char name[256];
        uint64_t off = 0;
        if (!cur.get(&name_size, 1) || !cur.get(name, name_size) || !cur.get(&off, off_bytes))
            return bad(err, KGMA_E_ARG, "record %lld: its index entry (nameSize, name, offset) runs past the end of the file", (long long)r);
        if (off > (uint64_t)file_size)
            return bad(err, KGMA_E_ARG, "record %lld: offset %llu lies past the end of the file (%lld bytes)", (long long)r, (unsigned long long)off,
                       (long long)file_size);
        out.recs[(size_t)r].name.assign(name, name_size);
        rec_off[(size_t)r] = (int64_t)off;
    }
    std::vector<uint32_t> tmp;
    for (int64_t r = 0; r < n_rec; r++) {
        TwoBitRecord &R = out.recs[(size_t)r];
        int64_t off = rec_off[(size_t)r];
        uint32_t dna_size = 0;
        if (!cur.get_at(off, &dna_size, 4))
            return bad(err, KGMA_E_ARG, "record %lld: dnaSize at offset %lld lies past the end of the file", (long long)r, (long long)off);
        off += 4;
        R.dna_size = dna_size;
        R.n_begin = (int64_t)out.n_blocks.size();
        int rc = read_blocks(cur, r, "nBlock", R.dna_size, off, out.n_blocks, tmp, err);
        if (rc != KGMA_OK) return rc;
        R.n_end = (int64_t)out.n_blocks.size();
        R.m_begin = (int64_t)out.m_blocks.size();
        rc = read_blocks(cur, r, "maskBlock", R.dna_size, off, out.m_blocks, tmp, err);
        if (rc != KGMA_OK) return rc;
        R.m_end = (int64_t)out.m_blocks.size();
        uint32_t reserved = 0;
        if (!cur.get_at(off, &reserved, 4))
            return bad(err, KGMA_E_ARG, "record %lld: the reserved field at offset %lld lies past the end of the file", (long long)r, (long long)off);
        off += 4;
        R.packed_off = off;
        R.packed_bytes = (R.dna_size + 3) / 4;
        if (R.packed_bytes > file_size - off)
            return bad(err, KGMA_E_ARG, "record %lld: packedDna (%lld bytes at offset %lld) runs past the end of the file (%lld bytes)", (long long)r,
                       (long long)R.packed_bytes, (long long)off, (long long)file_size);
        // (at most 2^31 records of less than 2^32 bases: the sums stay below 2^63; checked all the same)
        if (R.dna_size > INT64_MAX / 2 - out.total_bases)
            return bad(err, KGMA_E_ARG, "record %lld: the sum of dnaSize overflows 64 bits", (long long)r);
        out.total_bases += R.dna_size;
        out.packed_bytes += R.packed_bytes;
    }
    return KGMA_OK;
}

}  // namespace kgma

extern "C" int kgma_twobit_inspect(const char *path, kgma_twobit_info *info, char *err, int64_t err_cap)
{
    std::string msg;
    int rc = KGMA_OK;
    kgma::TwoBitFile f;
    if (info) memset(info, 0, sizeof *info);
    if (!path || !info) {
        msg = "kgma_twobit_inspect: null argument";
        rc = KGMA_E_ARG;
    } else {
        const int fd = open(path, O_RDONLY);
        struct stat sb;
        if (fd < 0 || fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {
            msg = std::string("cannot open ") + path + " as a regular file";
            rc = KGMA_E_ARG;
        } else {
            rc = kgma::twobit_parse(fd, (int64_t)sb.st_size, kgma::TWOBIT_MAX_RECORDS, f, msg);
        }
        if (fd >= 0) close(fd);
    }
    if (rc == KGMA_OK) {
        info->version = (int32_t)f.version;
        info->n_records = (int64_t)f.recs.size();
        info->total_bases = f.total_bases;
        info->n_blocks = (int64_t)f.n_blocks.size();
        info->mask_blocks = (int64_t)f.m_blocks.size();
        info->packed_bytes = f.packed_bytes;
    }
    if (err && err_cap > 0) snprintf(err, (size_t)err_cap, "%s", msg.c_str());
    return rc;
}
