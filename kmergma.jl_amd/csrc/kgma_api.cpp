// kgma_api.cpp -- host side of libkgma: the C ABI declared in include/kgma.h.
//
// Owns device memory, launches the gfx950 kernels of kgma_kernels.hip, stitches the per-lane dip
// fragments the scan kernel emits into dips, and replays the reference's hit state machine over
// them (src/GenomeMiner.jl:82-104, src/OmnGenomeMiner.jl:113-156) -- O(#dips) host work, with the
// optional alignment callback interleaved exactly where the reference calls BioAlignments.
//
// There is no CPU fallback for the scan itself: without a HIP device kgma_create fails.

#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <pthread.h>
#include <sched.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <optional>
#include <mutex>
#include <functional>
#include <thread>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/kgma.h"
#include "kgma_device.h"
#include "kgma_chain.h"
#include "kgma_assign.h"
#include "kgma_stage_fill.h"
#include "kgma_twobit.h"
#include "kgma_landscape.h"
#include "kgma_exact.h"
#include "kgma_motif.h"
#include "kgma_approx.h"
#include "kgma_pwm.h"
#include "kgma_codon.h"

namespace kgma {
hipError_t launch_scan(const ScanArgs &a, const GroupParams &gp, hipStream_t st);
hipError_t launch_stream(const ScanArgs &a, const GroupParams &gp, hipStream_t st);
bool filter_applies(int k, int64_t s_max);
hipError_t launch_filter(const FilterArgs &a, int k, int64_t s_max, int n_cus, unsigned int *host_count, int32_t *form, hipStream_t st);
bool pack_sums_applies(int k, int64_t s_max);
int stream_waves(int k, int nk, int n_kfv, int n_sizes);
int stream_slots_per_cu(int k, int nk, int nk_min, int n_longer, int n_kfv, int n_sizes, bool s16, int64_t n_ref, bool u8, int n_plus2, bool need_wide);
bool stream8_derive_applies(int k, int nk_min, int nk_max, int n_kfv, int64_t n_ref, bool s16);
bool stream8_wide_applies(int k, int nk_min, int nk_max, int n_kfv, int64_t n_ref, bool u8, bool s16, int n_plus1, int n_plus2);
bool stream8_applies(int k, int nk, int n_kfv, int64_t n_ref, bool s16);
int stream8_variant(int n_kfv);
int stream8_state_words(int k, int n_kfv);
bool stream8_c16_applies(int k, int nk, int n_kfv, int64_t n_ref, bool s16, bool need_wide);
int generic_slots_per_cu(int k, bool fp, int nk_max);
int generic_count_mode(int k, int nk_max);               // 0: counters in LDS, 1: in global memory (GenParams::ctab), 2: hash table in LDS
void generic_set_mode(GenParams &g, int nk_max);
hipError_t launch_generic(const ScanArgs &a, const GenParams &g, hipStream_t st);
int generic_chain_slots_per_cu(int k, int nk);
hipError_t launch_generic_chain(const ScanArgs &a, const GenParams &g, hipStream_t st);
int strobe_slots_per_cu(int s);
hipError_t launch_strobe(const ScanArgs &a, const StrobeParams &g, hipStream_t st);
hipError_t launch_pos(const ScanArgs &a, const GroupParams &gp, int j0, int nj, hipStream_t st);
bool chain_applies(int k, int nk, int64_t n_ref, bool s16, bool need_wide);
int chain_slots_per_cu(int k, bool s16, int nkfv, int nk, bool need_wide);
hipError_t launch_chain(const ScanArgs &a, const GroupParams &gp, hipStream_t st);
int pos_tables_per_pass(int k);
int64_t align_trace_bytes(int m, int n);
hipError_t launch_align(const uint8_t *ascii, const AlignJob *jobs, int n_jobs, const uint8_t *cons, int m, int go, int ge,
                        uint8_t *trace, int64_t trace_stride, int max_n, int64_t *out, hipStream_t st);
hipError_t launch_gather_ranges(const uint8_t *src, const int64_t *desc, int n, uint8_t *dst, hipStream_t st);
hipError_t launch_export(uint8_t *res, uint8_t *host, int64_t d0_slots, int64_t d0_used, unsigned int rec_cap, unsigned int inline_recs,
                         int do_gather, const TileDesc *tiles, const ContigDesc *cd, const uint8_t *ascii, const int64_t *Wtab,
                         unsigned int *done, hipStream_t st);
int scan_tile_stride_words(int nk);
int scan_nblocks(int nk);
int kdist_grid(int k, int64_t n_seqs);
hipError_t launch_kdist(int mode, const uint8_t *seqs, const int64_t *off, int64_t n_seqs, int k, const double *ref,
                        uint32_t *scratch, double scale, double *out, unsigned long long *first_bad, hipStream_t st);
}  // namespace kgma

using namespace kgma;

struct kgma_genome {
    int64_t n_contigs = 0;
    int64_t total_bases = 0;
    int64_t total_words = 0;      // plane words incl. padding
    int64_t ascii_bytes = 0;
    std::vector<kgma::ContigDesc> cd;
    std::vector<std::string> headers;          // FASTA header lines (without '>') or .2bit record names; empty for genomes built otherwise
    unsigned long long *first_bad = nullptr;   // pinned host copy, valid once pack_pending is cleared
    bool pack_pending = false;
    bool repack_deferred = false; // kgma_repack_scan_hits: the re-encoding is still to be launched -- by the next scan, group by group beside
                                  // its scan launches when that scan qualifies (launch_overlapped), else as one launch in front of it
    bool text_dirty = true;      // residue text changed since first_bad was last computed (new genome, poke)
    uint64_t uid = 0;
    uint8_t *d_ascii = nullptr;
    uint32_t *d_planes = nullptr;
    uint32_t *d_inter = nullptr;             // 2-bit interleaved copy (16 bases per dword), written by the pack kernel beside the planes
    // INTER_FULL: d_inter is the text as of the last pack, every word of it.  INTER_PARTIAL: the last pack was a step's sums-only pack
    // (pack_sums_kernel<K, false>), and only the blocks that step packed on demand are written.  Nothing but ensure_inter and the two
    // in-step consumers (pack_candidate_blocks, pack_record_blocks) may hand d_inter on while it is PARTIAL.
    int32_t inter_state = KGMA_INTER_FULL;
    int64_t inter_demand_blocks = 0;         // pack blocks the last step packed on demand (kgma_genome_inter_state)
    kgma::ContigDesc *d_cd = nullptr;
    unsigned long long *d_first_bad = nullptr;
    int32_t *d_block_contig = nullptr;       // record of the first word of every pack block (pack_kernel)
    // the prefilter's block sums (pack_sums_kernel): one uint16 per dword of d_inter, allocated by the first step that fuses them into
    // its pack.  bsum_fresh: written by the pack of the scan that is running (only that scan's filter reads them); bsum_k: the k of
    // the last step that wrote them (0: none; kgma_get_block_sums); bsum_failed: the allocation failed once, plain path from then on
    uint16_t *d_bsum = nullptr;
    bool bsum_fresh = false, bsum_failed = false;
    int bsum_k = 0;
    // The last step's pack made the prefilter's test itself (pack_sums_kernel<K, false, true>) and stored no sum: bsum_state is
    // DEFERRED and ensure_bsum writes them when somebody asks (kgma_get_block_sums), or before the text changes -- with the S table
    // of that step, kept in d_bsum_S (copied when the reference set changed since the last copy).  pack_tested: the pack of the
    // scan that is running tested; its entries are in the context's pinned list (filter_candidate_table).
    int bsum_state = KGMA_BSUM_NONE;
    bool pack_tested = false;
    int32_t *d_bsum_S = nullptr;
    uint64_t bsum_S_refs = ~(uint64_t)0;
    int64_t bsum_smax = 0;
    int64_t device_bytes = 0;
};

// Two pinned staging buffers used alternately: the CPU fills one while the DMA engine drains the other
// (host bytes -> device at the pace of the slower of memcpy and PCIe instead of their sum).
struct StagePipe {
    uint8_t *buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool busy[2] = {false, false};
    int cur = 0;
    size_t cap = 0;
    hipStream_t st = nullptr;
    bool init(size_t cap_, hipStream_t st_)
    {
        cap = cap_; st = st_;
        for (int i = 0; i < 2; i++)
            if (hipHostMalloc(reinterpret_cast<void **>(&buf[i]), cap, hipHostMallocDefault) != hipSuccess ||
                hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) return false;
        return true;
    }
    uint8_t *acquire()                        // buffer to fill next (waits for its previous copy)
    {
        if (busy[cur]) { (void)hipEventSynchronize(ev[cur]); busy[cur] = false; }
        return buf[cur];
    }
    hipError_t submit(uint8_t *dst, size_t n) // copy the buffer just filled to the device, switch buffers
    {
        hipError_t e = hipMemcpyAsync(dst, buf[cur], n, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(ev[cur], st);
        busy[cur] = true;
        cur ^= 1;
        return e;
    }
    void drain()
    {
        for (int i = 0; i < 2; i++)
            if (busy[i]) { (void)hipEventSynchronize(ev[i]); busy[i] = false; }
    }
    ~StagePipe()
    {
        drain();
        for (int i = 0; i < 2; i++) {
            if (buf[i]) (void)hipHostFree(buf[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
    }
};

namespace kgma { int pack_block_words(); }   // kgma_kernels.hip
namespace {

constexpr int64_t CONTIG_PAD_WORDS = 32;
// (the step's pack tests granules on sums of up to 63 consecutive blocks of ONE global block array: the 62 blocks behind a granule's
//  first one must not reach the next record -- pack_sums_kernel<K, false, true>, launch_filter's nblk <= 63)
static_assert(2 * CONTIG_PAD_WORDS >= 62, "a granule's blocks must end inside the padding behind its record");
// the step's pack that makes the prefilter's test: units a wave takes at a time, and the runs per wave below which it is not used
constexpr int PACK_TEST_RUN = 32;
constexpr int64_t PACK_TEST_MIN_RUNS = 4;
constexpr int64_t LEAD_PAD_WORDS = 8;
constexpr int64_t TAIL_PAD_WORDS = KGMA_TILE_WORDS + 128;
constexpr unsigned long long NO_BAD = ~0ull;

// What a context keeps for building and packing its genomes (kgma_create / kgma_destroy call init / release)
struct GenomeStore {
    // ingest: pinned staging pair and device scratch, kept between genomes (allocating and pinning them cost a third of a
    // 400 MB ingest); scratch beyond 2 GiB is given back after use
    StagePipe *pipe = nullptr;
    uint8_t *d_ingest = nullptr; int64_t ingest_cap = 0;                 // raw FASTA text on the device
    uint32_t *d_icounts = nullptr; int64_t icounts_cap = 0;
    uint64_t next_uid = 1;
    hipEvent_t evp0 = nullptr, evp1 = nullptr;                           // around the last pack genome_repack queued
    int numa_state = 0;                                  // 0: not looked up, 1: numa_cpus is the GPU's NUMA node, -1: none / not applicable
    cpu_set_t numa_cpus;                                 // CPUs of the NUMA node the GPU hangs on (NumaBind)
    // sparse step pack: the pack blocks the candidate streams read, sorted (pack_candidate_blocks)
    std::vector<int32_t> blist;
    int32_t *d_blist = nullptr; int64_t blist_cap = 0;
    // reverse complement (kgma_genome_revcomp): the tile table of the last call, on the device and as uploaded
    int64_t *d_rcprefix = nullptr; int64_t rcprefix_cap = 0;
    std::vector<int64_t> rcprefix;
    double twobit_ms = -1;                   // kgma_genome_from_2bit_file: device time of the last call's unpack kernel (-1: none yet)
    bool init() { return hipEventCreate(&evp0) == hipSuccess && hipEventCreate(&evp1) == hipSuccess; }
    void release()
    {
        delete pipe;
        for (void *p : {(void *)d_ingest, (void *)d_icounts, (void *)d_blist, (void *)d_rcprefix}) if (p) (void)hipFree(p);
        for (hipEvent_t e : {evp0, evp1}) if (e) (void)hipEventDestroy(e);
    }
};

// The ingest moves the genome through pinned staging buffers with a few copying threads; on a two-socket host it matters which
// socket they run on: measured on the GPU box (2 x EPYC 9575F, the GPU on node 0), a 1000 MB FASTA file: 45-46 GB/s with the
// process on the GPU's node, 33 GB/s on the other, and either of the two from run to run when left to the scheduler.  NumaBind
// narrows the CALLING thread's CPU affinity to the CPUs of the GPU's NUMA node (the PCI device's numa_node in sysfs) that it is
// allowed to run on, for the duration of an ingest call: the staging buffers are then allocated and pinned from that node and the
// copying threads, which inherit the mask, run there.  The previous mask is restored on return.  KGMA_NUMA_BIND=0: off.
struct NumaBind {
    bool bound = false;
    cpu_set_t saved;
    explicit NumaBind(kgma_ctx *ctx);
    ~NumaBind();
    NumaBind(const NumaBind &) = delete;
    NumaBind &operator=(const NumaBind &) = delete;
};

// Host side of the ingest on a few threads: fn(t, begin, end) over [0, n) cut into equal ranges (one range: inline).
int ingest_threads();
template <class F>
void parallel_ranges(int64_t n, int n_threads, int64_t min_per_thread, F fn)
{
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(n_threads, n / std::max<int64_t>(1, min_per_thread)));
    if (T <= 1) { fn(0, (int64_t)0, n); return; }
    std::vector<std::thread> pool;
    pool.reserve((size_t)T - 1);
    const int64_t per = (n + T - 1) / T;
    for (int t = 1; t < T; t++) pool.emplace_back([=]() { fn(t, std::min<int64_t>(n, t * per), std::min<int64_t>(n, (t + 1) * per)); });
    fn(0, (int64_t)0, std::min<int64_t>(n, per));
    for (std::thread &th : pool) th.join();
}

inline double now_ms()
{
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// what a pack that carries the prefilter's block sums needs of the references (pack_sums_kernel)
// test: the pack makes the prefilter's granule test itself, with this bound, geometry, run length and list capacity
struct PackSums { const int32_t *S; int k; int64_t s_max; int n_cus; bool test = false; uint32_t U = 0; int nblk = 0, nk = 0, run = 0; int64_t cap = 0; };

}  // namespace

namespace {

struct KfvInfo {
    int64_t W = 0;
    int64_t N = 0;
    double thr = 0;
    int64_t T = 0;       // below thr  <=>  D < T
    int64_t T_hi = -1;   // T <= D <= T_hi: at threshold (guard band, usually empty)
    int64_t sumS2 = 0;
    int64_t Smax = 0;
    std::vector<int64_t> S;   // natural k-mer order
    std::vector<double> ref;  // the KFV as given (Float64), for the tie resolver
    bool fits32 = true;       // the prefix E = (D - D0) / 2N and N * count differences fit the int32 kernels (stream8 8-bit form, bit-sliced, ...)
    bool big_ok = false;      // a 64-window step's LOCAL prefix fits int32: the 16-bit counter form of stream8_kernel (64-bit carries) applies
    bool fp = false;          // a general Float64 KFV (not S/N): Float64 form of the generic kernel.  N is then a power of two that only
                              // fixes the host's integer lattice D = round(d * 2kN^2); S is empty
    double sumR2 = 0;         // fp: sum_x ref[x]^2
    int ref_form = -1;        // how the Float64 entries follow from S, bit for bit, so that the device can form them from S (the chain
                              // kernel does): 0 = RN(S * RN(1/N)) (`answer .* (1/N)`, src/ReferenceGeneration.jl:35,40), 1 = RN(S / N)
                              // (`KFVs[i] ./= lens[i]`, :118) reproduced by the kernel's own division step, -1 = neither
    // k >= 11 (sparse): no 4^k table exists -- S and ref above stay empty, and the KFV is its non-zero entries in increasing natural
    // k-mer value (sk), their Float64 values (sv) and, integer form, their S (sS); sp_off / sp_log2: its open-addressed device table
    bool sparse = false;
    std::vector<uint32_t> sk;
    std::vector<double> sv;
    std::vector<int64_t> sS;
    size_t sp_off = 0;
    int sp_log2 = 0;
    size_t sp_find(uint64_t x) const
    {
        const auto it = std::lower_bound(sk.begin(), sk.end(), (uint32_t)x);
        return it != sk.end() && *it == (uint32_t)x ? (size_t)(it - sk.begin()) : SIZE_MAX;
    }
    double ref_at(uint64_t x) const
    {
        if (!sparse) return ref[(size_t)x];
        const size_t i = sp_find(x);
        return i == SIZE_MAX ? 0.0 : sv[i];
    }
    int64_t S_at(uint64_t x) const
    {
        if (!sparse) return S[(size_t)x];
        const size_t i = sp_find(x);
        return i == SIZE_MAX ? 0 : sS[i];
    }
    // the KFV for the host chain (kgma_chain.h): the dense table, or the sparse one
    void chain_ref(ChainJob &J) const
    {
        if (sparse) { J.ref = nullptr; J.sp_keys = sk.data(); J.sp_vals = sv.data(); J.sp_n = (int64_t)sk.size(); }
        else { J.ref = ref.data(); J.sp_keys = nullptr; J.sp_vals = nullptr; J.sp_n = 0; }
    }
};

// dwords of one wave slot's count table in global memory (cmode 1: 4^k 16-bit counters; 4: the wide hash table, 16 bytes per entry)
inline int64_t generic_ctab_dwords(const GenParams &gg) { return gg.cmode == 4 ? (int64_t)4 << gg.hash_log2m : ((int64_t)1 << (2 * gg.k)) / 2; }

struct Group {
    int64_t W;
    std::vector<int> kfvs;    // 0-based KFV indices
};

}  // namespace

// kgma_step_begin / kgma_step_end: one findGenes step run by a helper thread of the context, so that the
// caller's thread can queue other work (the hit exchange of the previous step) while the GPU scans.
struct StepWorker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    bool sleeping = false;
    std::atomic<int> state{0};      // 0 idle, 1 job posted, 2 done, -1 quit
    kgma_genome *g = nullptr;
    int32_t mode = 0;
    int64_t buff = 0, genome_pos0 = 0;
    uint32_t flags = 0;
    int rc = 0;
};

// One set of the device chain's output buffers (chunk records, pool of raw increments in units of 16 bytes, first-window D per
// stream) with the pinned mirror they come down into.  Two sets alternate: batch i comes down (copy stream) and is walked by
// the host while batch i + 1 runs
struct ChainBufferSet {
    ChainChunk *chunks = nullptr; int64_t chunks_cap = 0;
    ChainChunk *pool = nullptr; int64_t pool_cap = 0;
    int64_t *D0 = nullptr; int64_t D0_cap = 0;
    uint8_t *pin = nullptr; size_t pin_cap = 0;
};

struct kgma_ctx {
    StepWorker *worker = nullptr;
    int device = 0;
    int n_cus = 256;                                     // hipDeviceAttributeMultiprocessorCount (CPX / partitioned modes expose fewer)
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;
    uint8_t *h_pin = nullptr; size_t h_pin_cap = 0;     // pinned mirror of the result block, written by export_kernel
    uint8_t *h_pin_dev = nullptr;                        // the same memory as the device addresses it
    unsigned int *d_done = nullptr;                      // export_kernel's workgroup ticket
    bool counters_clean = false;                         // export_kernel left the block's counters and the ticket at zero
    int reserved_cus = 0;                                // CUs the stream kernel leaves free (kgma_set_reserved_cus)
    // pack / scan overlap of a step (launch_overlapped): a stream masked to `ov_cus` CUs for the pack launches, two streams masked to
    // the other CUs for the scan launches, events around every launch
    static constexpr int OV_MAX_GROUPS = 16;
    hipStream_t ov_pack = nullptr, ov_scan[2] = {nullptr, nullptr};
    hipEvent_t ov_begin = nullptr, ov_p0[OV_MAX_GROUPS] = {}, ov_p1[OV_MAX_GROUPS] = {}, ov_s0[OV_MAX_GROUPS] = {}, ov_s1[OV_MAX_GROUPS] = {};
    int ov_cus = 0;                                      // 0: not set up; -1: not available on this device / runtime
    int ov_groups = 0;                                   // groups of the overlapped launch whose events the next synchronisation reads
    char kernel_name[48] = "";
    uint8_t *d_gath = nullptr, *h_gath = nullptr; size_t gath_cap = 0;   // tie-replay residue gather: [desc | residues]
    uint32_t *h_chain = nullptr; size_t chain_cap = 0;                   // chain replay: pinned copy of the records' 2-bit codes (dwords)
    GenomeStore genome;                                                  // what building and packing genomes keeps
    // chain on the device (stream8_kernel<..., CHAIN>): stream table, the two sets of output buffers, hot-chunk bits,
    // {raw cursor, status}
    TileDesc *d_ctiles = nullptr; int64_t ctiles_cap = 0;
    ChainBufferSet cset[2];
    hipStream_t chain_copy_stream = nullptr;
    int32_t *d_wstate = nullptr; int64_t wstate_cap = 0;                 // k = 7 multi-KFV launches: per-stream state (ScanArgs::wave_state)
    uint32_t *d_chot = nullptr; int64_t chot_cap = 0;                    // [hot bit words | prefix per word]
    uint64_t *d_chmask = nullptr; int64_t chmask_cap = 0;                // hot steps of each hot chunk
    double cpool_per_step = 0;                                           // pool units per step the last chain launches needed beyond their hot steps
    unsigned int *d_cctl = nullptr;
    // key of the tile table currently on the device
    uint64_t tk_uid = 0, tk_version = 0; int tk_mode = -1, tk_k = 0; int64_t tk_maxws = 0;
    // references
    int k = 0, m = 0;
    // strobemer references (kgma_set_strobe_ref): k = w_max + s - 1, one KFV of 4^(2s) bins whose S / ref tables are in natural bin order
    bool strobe = false;
    int st_s = 0, st_wmin = 0, st_wmax = 0;
    int64_t st_q = 0;
    // The guard band around thr is 2^-band_log2 (relative): windows that close count as "at threshold", the chain replay samples
    // them, and a chain that has drifted more than half of it from the exact distances (2^-(band_log2 + 1) of max(distance, thr))
    // makes kgma_scan repeat the scan with a band wide enough for the drift it measured.  30 unless KGMA_BAND_LOG2 says otherwise
    // at kgma_create (tests: a narrow band forces the repeat on small inputs).
    int band_log2 = 30, band_log2_default = 30;
    std::vector<KfvInfo> kfv;
    int32_t *d_Stab = nullptr;        // m x 4^k, device index order (first base least significant)
    std::map<std::vector<int>, int16_t *> sinter;   // k = 7 stream kernel: interleaved int16 S tables per launch group (device)
    int32_t *d_StabC = nullptr;       // the same tables in the stream kernel's index order ((hi bits << k) | lo bits)
    double *d_Rtab = nullptr;         // m x 4^k Float64, device index order: the KFVs as given (only when one of them is not S/N)
    uint8_t *d_sparse = nullptr;      // k >= 11: the KFVs' open-addressed tables of non-zero entries (KfvInfo::sp_off: keys, S, Float64)
    uint32_t *d_gctab = nullptr; int64_t gctab_cap = 0;   // generic kernel at k >= 8: count tables of its wave slots (dwords)
    int64_t *d_Wtab = nullptr;        // window size per KFV (export_kernel's tie gather)
    int16_t *d_diff = nullptr; int64_t diff_cap = 0;   // two-kernel cluster path: per-window self-match differences of a tile chunk
    // scan scratch
    TileDesc *d_tiles = nullptr; int64_t tiles_cap = 0;
    // one device block: [counters KGMA_RES_HDR B: rec_count u32 @0, aux_used u32 @4, n_att u64 @8, n_cold u64 @16]
    // [D0: res_d0_slots int64][aux][records]
    uint8_t *d_res = nullptr; int64_t res_bytes = 0;
    int64_t res_d0_slots = 0; unsigned int rec_cap = 0;
    std::vector<double *> d_dist;     // per KFV
    std::vector<int64_t> dist_cap;
    // results of the last scan
    int last_mode = -1;
    std::vector<TileDesc> tiles;
    std::vector<int64_t> contig_tile_base;   // per contig: index of its first tile or -1
    // Distance-bound prefilter (kgma_filter.hip; filter_candidate_table): the candidate stream table of the last scan beside the
    // regular one above, which stays cached -- the fallback, the filter kernel itself and the chain path use it
    bool scan_filtered = false;              // the last scan ran over ftiles: stitch_dips and the first-window D read that table
    std::vector<TileDesc> ftiles;            // sorted by (record, first window)
    std::vector<int64_t> fcontig_tile_base;  // per contig: index of its first candidate stream or -1
    TileDesc *d_ftiles = nullptr; int64_t ftiles_cap = 0;
    unsigned int *d_fctl = nullptr;          // entries the filter kernel appended (left at zero by its publish kernel)
    // the step's pack that makes the test itself (plan_deferred_pack): the bound and capacity it was launched with, and what
    // kgma_get_pack_test_stats reports of the last step
    uint32_t ptest_U = 0; int64_t ptest_cap = 0;
    kgma_pack_test_stats ptest = {};
    uint8_t *h_fpin = nullptr, *h_fpin_dev = nullptr; size_t fpin_cap = 0;   // pinned: [count u32, pad][FilterEntry list]: the kernel writes it directly
    hipEvent_t evf0 = nullptr, evf1 = nullptr;
    std::vector<FilterEntry> fentries;       // the last scan's entries, sorted (kgma_get_filter_candidates)
    std::vector<int64_t> fnwin;              // ... and the records' window counts then (the granules past a record's end are never set)
    kgma_filter_stats fstats{};
    uint64_t refs_version = 0;
    struct FilterMemo { uint64_t uid = 0, refs = 0; int64_t T = 0, T_hi = 0; bool valid = false; } fmemo;   // the last fallback
    std::vector<int64_t> contig_nwin;        // evaluated windows per contig (0 = skipped)
    std::vector<int64_t> contig_looked;      // last residue the reference looks up (-1: BoundsError)
    int64_t tk_bases = 0, tk_windows = 0;
    std::vector<int64_t> D0;                 // [m][n_tiles] (slot = kfv index)
    std::vector<int64_t> firstD;             // [m][records]: D of every record's first window (-1: record skipped)
    std::vector<kgma_dip> dips;
    std::vector<int64_t> dip_argl;           // last window attaining the minimum (parallel to dips)
    std::vector<int64_t> dip_aux;            // byte offset of the dip's tied-stretch residues in the aux copy, or -1
    // Float64 chain replay (KGMA_F_CHAIN_REPLAY, kgma_chain.cpp)
    struct AttWin { int32_t contig, kfv; int64_t pos; };   // kfv 0-based
    std::vector<AttWin> att;                 // tested windows inside the threshold guard band, sorted by (record, KFV, window)
    std::vector<uint8_t> chain_pair;         // [m][records]: this (record, KFV) was decided by the chain replay
    std::vector<double> firstF;              // [m][records]: chain value of the first window (chain pairs only)
    std::vector<double> dip_fmin, dip_fexit; // parallel to dips: chain values of the minimum / the exit window (chain pairs only)
    const uint8_t *aux_host = nullptr;       // aux region of the last scan (pinned staging)
    unsigned int aux_used = 0;
    std::vector<kgma_hit> hits;
    kgma_fetch_fn fetch = nullptr; void *fetch_user = nullptr;   // residue source for kgma_replay_dips (dips found on other GPUs)
    kgma_chain_fn chain_src = nullptr; void *chain_user = nullptr;   // chain-value source for kgma_replay_dips (the residues are on other GPUs)
    std::vector<AttWin> att_next;            // guard-band windows handed over for the next kgma_replay_dips (kgma_set_att)
    // kgma_chain_export: one pair's chain material, kept for kgma_chain_export_copy
    std::vector<ChainStream> cx_streams; std::vector<ChainChunk> cx_chunks, cx_pool; double cx_first = 0;
    std::vector<kgma_alignment> aligns;      // alignments the hit state machine consumed (kgma_scan_aligned), in order
    int64_t n_align_device = 0, n_align_host = 0;
    ExactState exact;                        // exact search (kgma_exact.cpp)
    MotifState motif;                        // IUPAC motif search with mismatches (kgma_motif.cpp)
    ApproxState approx;                      // edit-distance search (kgma_approx_match; kgma_approx.cpp)
    PwmState pwm;                            // position-weight-matrix search (kgma_pwm_match; kgma_pwm.cpp)
    CodonState codon;                        // codon-weight-matrix search (kgma_codon_match; kgma_codon.cpp)
    // calibration (kgma_window_dists / kgma_mutation_dists; kgma_calib.hip): device buffers kept between calls.  d_cbtab is the
    // k >= 8 kernels' counter table, zeroed when allocated and left all-zero by every launch
    int64_t *d_cboff = nullptr; int64_t cboff_cap = 0;
    int64_t *d_cbD = nullptr; int64_t cbD_cap = 0;
    double *d_cbdist = nullptr; int64_t cbdist_cap = 0;
    uint32_t *d_cbtab = nullptr; int64_t cbtab_cap = 0;
    uint8_t *d_cbtext = nullptr; int64_t cbtext_cap = 0;
    uint64_t *d_cbP = nullptr; int64_t cbP_cap = 0;
    unsigned long long *d_cbbad = nullptr; int64_t cbbad_cap = 0;
    std::vector<int64_t> contig_len;
    int64_t n_dists_per_kfv = 0;
    int64_t tile_windows = KGMA_TILE_WINDOWS;
    bool have_dists = false;
    kgma_stats stats{};
    kgma_assign_stats assign_stats{};        // the last kgma_assign_seqs / kgma_assign_ranges (kgma_assign.cpp)
    kgma_kmat_stats kmat_stats{};            // the last kgma_kmer_dist_matrix / kgma_kmer_nearest (kgma_kmat.cpp)
    kgma_landscape_stats landscape_stats{};  // the last kgma_dist_bins / kgma_dist_sweep (kgma_landscape.cpp)
    kgma_spectrum_stats spectrum_stats{};    // the last kgma_genome_kmer_count (kgma_spectrum.cpp)
    int64_t device_bytes = 0;
};

// kgma_search.h, kgma_assign.h: the view the other host files have of the two structs above
namespace kgma {
int ctx_fail(kgma_ctx *ctx, int code, const char *message)
{
    if (ctx) ctx->err = message;
    return code;
}
void ctx_device(const kgma_ctx *ctx, int *device, hipStream_t *stream) { *device = ctx->device; *stream = ctx->stream; }
void ctx_events(const kgma_ctx *ctx, hipEvent_t *ev0, hipEvent_t *ev1) { *ev0 = ctx->ev0; *ev1 = ctx->ev1; }
kgma_stats *ctx_stats(kgma_ctx *ctx) { return &ctx->stats; }
int64_t *ctx_device_bytes(kgma_ctx *ctx) { return &ctx->device_bytes; }
int ctx_n_cus(const kgma_ctx *ctx) { return ctx->n_cus; }
kgma_assign_stats *ctx_assign_stats(kgma_ctx *ctx) { return &ctx->assign_stats; }
kgma_kmat_stats *ctx_kmat_stats(kgma_ctx *ctx) { return &ctx->kmat_stats; }
kgma_spectrum_stats *ctx_spectrum_stats(kgma_ctx *ctx) { return &ctx->spectrum_stats; }
void ctx_set_kernel_name(kgma_ctx *ctx, const char *name) { snprintf(ctx->kernel_name, sizeof ctx->kernel_name, "%s", name); }
GenomeText genome_text(const kgma_genome *g) { return GenomeText{g->d_ascii, g->d_cd, g->cd.data(), g->n_contigs, g->d_planes, g->d_inter}; }

// kgma_landscape.h: the kept distances of the last scan as kgma_landscape.cpp sees them
kgma_landscape_stats *ctx_landscape_stats(kgma_ctx *ctx) { return &ctx->landscape_stats; }
int ctx_dist_view(kgma_ctx *ctx, const char *fn, int32_t kfv, bool need_dists, DistView *view)
{
    char buf[256];
    if (ctx->strobe) {
        snprintf(buf, sizeof buf, "%s is not served for strobemer references (kgma_set_strobe_ref)", fn);
        return ctx_fail(ctx, KGMA_E_UNSUPPORTED, buf);
    }
    if (ctx->last_mode < 0) return ctx_fail(ctx, KGMA_E_STATE, need_dists ? "the last scan did not keep distances (KGMA_F_RETURN_DISTS)" : "no scan has been run");
    view->nwin = &ctx->contig_nwin;
    if (!need_dists) return KGMA_OK;
    if (!ctx->have_dists) return ctx_fail(ctx, KGMA_E_STATE, "the last scan did not keep distances (KGMA_F_RETURN_DISTS)");
    const int m_used = ctx->last_mode == KGMA_MODE_SINGLE ? 1 : ctx->m;
    if (kfv < 1 || kfv > m_used) {
        snprintf(buf, sizeof buf, "%s: kfv %d out of range", fn, kfv);
        return ctx_fail(ctx, KGMA_E_ARG, buf);
    }
    view->d_dist = ctx->d_dist[(size_t)(kfv - 1)];
    view->n = ctx->n_dists_per_kfv;
    return KGMA_OK;
}
}  // namespace kgma

namespace {

int fail(kgma_ctx *ctx, int code, const char *fmt, ...)
{
    if (ctx) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        ctx->err = buf;
    }
    return code;
}

#define HIP_TRY(ctx, expr)                                                                              \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess)                                                                          \
            return fail((ctx), KGMA_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e__)); \
    } while (0)

// Grow a pinned host buffer to `need` elements and `spare` more; false: no memory (the buffer is gone)
template <class T>
bool grow_pinned(T *&buf, size_t &cap, size_t need, size_t spare)
{
    if (need <= cap) return true;
    if (buf) (void)hipHostFree(buf);
    buf = nullptr; cap = 0;
    if (hipHostMalloc(reinterpret_cast<void **>(&buf), (need + spare) * sizeof(T), hipHostMallocDefault) != hipSuccess) return false;
    cap = need + spare;
    return true;
}

// natural k-mer value (first base most significant, 2 bits per base, Kmers.jl:37-43) -> index order
// used on the device: the same 2-bit codes with the FIRST base least significant (the order in
// which the 2-bit interleaved genome stream presents a k-mer).
uint32_t device_index_of(uint32_t v, int k)
{
    uint32_t idx = 0;
    for (int j = 0; j < k; j++) {
        const uint32_t code = (v >> (2 * (k - 1 - j))) & 3u;
        idx |= code << (2 * j);
    }
    return idx;
}

// Index of natural k-mer value v in the stream kernel's tables: bit i of the low half is the low code
// bit of base i (first base = bit 0), bit k+i the high code bit.
uint32_t stream_index_of(uint32_t v, int k)
{
    uint32_t H = 0, L = 0;
    for (int j = 0; j < k; j++) {
        const uint32_t code = (v >> (2 * (k - 1 - j))) & 3u;
        H |= (code >> 1) << j;
        L |= (code & 1u) << j;
    }
    return (H << k) | L;
}

// The scan is latency-critical (a chr22-size step is ~0.3 ms): poll the stream instead of sleeping in
// hipStreamSynchronize (interrupt wake-up costs 10-20 us per synchronisation).  The poll is bounded: after
// 2 ms of spinning the thread yields between polls (a long scan does not burn a core), and after
// KGMA_SYNC_TIMEOUT_S seconds (default 600) it gives up with hipErrorLaunchTimeOut -- the caller gets
// KGMA_E_HIP, the stream is left as it is for kgma_destroy, nothing is re-executed.
double sync_timeout_ms()
{
    static const double v = [] {
        const char *e = getenv("KGMA_SYNC_TIMEOUT_S");
        const double s = e ? atof(e) : 600.0;
        return (s > 0 ? s : 600.0) * 1e3;
    }();
    return v;
}

hipError_t sync_spin(hipStream_t st)
{
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    for (int it = 0;; it++) {
        const hipError_t e = hipStreamQuery(st);
        if (e != hipErrorNotReady) return e;
        if ((it & 63) != 63) continue;
        const double ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
        if (ms > sync_timeout_ms()) return hipErrorLaunchTimeOut;
        if (ms > 2.0) std::this_thread::sleep_for(std::chrono::microseconds(ms > 50.0 ? 200 : 20));
    }
}

// Integer thresholds of one KFV.  thr * 2kN^2 is formed exactly (thr is a dyadic rational); windows
// whose exact distance lies within a relative 2^-30 of thr are decided by accumulated rounding noise
// in the reference's rolling Float64 chain (GenomeMiner.jl:77), so they form a guard band:
//   T    = ceil (thr * 2kN^2 * (1 - 2^-30))   a window is below thr  <=>  D < T
//   T_hi = floor(thr * 2kN^2 * (1 + 2^-30))   T <= D <= T_hi  <=>  "at threshold" (flagged)
// For thresholds away from the distance lattice the band is empty (T_hi = T - 1) and T is exactly
// ceil(thr * 2kN^2).
void threshold_band(double thr, int k, int64_t N, int64_t *T_lo, int64_t *T_hi, int band_log2 = 30)
{
    *T_lo = 0; *T_hi = -1;
    if (!(thr > 0.0)) return;
    if (thr >= 4.0e18) { *T_lo = INT64_MAX; return; }
    int e;
    const double fr = std::frexp(thr, &e);
    const int64_t mant = (int64_t)std::ldexp(fr, 53);
    e -= 53;
    const __int128 scale = (__int128)2 * k * N * N;
    const __int128 prod = (__int128)mant * scale;
    const __int128 lo = prod - (prod >> band_log2), hi = prod + (prod >> band_log2);
    auto clamp = [](__int128 v) { return v > (__int128)INT64_MAX ? INT64_MAX : (int64_t)v; };
    if (e >= 0) {
        if (e > 60) { *T_lo = INT64_MAX; return; }
        *T_lo = clamp(lo << e);
        *T_hi = *T_lo == INT64_MAX ? -1 : clamp(hi << e);
        return;
    }
    const int sh = -e;
    if (sh >= 126) { *T_lo = 1; *T_hi = 0; return; }
    __int128 q = lo >> sh;
    if (lo - (q << sh) != 0) q += 1;
    *T_lo = clamp(q);
    *T_hi = *T_lo == INT64_MAX ? -1 : clamp(hi >> sh);
}

// Launch groups: KFVs sorted by window size; a launch takes up to KGMA_MAX_GROUP KFVs whose sizes
// span at most KGMA_MAX_DW with at most KGMA_MAX_SIZES distinct values (the match loop runs once, for
// the largest).  For the 8-bit stream kernel (s8): the KFVs of ONE window size, up to KGMA_MAX_GROUP -- or 2-4 KFVs of
// sizes W and W + 1 (the kernel keeps the table for W and derives the longer windows; int16 S tables only).
std::vector<Group> make_groups(const kgma_ctx *ctx, int mode, bool s8 = false)
{
    const char *de = getenv("KGMA_STREAM8_DERIVE");
    const bool derive_ok = s8 && !(de && atoi(de) == 0);
    // one window size: up to 8 KFVs per launch at k = 7; at k <= 6 two launches of up to 4 beat one of 5-8 (the 5-8 KFV
    // variant keeps 16 waves per CU instead of 22-24 and spills; measured, 400 Mb, 8 KFVs: 3.17 ms against 2.56 ms)
    int s8_max_same = ctx->k >= 7 ? KGMA_MAX_GROUP : 4;
    if (const char *mg = getenv("KGMA_S8_MAXGROUP")) s8_max_same = std::max(1, std::min(KGMA_MAX_GROUP, atoi(mg)));   // experiments
    std::vector<Group> gs;
    if (mode == KGMA_MODE_SINGLE) {
        gs.push_back(Group{ctx->kfv[0].W, {0}});
        return gs;
    }
    std::vector<int> order((size_t)ctx->m);
    for (int j = 0; j < ctx->m; j++) order[(size_t)j] = j;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ctx->kfv[(size_t)a].W < ctx->kfv[(size_t)b].W; });
    for (int j : order) {
        const int64_t W = ctx->kfv[(size_t)j].W;
        bool placed = false;
        if (!gs.empty()) {
            Group &g = gs.back();
            int distinct = 0;
            int64_t last = -1;
            for (int u : g.kfvs) { if (ctx->kfv[(size_t)u].W != last) { distinct++; last = ctx->kfv[(size_t)u].W; } }
            const int64_t wmin = ctx->kfv[(size_t)g.kfvs.front()].W;
            bool fits;
            if (s8) {
                bool s16 = ctx->kfv[(size_t)j].Smax <= 32767;
                for (int u : g.kfvs) s16 = s16 && ctx->kfv[(size_t)u].Smax <= 32767;
                // (longer windows, and KFVs whose prefix leaves int32: the 16-bit counter form with 64-bit carries, one size per launch;
                //  a launch holds KFVs of one form)
                const bool c8 = W - ctx->k + 1 <= 383 && ctx->kfv[(size_t)j].fits32;
                const bool c8_front = wmin - ctx->k + 1 <= 383 && ctx->kfv[(size_t)g.kfvs.front()].fits32;
                fits = c8 == c8_front &&
                       ((W == wmin && last == wmin && (int)g.kfvs.size() < std::min(s8_max_same, c8 ? KGMA_MAX_GROUP : 4) && (c8 || s16)) ||
                        (derive_ok && s16 && c8 && W <= wmin + 1 && (int)g.kfvs.size() < 4));
            } else {
                fits = (int)g.kfvs.size() < KGMA_MAX_GROUP && W - wmin <= KGMA_MAX_DW && (W == last || distinct < KGMA_MAX_SIZES);
            }
            if (fits) {
                g.kfvs.push_back(j);
                g.W = W;        // largest so far (sorted)
                placed = true;
            }
        }
        if (!placed) gs.push_back(Group{W, {j}});
    }
    // Two neighbouring launches with FIVE KFVs between them (k = 6: also SIX; k = 7: EIGHT), windows within two k-mers of each other (k <= 6: every
    // S below 256): one launch of the five- / eight-KFV variant (stream8_wide_applies; BASELINE configs[3] is {288, 288, 288, 289} +
    // {290}, configs[4] {288 x 4} + {289 x 3, 290})
    if (s8)
        for (size_t i = 0; i + 1 < gs.size(); i++) {
            Group &g0 = gs[i];
            const Group &g1 = gs[i + 1];
            const size_t total = g0.kfvs.size() + g1.kfvs.size();
            if (!(ctx->k >= 7 ? total == 8u : (total == 5u || (total == 6u && ctx->k == 6)))) continue;
            bool all32 = true;
            for (const Group *gp : {static_cast<const Group *>(&g0), &g1})
                for (int u : gp->kfvs) all32 = all32 && ctx->kfv[(size_t)u].fits32;
            if (!all32) continue;
            int64_t nmax = 0, smax = 0;
            const int64_t w0 = ctx->kfv[(size_t)g0.kfvs.front()].W;
            int n1 = 0, n2 = 0;
            for (const Group *gp : {static_cast<const Group *>(&g0), &g1})
                for (int u : gp->kfvs) {
                    nmax = std::max(nmax, ctx->kfv[(size_t)u].N); smax = std::max(smax, ctx->kfv[(size_t)u].Smax);
                    n1 += ctx->kfv[(size_t)u].W == w0 + 1 ? 1 : 0; n2 += ctx->kfv[(size_t)u].W == w0 + 2 ? 1 : 0;
                }
            const int nk0 = (int)(w0 - ctx->k + 1), nk1 = (int)(g1.W - ctx->k + 1);
            if (!stream8_wide_applies(ctx->k, nk0, nk1, (int)total, nmax, smax < 256, smax <= 32767, n1, n2)) continue;
            g0.kfvs.insert(g0.kfvs.end(), g1.kfvs.begin(), g1.kfvs.end());
            g0.W = g1.W;
            gs.erase(gs.begin() + (long)i + 1);
        }
    return gs;
}

}  // namespace

extern "C" {

int kgma_version(void) { return KGMA_VERSION_MAJOR * 1000 + KGMA_VERSION_MINOR; }

const char *kgma_status_string(int s)
{
    switch (s) {
    case KGMA_OK: return "ok";
    case KGMA_E_ARG: return "invalid argument";
    case KGMA_E_NODEVICE: return "no HIP device";
    case KGMA_E_HIP: return "HIP runtime error";
    case KGMA_E_BADBASE: return "residue outside A/C/G/T/N (KeyError in the reference)";
    case KGMA_E_BOUNDS: return "record shorter than k-1 (BoundsError in the reference)";
    case KGMA_E_UNSUPPORTED: return "unsupported parameters";
    case KGMA_E_OVERFLOW: return "device record buffer overflow";
    case KGMA_E_NOMEM: return "out of memory";
    case KGMA_E_STATE: return "invalid call sequence";
    default: return "unknown status";
    }
}

const char *kgma_last_error(const kgma_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int kgma_create(int device_ordinal, kgma_ctx **out)
{
    if (!out) return KGMA_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return KGMA_E_NODEVICE;
    if (device_ordinal < 0 || device_ordinal >= n) return KGMA_E_ARG;
    if (hipSetDevice(device_ordinal) != hipSuccess) return KGMA_E_NODEVICE;
    kgma_ctx *ctx = new (std::nothrow) kgma_ctx();
    if (!ctx) return KGMA_E_NOMEM;
    ctx->device = device_ordinal;
    if (const char *e = getenv("KGMA_BAND_LOG2")) {                   // tests: a narrower (or wider) threshold guard band
        const int b = atoi(e);
        if (b >= 10 && b <= 50) ctx->band_log2 = ctx->band_log2_default = b;
    }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_ordinal) == hipSuccess && cus > 0) ctx->n_cus = cus;
    }
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess || !ctx->genome.init()) {
        kgma_destroy(ctx);
        return KGMA_E_HIP;
    }
    *out = ctx;
    return KGMA_OK;
}

void kgma_destroy(kgma_ctx *ctx)
{
    if (!ctx) return;
    if (StepWorker *w = ctx->worker) {
        while (w->state.load(std::memory_order_acquire) == 1) std::this_thread::yield();    // a posted step runs to its end
        {
            std::lock_guard<std::mutex> lk(w->mu);
            w->state.store(-1, std::memory_order_release);
        }
        w->cv.notify_all();
        w->th.join();
        delete w;
        ctx->worker = nullptr;
    }
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (double *p : ctx->d_dist) if (p) (void)hipFree(p);
    if (ctx->d_Stab) (void)hipFree(ctx->d_Stab);
    if (ctx->d_StabC) (void)hipFree(ctx->d_StabC);
    if (ctx->d_Rtab) (void)hipFree(ctx->d_Rtab);
    if (ctx->d_sparse) (void)hipFree(ctx->d_sparse);
    if (ctx->d_gctab) (void)hipFree(ctx->d_gctab);
    for (auto &kv2 : ctx->sinter) (void)hipFree(kv2.second);
    if (ctx->d_Wtab) (void)hipFree(ctx->d_Wtab);
    if (ctx->d_diff) (void)hipFree(ctx->d_diff);
    if (ctx->d_tiles) (void)hipFree(ctx->d_tiles);
    if (ctx->d_ftiles) (void)hipFree(ctx->d_ftiles);
    if (ctx->d_fctl) (void)hipFree(ctx->d_fctl);
    if (ctx->h_fpin) (void)hipHostFree(ctx->h_fpin);
    if (ctx->evf0) (void)hipEventDestroy(ctx->evf0);
    if (ctx->evf1) (void)hipEventDestroy(ctx->evf1);
    if (ctx->d_res) (void)hipFree(ctx->d_res);
    if (ctx->h_pin) (void)hipHostFree(ctx->h_pin);
    if (ctx->d_done) (void)hipFree(ctx->d_done);
    if (ctx->ov_pack) (void)hipStreamDestroy(ctx->ov_pack);
    for (hipStream_t st : ctx->ov_scan) if (st) (void)hipStreamDestroy(st);
    if (ctx->ov_begin) (void)hipEventDestroy(ctx->ov_begin);
    for (int i = 0; i < kgma_ctx::OV_MAX_GROUPS; i++)
        for (hipEvent_t e : {ctx->ov_p0[i], ctx->ov_p1[i], ctx->ov_s0[i], ctx->ov_s1[i]}) if (e) (void)hipEventDestroy(e);
    if (ctx->h_gath) (void)hipHostFree(ctx->h_gath);
    if (ctx->h_chain) (void)hipHostFree(ctx->h_chain);
    ctx->genome.release();
    if (ctx->d_ctiles) (void)hipFree(ctx->d_ctiles);
    for (ChainBufferSet &cs : ctx->cset) {
        for (void *d : {(void *)cs.chunks, (void *)cs.pool, (void *)cs.D0}) if (d) (void)hipFree(d);
        if (cs.pin) (void)hipHostFree(cs.pin);
    }
    if (ctx->chain_copy_stream) (void)hipStreamDestroy(ctx->chain_copy_stream);
    if (ctx->d_wstate) (void)hipFree(ctx->d_wstate);
    if (ctx->d_chmask) (void)hipFree(ctx->d_chmask);
    if (ctx->d_chot) (void)hipFree(ctx->d_chot);
    if (ctx->d_cctl) (void)hipFree(ctx->d_cctl);
    if (ctx->d_gath) (void)hipFree(ctx->d_gath);
    ctx->exact.release();
    ctx->motif.release();
    ctx->approx.release();
    ctx->pwm.release();
    ctx->codon.release();
    for (void *q : {(void *)ctx->d_cboff, (void *)ctx->d_cbD, (void *)ctx->d_cbdist, (void *)ctx->d_cbtab, (void *)ctx->d_cbtext,
                    (void *)ctx->d_cbP, (void *)ctx->d_cbbad})
        if (q) (void)hipFree(q);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

// Batched device re-alignment of hits (single engine): see kgma_align.hip
int kgma_align_hits_device(kgma_ctx *ctx, const kgma_genome *g, const uint8_t *consensus, int64_t m, int32_t gap_open_score,
                           int32_t gap_extend_score, int64_t n_hits, const int32_t *contig, const int64_t *lo, const int64_t *hi,
                           int64_t *first_out, int64_t *last_out, int64_t *score_out)
{
    if (!ctx || !g) return KGMA_E_ARG;
    if (n_hits < 0 || !consensus || (n_hits > 0 && (!contig || !lo || !hi || !first_out || !last_out)))
        return fail(ctx, KGMA_E_ARG, "null argument");
    if (m < 1 || m > KGMA_ALIGN_MAX_CONSENSUS) return fail(ctx, KGMA_E_UNSUPPORTED, "consensus of %lld residues", (long long)m);
    if (n_hits == 0) return KGMA_OK;
    (void)hipSetDevice(ctx->device);
    std::vector<AlignJob> jobs((size_t)n_hits);
    int max_n = 1;
    for (int64_t i = 0; i < n_hits; i++) {
        if (contig[i] < 0 || contig[i] >= g->n_contigs) return fail(ctx, KGMA_E_ARG, "hit %lld: record %d out of range", (long long)i, contig[i]);
        const ContigDesc &d = g->cd[(size_t)contig[i]];
        const int64_t n = hi[i] - lo[i] + 1;
        if (lo[i] < 1 || hi[i] > d.len || n < 1) return fail(ctx, KGMA_E_ARG, "hit %lld: range %lld:%lld outside the record", (long long)i, (long long)lo[i], (long long)hi[i]);
        if (n > KGMA_ALIGN_MAX_SEGMENT) return fail(ctx, KGMA_E_UNSUPPORTED, "hit %lld: segment of %lld residues (max %d)", (long long)i, (long long)n, KGMA_ALIGN_MAX_SEGMENT);
        jobs[(size_t)i].ascii_off = d.ascii_off + (lo[i] - 1);
        jobs[(size_t)i].n = (int32_t)n;
        jobs[(size_t)i].pad = 0;
        max_n = std::max(max_n, (int)n);
    }
    const int64_t stride = (align_trace_bytes((int)m, max_n) + 255) & ~(int64_t)255;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n_hits, ((int64_t)1 << 30) / stride));
    AlignJob *d_jobs = nullptr;
    uint8_t *d_cons = nullptr, *d_trace = nullptr;
    int64_t *d_out = nullptr;
    std::vector<int64_t> out((size_t)n_hits * 4);
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_jobs), (size_t)n_hits * sizeof(AlignJob));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_cons), (size_t)m);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_out), (size_t)n_hits * 4 * sizeof(int64_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_trace), (size_t)(chunk * stride));
    if (e == hipSuccess) e = hipMemcpyAsync(d_jobs, jobs.data(), (size_t)n_hits * sizeof(AlignJob), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_cons, consensus, (size_t)m, hipMemcpyHostToDevice, ctx->stream);
    for (int64_t b = 0; b < n_hits && e == hipSuccess; b += chunk) {
        const int nb = (int)std::min<int64_t>(chunk, n_hits - b);
        e = launch_align(g->d_ascii, d_jobs + b, nb, d_cons, (int)m, -gap_open_score, -gap_extend_score, d_trace, stride, max_n,
                         d_out + 4 * b, ctx->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out.data(), d_out, (size_t)n_hits * 4 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (d_jobs) (void)hipFree(d_jobs);
    if (d_cons) (void)hipFree(d_cons);
    if (d_out) (void)hipFree(d_out);
    if (d_trace) (void)hipFree(d_trace);
    if (e != hipSuccess) return fail(ctx, KGMA_E_HIP, "device alignment failed: %s", hipGetErrorString(e));
    for (int64_t i = 0; i < n_hits; i++) {
        first_out[i] = out[(size_t)i * 4];
        last_out[i] = out[(size_t)i * 4 + 1];
        if (score_out) score_out[i] = out[(size_t)i * 4 + 2];
    }
    return KGMA_OK;
}

// kmer_count (mode 1) / kmer_dist against one KFV (mode 0) of n sequences: src/Kmers.jl:14-28,58-60.
static int kmer_batch(kgma_ctx *ctx, int mode, int32_t k, const double *kfv, const uint8_t *seqs, const int64_t *offsets,
                      int64_t n, double *out)
{
    if (!ctx) return KGMA_E_ARG;
    if (n < 0 || !offsets || !out || (mode == 0 && !kfv)) return fail(ctx, KGMA_E_ARG, "null argument");
    if (k < 1 || k > 10) return fail(ctx, KGMA_E_UNSUPPORTED, "k = %d: the device path supports 1 <= k <= 10 here", k);
    for (int64_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return fail(ctx, KGMA_E_ARG, "offsets[%lld] > offsets[%lld]", (long long)i, (long long)(i + 1));
    if (n == 0) return KGMA_OK;
    const int64_t base = offsets[0], bytes = offsets[n] - base;
    if (bytes > 0 && !seqs) return fail(ctx, KGMA_E_ARG, "null argument");
    const int64_t nb = (int64_t)1 << (2 * k);
    const int64_t out_n = mode == 0 ? n : n * nb;
    if (out_n > ((int64_t)1 << 30)) return fail(ctx, KGMA_E_UNSUPPORTED, "%lld sequences x 4^%d bins in one call", (long long)n, k);
    (void)hipSetDevice(ctx->device);
    std::vector<int64_t> off((size_t)n + 1);
    for (int64_t i = 0; i <= n; i++) off[(size_t)i] = offsets[i] - base;
    uint8_t *d_seq = nullptr;
    int64_t *d_off = nullptr;
    double *d_ref = nullptr, *d_out = nullptr;
    uint32_t *d_scr = nullptr;
    unsigned long long *d_bad = nullptr, bad = NO_BAD;
    const size_t scr_bytes = k > 7 ? (size_t)kdist_grid(k, n) * (size_t)nb * 4 : 0;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_seq), (size_t)std::max<int64_t>(bytes, 1));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_off), (size_t)(n + 1) * 8);
    if (e == hipSuccess && mode == 0) e = hipMalloc(reinterpret_cast<void **>(&d_ref), (size_t)nb * 8);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_out), (size_t)out_n * 8);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_bad), 8);
    if (e == hipSuccess && scr_bytes) e = hipMalloc(reinterpret_cast<void **>(&d_scr), scr_bytes);
    if (e == hipSuccess && scr_bytes) e = hipMemsetAsync(d_scr, 0, scr_bytes, ctx->stream);
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(d_seq, seqs + base, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off, off.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && mode == 0) e = hipMemcpyAsync(d_ref, kfv, (size_t)nb * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_bad, &bad, 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = launch_kdist(mode, d_seq, d_off, n, k, d_ref, d_scr, 1.0 / (2 * k), d_out, d_bad, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (size_t)out_n * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    for (void *q : {(void *)d_seq, (void *)d_off, (void *)d_ref, (void *)d_out, (void *)d_bad, (void *)d_scr})
        if (q) (void)hipFree(q);
    if (e != hipSuccess) return fail(ctx, KGMA_E_HIP, "kmer batch failed: %s", hipGetErrorString(e));
    if (bad != NO_BAD) {
        const int64_t si = (int64_t)(std::upper_bound(off.begin(), off.end(), (int64_t)bad) - off.begin()) - 1;
        return fail(ctx, KGMA_E_BADBASE, "sequence %lld position %lld: residue is not one of A/C/G/T/N (KeyError, Consts.jl:22-28)",
                    (long long)si, (long long)((int64_t)bad - off[(size_t)si] + 1));
    }
    return KGMA_OK;
}

int kgma_kmer_dist_batch(kgma_ctx *ctx, int32_t k, const double *kfv, const uint8_t *seqs, const int64_t *offsets, int64_t n,
                         double *out)
{
    return kmer_batch(ctx, 0, k, kfv, seqs, offsets, n, out);
}

int kgma_kmer_count_batch(kgma_ctx *ctx, int32_t k, const uint8_t *seqs, const int64_t *offsets, int64_t n, double *bins)
{
    return kmer_batch(ctx, 1, k, nullptr, seqs, offsets, n, bins);
}

// One findGenes step in one call: re-encode the resident residues (Consts.jl:22-28), scan, replay, and
// copy the hits out (two-call pattern collapsed: `cap` hits fit or KGMA_E_ARG with *n = needed).
static bool overlap_setup(kgma_ctx *ctx);
static bool fuse_sums_possible(const kgma_ctx *ctx, int32_t mode);
static int64_t overlap_min_bases()                                   // (KGMA_OVERLAP_MIN_BASES: tests force the overlapped step on small genomes)
{
    if (const char *e = getenv("KGMA_OVERLAP_MIN_BASES")) return std::max<int64_t>(1, atoll(e));
    return 2000000000ll;
}

int kgma_repack_scan_hits(kgma_ctx *ctx, kgma_genome *g, int32_t mode, int64_t buff, int64_t genome_pos0, uint32_t flags,
                          kgma_hit *out, int64_t cap, int64_t *n)
{
    if (ctx && ctx->strobe) return fail(ctx, KGMA_E_UNSUPPORTED, "%s is not served for strobemer references (kgma_set_strobe_ref)", __func__);
    if (!ctx || !g || !n) return KGMA_E_ARG;
    // a large genome's re-encoding is left to the scan, which may run it beside its own launches (launch_overlapped)
    int rc = KGMA_OK;
    ctx->ptest = kgma_pack_test_stats{};                               // (of the last step, whatever its pack turns out to be)
    // ... or put the prefilter's block sums into it (pack_sums_kernel), which only the scan can decide
    if (mode == KGMA_MODE_SINGLE && g->n_contigs >= 4 && g->total_bases >= overlap_min_bases() && overlap_setup(ctx)) g->repack_deferred = true;
    else if (fuse_sums_possible(ctx, mode)) g->repack_deferred = true;
    else rc = kgma_genome_repack(ctx, g);
    if (rc) return rc;
    rc = kgma_scan(ctx, g, mode, buff, genome_pos0, flags, nullptr, nullptr);
    if (rc) return rc;
    return kgma_get_hits(ctx, out, cap, n);
}

// The same step in two halves.  kgma_step_begin hands (repack, scan, replay) to the context's helper thread
// and returns at once; kgma_step_end waits for it and copies the hits out like kgma_get_hits.  Between the
// two the caller must not touch the context or the genome.
static void step_worker_main(kgma_ctx *ctx)
{
    StepWorker *w = ctx->worker;
    (void)hipSetDevice(ctx->device);
    for (;;) {
        // a step follows the previous one within microseconds in a step loop: poll first, sleep after ~2 ms idle
        int st = w->state.load(std::memory_order_acquire);
        const double t0 = now_ms();
        while (st != 1 && st != -1) {
            if (now_ms() - t0 > 2.0) {
                std::unique_lock<std::mutex> lk(w->mu);
                w->sleeping = true;
                w->cv.wait(lk, [&] { const int s = w->state.load(std::memory_order_acquire); return s == 1 || s == -1; });
                w->sleeping = false;
            }
            st = w->state.load(std::memory_order_acquire);
        }
        if (st == -1) return;
        int rc = KGMA_OK;
        ctx->ptest = kgma_pack_test_stats{};
        if (w->mode == KGMA_MODE_SINGLE && w->g->n_contigs >= 4 && w->g->total_bases >= overlap_min_bases() && overlap_setup(ctx)) w->g->repack_deferred = true;
        else if (fuse_sums_possible(ctx, w->mode)) w->g->repack_deferred = true;
        else rc = kgma_genome_repack(ctx, w->g);
        if (!rc) rc = kgma_scan(ctx, w->g, w->mode, w->buff, w->genome_pos0, w->flags, nullptr, nullptr);
        w->rc = rc;
        w->state.store(2, std::memory_order_release);
    }
}

int kgma_step_begin(kgma_ctx *ctx, kgma_genome *g, int32_t mode, int64_t buff, int64_t genome_pos0, uint32_t flags)
{
    if (ctx && ctx->strobe) return fail(ctx, KGMA_E_UNSUPPORTED, "%s is not served for strobemer references (kgma_set_strobe_ref)", __func__);
    if (!ctx || !g) return KGMA_E_ARG;
    if (!ctx->worker) {
        ctx->worker = new StepWorker();
        ctx->worker->th = std::thread(step_worker_main, ctx);
    }
    StepWorker *w = ctx->worker;
    if (w->state.load(std::memory_order_acquire) != 0) return fail(ctx, KGMA_E_STATE, "kgma_step_begin: a step is already in flight");
    w->g = g; w->mode = mode; w->buff = buff; w->genome_pos0 = genome_pos0; w->flags = flags;
    bool wake;
    {
        std::lock_guard<std::mutex> lk(w->mu);
        w->state.store(1, std::memory_order_release);
        wake = w->sleeping;
    }
    if (wake) w->cv.notify_one();
    return KGMA_OK;
}

int kgma_step_end(kgma_ctx *ctx, kgma_hit *out, int64_t cap, int64_t *n)
{
    if (ctx && ctx->strobe) return fail(ctx, KGMA_E_UNSUPPORTED, "%s is not served for strobemer references (kgma_set_strobe_ref)", __func__);
    if (!ctx || !n) return KGMA_E_ARG;
    StepWorker *w = ctx->worker;
    if (!w || w->state.load(std::memory_order_acquire) == 0) return fail(ctx, KGMA_E_STATE, "kgma_step_end without kgma_step_begin");
    {   // the caller would otherwise poll the stream itself; after 2 ms the poll yields between looks
        const double t0 = now_ms();
        for (int it = 0; w->state.load(std::memory_order_acquire) != 2; it++)
            if ((it & 255) == 255 && now_ms() - t0 > 2.0) std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    const int rc = w->rc;
    w->state.store(0, std::memory_order_release);
    if (rc) return rc;
    return kgma_get_hits(ctx, out, cap, n);
}

int kgma_set_reserved_cus(kgma_ctx *ctx, int32_t n)
{
    if (!ctx) return KGMA_E_ARG;
    if (n < 0 || n > ctx->n_cus / 2) return fail(ctx, KGMA_E_ARG, "reserved CUs must be 0..%d (half of the device's %d CUs)", ctx->n_cus / 2, ctx->n_cus);
    ctx->reserved_cus = n;
    return KGMA_OK;
}

void *kgma_stream(kgma_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

const char *kgma_scan_kernel_name(const kgma_ctx *ctx) { return ctx ? ctx->kernel_name : ""; }

int kgma_set_thresholds(kgma_ctx *ctx, const double *thr)
{
    if (!ctx) return KGMA_E_ARG;
    if (!thr) return fail(ctx, KGMA_E_ARG, "thr is NULL");
    if (ctx->m == 0) return fail(ctx, KGMA_E_STATE, "kgma_set_refs has not been called");
    for (int j = 0; j < ctx->m; j++) {
        ctx->kfv[j].thr = thr[j];
        threshold_band(thr[j], ctx->k, ctx->kfv[j].N, &ctx->kfv[j].T, &ctx->kfv[j].T_hi, ctx->band_log2);
    }
    return KGMA_OK;
}

}  // extern "C"

// the generic kernels' view of a sparse KFV (k >= 11): its device table, S values (integer form) or Float64 ones
static void set_sparse_params(const kgma_ctx *ctx, const KfvInfo &f, GenParams &gg, bool fp)
{
    const size_t P = (size_t)1 << f.sp_log2;
    gg.S = nullptr; gg.R = nullptr;
    gg.sp_keys = reinterpret_cast<const uint32_t *>(ctx->d_sparse + f.sp_off);
    gg.sp_vals = reinterpret_cast<const uint64_t *>(ctx->d_sparse + f.sp_off + (fp ? 12 : 4) * P);
    gg.sp_log2 = f.sp_log2;
}

// One KFV of kgma_set_refs / kgma_set_refs_sparse from its non-zero entries (natural k-mer values, increasing; their values): the
// window checks, the S/N inference, the Float64 form and its magnitude bound, fits32 / big_ok, ref_form, the threshold and every
// error and message -- ONE routine for both entry points, so their semantics are the same by construction.  Every test and sum runs
// over the non-zero entries only, which is exact: a zero entry passes each test (0 * N is the integer 0, S = 0 gives RN(0 * invN)
// = RN(0 / N) = 0) and adds +0.0 or 0 to each sum (sumR2 in increasing k-mer value: the dense left-to-right sum's bits).  Fills
// f.sk / f.sv and, integer form, f.sS; the dense tables are the caller's business.
static int kfv_from_nonzeros(kgma_ctx *ctx, int32_t k, int j, std::vector<uint32_t> &&kj, std::vector<double> &&nz, const int64_t *windowsizes,
                             const double *thr, const int64_t *n_refs, KfvInfo &f)
{
    f.W = windowsizes[j];
    if (k >= f.W)   // src/API.jl:70,177
        return fail(ctx, KGMA_E_ARG, "the average reference sequence length %lld exceeds/is equal to the chosen kmer length %d. please reduce k.",
                    (long long)f.W, k);
    const int64_t nk = f.W - k + 1;
    if (nk > KGMA_MAX_NK_WIDE)
        return fail(ctx, KGMA_E_UNSUPPORTED, "window size %lld: at most %d k-mers per window are supported (16-bit window counts)", (long long)f.W,
                    KGMA_MAX_NK_WIDE);
    // Is the KFV S/N with integer S (what gen_ref_ws_cons / cluster_ref_API produce: an average of integer histograms)?  Then the
    // device computes in exact integers.  Anything else -- refVec::Vector{Float64} may be any vector (src/GenomeMiner.jl:6,
    // src/OmnGenomeMiner.jl:9) -- takes the Float64 form of the generic kernel.  "Is S/N": every entry times N within 1e-14
    // (relative) of a non-negative integer, i.e. S/N up to the rounding of its own division or multiplication (a looser test
    // finds "N" for irrational vectors too: 1/sqrt(2)-weighted averages are within 5e-13 of S/665857, a convergent).
    auto is_s_over_n = [&](const int64_t cand, const double tol) {
        for (const double e : nz) {
            const double v = e * (double)cand, rv = std::nearbyint(v);
            if (!(std::fabs(v - rv) <= tol * std::max(1.0, std::fabs(v))) || rv < 0 || rv > 2.0e9) return false;
        }
        return true;
    };
    int64_t N = 0;
    bool fp = false;
    for (size_t i = 0; i < nz.size(); i++)
        if (!std::isfinite(nz[i])) return fail(ctx, KGMA_E_ARG, "KFV %d entry %lld is not finite", j + 1, (long long)kj[i]);
    if (n_refs) {
        N = n_refs[j];
        if (N < 1) return fail(ctx, KGMA_E_ARG, "n_refs[%d] = %lld", j, (long long)N);
        if (!is_s_over_n(N, 1e-14)) fp = true;
    } else {
        for (int64_t cand = 1; cand <= (1 << 20) && N == 0; cand++)
            if (is_s_over_n(cand, 1e-14)) N = cand;
        if (N == 0) fp = true;
    }
    f.sk = std::move(kj);
    f.sv = std::move(nz);
    for (const double e : f.sv) f.sumR2 += e * e;                      // (the Float64 kernels' first-window identity)
    __int128 s2 = 0;
    if (fp) {
        // Float64 form.  The host keeps every distance on an integer lattice D = round(d * 2kN^2) with N a power of two chosen so
        // that the largest possible D stays below 2^61 (resolution 1 / (2kN^2): 8e-14 at k = 6 for windows of a few hundred k-mers)
        double r2 = 0, amax = 0;
        for (const double e : f.sv) { r2 += e * e; amax = std::max(amax, std::fabs(e)); }
        const double fmax = r2 + (double)nk * (double)nk + 2.0 * (double)nk * amax + 1.0;     // >= sum (ref - c)^2 for any window
        int q = 20;
        while (q > 0 && fmax * std::ldexp(1.0, 2 * q) >= std::ldexp(1.0, 61)) q--;
        if (fmax >= std::ldexp(1.0, 61)) return fail(ctx, KGMA_E_UNSUPPORTED, "KFV %d: entries of magnitude %.3g are outside the device path's range", j + 1, amax);
        f.fp = true; f.N = (int64_t)1 << q;
        f.Smax = INT64_MAX; f.sumS2 = 0;
        f.fits32 = false; f.big_ok = false; f.ref_form = -1;
        f.thr = thr[j];
        threshold_band(thr[j], k, f.N, &f.T, &f.T_hi, ctx->band_log2);
        return KGMA_OK;
    }
    f.N = N;
    f.sS.resize(f.sv.size());
    for (size_t i = 0; i < f.sv.size(); i++) {
        const double rv = std::nearbyint(f.sv[i] * (double)N);
        f.sS[i] = (int64_t)rv;
        f.Smax = std::max(f.Smax, (int64_t)rv);
        s2 += (__int128)f.sS[i] * f.sS[i];
    }
    // What the kernels keep in 32 bits: the int32 kernels E = (D - D0)/(2N) and N * (count difference); the 16-bit counter form of
    // stream8_kernel the LOCAL prefix of a 64-window step, |e| <= Smax + N n per window (its carries are 64-bit); the generic
    // kernel nothing (int64 throughout: D itself must fit)
    // (fits32's second clause never decides: N n >= 2^30 gives dmax / 2N >= N n^2 / 2 >= 2^29 n.  big_ok's N < 2^22 decides alone
    //  only for windows of 1, 2 or 3 k-mers -- Smax + N n <= 2^24 admits N up to 2^24 / n -- and every user of big_ok asks
    //  stream8_c16_applies, which repeats it: tests/test_range_cases.py enumerates both.  The int32 kernels clamp their threshold
    //  prefix TE at +-(2^30 - 1), twice what fits32 lets E reach; tests/test_gpu_range.py holds either side of each bound.)
    const __int128 dmax = s2 + (__int128)N * N * nk * nk;
    f.fits32 = !(dmax / (2 * N) >= ((__int128)1 << 29) || (__int128)N * nk >= ((__int128)1 << 30));
    f.big_ok = (__int128)64 * ((__int128)f.Smax + (__int128)N * nk) <= ((__int128)1 << 30) && N < ((int64_t)1 << 22);
    if (dmax >= ((__int128)1 << 61))
        return fail(ctx, KGMA_E_UNSUPPORTED, "KFV %d: N = %lld with %lld k-mers per window exceeds the int64 range of the device path", j + 1,
                    (long long)N, (long long)nk);
    f.sumS2 = (int64_t)s2;
    {
        const double invN = 1.0 / (double)N, Nd = (double)N;
        bool mul = true, div = true;
        for (size_t i = 0; i < f.sv.size() && (mul || div); i++) {
            const double Sd = (double)f.sS[i], q = Sd * invN;
            mul = mul && f.sv[i] == q;
            div = div && f.sv[i] == std::fma(std::fma(-q, Nd, Sd), invN, q) && f.sv[i] == Sd / Nd;
        }
        f.ref_form = mul ? 0 : (div ? 1 : -1);
    }
    f.thr = thr[j];
    threshold_band(thr[j], k, N, &f.T, &f.T_hi, ctx->band_log2);
    return KGMA_OK;
}

// kgma_set_refs at k >= 11, from each KFV's non-zero entries: kfv_from_nonzeros, and on the device per KFV an open-addressed table of
// those entries (load <= 1/2) instead of the 4^k tables.
static int set_refs_sparse_core(kgma_ctx *ctx, int32_t k, int32_t m, std::vector<std::vector<uint32_t>> &keys,
                                std::vector<std::vector<double>> &vals, const int64_t *windowsizes, const double *thr, const int64_t *n_refs)
{
    std::vector<KfvInfo> kv((size_t)m);
    for (int j = 0; j < m; j++) {
        KfvInfo &f = kv[(size_t)j];
        const int rc = kfv_from_nonzeros(ctx, k, j, std::move(keys[(size_t)j]), std::move(vals[(size_t)j]), windowsizes, thr, n_refs, f);
        if (rc != KGMA_OK) return rc;
        f.sparse = true;
    }
    // device tables: per KFV [keys: 2^p u32 | S: 2^p int64 | Float64: 2^p], keys in the kernels' index order (kgma_device.h, GenParams)
    size_t total = 0;
    for (int j = 0; j < m; j++) {
        KfvInfo &f = kv[(size_t)j];
        int lg = 6;
        while (((size_t)1 << lg) < 2 * f.sk.size()) lg++;
        f.sp_log2 = lg;
        f.sp_off = total;
        total += ((size_t)20 << lg);
    }
    std::vector<uint8_t> host(total, 0);
    for (int j = 0; j < m; j++) {
        const KfvInfo &f = kv[(size_t)j];
        const size_t P = (size_t)1 << f.sp_log2;
        uint32_t *hk = reinterpret_cast<uint32_t *>(host.data() + f.sp_off);
        int64_t *hs = reinterpret_cast<int64_t *>(host.data() + f.sp_off + 4 * P);
        double *hr = reinterpret_cast<double *>(host.data() + f.sp_off + 12 * P);
        for (size_t i = 0; i < P; i++) hk[i] = KGMA_SP_EMPTY;
        for (size_t i = 0; i < f.sk.size(); i++) {
            const uint32_t key = device_index_of(f.sk[i], k);
            uint32_t h = (key * 2654435761u) >> (32 - f.sp_log2);
            while (hk[h] != KGMA_SP_EMPTY) h = (h + 1u) & (uint32_t)(P - 1);
            hk[h] = key;
            hs[h] = f.fp ? 0 : f.sS[i];
            hr[h] = f.sv[i];
        }
    }
    for (void *p : {(void *)ctx->d_Stab, (void *)ctx->d_StabC, (void *)ctx->d_Rtab, (void *)ctx->d_sparse, (void *)ctx->d_Wtab}) if (p) (void)hipFree(p);
    ctx->d_Stab = nullptr; ctx->d_StabC = nullptr; ctx->d_Rtab = nullptr; ctx->d_sparse = nullptr; ctx->d_Wtab = nullptr;
    for (auto &kv2 : ctx->sinter) (void)hipFree(kv2.second);
    ctx->sinter.clear();
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_sparse), total));
    HIP_TRY(ctx, hipMemcpy(ctx->d_sparse, host.data(), total, hipMemcpyHostToDevice));
    {
        std::vector<int64_t> wt((size_t)m);
        for (int j = 0; j < m; j++) wt[(size_t)j] = kv[(size_t)j].W;
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_Wtab), wt.size() * sizeof(int64_t)));
        HIP_TRY(ctx, hipMemcpy(ctx->d_Wtab, wt.data(), wt.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    ctx->k = k;
    ctx->m = m;
    ctx->strobe = false;
    ctx->kfv.swap(kv);
    ctx->refs_version++;                                              // (the prefilter remembers its fallbacks per reference set)
    for (double *p : ctx->d_dist) if (p) (void)hipFree(p);
    ctx->d_dist.assign((size_t)m, nullptr);
    ctx->dist_cap.assign((size_t)m, 0);
    ctx->last_mode = -1;
    ctx->tk_uid = 0;
    return KGMA_OK;
}

extern "C" {

int kgma_set_refs(kgma_ctx *ctx, int32_t k, int32_t m, const double *ref, const int64_t *windowsizes,
                  const double *thr, const int64_t *n_refs)
{
    if (!ctx) return KGMA_E_ARG;
    if (!ref || !windowsizes || !thr || m < 1) return fail(ctx, KGMA_E_ARG, "null argument or m < 1");
    if (k < 1 || k > KGMA_MAX_K) return fail(ctx, KGMA_E_UNSUPPORTED, "k = %d: the device path supports 1 <= k <= %d", k, KGMA_MAX_K);
    (void)hipSetDevice(ctx->device);
    const int64_t NB = (int64_t)1 << (2 * k);
    if (k >= KGMA_WIDE_MIN_K) {
        // (one pass over the caller's vectors: their non-zero entries; no 4^k copy is kept)
        std::vector<std::vector<uint32_t>> keys((size_t)m);
        std::vector<std::vector<double>> vals((size_t)m);
        for (int j = 0; j < m; j++) {
            const double *r = ref + (size_t)j * (size_t)NB;
            for (int64_t x = 0; x < NB; x++)
                if (r[x] != 0.0) { keys[(size_t)j].push_back((uint32_t)x); vals[(size_t)j].push_back(r[x]); }
        }
        return set_refs_sparse_core(ctx, k, m, keys, vals, windowsizes, thr, n_refs);
    }
    std::vector<KfvInfo> kv((size_t)m);
    for (int j = 0; j < m; j++) {
        KfvInfo &f = kv[(size_t)j];
        const double *r = ref + (size_t)j * (size_t)NB;
        // (only the non-zero entries can fail a test: a KFV at k = 10 has a million entries, nearly all of them zero)
        std::vector<uint32_t> keys;
        std::vector<double> nz;
        for (int64_t x = 0; x < NB; x++)
            if (r[x] != 0.0) { keys.push_back((uint32_t)x); nz.push_back(r[x]); }
        const int rc = kfv_from_nonzeros(ctx, k, j, std::move(keys), std::move(nz), windowsizes, thr, n_refs, f);
        if (rc != KGMA_OK) return rc;
        // k <= 10: the dense tables (natural k-mer order) the kernels' uploads below and the host replays read
        f.ref.assign(r, r + NB);
        if (!f.fp) {
            f.S.assign((size_t)NB, 0);
            for (size_t i = 0; i < f.sk.size(); i++) f.S[f.sk[i]] = f.sS[i];
        }
        f.sk.clear(); f.sv.clear(); f.sS.clear();
        f.sk.shrink_to_fit(); f.sv.shrink_to_fit(); f.sS.shrink_to_fit();
    }
    // upload the plane-index permuted tables
    std::vector<int32_t> tab((size_t)m * (size_t)NB, 0);
    bool any_fp = false;
    for (int j = 0; j < m; j++) {
        any_fp = any_fp || kv[(size_t)j].fp;
        if (kv[(size_t)j].fp) continue;
        for (int64_t v = 0; v < NB; v++)
            tab[(size_t)j * (size_t)NB + device_index_of((uint32_t)v, k)] = (int32_t)kv[(size_t)j].S[(size_t)v];
    }
    if (ctx->d_Rtab) { (void)hipFree(ctx->d_Rtab); ctx->d_Rtab = nullptr; }
    if (ctx->d_sparse) { (void)hipFree(ctx->d_sparse); ctx->d_sparse = nullptr; }
    (void)any_fp;
    {
        // the KFVs as given (Float64), in the kernels' index order: what the Float64 form of the generic kernel and its chain
        // kernel read (the chain forms the reference's increments from the caller's own table)
        std::vector<double> rt((size_t)m * (size_t)NB);
        for (int j = 0; j < m; j++)
            for (int64_t v = 0; v < NB; v++)
                rt[(size_t)j * (size_t)NB + device_index_of((uint32_t)v, k)] = kv[(size_t)j].ref[(size_t)v];
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_Rtab), rt.size() * sizeof(double)));
        HIP_TRY(ctx, hipMemcpy(ctx->d_Rtab, rt.data(), rt.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (ctx->d_Stab) { (void)hipFree(ctx->d_Stab); ctx->d_Stab = nullptr; }
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_Stab), tab.size() * sizeof(int32_t)));
    HIP_TRY(ctx, hipMemcpy(ctx->d_Stab, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (ctx->d_StabC) { (void)hipFree(ctx->d_StabC); ctx->d_StabC = nullptr; }
    for (auto &kv2 : ctx->sinter) (void)hipFree(kv2.second);
    ctx->sinter.clear();
    if (k <= KGMA_STREAM_MAX_K) {
        for (int j = 0; j < m; j++) {
            if (kv[(size_t)j].fp) continue;
            for (int64_t v = 0; v < NB; v++)
                tab[(size_t)j * (size_t)NB + stream_index_of((uint32_t)v, k)] = (int32_t)kv[(size_t)j].S[(size_t)v];
        }
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_StabC), tab.size() * sizeof(int32_t)));
        HIP_TRY(ctx, hipMemcpy(ctx->d_StabC, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    {
        std::vector<int64_t> wt((size_t)m);
        for (int j = 0; j < m; j++) wt[(size_t)j] = kv[(size_t)j].W;
        if (ctx->d_Wtab) { (void)hipFree(ctx->d_Wtab); ctx->d_Wtab = nullptr; }
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_Wtab), wt.size() * sizeof(int64_t)));
        HIP_TRY(ctx, hipMemcpy(ctx->d_Wtab, wt.data(), wt.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    ctx->k = k;
    ctx->m = m;
    ctx->strobe = false;
    ctx->kfv.swap(kv);
    ctx->refs_version++;                                              // (the prefilter remembers its fallbacks per reference set)
    for (double *p : ctx->d_dist) if (p) (void)hipFree(p);
    ctx->d_dist.assign((size_t)m, nullptr);
    ctx->dist_cap.assign((size_t)m, 0);
    ctx->last_mode = -1;
    ctx->tk_uid = 0;
    return KGMA_OK;
}

// The same references as their non-zero entries: nnz[j] (keys, vals) pairs per KFV, natural k-mer values (0-based, first base most
// significant), strictly increasing.  k <= 10: the dense vectors, through kgma_set_refs.
int kgma_set_refs_sparse(kgma_ctx *ctx, int32_t k, int32_t m, const int64_t *nnz, const uint32_t *keys, const double *vals,
                         const int64_t *windowsizes, const double *thr, const int64_t *n_refs)
{
    if (!ctx) return KGMA_E_ARG;
    if (!nnz || !windowsizes || !thr || m < 1) return fail(ctx, KGMA_E_ARG, "null argument or m < 1");
    if (k < 1 || k > KGMA_MAX_K) return fail(ctx, KGMA_E_UNSUPPORTED, "k = %d: the device path supports 1 <= k <= %d", k, KGMA_MAX_K);
    const uint64_t NB = (uint64_t)1 << (2 * k);
    int64_t total = 0;
    for (int j = 0; j < m; j++) {
        if (nnz[j] < 0 || (uint64_t)nnz[j] > NB) return fail(ctx, KGMA_E_ARG, "nnz[%d] = %lld", j, (long long)nnz[j]);
        total += nnz[j];
    }
    if (total > 0 && (!keys || !vals)) return fail(ctx, KGMA_E_ARG, "null argument or m < 1");
    int64_t at = 0;
    for (int j = 0; j < m; j++)
        for (int64_t i = 0; i < nnz[j]; i++, at++)
            if ((uint64_t)keys[at] >= NB || (i > 0 && keys[at] <= keys[at - 1]))
                return fail(ctx, KGMA_E_ARG, "KFV %d: key %lld is not below 4^k or not above the one before it", j + 1, (long long)keys[at]);
    if (k < KGMA_WIDE_MIN_K) {
        std::vector<double> dense((size_t)m * (size_t)NB, 0.0);
        at = 0;
        for (int j = 0; j < m; j++)
            for (int64_t i = 0; i < nnz[j]; i++, at++) dense[(size_t)j * (size_t)NB + keys[at]] = vals[at];
        return kgma_set_refs(ctx, k, m, dense.data(), windowsizes, thr, n_refs);
    }
    (void)hipSetDevice(ctx->device);
    std::vector<std::vector<uint32_t>> kk((size_t)m);
    std::vector<std::vector<double>> vv((size_t)m);
    at = 0;
    for (int j = 0; j < m; j++)
        for (int64_t i = 0; i < nnz[j]; i++, at++)
            if (vals[at] != 0.0) { kk[(size_t)j].push_back(keys[at]); vv[(size_t)j].push_back(vals[at]); }   // (explicit zeros: absent)
    return set_refs_sparse_core(ctx, k, m, kk, vv, windowsizes, thr, n_refs);
}

// The strobemer method's reference (kgma.h): one KFV over the 4^(2s) randstrobe bins, S/N only.  kfv_from_nonzeros does the S/N
// inference, the range checks (its "k-mers per window" W - k + 1 is the window's item count here: W - k sliding strobemers plus
// the permanent one) and the threshold band; the tables stay in natural bin order, which is the order strobe_kernel forms.
int kgma_set_strobe_ref(kgma_ctx *ctx, int32_t s, int32_t w_min, int32_t w_max, int64_t q, const double *ref, int64_t windowsize,
                        double thr, int64_t n_refs)
{
    if (!ctx) return KGMA_E_ARG;
    if (!ref) return fail(ctx, KGMA_E_ARG, "null argument");
    if (s < 1 || w_min < 1 || w_min > w_max || q < 1)
        return fail(ctx, KGMA_E_ARG, "invalid randstrobe parameters s = %d, w_min = %d, w_max = %d, q = %lld", s, w_min, w_max, (long long)q);
    if (n_refs < 0) return fail(ctx, KGMA_E_ARG, "n_refs = %lld", (long long)n_refs);
    const int64_t k64 = (int64_t)w_max + s - 1;
    if (k64 >= windowsize)
        return fail(ctx, KGMA_E_ARG, "the window size %lld does not exceed the strobemer span %lld (w_max + s - 1)", (long long)windowsize, (long long)k64);
    if (s > KGMA_STROBE_MAX_S)
        return fail(ctx, KGMA_E_UNSUPPORTED, "s = %d: the device path supports 1 <= s <= %d (4^(2s) window counts per wave in LDS)", s, KGMA_STROBE_MAX_S);
    if (k64 > KGMA_STROBE_MAX_K)
        return fail(ctx, KGMA_E_UNSUPPORTED, "w_max + s - 1 = %lld: a strobemer of at most %d residues is supported", (long long)k64, KGMA_STROBE_MAX_K);
    (void)hipSetDevice(ctx->device);
    const int k = (int)k64;
    const int64_t NB = (int64_t)1 << (4 * s);
    std::vector<KfvInfo> kv(1);
    KfvInfo &f = kv[0];
    {
        std::vector<uint32_t> keys;
        std::vector<double> nz;
        for (int64_t x = 0; x < NB; x++)
            if (ref[x] != 0.0) { keys.push_back((uint32_t)x); nz.push_back(ref[x]); }
        const int rc = kfv_from_nonzeros(ctx, k, 0, std::move(keys), std::move(nz), &windowsize, &thr, n_refs > 0 ? &n_refs : nullptr, f);
        if (rc != KGMA_OK) return rc;
    }
    if (f.fp) return fail(ctx, KGMA_E_UNSUPPORTED, "the strobemer engine scans KFVs that are S/N with integer S (gen_ref_ws_cons's); this one is not");
    if (f.Smax > INT32_MAX) return fail(ctx, KGMA_E_UNSUPPORTED, "KFV entries beyond int32");
    f.ref.assign(ref, ref + NB);
    f.S.assign((size_t)NB, 0);
    for (size_t i = 0; i < f.sk.size(); i++) f.S[f.sk[i]] = f.sS[i];
    f.sk.clear(); f.sv.clear(); f.sS.clear();
    std::vector<int32_t> tab((size_t)NB);
    for (int64_t x = 0; x < NB; x++) tab[(size_t)x] = (int32_t)f.S[(size_t)x];
    for (void *p : {(void *)ctx->d_Stab, (void *)ctx->d_StabC, (void *)ctx->d_Rtab, (void *)ctx->d_sparse, (void *)ctx->d_Wtab}) if (p) (void)hipFree(p);
    ctx->d_Stab = nullptr; ctx->d_StabC = nullptr; ctx->d_Rtab = nullptr; ctx->d_sparse = nullptr; ctx->d_Wtab = nullptr;
    for (auto &kv2 : ctx->sinter) (void)hipFree(kv2.second);
    ctx->sinter.clear();
    ctx->m = 0;                                                        // (no references until the uploads below have succeeded)
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_Stab), tab.size() * sizeof(int32_t)));
    HIP_TRY(ctx, hipMemcpy(ctx->d_Stab, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_Wtab), sizeof(int64_t)));
    HIP_TRY(ctx, hipMemcpy(ctx->d_Wtab, &windowsize, sizeof(int64_t), hipMemcpyHostToDevice));
    ctx->k = k;
    ctx->m = 1;
    ctx->strobe = true;
    ctx->st_s = s; ctx->st_wmin = w_min; ctx->st_wmax = w_max; ctx->st_q = q;
    ctx->kfv.swap(kv);
    ctx->refs_version++;                                              // (the prefilter remembers its fallbacks per reference set)
    for (double *p : ctx->d_dist) if (p) (void)hipFree(p);
    ctx->d_dist.assign(1, nullptr);
    ctx->dist_cap.assign(1, 0);
    ctx->last_mode = -1;
    ctx->tk_uid = 0;
    return KGMA_OK;
}

}  // extern "C"

// ---- genomes: layout, ingests, constructors, pack launches, the state of the 2-bit copy ------------------------------------------
namespace kgma {
hipError_t launch_pack(const uint8_t *ascii, uint32_t *planes, uint32_t *inter, const ContigDesc *cd, int n_contigs, int64_t total_words,
                       const int32_t *block_contig, unsigned long long *first_bad, hipStream_t st, int64_t block0 = 0, int64_t n_blocks = -1);
hipError_t launch_pack(const uint8_t *ascii, uint32_t *planes, uint32_t *inter, const ContigDesc *cd, int n_contigs, int64_t total_words,
                       const int32_t *block_contig, unsigned long long *first_bad, hipStream_t st, const int32_t *block_list, int64_t n_list);
hipError_t launch_pack_sums(const PackSumsArgs &a, int k, int64_t s_max, int n_cus, bool sums_only, hipStream_t st, unsigned int *host_count = nullptr);
int64_t pack_sums_waves(int n_cus);
hipError_t launch_synth(uint8_t *ascii, const ContigDesc *cd, int n_contigs, int64_t total_words, uint64_t seed, hipStream_t st);
hipError_t launch_fasta_count(const uint8_t *raw, int64_t n, uint32_t *counts, hipStream_t st);
hipError_t launch_fasta_blank(uint8_t *raw, const int64_t *ranges, int n_ranges, hipStream_t st);
hipError_t launch_fasta_scatter(const uint8_t *raw, int64_t n, const int64_t *block_base, const int64_t *rec_start, const ContigDesc *cd, int n_rec,
                                uint8_t *ascii, hipStream_t st);
int64_t revcomp_tile_bytes();
hipError_t launch_revcomp(const RevcompArgs &a, int64_t n_tiles, hipStream_t st);
int64_t twobit_tile_bytes();
hipError_t launch_twobit_unpack(const TwobitArgs &a, int64_t n_tiles, hipStream_t st);
}  // namespace kgma

namespace {

bool parse_cpulist(const char *txt, cpu_set_t *out)
{
    CPU_ZERO(out);
    const char *p = txt;
    bool any = false;
    while (*p) {
        while (*p == ',' || *p == ' ' || *p == '\n') p++;
        if (!*p) break;
        char *e = nullptr;
        const long a = strtol(p, &e, 10);
        if (e == p || a < 0) return false;
        long b = a;
        p = e;
        if (*p == '-') { b = strtol(p + 1, &e, 10); if (e == p + 1 || b < a) return false; p = e; }
        for (long c = a; c <= b && c < CPU_SETSIZE; c++) { CPU_SET((int)c, out); any = true; }
    }
    return any;
}

void numa_lookup(kgma_ctx *ctx)
{
    ctx->genome.numa_state = -1;
    const char *env = getenv("KGMA_NUMA_BIND");
    if (env && atoi(env) == 0) return;
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf - 1, ctx->device) != hipSuccess) { (void)hipGetLastError(); return; }
    for (char *q = bdf; *q; q++) if (*q >= 'A' && *q <= 'F') *q = (char)(*q - 'A' + 'a');
    char path[256], buf[4096];
    auto slurp = [&](const char *pth) -> bool {
        FILE *f = fopen(pth, "r");
        if (!f) return false;
        const size_t got = fread(buf, 1, sizeof buf - 1, f);
        fclose(f);
        buf[got] = 0;
        return got > 0;
    };
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bdf);
    if (!slurp(path)) return;
    const int node = atoi(buf);
    if (node < 0) return;
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    if (!slurp(path)) return;
    cpu_set_t node_cpus;
    if (!parse_cpulist(buf, &node_cpus)) return;
    ctx->genome.numa_cpus = node_cpus;
    ctx->genome.numa_state = 1;
}

NumaBind::NumaBind(kgma_ctx *ctx)
{
    if (ctx->genome.numa_state == 0) numa_lookup(ctx);
    if (ctx->genome.numa_state != 1) return;
    if (pthread_getaffinity_np(pthread_self(), sizeof saved, &saved) != 0) return;
    cpu_set_t want;
    CPU_AND(&want, &saved, &ctx->genome.numa_cpus);
    const int n = CPU_COUNT(&want);
    if (n < 1 || n == CPU_COUNT(&saved)) return;                  // (not allowed there, or already there)
    bound = pthread_setaffinity_np(pthread_self(), sizeof want, &want) == 0;
}
NumaBind::~NumaBind() { if (bound) (void)pthread_setaffinity_np(pthread_self(), sizeof saved, &saved); }

int ingest_threads()
{
    int t = (int)std::thread::hardware_concurrency() / 2;
    if (const char *e = getenv("KGMA_INGEST_THREADS")) t = atoi(e);
    return std::max(1, std::min(t, 8));
}

// the one place that spells out the pack kernel's arguments: one pack launch over all blocks (the default), over [block0, block0 + n_blocks),
// or over a sorted list on the device; st null: the context's stream
#define PACK_ARGS(g, st) (g)->d_ascii, (g)->d_planes, (g)->d_inter, (g)->d_cd, (int)(g)->n_contigs, (g)->total_words, (g)->d_block_contig, (g)->d_first_bad, (st)
hipError_t pack_blocks(kgma_ctx *ctx, const kgma_genome *g, int64_t block0 = 0, int64_t n_blocks = -1, hipStream_t st = nullptr) { return launch_pack(PACK_ARGS(g, st ? st : ctx->stream), block0, n_blocks); }
hipError_t pack_blocks(kgma_ctx *ctx, const kgma_genome *g, const int32_t *block_list, int64_t n_list) { return launch_pack(PACK_ARGS(g, ctx->stream), block_list, n_list); }

// Waits for a pending pack of `g` (the pack kernel is launched asynchronously).
int genome_sync(kgma_ctx *ctx, kgma_genome *g)
{
    if (!g->pack_pending) return KGMA_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->genome.evp0, ctx->genome.evp1);
    ctx->stats.pack_ms = ms;
    g->pack_pending = false;
    return KGMA_OK;
}

// ---- the state of the 2-bit copy (kgma_genome::inter_state) ------------------------------------------------
// ensure_inter is the ONE way a reader gets a complete copy: every site that hands g->d_inter to a kernel or to a copy calls it
// first (or is one of the two in-step consumers below), and everything that changes the resident text of an existing genome calls
// it BEFORE the change -- so the copy is, as ever, the text as of the last pack.  PARTIAL: the full plain pack runs on the context's
// stream (planes too, if the genome has got them since) and the state is FULL; FULL: nothing.
int ensure_inter(kgma_ctx *ctx, kgma_genome *g)
{
    if (g->inter_state == KGMA_INTER_FULL) return KGMA_OK;
    (void)hipSetDevice(ctx->device);
    if (g->n_contigs > 0) HIP_TRY(ctx, pack_blocks(ctx, g));
    g->inter_state = KGMA_INTER_FULL;
    if (getenv("KGMA_GEOM_DEBUG")) fprintf(stderr, "sparse pack: the 2-bit copy completed by a full pack (%lld blocks had been packed on demand)\n", (long long)g->inter_demand_blocks);
    g->inter_demand_blocks = 0;
    return KGMA_OK;
}

// Words the stream and chain kernels LOAD of a stream that starts at plane word `word_base` and evaluates n_valid windows of nk
// k-mers (stream8_kernel and gen_kernel alike): the stream's positions are n_pos = n_valid + nk - 1 (+ up to 2 for derived windows),
// walked in n_blocks = ceil(n_pos / 64) steps of 64; step b loads the dword pair of its entering k-mers, dwords 4 b + (lane >> 4) and
// the one behind it, i.e. up to 4 b + 4, and the pair of its leaving ones, nk positions back and never before dword 0 (the index
// is clamped in the warm-up; nothing is read in front of word_base).  The loads run ONE step ahead of the walk, up to b = n_blocks,
// and the steady steps go through a buffer descriptor of 16 (n_blocks + 2) bytes.  So a stream loads no dword at or past
// 4 (n_blocks + 2): plane words word_base ... word_base + 2 (n_blocks + 2) - 1.  (export_kernel reads the residue text only.)
static inline int64_t stream_words_loaded(int64_t n_valid, int64_t nk)
{
    const int64_t n_blocks = (n_valid + nk - 1 + 2 + 63) >> 6;
    return 2 * (n_blocks + 2);
}

// In-step consumer 1 (PARTIAL only): the sorted, de-duplicated pack blocks that the candidate streams `streams` load, packed whole
// by the list form of pack_kernel in front of the exact scan.  A block shared by two records is packed whole like any other.
int pack_candidate_blocks(kgma_ctx *ctx, kgma_genome *g, const std::vector<TileDesc> &streams, int64_t nk)
{
    if (g->inter_state != KGMA_INTER_PARTIAL) return KGMA_OK;
    const int64_t PBW = pack_block_words();
    const int64_t total_blocks = (g->total_words + PBW - 1) / PBW;
    std::vector<int32_t> &bl = ctx->genome.blist;
    bl.clear();
    for (const TileDesc &td : streams) {                               // (sorted by record and window: so are the blocks)
        const int64_t w0 = td.word_base, w1 = std::min<int64_t>(g->total_words, w0 + stream_words_loaded(td.n_valid, nk)) - 1;
        if (w0 < 0 || w0 >= g->total_words) return ctx_fail(ctx, KGMA_E_HIP, "internal: candidate stream outside the genome");
        for (int64_t b = w0 / PBW; b <= w1 / PBW && b < total_blocks; b++)
            if (bl.empty() || bl.back() < (int32_t)b) bl.push_back((int32_t)b);
    }
    if (!std::is_sorted(bl.begin(), bl.end())) { std::sort(bl.begin(), bl.end()); bl.erase(std::unique(bl.begin(), bl.end()), bl.end()); }
    if (bl.empty()) return KGMA_OK;
    const int rc = dev_reserve(ctx, ctx->genome.d_blist, ctx->genome.blist_cap, (int64_t)bl.size());
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->genome.d_blist, bl.data(), bl.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, pack_blocks(ctx, g, ctx->genome.d_blist, (int64_t)bl.size()));
    g->inter_demand_blocks += (int64_t)bl.size();
    if (getenv("KGMA_GEOM_DEBUG")) fprintf(stderr, "sparse pack: %zu of %lld blocks packed for %zu candidate streams\n", bl.size(), (long long)total_blocks, streams.size());
    return KGMA_OK;
}

// In-step consumer 2 (PARTIAL only): the block range of every record in `records`, with the range form of the pack, in front of
// a chain launch or a download of a record's codes.  A chain's streams start at the record's first word and the last one ends
// with the record's last k-mer: by stream_words_loaded it loads fewer than 8 words past the record's last word, inside the
// CONTIG_PAD_WORDS that are taken here (past the last record: the tail padding).
int pack_record_blocks(kgma_ctx *ctx, kgma_genome *g, std::vector<int32_t> records)
{
    if (g->inter_state != KGMA_INTER_PARTIAL) return KGMA_OK;
    (void)hipSetDevice(ctx->device);
    const int64_t PBW = pack_block_words();
    const int64_t total_blocks = (g->total_words + PBW - 1) / PBW;
    std::sort(records.begin(), records.end());
    records.erase(std::unique(records.begin(), records.end()), records.end());
    int64_t done_to = 0;                                               // blocks below it are packed already (a block two records share)
    for (const int32_t c : records) {
        if (c < 0 || c >= g->n_contigs) return ctx_fail(ctx, KGMA_E_HIP, "internal: chained record outside the genome");
        const ContigDesc &d = g->cd[(size_t)c];
        const int64_t w1 = std::min<int64_t>(g->total_words, d.word_off + (d.len + 31) / 32 + CONTIG_PAD_WORDS) - 1;
        const int64_t b0 = std::max<int64_t>(done_to, d.word_off / PBW), b1 = std::min<int64_t>(total_blocks, w1 / PBW + 1);
        if (b1 <= b0) continue;
        HIP_TRY(ctx, pack_blocks(ctx, g, b0, b1 - b0));
        g->inter_demand_blocks += b1 - b0;
        done_to = b1;
    }
    return KGMA_OK;
}

// The bit-plane copy of the genome (read by the bit-sliced kernel, its window pass and the 16-bit stream kernel) is
// made the first time a scan needs it and kept up to date by every later pack; genomes that only the 8-bit stream
// kernel scans never have one.
int ensure_planes(kgma_ctx *ctx, kgma_genome *g)
{
    if (g->d_planes) return KGMA_OK;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&g->d_planes), (size_t)g->total_words * 8));
    g->device_bytes += g->total_words * 8;
    if (g->n_contigs > 0)
        HIP_TRY(ctx, pack_blocks(ctx, g));
    else
        HIP_TRY(ctx, hipMemsetAsync(g->d_planes, 0, (size_t)g->total_words * 8, ctx->stream));
    g->inter_state = KGMA_INTER_FULL;                                  // (a full pack: it writes the 2-bit copy beside the planes)
    g->inter_demand_blocks = 0;
    return KGMA_OK;
}

static void pack_sums_args(const kgma_genome *g, const int32_t *S, PackSumsArgs &a)
{
    a.ascii = g->d_ascii; a.planes = g->d_planes; a.inter = g->d_inter; a.bsum = g->d_bsum;
    a.cd = g->d_cd; a.total_words = g->total_words; a.block_contig = g->d_block_contig; a.first_bad = g->d_first_bad;
    a.S = S; a.n_contigs = (int32_t)g->n_contigs;
    const int bw = pack_block_words();
    a.block_shift = (bw & (bw - 1)) == 0 ? __builtin_ctz((unsigned)bw) : -1;
}

// The state of the block sums (kgma_genome::bsum_state).  DEFERRED: the storing sums-only pack runs now, on the
// resident text and the S table of the step that deferred them, and the state is WRITTEN.  Called by whoever reads the sums and,
// like ensure_inter, BEFORE anything changes the resident text of an existing genome: the sums are those of the text the step packed.
// must: the caller reads the sums (a failed allocation is its error); else the text is about to change, and a failed allocation
// only drops the sums (state NONE: kgma_get_block_sums then says that no step has left any) -- the change itself goes on.
int ensure_bsum(kgma_ctx *ctx, kgma_genome *g, bool must)
{
    if (g->bsum_state != KGMA_BSUM_DEFERRED) return KGMA_OK;
    (void)hipSetDevice(ctx->device);
    if (!g->d_bsum) {
        if (hipMalloc(reinterpret_cast<void **>(&g->d_bsum), (size_t)g->total_words * 4) != hipSuccess) {
            (void)hipGetLastError();
            g->d_bsum = nullptr;
            if (must) return fail(ctx, KGMA_E_NOMEM, "kgma_get_block_sums: no device memory for the block sums (%lld bytes)", (long long)g->total_words * 4);
            g->bsum_state = KGMA_BSUM_NONE;
            return KGMA_OK;
        }
        g->device_bytes += g->total_words * 4;
    }
    PackSumsArgs a;
    memset(&a, 0, sizeof a);
    pack_sums_args(g, g->d_bsum_S, a);
    a.planes = nullptr; a.inter = nullptr;                             // (the sums-only form writes neither)
    HIP_TRY(ctx, launch_pack_sums(a, g->bsum_k, g->bsum_smax, ctx->n_cus, true, ctx->stream));
    g->bsum_state = KGMA_BSUM_WRITTEN;
    return KGMA_OK;
}

// sums: the step's pack with the prefilter's block sums of KFV 0 (pack_sums_kernel; the caller has checked that it applies and
// that g->d_bsum exists, or that the pack tests).  sparse (with sums, a genome without planes): the sums-only form -- the 2-bit copy is left PARTIAL and the
// step packs the blocks it reads (pack_candidate_blocks, pack_record_blocks).  Every other pack is a full one: FULL
int genome_repack(kgma_ctx *ctx, kgma_genome *g, const PackSums *sums, bool sparse = false)
{
    sparse = sparse && sums && g->n_contigs > 0 && g->d_planes == nullptr;
    g->inter_demand_blocks = 0;
    (void)hipSetDevice(ctx->device);
    // first_bad (smallest position of a residue outside A/C/G/T/N per record) is a function of the residue
    // text: re-encoding unchanged text finds the same minima, so the reset and the download of the table
    // are only queued when the text changed (new genome, kgma_genome_poke)
    const bool dirty = g->text_dirty;
    if (dirty) HIP_TRY(ctx, hipMemsetAsync(g->d_first_bad, 0xFF, std::max<size_t>(1, (size_t)g->n_contigs) * 8, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->genome.evp0, ctx->stream));
    if (g->n_contigs > 0 && sums) {
        PackSumsArgs a;
        memset(&a, 0, sizeof a);
        const bool test = sums->test && sparse;
        pack_sums_args(g, sums->S, a);
        if (test) {
            a.bsum = nullptr;
            a.U = sums->U; a.nblk = sums->nblk; a.nk = sums->nk; a.run = sums->run; a.cap = (unsigned int)sums->cap;
            a.list = reinterpret_cast<FilterEntry *>(ctx->h_fpin_dev + 16);
            a.ctl = ctx->d_fctl;
        }
        HIP_TRY(ctx, launch_pack_sums(a, sums->k, sums->s_max, sums->n_cus, sparse, ctx->stream, test ? reinterpret_cast<unsigned int *>(ctx->h_fpin_dev) : nullptr));
        g->bsum_fresh = !test;
        g->pack_tested = test;
        g->bsum_state = test ? KGMA_BSUM_DEFERRED : KGMA_BSUM_WRITTEN;
        g->bsum_k = sums->k;
        g->bsum_smax = sums->s_max;
    } else if (g->n_contigs > 0)
        HIP_TRY(ctx, pack_blocks(ctx, g));
    else
    {
        if (g->d_planes) HIP_TRY(ctx, hipMemsetAsync(g->d_planes, 0, (size_t)g->total_words * 8, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(g->d_inter, 0, (size_t)g->total_words * 8, ctx->stream));
    }
    HIP_TRY(ctx, hipEventRecord(ctx->genome.evp1, ctx->stream));
    g->inter_state = sparse ? KGMA_INTER_PARTIAL : KGMA_INTER_FULL;
    if (sparse) {
        // KGMA_SPARSE_POISON=1 (tests): every word of the copy is allocated memory, so a read of a block that nobody packed shows up
        // as a wrong result, never as a fault
        const char *pz = getenv("KGMA_SPARSE_POISON");
        if (pz && atoi(pz) != 0) HIP_TRY(ctx, hipMemsetAsync(g->d_inter, 0x5A, (size_t)g->total_words * 8, ctx->stream));
    }
    if (dirty) HIP_TRY(ctx, hipMemcpyAsync(g->first_bad, g->d_first_bad, std::max<size_t>(1, (size_t)g->n_contigs) * 8, hipMemcpyDeviceToHost, ctx->stream));
    g->text_dirty = false;
    g->pack_pending = true;     // completed by the next scan's single synchronisation (or genome_sync)
    return KGMA_OK;
}

// What the pack kernel knows about the residues (first_bad) and the copy the caller reads must be current: a pack that is deferred,
// or never queued since the text changed, runs now; then the copy is completed and the pack waited for.
int genome_ready(kgma_ctx *ctx, kgma_genome *g, bool planes)   // planes: the reader needs the bit planes, else the 2-bit copy
{
    if (g->repack_deferred || g->text_dirty) {
        g->repack_deferred = false;
        const int prc = genome_repack(ctx, g, nullptr);
        if (prc) return prc;
    }
    const int rc = planes ? ensure_planes(ctx, g) : ensure_inter(ctx, g);
    if (rc) return rc;
    return genome_sync(ctx, g);
}

// the context's staging pair (2 x 32 MiB of pinned memory), made on first use
StagePipe *ctx_pipe(kgma_ctx *ctx)
{
    if (ctx->genome.pipe) { ctx->genome.pipe->drain(); return ctx->genome.pipe; }
    StagePipe *p = new (std::nothrow) StagePipe();
    if (!p) return nullptr;
    if (!p->init((size_t)32 << 20, ctx->stream)) { delete p; return nullptr; }
    ctx->genome.pipe = p;
    return p;
}

// ---- a genome under construction: one owner, one way in, one way out -------------------------------------------------------------
struct GenomeRelease { kgma_ctx *ctx; void operator()(kgma_genome *g) const { kgma_genome_free(ctx, g); } };
using GenomeOwner = std::unique_ptr<kgma_genome, GenomeRelease>;

// in: a genome of records of these lengths, laid out and allocated, its text still to be written
int genome_begin(kgma_ctx *ctx, const int64_t *contig_len, int64_t n_contigs, GenomeOwner &owner)
{
    owner = GenomeOwner(new (std::nothrow) kgma_genome(), GenomeRelease{ctx});
    kgma_genome *g = owner.get();
    if (!g) return ctx_fail(ctx, KGMA_E_NOMEM, "out of host memory");
    g->n_contigs = n_contigs;
    g->cd.resize((size_t)n_contigs);
    int64_t aoff = 0, woff = LEAD_PAD_WORDS, total = 0;
    for (int64_t c = 0; c < n_contigs; c++) {
        const int64_t L = contig_len[c];
        if (L < 0) return fail(ctx, KGMA_E_ARG, "contig_len[%lld] < 0", (long long)c);
        g->cd[(size_t)c] = ContigDesc{aoff, woff, L};
        aoff += record_slot_bytes(L);
        woff += (L + 31) / 32 + CONTIG_PAD_WORDS;
        total += L;
    }
    g->ascii_bytes = aoff + 64;
    g->total_words = woff + TAIL_PAD_WORDS;
    g->total_bases = total;
    (void)hipSetDevice(ctx->device);
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&g->d_ascii), (size_t)g->ascii_bytes));
    g->d_planes = nullptr;       // bit planes: allocated and written once a scan needs them (ensure_planes)
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&g->d_inter), (size_t)g->total_words * 8));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&g->d_cd), std::max<size_t>(1, (size_t)n_contigs) * sizeof(ContigDesc)));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&g->d_first_bad), std::max<size_t>(1, (size_t)n_contigs) * sizeof(unsigned long long)));
    HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&g->first_bad), std::max<size_t>(1, (size_t)n_contigs) * sizeof(unsigned long long), hipHostMallocDefault));
    g->uid = ctx->genome.next_uid++;
    {
        // pack_kernel: record of the first plane word of every block (words before a record's first one -- lead /
        // inter-record padding -- belong to the record before; the kernel walks forward from there)
        const int64_t bw = pack_block_words();
        const int64_t nblk = (g->total_words + bw - 1) / bw;
        std::vector<int32_t> bc((size_t)std::max<int64_t>(nblk, 1), 0);
        int32_t c = 0;
        for (int64_t b = 0; b < nblk; b++) {
            const int64_t w = b * bw;
            while (c + 1 < n_contigs && g->cd[(size_t)c + 1].word_off <= w) c++;
            bc[(size_t)b] = c;
        }
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&g->d_block_contig), bc.size() * sizeof(int32_t)));
        HIP_TRY(ctx, hipMemcpy(g->d_block_contig, bc.data(), bc.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        g->device_bytes += (int64_t)bc.size() * 4;
    }
    g->device_bytes += g->ascii_bytes + g->total_words * 8 + n_contigs * (int64_t)(sizeof(ContigDesc) + 8);
    if (n_contigs > 0)
        HIP_TRY(ctx, hipMemcpy(g->d_cd, g->cd.data(), (size_t)n_contigs * sizeof(ContigDesc), hipMemcpyHostToDevice));
    return KGMA_OK;
}

// out: the text is written (or queued on the context's stream); the first pack is queued behind it and the caller gets the genome
int genome_finish(kgma_ctx *ctx, GenomeOwner &g, kgma_genome **out)
{
    const int rc = genome_repack(ctx, g.get(), nullptr);
    if (rc == KGMA_OK) *out = g.release();
    return rc;
}

// The transient device memory and events of one ingest (DeviceHold) and the staging pair it fills.  Destroyed (reset()) where the
// ingest is done with them, in front of the first pack, and on every other path out: waits for the staging copies, frees the
// transients and, fasta: gives the context's FASTA scratch back where it has grown beyond 2 GiB.
struct IngestScratch : DeviceHold {
    kgma_ctx *ctx; StagePipe &pipe; bool fasta;
    IngestScratch(kgma_ctx *ctx_, StagePipe &pipe_, bool fasta_) : ctx(ctx_), pipe(pipe_), fasta(fasta_) {}
    ~IngestScratch()
    {
        pipe.drain();
        if (!fasta || ctx->genome.ingest_cap <= ((int64_t)2 << 30)) return;   // (large scratch is not kept)
        (void)hipFree(ctx->genome.d_ingest); ctx->genome.d_ingest = nullptr; ctx->device_bytes -= ctx->genome.ingest_cap; ctx->genome.ingest_cap = 0;
    }
};

struct IngestLap {   // KGMA_INGEST_DEBUG: the host's time from one point of an ingest to the next
    const char *tag;
    const bool on = getenv("KGMA_INGEST_DEBUG") != nullptr;
    double tq = now_ms();
    void operator()(const char *what) { const double t = now_ms(); if (on) fprintf(stderr, "  %s: %-28s %8.3f ms\n", tag, what, t - tq); tq = t; }
};

// One staged upload for every ingest: device bytes dst[0, bytes) are the segments `segs` (kgma_stage_fill.h) with `gap` between
// them, moved window by window through the staging pair -- a few threads fill one buffer (at least min_per_thread bytes each) while
// the DMA engine drains the other.  hook (optional) runs on the thread that has just filled bytes [b0, e0) of the window that
// starts at device byte w0: the bytes are in its cache.  0, UPLOAD_UNREAD (a read failed), or the hipError_t of the copy that failed.
constexpr int UPLOAD_UNREAD = -1;
using RangeHook = std::function<void(int t, const uint8_t *stage, int64_t w0, int64_t b0, int64_t e0)>;
int staged_upload(StagePipe &pipe, uint8_t *dst, int64_t bytes, const std::vector<StageSeg> &segs, uint8_t gap, int64_t min_per_thread,
                  const RangeHook &hook = nullptr)
{
    const int64_t stage_cap = (int64_t)pipe.cap;
    std::atomic<int> unread{0};
    for (int64_t w0 = 0; w0 < bytes; w0 += stage_cap) {
        uint8_t *stage = pipe.acquire();               // (the other buffer may still be on its way to the device)
        const int64_t len = std::min<int64_t>(stage_cap, bytes - w0);
        parallel_ranges(len, ingest_threads(), min_per_thread, [&](int t, int64_t b0, int64_t e0) {
            if (!stage_fill(stage, w0, b0, e0, segs.data(), segs.size(), gap)) unread.store(1);
            if (hook) hook(t, stage, w0, b0, e0);
        });
        if (unread.load()) return UPLOAD_UNREAD;
        const hipError_t e = pipe.submit(dst + w0, (size_t)len);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

}  // namespace

// kgma_search.h and the headers of the four searches: their states in the context, and the genome made ready for a search
namespace kgma {
ExactState *ctx_exact(kgma_ctx *ctx) { return &ctx->exact; }
MotifState *ctx_motif(kgma_ctx *ctx) { return &ctx->motif; }
ApproxState *ctx_approx(kgma_ctx *ctx) { return &ctx->approx; }
PwmState *ctx_pwm(kgma_ctx *ctx) { return &ctx->pwm; }
CodonState *ctx_codon(kgma_ctx *ctx) { return &ctx->codon; }
int genome_searchable(kgma_ctx *ctx, const kgma_genome *gc, PackedCopy copy, bool *clean)
{
    kgma_genome *g = const_cast<kgma_genome *>(gc);   // only its pack bookkeeping and its lazily made plane copy are updated
    (void)hipSetDevice(ctx->device);
    const int rc = genome_ready(ctx, g, copy == PackedCopy::Planes);   // (first_bad is current)
    if (rc) return rc;
    ctx->stats.bases_scanned = g->total_bases;
    ctx->stats.scan_ms = 0;
    ctx->stats.n_launches = 0;
    if (clean) *clean = true;
    for (int64_t c = 0; c < g->n_contigs; c++)
        if (g->first_bad[(size_t)c] != NO_BAD) {
            if (!clean) return fail(ctx, KGMA_E_BADBASE, "record %lld: residue %llu is not one of A/C/G/T/N", (long long)c, g->first_bad[(size_t)c]);   // (first_bad is 1-based)
            *clean = false;
        }
    return KGMA_OK;
}
}  // namespace kgma

extern "C" {

int kgma_genome_repack(kgma_ctx *ctx, kgma_genome *g)
{
    if (!ctx || !g) return KGMA_E_ARG;
    return genome_repack(ctx, g, nullptr);
}

int kgma_genome_from_host(kgma_ctx *ctx, const uint8_t *const *contig_ascii, const int64_t *contig_len,
                          int64_t n_contigs, kgma_genome **out)
{
    if (!ctx) return KGMA_E_ARG;
    if (!out || n_contigs < 0 || (n_contigs > 0 && (!contig_ascii || !contig_len)))
        return ctx_fail(ctx, KGMA_E_ARG, "null argument");
    if (n_contigs > 0x7FFFFFF0ll) return ctx_fail(ctx, KGMA_E_UNSUPPORTED, "too many records");
    *out = nullptr;
    NumaBind numa(ctx);                                              // (staging buffers and copying threads on the GPU's NUMA node)
    GenomeOwner g;
    const int rc = genome_begin(ctx, contig_len, n_contigs, g);
    if (rc != KGMA_OK) return rc;
    // stream the records through two pinned staging buffers (fill one while the other is copied): every record's residues at
    // its place in the text, zeros in the padding behind them (the text's 64 tail bytes are not written)
    StagePipe *pipe = ctx_pipe(ctx);
    if (!pipe) return ctx_fail(ctx, KGMA_E_NOMEM, "cannot allocate the pinned staging buffers");
    std::vector<StageSeg> segs;
    for (int64_t c = 0; c < n_contigs; c++)
        if (g->cd[(size_t)c].len > 0) segs.push_back(StageSeg{g->cd[(size_t)c].ascii_off, g->cd[(size_t)c].len, contig_ascii[c], -1, 0});
    const int up = staged_upload(*pipe, g->d_ascii, g->ascii_bytes - 64, segs, 0, (int64_t)2 << 20);
    pipe->drain();
    if (up) return fail(ctx, KGMA_E_HIP, "host-to-device copy failed: %s", hipGetErrorString((hipError_t)up));
    return genome_finish(ctx, g, out);
}

int kgma_genome_synthetic(kgma_ctx *ctx, const int64_t *contig_len, int64_t n_contigs, uint64_t seed,
                          const uint8_t *plant, int64_t plant_len, const int64_t *plant_contig,
                          const int64_t *plant_pos, int64_t n_plants, kgma_genome **out)
{
    if (!ctx) return KGMA_E_ARG;
    if (!out || !contig_len || n_contigs < 1) return ctx_fail(ctx, KGMA_E_ARG, "null argument");
    if (n_plants > 0 && (!plant || !plant_contig || !plant_pos || plant_len < 1)) return ctx_fail(ctx, KGMA_E_ARG, "bad plant arguments");
    *out = nullptr;
    GenomeOwner g;
    const int rc = genome_begin(ctx, contig_len, n_contigs, g);
    if (rc != KGMA_OK) return rc;
    hipError_t he = launch_synth(g->d_ascii, g->d_cd, (int)n_contigs, g->total_words, seed, ctx->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(ctx->stream);
    for (int64_t i = 0; i < n_plants && he == hipSuccess; i++) {
        const int64_t c = plant_contig[i], pos = plant_pos[i];
        if (c < 0 || c >= n_contigs || pos < 1 || pos + plant_len - 1 > contig_len[c])
            return fail(ctx, KGMA_E_ARG, "plant %lld does not fit its record", (long long)i);
        he = hipMemcpy(g->d_ascii + g->cd[(size_t)c].ascii_off + (pos - 1), plant, (size_t)plant_len, hipMemcpyHostToDevice);
    }
    if (he != hipSuccess) return fail(ctx, KGMA_E_HIP, "synthetic genome generation failed: %s", hipGetErrorString(he));
    return genome_finish(ctx, g, out);
}

// ------------------------------------------------------------------------------------------
// reverse complement of a resident genome (kgma_revcomp.hip)
// ------------------------------------------------------------------------------------------
int kgma_genome_revcomp_into(kgma_ctx *ctx, const kgma_genome *g, kgma_genome *rc)
{
    if (!ctx) return KGMA_E_ARG;
    if (!g || !rc) return ctx_fail(ctx, KGMA_E_ARG, "kgma_genome_revcomp_into: null argument");
    if (g == rc) return ctx_fail(ctx, KGMA_E_ARG, "kgma_genome_revcomp_into: source and destination are the same genome");
    const int64_t nc = g->n_contigs;
    bool same = rc->n_contigs == nc && rc->ascii_bytes == g->ascii_bytes;
    for (int64_t c = 0; c < nc && same; c++) same = rc->cd[(size_t)c].len == g->cd[(size_t)c].len;
    if (!same) return ctx_fail(ctx, KGMA_E_ARG, "kgma_genome_revcomp_into: the genomes' record lengths differ");
    (void)hipSetDevice(ctx->device);
    {
        const int irc = ensure_inter(ctx, rc);                         // (rc's text is about to change: its 2-bit copy is completed from the old one first)
        if (irc) return irc;
        const int brc = ensure_bsum(ctx, rc, false);                       // (and its block sums, where a step left them to be written)
        if (brc) return brc;
    }
    // the kernel writes all of a record's slot in the text
    const std::vector<int64_t> prefix = tile_prefix(nc, revcomp_tile_bytes(), true, [&](int64_t c) { return g->cd[(size_t)c].len; });
    const int64_t n_tiles = prefix[(size_t)nc];
    if (n_tiles > 0x7FFFFFFFll) return fail(ctx, KGMA_E_UNSUPPORTED, "kgma_genome_revcomp: %lld tiles exceed one launch", (long long)n_tiles);
    if (!ctx->genome.d_rcprefix || prefix != ctx->genome.rcprefix) {
        // (a launch of an earlier call may still be reading the table it was given)
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ctx->genome.rcprefix.clear();
        int rc_ = dev_reserve(ctx, ctx->genome.d_rcprefix, ctx->genome.rcprefix_cap, nc + 1);
        if (rc_) return rc_;
        HIP_TRY(ctx, hipMemcpy(ctx->genome.d_rcprefix, prefix.data(), prefix.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        ctx->genome.rcprefix = prefix;
    }
    RevcompArgs a{};
    a.src = g->d_ascii; a.dst = rc->d_ascii; a.cd = rc->d_cd; a.tile_prefix = ctx->genome.d_rcprefix; a.n_contigs = (int32_t)nc;
    HIP_TRY(ctx, launch_revcomp(a, n_tiles, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(rc->d_ascii + (rc->ascii_bytes - 64), 0, 64, ctx->stream));      // the text's 64 tail bytes
    rc->text_dirty = true;
    return KGMA_OK;
}

int kgma_genome_revcomp(kgma_ctx *ctx, const kgma_genome *src, kgma_genome **out)
{
    if (!ctx) return KGMA_E_ARG;
    if (!src || !out) return ctx_fail(ctx, KGMA_E_ARG, "kgma_genome_revcomp: null argument");
    *out = nullptr;
    std::vector<int64_t> lens((size_t)src->n_contigs);
    for (int64_t c = 0; c < src->n_contigs; c++) lens[(size_t)c] = src->cd[(size_t)c].len;
    GenomeOwner g;
    int rc = genome_begin(ctx, lens.data(), src->n_contigs, g);
    if (rc != KGMA_OK) return rc;
    g->headers = src->headers;
    rc = kgma_genome_revcomp_into(ctx, src, g.get());
    if (rc != KGMA_OK) return rc;
    return genome_finish(ctx, g, out);
}

// ------------------------------------------------------------------------------------------
// FASTA text -> device genome (ingest on the device)
// ------------------------------------------------------------------------------------------
// (fd >= 0: `text` is a mapping of that file.  The bulk of it is then read with pread() straight into the pinned staging
//  buffers -- the same single copy out of the page cache as a memcpy from the mapping, without one minor fault per 4 KiB page of
//  a mapping that is touched exactly once (400 MB of text: 17.0 -> see DESIGN section 3) -- and the mapping serves the few bytes the
//  record table needs around the header lines.)
static int genome_from_fasta_impl(kgma_ctx *ctx, const uint8_t *text, int64_t n, int fd, kgma_genome **out)
{
    if (!ctx) return KGMA_E_ARG;
    if (!out || n < 0 || (n > 0 && !text)) return ctx_fail(ctx, KGMA_E_ARG, "null argument");
    *out = nullptr;
    IngestLap lap{"ingest"};
    (void)hipSetDevice(ctx->device);
    NumaBind numa(ctx);                                              // (staging buffers and copying threads on the GPU's NUMA node)
    constexpr int64_t FB = 4096;
    // ---- upload the raw text through the staging pair, padded with '\n' to a block multiple; the threads that fill a
    //      staging buffer also look for the header lines in the stretch they have just copied (a '>' at the start of a
    //      line: the text is in their cache), so that the search costs no pass of its own.  The header lines are turned
    //      into line breaks on the device afterwards (fasta_blank_kernel) ------------------------------------------
    struct Hdr { int64_t begin, end; };            // [begin, end): from '>' to just past its '\n'
    std::vector<Hdr> hdrs;
    const int n_thr = ingest_threads();
    const int64_t nb = (n + FB - 1) / FB;
    const int64_t n_pad = std::max<int64_t>(nb, 1) * FB;
    int64_t *d_base = nullptr, *d_rs = nullptr, *d_ranges = nullptr;
    StagePipe *pipe = ctx_pipe(ctx);
    if (!pipe) return ctx_fail(ctx, KGMA_E_NOMEM, "cannot allocate the pinned staging buffers");
    int rc = dev_reserve(ctx, ctx->genome.d_ingest, ctx->genome.ingest_cap, n_pad);
    if (rc) return rc;
    rc = dev_reserve(ctx, ctx->genome.d_icounts, ctx->genome.icounts_cap, std::max<int64_t>(nb, 1));
    if (rc) return rc;
    uint8_t *d_raw = ctx->genome.d_ingest;
    std::optional<IngestScratch> scratch;
    scratch.emplace(ctx, *pipe, true);
    lap("scratch + staging");
    {
        // (file: pread into the staging buffer.  Measured against the alternatives on a 400 MB file in the page cache:
        //  memcpy from the mapping with a fault per page 17.0 ms per ingest, pread 13.7, MADV_POPULATE_READ of the
        //  stretch + memcpy 14.8 -- KGMA_INGEST_POPULATE=1 keeps the last one reachable)
        const bool from_mapping = fd < 0 || getenv("KGMA_INGEST_POPULATE");
        std::vector<StageSeg> segs;
        if (n > 0) segs.push_back(StageSeg{0, n, from_mapping ? text : nullptr, fd, 0});
        // header lines found by thread t in the window at device byte w0: found[w0 / window * n_thr + t], in text order
        const int64_t window = (int64_t)pipe->cap;
        std::vector<std::vector<Hdr>> found((size_t)((n_pad + window - 1) / window) * (size_t)n_thr);
        const RangeHook search = [&](int t, const uint8_t *stage, int64_t off, int64_t b0, int64_t e0) {
            std::vector<Hdr> &mine = found[(size_t)(off / window) * (size_t)n_thr + (size_t)t];
            const uint8_t *p = stage + b0, *e = stage + e0;
            while (p < e) {
                const uint8_t *q = static_cast<const uint8_t *>(memchr(p, '>', (size_t)(e - p)));
                if (!q) break;
                const int64_t pos = off + (q - stage);                   // position in the text
                if (pos == 0 || text[pos - 1] == '\n') {
                    const uint8_t *nl = static_cast<const uint8_t *>(memchr(text + pos, '\n', (size_t)(n - pos)));
                    const int64_t he = nl ? (nl - text) + 1 : n;
                    mine.push_back(Hdr{pos, he});
                    if (he >= off + e0) break;                            // (the line runs past this thread's stretch)
                    p = stage + (he - off);
                } else {
                    p = q + 1;
                }
            }
        };
        const int up = staged_upload(*pipe, d_raw, n_pad, segs, '\n', (int64_t)2 << 20, search);
        if (up == UPLOAD_UNREAD) return ctx_fail(ctx, KGMA_E_ARG, "cannot read the FASTA file");
        if (up) return fail(ctx, KGMA_E_HIP, "pipe.submit(d_raw + off, (size_t)len) failed: %s", hipGetErrorString((hipError_t)up));
        int64_t hdr_done = 0;                              // text before this offset belongs to a header line already found
        for (const std::vector<Hdr> &f : found)
            for (const Hdr &h : f)
                if (h.begin >= hdr_done) { hdrs.push_back(h); hdr_done = h.end; }   // (a '>' inside a header line found earlier is text)
    }
    lap("staged upload + header search");
    const int64_t n_rec = (int64_t)hdrs.size();
    if (n_rec > 0x7FFFFFF0ll) return ctx_fail(ctx, KGMA_E_UNSUPPORTED, "too many records");
    {
        const int64_t lead = n_rec > 0 ? hdrs[0].begin : n;
        for (int64_t i = 0; i < lead; i++)
            if (text[i] > 0x20) return ctx_fail(ctx, KGMA_E_ARG, "FASTA text has sequence data before the first '>' header");
    }
    if (n_rec > 0) {
        static_assert(sizeof(Hdr) == 16, "header ranges are uploaded as int64 pairs");
        HIP_TRY(ctx, scratch->alloc(d_ranges, (size_t)n_rec * 2));
        HIP_TRY(ctx, hipMemcpyAsync(d_ranges, hdrs.data(), (size_t)n_rec * sizeof(Hdr), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, launch_fasta_blank(d_raw, d_ranges, (int)n_rec, ctx->stream));
    }
    // ---- kernel 1: residues per block; host prefix sum -> block bases --------------------------
    HIP_TRY(ctx, launch_fasta_count(d_raw, n_pad, ctx->genome.d_icounts, ctx->stream));
    std::vector<uint32_t> counts((size_t)std::max<int64_t>(nb, 1), 0);
    HIP_TRY(ctx, hipMemcpyAsync(counts.data(), ctx->genome.d_icounts, (size_t)std::max<int64_t>(nb, 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    lap("upload drained + count kernel");
    std::vector<int64_t> base((size_t)std::max<int64_t>(nb, 1) + 1, 0);
    for (int64_t b = 0; b < nb; b++) base[(size_t)b + 1] = base[(size_t)b] + counts[(size_t)b];
    const int64_t total_res = nb > 0 ? base[(size_t)nb] : 0;
    // residue index of each record's first residue = residues before its header line
    auto residues_before = [&](int64_t pos) -> int64_t {   // pos is a header start: bytes [blk, pos) hold no header tail
        const int64_t blk = pos / FB;
        int64_t c = base[(size_t)blk];
        size_t h = 0;
        // count residues in [blk*FB, pos) skipping header bytes (a header may start before the block)
        int64_t i = blk * FB;
        // binary search the first header ending after i
        {
            size_t lo = 0, hi2 = hdrs.size();
            while (lo < hi2) { const size_t mid = (lo + hi2) / 2; if (hdrs[mid].end <= i) lo = mid + 1; else hi2 = mid; }
            h = lo;
        }
        while (i < pos) {
            if (h < hdrs.size() && i >= hdrs[h].begin && i < hdrs[h].end) { i = hdrs[h].end; h++; continue; }
            const int64_t stop = (h < hdrs.size() && hdrs[h].begin < pos) ? hdrs[h].begin : pos;
            for (; i < stop; i++) c += text[i] > 0x20;
        }
        return c;
    };
    std::vector<int64_t> rs((size_t)n_rec + 1, 0), lens((size_t)std::max<int64_t>(n_rec, 1), 0);
    for (int64_t c = 0; c < n_rec; c++) rs[(size_t)c] = residues_before(hdrs[(size_t)c].begin);
    rs[(size_t)n_rec] = total_res;
    for (int64_t c = 0; c < n_rec; c++) lens[(size_t)c] = rs[(size_t)c + 1] - rs[(size_t)c];
    lap("record table (host)");
    // ---- layout, kernel 2 (scatter), pack ---------------------------------------------------------
    GenomeOwner g;
    rc = genome_begin(ctx, lens.data(), n_rec, g);
    if (rc != KGMA_OK) return rc;
    g->headers.resize((size_t)n_rec);
    for (int64_t c = 0; c < n_rec; c++) {
        int64_t b = hdrs[(size_t)c].begin + 1, e = hdrs[(size_t)c].end;
        while (e > b && (text[e - 1] == '\n' || text[e - 1] == '\r')) e--;
        g->headers[(size_t)c].assign(reinterpret_cast<const char *>(text + b), (size_t)(e - b));
    }
    if (n_rec > 0) {
        HIP_TRY(ctx, scratch->alloc(d_base, base.size()));
        HIP_TRY(ctx, scratch->alloc(d_rs, rs.size()));
        HIP_TRY(ctx, hipMemcpy(d_base, base.data(), base.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(d_rs, rs.data(), rs.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemsetAsync(g->d_ascii, 0, (size_t)g->ascii_bytes, ctx->stream));
        HIP_TRY(ctx, launch_fasta_scatter(d_raw, n_pad, d_base, d_rs, g->d_cd, (int)n_rec, g->d_ascii, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    lap("layout + scatter kernel");
    scratch.reset();
    lap("free scratch");
    rc = genome_finish(ctx, g, out);
    lap("pack launched");
    return rc;
}

int kgma_genome_from_fasta(kgma_ctx *ctx, const uint8_t *text, int64_t n, kgma_genome **out)
{
    return genome_from_fasta_impl(ctx, text, n, -1, out);
}

int kgma_genome_from_fasta_file(kgma_ctx *ctx, const char *path, kgma_genome **out)
{
    if (!ctx) return KGMA_E_ARG;
    if (!path || !out) return ctx_fail(ctx, KGMA_E_ARG, "null argument");
    *out = nullptr;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(ctx, KGMA_E_ARG, "cannot open %s", path);
    struct stat sb;
    if (fstat(fd, &sb) != 0 || sb.st_size < 0) { close(fd); return fail(ctx, KGMA_E_ARG, "cannot stat %s", path); }
    if (!S_ISREG(sb.st_mode)) { close(fd); return fail(ctx, KGMA_E_ARG, "%s is not a regular file (pipes are not read: pass the text to kgma_genome_from_fasta)", path); }
    const int64_t n = (int64_t)sb.st_size;
    if (n == 0) { close(fd); return genome_from_fasta_impl(ctx, nullptr, 0, -1, out); }
    void *map = mmap(nullptr, (size_t)n, PROT_READ, MAP_PRIVATE, fd, 0);
    if (map == MAP_FAILED) { close(fd); return fail(ctx, KGMA_E_ARG, "cannot map %s", path); }
    const int rc = genome_from_fasta_impl(ctx, static_cast<const uint8_t *>(map), n, fd, out);
    (void)munmap(map, (size_t)n);
    close(fd);
    return rc;
}

// ------------------------------------------------------------------------------------------
// .2bit file -> device genome (parser: kgma_twobit.cpp, kernel: kgma_twobit.hip)
// ------------------------------------------------------------------------------------------
int kgma_genome_from_2bit_file(kgma_ctx *ctx, const char *path, uint32_t flags, kgma_genome **out)
{
    if (!ctx) return KGMA_E_ARG;
    if (!path || !out) return ctx_fail(ctx, KGMA_E_ARG, "null argument");
    *out = nullptr;
    if (flags & ~(uint32_t)KGMA_2BIT_NOMASK) return fail(ctx, KGMA_E_ARG, "kgma_genome_from_2bit_file: unknown flags 0x%x", flags);
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(ctx, KGMA_E_ARG, "cannot open %s", path);
    struct FdGuard { int fd; ~FdGuard() { close(fd); } } fd_guard{fd};
    struct stat sb;
    if (fstat(fd, &sb) != 0 || sb.st_size < 0) return fail(ctx, KGMA_E_ARG, "cannot stat %s", path);
    if (!S_ISREG(sb.st_mode)) return fail(ctx, KGMA_E_ARG, "%s is not a regular file", path);
    IngestLap lap{"2bit ingest"};
    // ---- the host reads and validates header, index and block tables: nothing below indexes with a value it has not checked ----
    TwoBitFile f;
    {
        std::string msg;
        const int prc = twobit_parse(fd, (int64_t)sb.st_size, TWOBIT_MAX_RECORDS, f, msg);
        if (prc != KGMA_OK) return fail(ctx, prc, "%s: %s", path, msg.c_str());
    }
    lap("parse + validate (host)");
    const int64_t nc = (int64_t)f.recs.size();
    const bool masks = !(flags & KGMA_2BIT_NOMASK);
    const int64_t n_nblk = (int64_t)f.n_blocks.size(), n_mblk = masks ? (int64_t)f.m_blocks.size() : 0;
    static_assert(sizeof(TwoBitBlock) == sizeof(TwobitBlock) && sizeof(TwobitBlock) == 8, "the parser's blocks are uploaded as the kernel's");
    std::vector<int64_t> lens((size_t)std::max<int64_t>(nc, 1), 0);
    for (int64_t c = 0; c < nc; c++) lens[(size_t)c] = f.recs[(size_t)c].dna_size;
    // one table of int64 for the kernel: [tile_prefix: nc + 1][packed_off: nc][n_prefix: nc + 1][m_prefix: nc + 1]
    std::vector<int64_t> tab((size_t)(4 * nc + 3), 0);
    int64_t *tile_prefix_ = tab.data(), *packed_off = tile_prefix_ + (nc + 1), *n_prefix = packed_off + nc, *m_prefix = n_prefix + (nc + 1);
    {
        const std::vector<int64_t> prefix = tile_prefix(nc, twobit_tile_bytes(), true, [&](int64_t c) { return lens[(size_t)c]; });   // (the kernel writes all of a record's slot)
        std::copy(prefix.begin(), prefix.end(), tile_prefix_);
    }
    int64_t packed_total = 0;
    for (int64_t c = 0; c < nc; c++) {
        const TwoBitRecord &R = f.recs[(size_t)c];
        packed_off[c] = packed_total;                                   // 16-byte aligned, whatever the byte it starts at in the file
        packed_total += (R.packed_bytes + 15) & ~15ll;
        n_prefix[c] = R.n_begin;
        m_prefix[c] = n_nblk + (masks ? R.m_begin : 0);
    }
    n_prefix[nc] = n_nblk;
    m_prefix[nc] = n_nblk + n_mblk;
    const int64_t n_tiles = tile_prefix_[nc];
    if (n_tiles > 0x7FFFFFFFll) return fail(ctx, KGMA_E_UNSUPPORTED, "kgma_genome_from_2bit_file: %lld tiles exceed one launch", (long long)n_tiles);
    (void)hipSetDevice(ctx->device);
    NumaBind numa(ctx);                                              // (staging buffers and reading threads on the GPU's NUMA node)
    StagePipe *pipe = ctx_pipe(ctx);
    if (!pipe) return ctx_fail(ctx, KGMA_E_NOMEM, "cannot allocate the pinned staging buffers");
    GenomeOwner g;
    int rc = genome_begin(ctx, lens.data(), nc, g);
    if (rc != KGMA_OK) return rc;
    g->headers.resize((size_t)nc);
    for (int64_t c = 0; c < nc; c++) g->headers[(size_t)c] = f.recs[(size_t)c].name;
    lap("layout (genome allocations)");
    // ONE transient device buffer, freed once the kernel is done: [table][N blocks][mask blocks][packed bytes, every record at a
    // 16-byte aligned offset].  It is filled as one byte stream through the pinned staging pair: the host's tables are copied,
    // the packed bytes are pread straight from the file, the gaps are zeros.
    std::vector<StageSeg> segs;
    const int64_t tab_bytes = (int64_t)(tab.size() * sizeof(int64_t));
    const int64_t blk_off = (tab_bytes + 15) & ~15ll;
    const int64_t packed_base = (blk_off + (n_nblk + n_mblk) * (int64_t)sizeof(TwobitBlock) + 15) & ~15ll;
    const int64_t buf_bytes = std::max<int64_t>(packed_base + packed_total, 16);
    segs.push_back(StageSeg{0, tab_bytes, reinterpret_cast<const uint8_t *>(tab.data()), -1, 0});
    if (n_nblk > 0) segs.push_back(StageSeg{blk_off, n_nblk * 8, reinterpret_cast<const uint8_t *>(f.n_blocks.data()), -1, 0});
    if (n_mblk > 0) segs.push_back(StageSeg{blk_off + n_nblk * 8, n_mblk * 8, reinterpret_cast<const uint8_t *>(f.m_blocks.data()), -1, 0});
    for (int64_t c = 0; c < nc; c++)
        if (f.recs[(size_t)c].packed_bytes > 0)
            segs.push_back(StageSeg{packed_base + packed_off[c], f.recs[(size_t)c].packed_bytes, nullptr, fd, f.recs[(size_t)c].packed_off});
    std::optional<IngestScratch> scratch;
    scratch.emplace(ctx, *pipe, false);
    uint8_t *d_buf = nullptr;
    hipEvent_t &e0 = scratch->ev[0], &e1 = scratch->ev[1];
    HIP_TRY(ctx, scratch->alloc(d_buf, (size_t)buf_bytes));
    HIP_TRY(ctx, hipEventCreate(&e0));
    HIP_TRY(ctx, hipEventCreate(&e1));
    lap("transient buffer");
    const int up = staged_upload(*pipe, d_buf, buf_bytes, segs, 0, (int64_t)1 << 20);
    if (up == UPLOAD_UNREAD) return fail(ctx, KGMA_E_ARG, "cannot read the packed bases of %s", path);
    if (up) return fail(ctx, KGMA_E_HIP, "pipe.submit(d_buf + w0, (size_t)len) failed: %s", hipGetErrorString((hipError_t)up));
    lap("staged upload queued");
    // ---- kernel, tail ----
    const int64_t *d_tab = reinterpret_cast<const int64_t *>(d_buf);
    const uint8_t *d_packed = d_buf + packed_base;
    const TwobitBlock *d_blk = reinterpret_cast<const TwobitBlock *>(d_buf + blk_off);
    TwobitArgs a{};
    a.packed = d_packed; a.dst = g->d_ascii; a.cd = g->d_cd;
    a.tile_prefix = d_tab; a.packed_off = d_tab + (nc + 1); a.n_prefix = d_tab + (2 * nc + 1); a.m_prefix = d_tab + (3 * nc + 2);
    a.blk = d_blk; a.n_contigs = (int32_t)nc;
    HIP_TRY(ctx, hipEventRecord(e0, ctx->stream));
    HIP_TRY(ctx, launch_twobit_unpack(a, n_tiles, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(e1, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(g->d_ascii + (g->ascii_bytes - 64), 0, 64, ctx->stream));              // the text's 64 tail bytes
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    {
        float ms = 0;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, e0, e1));
        ctx->genome.twobit_ms = n_tiles > 0 ? ms : 0.0;
    }
    lap("upload drained + kernel");
    scratch.reset();
    lap("free transients");
    rc = genome_finish(ctx, g, out);
    lap("pack launched");
    return rc;
}

int kgma_get_2bit_unpack_ms(kgma_ctx *ctx, double *ms)
{
    if (!ctx) return KGMA_E_ARG;
    if (!ms) return ctx_fail(ctx, KGMA_E_ARG, "null argument");
    const double last = ctx->genome.twobit_ms;
    if (last < 0) return ctx_fail(ctx, KGMA_E_STATE, "kgma_get_2bit_unpack_ms: no kgma_genome_from_2bit_file has completed on this context");
    *ms = last;
    return KGMA_OK;
}

int kgma_genome_header(const kgma_genome *g, int64_t contig, const char **text, int64_t *len)
{
    if (!g || !text || !len || contig < 0 || contig >= g->n_contigs || (size_t)contig >= g->headers.size()) return KGMA_E_ARG;
    *text = g->headers[(size_t)contig].c_str();
    *len = (int64_t)g->headers[(size_t)contig].size();
    return KGMA_OK;
}

int kgma_genome_fetch(kgma_ctx *ctx, const kgma_genome *g, int64_t contig, int64_t pos, int64_t len, uint8_t *outp)
{
    if (!ctx || !g) return KGMA_E_ARG;
    if (contig < 0 || contig >= g->n_contigs || pos < 1 || len < 0 || pos + len - 1 > g->cd[(size_t)contig].len || (!outp && len > 0))
        return ctx_fail(ctx, KGMA_E_ARG, "kgma_genome_fetch: range outside the record");
    if (len == 0) return KGMA_OK;
    (void)hipSetDevice(ctx->device);
    HIP_TRY(ctx, hipMemcpy(outp, g->d_ascii + g->cd[(size_t)contig].ascii_off + (pos - 1), (size_t)len, hipMemcpyDeviceToHost));
    return KGMA_OK;
}

int kgma_genome_poke(kgma_ctx *ctx, kgma_genome *g, int64_t contig, int64_t pos, int64_t len, const uint8_t *bytes)
{
    if (!ctx || !g) return KGMA_E_ARG;
    if (contig < 0 || contig >= g->n_contigs || pos < 1 || len < 0 || pos + len - 1 > g->cd[(size_t)contig].len || (!bytes && len > 0))
        return ctx_fail(ctx, KGMA_E_ARG, "kgma_genome_poke: range outside the record");
    if (len == 0) return KGMA_OK;
    (void)hipSetDevice(ctx->device);
    if (g->bsum_state == KGMA_BSUM_DEFERRED) {                         // (so do the block sums)
        const int brc = ensure_bsum(ctx, g, false);
        if (brc) return brc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (g->inter_state != KGMA_INTER_FULL) {
        // the 2-bit copy stays the text as of the last pack: completed, to the end, before the text changes (the copy below does
        // not wait for the context's stream)
        const int irc = ensure_inter(ctx, g);
        if (irc) return irc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    HIP_TRY(ctx, hipMemcpy(g->d_ascii + g->cd[(size_t)contig].ascii_off + (pos - 1), bytes, (size_t)len, hipMemcpyHostToDevice));
    g->text_dirty = true;
    return KGMA_OK;
}

int kgma_genome_inter_state(const kgma_genome *g, int32_t *state, int64_t *demand_blocks)
{
    if (!g) return KGMA_E_ARG;
    if (state) *state = g->inter_state;
    if (demand_blocks) *demand_blocks = g->inter_demand_blocks;
    return KGMA_OK;
}

int64_t kgma_genome_num_contigs(const kgma_genome *g) { return g ? g->n_contigs : 0; }
int64_t kgma_genome_contig_len(const kgma_genome *g, int64_t c)
{
    return (g && c >= 0 && c < g->n_contigs) ? g->cd[(size_t)c].len : -1;
}
int64_t kgma_genome_total_bases(const kgma_genome *g) { return g ? g->total_bases : 0; }

void kgma_genome_free(kgma_ctx *ctx, kgma_genome *g)
{
    if (!g) return;
    if (ctx) (void)hipSetDevice(ctx->device);
    for (void *p : {(void *)g->d_ascii, (void *)g->d_planes, (void *)g->d_inter, (void *)g->d_cd, (void *)g->d_first_bad, (void *)g->d_block_contig, (void *)g->d_bsum, (void *)g->d_bsum_S})
        if (p) (void)hipFree(p);
    if (g->first_bad) (void)hipHostFree(g->first_bad);
    if (ctx && ctx->tk_uid == g->uid) ctx->tk_uid = 0;
    delete g;
}

}  // extern "C"

extern "C" {

int kgma_genome_fetch_batch(kgma_ctx *ctx, const kgma_genome *g, int64_t n, const int64_t *contig, const int64_t *pos,
                            const int64_t *len, uint8_t *outp, int64_t out_cap)
{
    if (!ctx || !g) return KGMA_E_ARG;
    if (n < 0 || (n > 0 && (!contig || !pos || !len))) return fail(ctx, KGMA_E_ARG, "kgma_genome_fetch_batch: null argument");
    if (n > 0x7FFFFFF0ll) return fail(ctx, KGMA_E_UNSUPPORTED, "kgma_genome_fetch_batch: too many ranges");
    std::vector<int64_t> desc;
    desc.reserve((size_t)n * 3);
    int64_t total = 0;
    for (int64_t i = 0; i < n; i++) {
        const int64_t c = contig[i];
        if (c < 0 || c >= g->n_contigs || pos[i] < 1 || len[i] < 0 || pos[i] + len[i] - 1 > g->cd[(size_t)c].len)
            return fail(ctx, KGMA_E_ARG, "kgma_genome_fetch_batch: range %lld outside its record", (long long)i);
        if (len[i] == 0) continue;
        desc.push_back(g->cd[(size_t)c].ascii_off + (pos[i] - 1));
        desc.push_back(total);
        desc.push_back(len[i]);
        total += len[i];
    }
    if (total > out_cap || (total > 0 && !outp)) return fail(ctx, KGMA_E_ARG, "kgma_genome_fetch_batch: output buffer too small (%lld bytes needed)", (long long)total);
    if (total == 0) return KGMA_OK;
    (void)hipSetDevice(ctx->device);
    // one gather kernel into a staging buffer + one download (the tie resolver's buffers)
    const size_t desc_bytes = (desc.size() * sizeof(int64_t) + 255) & ~(size_t)255;
    const size_t need = desc_bytes + (size_t)total;
    if (need > ctx->gath_cap) {
        if (ctx->h_gath) (void)hipHostFree(ctx->h_gath);
        if (ctx->d_gath) (void)hipFree(ctx->d_gath);
        ctx->h_gath = ctx->d_gath = nullptr; ctx->gath_cap = 0;
        const size_t cap = need + (need >> 1) + 65536;
        HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->h_gath), cap, hipHostMallocDefault));
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_gath), cap));
        ctx->gath_cap = cap;
    }
    memcpy(ctx->h_gath, desc.data(), desc.size() * sizeof(int64_t));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_gath, ctx->h_gath, desc_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, launch_gather_ranges(g->d_ascii, reinterpret_cast<const int64_t *>(ctx->d_gath), (int)(desc.size() / 3), ctx->d_gath + desc_bytes, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_gath + desc_bytes, ctx->d_gath + desc_bytes, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, sync_spin(ctx->stream));
    memcpy(outp, ctx->h_gath + desc_bytes, (size_t)total);
    return KGMA_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// scan: device part
// ------------------------------------------------------------------------------------------
namespace {

// Two integer distances D of KFV `f` that rounding noise may order either way.  S/N KFVs: exact arithmetic, only equal values tie.
// Float64 KFVs (f.fp): the device's values and the reference's running value each carry a relative error far below 2^-31, so
// values within 2^-30 of each other are treated as tied (flagged; the chain replay decides them).
inline int64_t tie_tol(const KfvInfo &f, int64_t D) { return f.fp ? (int64_t)((double)(D < 0 ? -D : D) * 9.313225746154785e-10 /* 2^-30 */) + 2 : 0; }
inline bool near_tie(const KfvInfo &f, int64_t a, int64_t b)
{
    const int64_t d = a > b ? a - b : b - a;
    return d <= tie_tol(f, std::max(a, b));
}
// a Float64 distance on the host's integer lattice D = round(d * 2kN^2)
inline int64_t lattice_of(const KfvInfo &f, int k, double d) { return (int64_t)std::llround(d * 2.0 * (double)k * (double)f.N * (double)f.N); }

struct Frag {             // one device record in global coordinates
    int32_t contig, kfv;  // kfv 0-based
    int32_t kind;
    int64_t start, end;   // 1-based window starts
    int64_t minD, exitD;
    int64_t argf, argl;
    int64_t nmin;
    bool has_exit;
    int64_t aux;          // byte offset of the residues under [argf, argl + W) in the aux region, or -1
};

int stitch_dips(kgma_ctx *ctx, const std::vector<DevRecord> &recs)
{
    // (a filtered scan ran over the candidate stream table: streams of any length at 64-window boundaries, sorted by record and window)
    const std::vector<TileDesc> &tiles = ctx->scan_filtered ? ctx->ftiles : ctx->tiles;
    const int64_t n_tiles = (int64_t)tiles.size();
    const int64_t P = ctx->tile_windows;
    std::vector<Frag> fr;
    fr.reserve(recs.size());
    for (const DevRecord &r : recs) {
        if (r.tile < 0 || r.tile >= n_tiles) return fail(ctx, KGMA_E_HIP, "corrupt device record (tile %d)", r.tile);
        const TileDesc &td = tiles[(size_t)r.tile];
        const int kfv = (r.kind_kfv >> 8) - 1;
        if (kfv < 0 || kfv >= ctx->m) return fail(ctx, KGMA_E_HIP, "corrupt device record (kfv %d)", kfv + 1);
        const int64_t D0 = ctx->D0[(size_t)kfv * (size_t)n_tiles + (size_t)r.tile];
        const KfvInfo &kf = ctx->kfv[(size_t)kfv];
        const int64_t twoN = 2 * kf.N;
        Frag f;
        f.contig = td.contig; f.kfv = kfv; f.kind = r.kind_kfv & REC_KIND_MASK;
        if (f.kind == REC_FAULT) return fail(ctx, KGMA_E_HIP, "internal: the scan kernel gave up on stream %d (hash table of the window's k-mers)", r.tile);
        f.start = td.win0 + r.start; f.end = td.win0 + r.end;
        if (r.kind_kfv & REC_WIDE) {
            // 64-bit values: an int64 prefix E, or (Float64 KFV) the distance itself
            const int64_t mv = (int64_t)(((uint64_t)(uint32_t)r.minE_hi << 32) | (uint32_t)r.minE);
            const int64_t xv = (int64_t)(((uint64_t)(uint32_t)r.exitE_hi << 32) | (uint32_t)r.exitE);
            if (kf.fp) {
                double md, xd;
                memcpy(&md, &mv, sizeof md); memcpy(&xd, &xv, sizeof xd);
                f.minD = lattice_of(kf, ctx->k, md); f.exitD = lattice_of(kf, ctx->k, xd);
            } else {
                f.minD = D0 + twoN * mv; f.exitD = D0 + twoN * xv;
            }
        } else {
            if (kf.fp) return fail(ctx, KGMA_E_HIP, "corrupt device record (int32 values for a Float64 KFV)");
            f.minD = D0 + twoN * (int64_t)r.minE;
            f.exitD = D0 + twoN * (int64_t)r.exitE;
        }
        f.argf = td.win0 + r.argf; f.argl = td.win0 + r.argl;
        f.nmin = r.nmin; f.has_exit = (r.has_exit & 1) != 0;
        f.aux = (r.has_exit >> 1) > 0 ? (int64_t)((r.has_exit >> 1) - 1) * 16 : -1;
        fr.push_back(f);
    }
    std::sort(fr.begin(), fr.end(), [](const Frag &a, const Frag &b) {
        if (a.contig != b.contig) return a.contig < b.contig;
        if (a.kfv != b.kfv) return a.kfv < b.kfv;
        if (a.start != b.start) return a.start < b.start;
        return a.kind < b.kind;
    });
    ctx->dips.clear();
    ctx->dip_argl.clear();
    ctx->dip_aux.clear();
    ctx->att.clear();
    ctx->chain_pair.clear();
    ctx->firstF.clear();
    ctx->dip_fmin.clear();
    ctx->dip_fexit.clear();
    for (const Frag &f : fr)                                   // (sorted by record, KFV, window)
        if (f.kind == REC_ATT) ctx->att.push_back(kgma_ctx::AttWin{f.contig, f.kfv, f.start});
    int64_t n_tie = 0;
    size_t i = 0;
    const size_t n = fr.size();
    // positions (contig,kfv) -> set of ATT positions for flagging
    auto att_at = [&](int32_t contig, int32_t kfv, int64_t pos) -> bool {
        Frag key; key.contig = contig; key.kfv = kfv; key.start = pos; key.kind = REC_ATT;
        auto it = std::lower_bound(fr.begin(), fr.end(), key, [](const Frag &a, const Frag &b) {
            if (a.contig != b.contig) return a.contig < b.contig;
            if (a.kfv != b.kfv) return a.kfv < b.kfv;
            if (a.start != b.start) return a.start < b.start;
            return a.kind < b.kind;
        });
        return it != fr.end() && it->contig == contig && it->kfv == kfv && it->start == pos && it->kind == REC_ATT;
    };
    while (i < n) {
        if (fr[i].kind != REC_RUN) { i++; continue; }
        Frag cur = fr[i];
        size_t jx = i + 1;
        // merge fragments that continue the run (skipping EXIT/ATT records in between is not
        // needed: a continuing RUN starts exactly at cur.end + 1)
        while (true) {
            size_t nx = jx;
            while (nx < n && fr[nx].contig == cur.contig && fr[nx].kfv == cur.kfv && fr[nx].kind != REC_RUN && fr[nx].start <= cur.end + 1) nx++;
            if (!cur.has_exit && nx < n && fr[nx].kind == REC_RUN && fr[nx].contig == cur.contig && fr[nx].kfv == cur.kfv &&
                fr[nx].start == cur.end + 1) {
                const Frag &b = fr[nx];
                const KfvInfo &kf = ctx->kfv[(size_t)cur.kfv];
                if (kf.fp && near_tie(kf, b.minD, cur.minD)) {                                          // (Float64 KFV: a near tie across fragments)
                    if (b.minD < cur.minD) { cur.minD = b.minD; cur.argf = b.argf; }
                    cur.argl = b.argl; cur.nmin += b.nmin; cur.aux = -1;
                }
                else if (b.minD < cur.minD) { cur.minD = b.minD; cur.argf = b.argf; cur.argl = b.argl; cur.nmin = b.nmin; cur.aux = b.aux; }
                else if (b.minD == cur.minD) { cur.argl = b.argl; cur.nmin += b.nmin; cur.aux = -1; }   // tied stretch spans fragments
                cur.end = b.end; cur.has_exit = b.has_exit; cur.exitD = b.exitD;
                jx = nx + 1;
            } else break;
        }
        kgma_dip d;
        memset(&d, 0, sizeof d);
        d.contig = cur.contig; d.kfv = cur.kfv + 1;
        d.start = cur.start; d.end = cur.end; d.argmin = cur.argf; d.D_min = cur.minD;
        const int64_t nwin = ctx->contig_nwin[(size_t)cur.contig];
        if (cur.has_exit) { d.exit_pos = cur.end + 1; d.D_exit = cur.exitD; }
        else if (cur.end + 1 <= nwin) {
            // exit window lies in another lane / tile: an EXIT record, or the next tile's D0
            const int64_t e = cur.end + 1;
            bool found = false;
            for (size_t u = i; u < n && fr[u].contig == cur.contig && fr[u].kfv == cur.kfv && fr[u].start <= e; u++)
                if (fr[u].kind == REC_EXIT && fr[u].start == e) { d.exit_pos = e; d.D_exit = fr[u].exitD; found = true; break; }
            if (!found) {
                int64_t t = -1;
                if (ctx->scan_filtered) {
                    // the candidate stream that starts at the exit window: a region cut into consecutive streams (every dip
                    // closes inside its region)
                    const auto it = std::lower_bound(tiles.begin(), tiles.end(), std::make_pair((int32_t)cur.contig, e), [](const TileDesc &a, const std::pair<int32_t, int64_t> &b) {
                        return a.contig != b.first ? a.contig < b.first : a.win0 < b.second;
                    });
                    if (it != tiles.end() && it->contig == cur.contig && it->win0 == e) t = (int64_t)(it - tiles.begin());
                } else if ((e - 1) % P == 0) {
                    t = ctx->contig_tile_base[(size_t)cur.contig] + (e - 1) / P;
                }
                if (t < 0) return fail(ctx, KGMA_E_HIP, "internal: dip exit at window %lld of record %d not found", (long long)e, cur.contig);
                d.exit_pos = e;
                d.D_exit = ctx->D0[(size_t)cur.kfv * (size_t)n_tiles + (size_t)t];
            }
        }
        // several windows attain the minimum: separated ones always need the Float64 replay; a contiguous
        // plateau only when N is not a power of two (ref = S/N is then inexact and the reference's
        // mathematically-zero increments are +-1 ulp noise; with dyadic ref they are exactly 0)
        const int64_t Nk = ctx->kfv[(size_t)cur.kfv].N;
        // (Float64 KFV: the device counts the windows within 2^-30 of the minimum, one per plateau of bitwise equal values)
        if (cur.nmin > 1 && (ctx->kfv[(size_t)cur.kfv].fp || cur.nmin != cur.argl - cur.argf + 1 || (Nk & (Nk - 1)) != 0)) { d.flags |= KGMA_HIT_TIE; n_tie++; }
        if ((d.exit_pos && d.D_exit <= ctx->kfv[(size_t)cur.kfv].T_hi) || att_at(cur.contig, cur.kfv, cur.start - 1))
            d.flags |= KGMA_HIT_AT_THRESHOLD;
        ctx->dips.push_back(d);
        ctx->dip_argl.push_back(cur.argl);
        ctx->dip_aux.push_back(cur.aux);
        i = jx > i ? jx : i + 1;
    }
    ctx->stats.n_dips = (int64_t)ctx->dips.size();
    ctx->stats.n_tie_flagged = n_tie;
    return KGMA_OK;
}

}  // namespace

// ---- pack / scan overlap of a step (kgma_repack_scan_hits) ---------------------------------------------------------------------
// The step's two big kernels are complementary: the pack kernel is HBM-bound (0.71 of the peak on the whole chip), the scan
// kernel moves 2 % of the HBM peak and keeps every wave slot and the whole LDS of the CUs it runs on -- so a pack launched beside
// it on an ordinary stream only runs in its gaps (EXPERIMENTS.md).  Here the records are cut into groups; group 0 is packed on the
// whole chip, every later group on a stream masked to a few CUs (hipExtStreamCreateWithCUMask: two or three per XCD are enough to
// re-encode at the pace of the scan) WHILE the previous group is scanned on streams masked to the other CUs; the scan launches
// alternate between two such streams so that one launch's last round overlaps the next one's first.
static bool overlap_setup(kgma_ctx *ctx)
{
    if (ctx->ov_cus != 0) return ctx->ov_cus > 0;
    ctx->ov_cus = -1;
    // OFF unless KGMA_OVERLAP=1: measured on the 100 Gb bench genome it does not pay -- sequential 172.6 ms per step (pack 22.0 on
    // the whole chip + scan 142.0), overlapped with 24 CUs for the pack 176.9 ms, with 16 CUs 233.6 ms (the pack then needs 205 ms
    // and the scans wait for it).  The pack costs ~3800 CU-ms wherever it runs (0.53 TB/s on 16 CUs, 0.78 on 24), i.e. >= 15 ms of
    // the whole chip against the 22 ms it takes alone, so at most 7 ms could be hidden, and the scan beside it loses more than
    // that to the CUs it gives up for its whole duration and to the pack's L2 / HBM traffic.  Kept for tests and other devices.
    {
        const char *e = getenv("KGMA_OVERLAP");
        if (!(e && atoi(e) == 1)) return false;
    }
    if (ctx->n_cus != 256) return false;                               // (the mask layout below is the MI355X's in SPX mode)
    int R = 16;                                                        // (16 CUs re-encode 100 Gb in ~125 ms, the other 240 scan it in ~150)
    if (const char *e = getenv("KGMA_OVERLAP_CUS")) R = atoi(e);
    if (R < 8 || R > 128 || R % 8 != 0) return false;                  // (bit i of the mask is CU i / 8 of XCD i % 8: whole rows keep the XCDs even)
    uint32_t pm[8], sm[8];
    for (int w = 0; w < 8; w++) {
        uint32_t m = 0;
        for (int b = 0; b < 32; b++) m |= (w * 32 + b < R) ? 1u << b : 0u;
        pm[w] = m; sm[w] = ~m;
    }
    bool ok = hipExtStreamCreateWithCUMask(&ctx->ov_pack, 8, pm) == hipSuccess && hipExtStreamCreateWithCUMask(&ctx->ov_scan[0], 8, sm) == hipSuccess &&
              hipExtStreamCreateWithCUMask(&ctx->ov_scan[1], 8, sm) == hipSuccess && hipEventCreate(&ctx->ov_begin) == hipSuccess;
    for (int i = 0; ok && i < kgma_ctx::OV_MAX_GROUPS; i++)
        ok = hipEventCreate(&ctx->ov_p0[i]) == hipSuccess && hipEventCreate(&ctx->ov_p1[i]) == hipSuccess && hipEventCreate(&ctx->ov_s0[i]) == hipSuccess &&
             hipEventCreate(&ctx->ov_s1[i]) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); return false; }
    ctx->ov_cus = R;
    return true;
}

// One stream8 launch (args a0 / gp over the whole stream table of `n_tiles` streams) as G (pack, scan) pairs.  ctx->stream holds
// the step's order: everything here starts after what is queued on it and it waits for everything here at the end.
static int launch_overlapped(kgma_ctx *ctx, kgma_genome *g, const ScanArgs &a0, const GroupParams &gp, int64_t n_tiles)
{
    const int64_t nc = g->n_contigs;
    const int64_t PBW = pack_block_words();
    const int64_t total_blocks = (g->total_words + PBW - 1) / PBW;
    int G = 8;
    if (const char *e = getenv("KGMA_OVERLAP_GROUPS")) G = atoi(e);
    G = (int)std::max<int64_t>(2, std::min<int64_t>(std::min<int64_t>(G, kgma_ctx::OV_MAX_GROUPS), nc));
    // group boundaries at records, equal shares of the genome's words
    std::vector<int64_t> c_of((size_t)G + 1, nc);
    c_of[0] = 0;
    {
        int gi = 1;
        for (int64_t c = 1; c < nc && gi < G; c++)
            while (gi < G && g->cd[(size_t)c].word_off * G >= g->total_words * gi) c_of[(size_t)gi++] = c;   // (a record longer than a share: empty groups)
    }
    auto first_tile_from = [&](int64_t c) {                            // first stream of the first scanned record at or after c
        for (; c < nc; c++)
            if (ctx->contig_tile_base[(size_t)c] >= 0) return ctx->contig_tile_base[(size_t)c];
        return n_tiles;
    };
    const bool dirty = g->text_dirty;
    if (dirty) HIP_TRY(ctx, hipMemsetAsync(g->d_first_bad, 0xFF, std::max<size_t>(1, (size_t)nc) * 8, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ov_begin, ctx->stream));
    for (hipStream_t st : {ctx->ov_pack, ctx->ov_scan[0], ctx->ov_scan[1]}) HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ov_begin, 0));
    for (int gi = 0; gi < G; gi++) {
        // a pack block belongs to the group of its first word (the head of the next group that shares the block is packed with it)
        const int64_t b0 = gi == 0 ? 0 : (g->cd[(size_t)c_of[(size_t)gi]].word_off + PBW - 1) / PBW;
        const int64_t b1 = c_of[(size_t)gi + 1] >= nc ? total_blocks : (g->cd[(size_t)c_of[(size_t)gi + 1]].word_off + PBW - 1) / PBW;
        hipStream_t ps = gi == 0 ? ctx->stream : ctx->ov_pack;
        HIP_TRY(ctx, hipEventRecord(ctx->ov_p0[gi], ps));
        HIP_TRY(ctx, pack_blocks(ctx, g, b0, std::max<int64_t>(0, b1 - b0), ps));
        HIP_TRY(ctx, hipEventRecord(ctx->ov_p1[gi], ps));
    }
    for (int gi = 0; gi < G; gi++) {
        const int64_t t0 = first_tile_from(c_of[(size_t)gi]), t1 = first_tile_from(c_of[(size_t)gi + 1]);
        hipStream_t ss = ctx->ov_scan[gi & 1];
        HIP_TRY(ctx, hipStreamWaitEvent(ss, ctx->ov_p1[gi], 0));
        HIP_TRY(ctx, hipEventRecord(ctx->ov_s0[gi], ss));
        if (t1 > t0) {
            ScanArgs a = a0;
            a.tiles = a0.tiles + t0;
            a.D0out = a0.D0out + t0;                                   // (one KFV, slot 0: D0 of stream t is D0out[t])
            a.n_tiles = (int32_t)(t1 - t0);
            a.n_chunk_tiles = a.n_tiles;
            a.tile0 = (int32_t)t0;
            HIP_TRY(ctx, launch_stream(a, gp, ss));
        }
        HIP_TRY(ctx, hipEventRecord(ctx->ov_s1[gi], ss));
    }
    for (int gi = 0; gi < G; gi++) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ov_s1[gi], 0));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ov_p1[G - 1], 0));
    if (dirty) HIP_TRY(ctx, hipMemcpyAsync(g->first_bad, g->d_first_bad, std::max<size_t>(1, (size_t)nc) * 8, hipMemcpyDeviceToHost, ctx->stream));
    g->text_dirty = false;
    g->pack_pending = true;
    g->repack_deferred = false;
    g->inter_state = KGMA_INTER_FULL;                                  // (the groups' packs cover every block)
    g->inter_demand_blocks = 0;
    ctx->ov_groups = G;
    return KGMA_OK;
}

// stream8_kernel at k = 7 gathers its S values from global memory, one row of `nv` int16 slots per k-mer for all KFVs of the
// launch -- COMPACTED (kgma_device.h, ScanArgs::Sinter / Sbits): [per 32 k-mers {bitmap of the rows with a non-zero entry, 1 + number
// of such rows before them}][row 0 = zeros][the non-zero rows in k-mer order].  Built once per launch group, kept by the context.
static int sinter_tables(kgma_ctx *ctx, const std::vector<int> &kfvs, int nv, const int16_t **rows, const uint32_t **bits)
{
    const int k = ctx->k;
    const int64_t NBk = (int64_t)1 << (2 * k), n_words = NBk / 32;
    const bool compact = nv >= 8;                                            // (the kernel variants of 5-8 KFVs; narrower rows stay dense)
    std::vector<int> key = kfvs;
    key.push_back(-nv);
    auto it = ctx->sinter.find(key);
    if (it == ctx->sinter.end()) {
        std::vector<int16_t> dense((size_t)NBk * (size_t)nv, 0);
        for (size_t u = 0; u < kfvs.size(); u++)
            for (int64_t v = 0; v < NBk; v++)
                dense[(size_t)device_index_of((uint32_t)v, k) * (size_t)nv + u] = (int16_t)ctx->kfv[(size_t)kfvs[u]].S[(size_t)v];
        std::vector<uint32_t> bw((size_t)n_words * 2, 0u);
        std::vector<int16_t> packed((size_t)nv, 0);                          // row 0: all zero
        uint32_t n_rows = 1;
        if (!compact) packed = dense;                                        // (dense: the rows as they are, indexed by k-mer)
        for (int64_t w = 0; compact && w < n_words; w++) {
            uint32_t m = 0;
            bw[(size_t)w * 2 + 1] = n_rows;
            for (int b = 0; b < 32; b++) {
                const int16_t *row = &dense[(size_t)(w * 32 + b) * (size_t)nv];
                bool nz = false;
                for (int u = 0; u < nv; u++) nz = nz || row[u] != 0;
                if (!nz) continue;
                m |= 1u << b;
                packed.insert(packed.end(), row, row + nv);
                n_rows++;
            }
            bw[(size_t)w * 2] = m;
        }
        const size_t bits_bytes = bw.size() * 4, rows_bytes = packed.size() * 2;
        uint8_t *d = nullptr;
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&d), bits_bytes + rows_bytes + 64));
        if (hipMemcpy(d, bw.data(), bits_bytes, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d + bits_bytes, packed.data(), rows_bytes, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(d);
            return fail(ctx, KGMA_E_HIP, "cannot upload the interleaved S tables");
        }
        it = ctx->sinter.emplace(key, reinterpret_cast<int16_t *>(d)).first;
    }
    *bits = compact ? reinterpret_cast<const uint32_t *>(it->second) : nullptr;
    *rows = it->second + (size_t)n_words * 4;                                // (n_words x 8 bytes of bitmap entries in front)
    return KGMA_OK;
}

extern "C" {

// ---- distance-bound prefilter of the one-KFV scan (kgma_filter.hip) -------------------------------------------------------------
// D >= sumS2 - 2N sumS + N^2 n for every window (c^2 >= c, sum c = n), so only windows whose sum of S over their k-mer positions
// reaches U = ceil((sumS2 + N^2 n - Dmax) / 2N) can have D <= Dmax = max(T - 1, T_hi): the largest D anything reacts to (dips and
// their minima are below T, guard-band windows up to T_hi -- the band kgma_scan widens for a drift rescan arrives here in T / T_hi).
// The filter kernel walks the regular stream table and names the candidate GRANULES (16 window starts); the host merges them into
// regions and builds a second stream table for the exact kernel, which takes any (word_base, win0, n_valid, first_test, contig)
// streams and forms every stream's own D0:
//   * a region starts and ends on 64-window boundaries (streams start on plane words) with at least 64 windows in front of its
//     first and behind its last candidate window, clipped to the record: every dip closes inside its region, exit window
//     included, and candidate windows sit in steady steps (a stream's warm-up steps hold windows 0 ... 63 at most);
//   * regions closer than a stream's warm-up (n k-mers) are merged: walking the gap costs less than starting again;
//   * every record with windows has a region at its first window (first_test = 1): its D is kgma_get_first_window's and the
//     anchor of the chain's drift check;
//   * a region longer than the regular stream length is cut into consecutive streams (a dip across the cut is joined by
//     stitch_dips like one across two regular streams).
// Fallback to the regular table (same results): the list overflowed, more candidate streams than regular ones, or the candidate
// streams' positions (windows + warm-ups) exceed FILTER_MAX_FRACTION of the windows.  A fallback is remembered for the (genome,
// references, thresholds) triple: later scans of it skip the filter.
// FILTER_MAX_FRACTION: break-even is 1 - filter time / scan time per window, less a margin for the short streams' warm-ups and
// uneven lengths.  FILTER_MIN_WINDOWS: small genomes keep the plain scan -- the filter adds a launch and a host round trip to a step
// of a fraction of a millisecond (KGMA_FILTER_MIN_WINDOWS overrides it: tests run the filter on small genomes).  Both values and
// what they rest on: EXPERIMENTS.md section 12.
constexpr double FILTER_MAX_FRACTION = 0.5;
constexpr int64_t FILTER_MIN_WINDOWS = 1000000000ll;
static int64_t filter_min_windows()
{
    if (const char *e = getenv("KGMA_FILTER_MIN_WINDOWS")) return std::max<int64_t>(1, atoll(e));
    return FILTER_MIN_WINDOWS;
}

// The filter's threshold U on a granule's sum of S for KFV 0; false: the filter does not run (a genome below the size limit, a
// negative S entry, or U <= 0).
static bool filter_bound(const kgma_ctx *ctx, int nk, int64_t total_nwin, uint32_t *U)
{
    const KfvInfo &f = ctx->kfv[0];
    if (total_nwin < filter_min_windows()) return false;
    if (*std::min_element(f.S.begin(), f.S.end()) < 0) return false;    // (the granule sums bound sumS only for S >= 0: sums of counts are)
    const int64_t Dmax = std::max(f.T - 1, f.T_hi);
    const __int128 num = (__int128)f.sumS2 + (__int128)f.N * (__int128)f.N * (__int128)nk - (__int128)Dmax;
    if (num <= 0) return false;                                         // U <= 0: every window is a candidate
    const __int128 twoN = 2 * (__int128)f.N;
    const __int128 U128 = (num + twoN - 1) / twoN;
    *U = U128 > 0x7FFFFFFF ? 0x7FFFFFFFu : (uint32_t)U128;              // (a granule's sum stays below 2^26: no candidates)
    return true;
}
static bool filter_remembered(const kgma_ctx *ctx, const kgma_genome *g)
{
    const KfvInfo &f = ctx->kfv[0];
    const auto &memo = ctx->fmemo;
    return memo.valid && memo.uid == g->uid && memo.refs == ctx->refs_version && memo.T == f.T && memo.T_hi == f.T_hi;
}

// The step's pack may carry the prefilter's block sums (pack_sums_kernel; KGMA_FUSE_SUMS=0: never): what the step entry points can
// tell before the scan -- they then leave the pack to it, which knows whether the filter will run (kgma_scan_device).
static bool fuse_sums_possible(const kgma_ctx *ctx, int32_t mode)
{
    const char *e = getenv("KGMA_FUSE_SUMS"), *fe = getenv("KGMA_FILTER"), *ov = getenv("KGMA_OVERLAP");
    if ((e && atoi(e) == 0) || (fe && atoi(fe) == 0) || (ov && atoi(ov) == 1)) return false;
    return mode == KGMA_MODE_SINGLE && !ctx->strobe && ctx->m >= 1 && !ctx->kfv[0].fp && pack_sums_applies(ctx->k, ctx->kfv[0].Smax);
}

// The candidate list's buffers, for whichever kernel appends to it (the filter's, or the step's pack when it tests): the list lives
// in pinned host memory (the kernel appends a few thousand 16-byte entries), its counters on the device.  *cap: entries it holds
static int filter_reserve_list(kgma_ctx *ctx, int64_t *cap_out)
{
    int64_t cap = 1 << 18;
    if (const char *e = getenv("KGMA_FILTER_CAP")) cap = std::min<int64_t>(std::max<int64_t>(1, atoll(e)), 1 << 24);
    const size_t pin_need = 16 + (size_t)cap * sizeof(FilterEntry);
    if (pin_need > ctx->fpin_cap) {
        if (ctx->h_fpin) (void)hipHostFree(ctx->h_fpin);
        ctx->h_fpin = nullptr; ctx->fpin_cap = 0;
        HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->h_fpin), pin_need, hipHostMallocDefault));
        ctx->fpin_cap = pin_need;
        HIP_TRY(ctx, hipHostGetDevicePointer(reinterpret_cast<void **>(&ctx->h_fpin_dev), ctx->h_fpin, 0));
    }
    if (!ctx->d_fctl) {
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_fctl), 16));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_fctl, 0, 16, ctx->stream));
    }
    if (!ctx->evf0) { HIP_TRY(ctx, hipEventCreate(&ctx->evf0)); HIP_TRY(ctx, hipEventCreate(&ctx->evf1)); }
    *cap_out = cap;
    return KGMA_OK;
}

static int filter_candidate_table(kgma_ctx *ctx, kgma_genome *g, int nk, int64_t n_tiles, bool *filtered)
{
    *filtered = false;
    kgma_filter_stats &fs = ctx->fstats;
    const KfvInfo &f = ctx->kfv[0];
    const int64_t nc = g->n_contigs;
    int64_t total_nwin = 0;
    for (int64_t c = 0; c < nc; c++) total_nwin += ctx->contig_nwin[(size_t)c];
    fs.total_windows = total_nwin;
    uint32_t U = 0;
    if (!filter_bound(ctx, nk, total_nwin, &U)) return KGMA_OK;
    fs.bound = (int64_t)U;
    const bool geom_debug = getenv("KGMA_GEOM_DEBUG") != nullptr;
    auto &memo = ctx->fmemo;
    if (filter_remembered(ctx, g)) {
        fs.fell_back = 1; fs.reason = KGMA_FILTER_REMEMBERED;
        if (geom_debug) fprintf(stderr, "scan filter: skipped, this genome fell back before\n");
        return KGMA_OK;
    }
    int64_t cap = 0;
    int32_t form = 0;
    if (g->pack_tested) {
        // ---- this scan's pack has made the test (plan_deferred_pack): no kernel here, its list is waited for and read like the filter's
        if (U != ctx->ptest_U) return fail(ctx, KGMA_E_HIP, "internal: the pack tested against bound %u, the scan's is %u", ctx->ptest_U, U);
        cap = ctx->ptest_cap;
        HIP_TRY(ctx, hipEventRecord(ctx->evf0, ctx->stream));           // (kgma_stats::scan_ms runs from here: read-back, table, exact launch)
        HIP_TRY(ctx, sync_spin(ctx->stream));
        form = 1 | (32 << 8) | (1 << 16);                               // (what launch_filter reports for the form on the block sums)
        fs.filter_ms = 0;                                               // (the time is the pack's: kgma_stats::pack_ms)
        const unsigned int *hc = reinterpret_cast<const unsigned int *>(ctx->h_fpin);
        ctx->ptest.slow_units = hc[1]; ctx->ptest.primed_chunks = hc[2];     // (both counted by the kernel)
    } else {
        const int lrc = filter_reserve_list(ctx, &cap);
        if (lrc) return lrc;
        if (!g->bsum_fresh) {                                           // (only the form on this step's block sums leaves the 2-bit copy alone)
            const int irc = ensure_inter(ctx, g);
            if (irc) return irc;
        }
        FilterArgs a;
        memset(&a, 0, sizeof a);
        a.inter = g->d_inter; a.n_dwords = 2 * g->total_words;
        a.tiles = ctx->d_tiles; a.n_tiles = (int32_t)n_tiles;
        a.nblk = (nk + 14) / 16 + 1;
        a.cd = g->d_cd;
        a.S = ctx->d_Stab;
        a.U = U;
        a.cap = (unsigned int)cap;
        a.list = reinterpret_cast<FilterEntry *>(ctx->h_fpin_dev + 16);
        a.ctl = ctx->d_fctl;
        a.bsum = g->bsum_fresh ? g->d_bsum : nullptr;                   // (this scan's pack wrote the block sums: the PRESUMMED form)
        HIP_TRY(ctx, hipEventRecord(ctx->evf0, ctx->stream));
        HIP_TRY(ctx, launch_filter(a, ctx->k, f.Smax, ctx->n_cus, reinterpret_cast<unsigned int *>(ctx->h_fpin_dev), &form, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ctx->evf1, ctx->stream));
        HIP_TRY(ctx, sync_spin(ctx->stream));
        float fms = 0;
        (void)hipEventElapsedTime(&fms, ctx->evf0, ctx->evf1);
        fs.filter_ms = fms;
    }
    fs.ran = 1;
    fs.form = form;
    const unsigned int count = *reinterpret_cast<const unsigned int *>(ctx->h_fpin);
    const size_t n_e = (size_t)std::min<int64_t>(count, cap);
    const FilterEntry *he = reinterpret_cast<const FilterEntry *>(ctx->h_fpin + 16);
    ctx->fentries.assign(he, he + n_e);
    std::sort(ctx->fentries.begin(), ctx->fentries.end(), [](const FilterEntry &x, const FilterEntry &y) {
        // (by first candidate granule: the entries of two neighbouring streams may share a base, their bits never overlap)
        return x.contig != y.contig ? x.contig < y.contig : (int64_t)x.gbase + __builtin_ctzll(x.mask) < (int64_t)y.gbase + __builtin_ctzll(y.mask);
    });
    ctx->fnwin = ctx->contig_nwin;
    for (const FilterEntry &e : ctx->fentries) fs.granules += __builtin_popcountll(e.mask);

    const int64_t P = ctx->tile_windows;
    const int64_t merge_gap = (((int64_t)nk + 63) / 64) * 64;
    int reason = (int64_t)count > cap ? KGMA_FILTER_OVERFLOW : KGMA_FILTER_OK;
    ctx->ftiles.clear();
    ctx->fcontig_tile_base.assign((size_t)nc, -1);
    size_t ei = 0;
    for (int64_t c = 0; c < nc && reason == KGMA_FILTER_OK; c++) {
        const int64_t nwin = ctx->contig_nwin[(size_t)c];
        while (ei < ctx->fentries.size() && ctx->fentries[ei].contig < c) ei++;
        if (nwin <= 0) continue;
        ctx->fcontig_tile_base[(size_t)c] = (int64_t)ctx->ftiles.size();
        int64_t rs = 0, re = std::min<int64_t>(nwin, 64);               // the region being grown (0-based windows [rs, re))
        auto flush = [&]() {
            fs.regions++;
            for (int64_t t = rs; t < re; t += P) {
                TileDesc td;
                td.word_base = g->cd[(size_t)c].word_off + t / 32;
                td.win0 = t + 1;
                td.dist_base = -1;
                td.n_valid = (int32_t)std::min<int64_t>(P, re - t);
                td.first_test = t == 0 ? 1 : 0;
                td.contig = (int32_t)c;
                td.pad = 0;
                ctx->ftiles.push_back(td);
                fs.windows += td.n_valid;
                fs.positions += (int64_t)td.n_valid + nk - 1;
            }
        };
        for (; ei < ctx->fentries.size() && ctx->fentries[ei].contig == c; ei++) {
            const FilterEntry &e = ctx->fentries[ei];
            uint64_t m = e.mask;
            while (m) {
                const int b0 = __builtin_ctzll(m);
                const uint64_t inv = ~(m >> b0);
                const int len = inv ? __builtin_ctzll(inv) : 64 - b0;    // run of set bits b0 ... b0 + len - 1
                m = b0 + len >= 64 ? 0 : m & (~(uint64_t)0 << (b0 + len));
                const int64_t wa = 16 * ((int64_t)e.gbase + b0), wb = std::min<int64_t>(16 * ((int64_t)e.gbase + b0 + len) - 1, nwin - 1);
                if (wa < 0 || wa >= nwin) return fail(ctx, KGMA_E_HIP, "internal: filter candidate outside record %lld", (long long)c);
                const int64_t s = std::max<int64_t>(0, (wa / 64) * 64 - 64), en = std::min<int64_t>(nwin, ((wb + 1 + 63) / 64) * 64 + 64);
                if (s <= re + merge_gap) { rs = std::min(rs, s); re = std::max(re, en); }
                else { flush(); rs = s; re = en; }
            }
        }
        flush();
        // (the walk ends as soon as the candidate streams cover too much: that also bounds the table; where both limits are passed
        //  the fraction is the reason reported)
        if ((double)fs.positions > FILTER_MAX_FRACTION * (double)total_nwin) reason = KGMA_FILTER_FRACTION;
    }
    fs.streams = (int64_t)ctx->ftiles.size();
    if (reason == KGMA_FILTER_OK && fs.streams > n_tiles) reason = KGMA_FILTER_STREAMS;
    if (geom_debug)
        fprintf(stderr, "scan filter (%s): U %u, %lld granules, %lld regions, %lld candidate streams, %lld of %lld windows, %.3f ms%s%s\n", g->pack_tested ? "tested in the pack" : g->bsum_fresh ? "filter kernel on the pack's sums" : "filter kernel", U, (long long)fs.granules,
                (long long)fs.regions, (long long)fs.streams, (long long)fs.windows, (long long)total_nwin, fs.filter_ms, reason ? ", fallback: " : "",
                reason == KGMA_FILTER_OVERFLOW ? "list overflow" : reason == KGMA_FILTER_STREAMS ? "too many streams" : reason == KGMA_FILTER_FRACTION ? "too many windows" : "");
    if (reason != KGMA_FILTER_OK) {
        fs.fell_back = 1; fs.reason = reason;
        memo.valid = true; memo.uid = g->uid; memo.refs = ctx->refs_version; memo.T = f.T; memo.T_hi = f.T_hi;
        return KGMA_OK;
    }
    int rc = dev_reserve(ctx, ctx->d_ftiles, ctx->ftiles_cap, (int64_t)ctx->ftiles.size());
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_ftiles, ctx->ftiles.data(), ctx->ftiles.size() * sizeof(TileDesc), hipMemcpyHostToDevice, ctx->stream));
    rc = pack_candidate_blocks(ctx, g, ctx->ftiles, nk);                             // (a sparse step: the blocks these streams load, in front of the exact scan)
    if (rc) return rc;
    *filtered = true;
    return KGMA_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// The host side of a scan (kgma_scan_device), in five steps: plan_scan decides which kernel serves the scan and how it is launched;
// build_stream_table which windows each record evaluates and how they are cut into streams; reserve_results sizes the result block
// and its pinned mirror; launch_group fills the parameters of one launch group and launches it (inside the overflow-retry loop);
// collect_results reads the mirror back and hands the records to stitch_dips.
// ------------------------------------------------------------------------------------------
namespace {

// One launch of the scan: the KFVs it takes and what the plan needs to know about them, worked out once
struct LaunchGroup {
    Group gr;
    int nk = 0, nk_min = 0;            // k-mers of the launch's longest / shortest window
    int n_sizes = 0;                   // distinct window sizes
    int n_longer = 0;                  // KFVs whose window is longer than the launch's shortest
    int n_plus1 = 0, n_plus2 = 0;      // ... one / two k-mers longer (five-KFV launches)
    int64_t nmax = 0;                  // largest N
    bool s16 = true, u8 = true;        // every S entry fits int16 / is below 256
    bool need_wide = false;            // a KFV whose prefix leaves int32
    bool one_size = true;
    bool s8 = false;                   // stream8_kernel serves it (the generic and strobemer kernels count: they read the interleaved genome copy too)
    int slots = 0;                     // streams resident per CU (stream kernels)
    double weight = 0;                 // what the launch costs, in arbitrary units
};

// What kgma_scan_device decides before it touches the stream table: made once per scan by plan_scan
struct ScanPlan {
    int32_t mode = 0;
    uint32_t flags = 0;
    int k = 0, m_used = 0;
    int64_t maxws = 0;
    bool strobe = false, generic_all = false, generic_fp = false, use_stream = false;
    bool overlap = false;              // the deferred pack runs beside the scan's launches (launch_overlapped)
    bool natural_slots = false;        // every launch runs at its own residency, in rounds over one stream table
    bool planes_needed = false;        // a launch reads the bit-plane copy of the genome
    bool want_dists = false;
    int eff_reserved = 0;              // CUs the streams are NOT sized for
    int stream_nw = 0;                 // streams per CU the table is sized for
    uint64_t geom_version = 0;         // what the stream table was sized for (its cache key)
    char kernel_name[sizeof kgma_ctx::kernel_name] = "";
    // the environment, read once per scan (not cached across scans: tests change it between scans of one process)
    const char *kernel_env = nullptr;  // KGMA_KERNEL
    bool filter_off = false;           // KGMA_FILTER=0
    int debug_skip = 0;                // KGMA_DEBUG_SKIP (timing experiments only)
    bool minslots = false;             // KGMA_STREAM_MINSLOTS
    int rounds = 0, round_windows = 0; // KGMA_STREAM_ROUNDS, KGMA_STREAM_ROUND_WINDOWS (experiments; 0: not set)
    int twokernel = -1;                // KGMA_TWOKERNEL (-1: not set)
    bool geom_debug = false;           // KGMA_GEOM_DEBUG
    std::vector<LaunchGroup> groups;
};

void read_scan_env(ScanPlan &p)
{
    p.kernel_env = getenv("KGMA_KERNEL");                        // testing only: run the other kernel where both apply
    if (const char *e = getenv("KGMA_FILTER")) p.filter_off = atoi(e) == 0;
    if (const char *e = getenv("KGMA_DEBUG_SKIP")) p.debug_skip = atoi(e);
    p.minslots = getenv("KGMA_STREAM_MINSLOTS") != nullptr;
    if (const char *e = getenv("KGMA_STREAM_ROUNDS")) p.rounds = std::max(1, atoi(e));
    if (const char *e = getenv("KGMA_STREAM_ROUND_WINDOWS")) p.round_windows = std::max(64, atoi(e));
    if (const char *e = getenv("KGMA_TWOKERNEL")) p.twokernel = atoi(e) != 0 ? 1 : 0;
    p.geom_debug = getenv("KGMA_GEOM_DEBUG") != nullptr;
}

// (the KFVs of a group are in ascending window size)
LaunchGroup describe_group(const kgma_ctx *ctx, Group &&group, bool generic_all)
{
    LaunchGroup L;
    L.gr = std::move(group);
    const Group &gr = L.gr;
    const int k = ctx->k, n = (int)gr.kfvs.size();
    const int64_t w0 = ctx->kfv[(size_t)gr.kfvs.front()].W;
    L.nk = (int)(gr.W - k + 1);
    L.nk_min = (int)(w0 - k + 1);
    L.one_size = w0 == ctx->kfv[(size_t)gr.kfvs.back()].W;
    int64_t prev = -1;
    for (int j : gr.kfvs) {
        const KfvInfo &f = ctx->kfv[(size_t)j];
        if (f.W != prev) L.n_sizes++;
        prev = f.W;
        L.n_longer += f.W != w0 ? 1 : 0;
        L.n_plus1 += f.W == w0 + 1 ? 1 : 0;
        L.n_plus2 += f.W == w0 + 2 ? 1 : 0;
        L.nmax = std::max(L.nmax, f.N);
        L.s16 = L.s16 && f.Smax <= 32767;
        L.u8 = L.u8 && f.Smax < 256;
        L.need_wide = L.need_wide || !f.fits32;
    }
    if (generic_all) L.s8 = true;
    else if (L.one_size && stream8_c16_applies(k, L.nk, n, L.nmax, L.s16, L.need_wide)) L.s8 = true;
    else if (L.need_wide) L.s8 = false;
    else if (stream8_wide_applies(k, L.nk_min, L.nk, n, L.nmax, L.u8, L.s16, L.n_plus1, L.n_plus2)) L.s8 = true;
    else if (L.one_size) L.s8 = stream8_applies(k, L.nk, n, L.nmax, L.s16);
    else L.s8 = stream8_derive_applies(k, L.nk_min, L.nk, n, L.nmax, L.s16);
    return L;
}

// The distance-bound prefilter applies: one integer KFV on the 8-bit count-table kernel at k = 5, 6, no distance output
// (filter_candidate_table decides whether it runs)
bool filter_wanted(const kgma_ctx *ctx, const ScanPlan &p, bool ovl)
{
    const int k = p.k;
    const KfvInfo &f0 = ctx->kfv[0];
    const int nk0 = (int)(f0.W - k + 1);
    return !p.filter_off && p.use_stream && !p.generic_all && p.m_used == 1 && p.groups.size() == 1 && p.groups[0].gr.kfvs.size() == 1 && p.groups[0].gr.kfvs[0] == 0 &&
           !p.want_dists && !ovl && p.debug_skip == 0 && !f0.fp && f0.fits32 && !f0.S.empty() && stream8_applies(k, nk0, 1, f0.N, f0.Smax <= 32767) &&
           !stream8_c16_applies(k, nk0, 1, f0.N, f0.Smax <= 32767, false) && filter_applies(k, f0.Smax);
}

// a re-encoding left to this scan (kgma_repack_scan_hits): beside the scan's launches when it is ONE stream8 launch of one KFV
// (launch_overlapped), else one launch in front of it
int plan_deferred_pack(kgma_ctx *ctx, kgma_genome *g, ScanPlan &p)
{
    g->bsum_fresh = false;                                             // (block sums are only good inside the scan whose pack wrote them)
    g->pack_tested = false;
    if (!g->repack_deferred) return KGMA_OK;
    p.overlap = p.use_stream && !p.generic_all && p.groups.size() == 1 && p.groups[0].gr.kfvs.size() == 1 && p.m_used == 1 && p.groups[0].s8 &&
                g->d_planes == nullptr && overlap_setup(ctx);
    if (p.overlap) return KGMA_OK;
    g->repack_deferred = false;
    // the pack carries the filter's block sums when the filter is going to run on byte entries (else: the plain pack, and
    // the filter, if it runs after all, cuts its k-mers itself)
    bool sums = false;
    uint32_t U = 0;
    const int nk0 = (int)(ctx->kfv[0].W - p.k + 1);
    if (fuse_sums_possible(ctx, p.mode) && !g->bsum_failed && filter_wanted(ctx, p, false) && !filter_remembered(ctx, g)) {
        const int64_t W0 = ctx->kfv[0].W;
        int64_t total_nwin = 0;
        for (const ContigDesc &d : g->cd) total_nwin += d.len >= W0 ? d.len - W0 + 1 : 0;
        sums = filter_bound(ctx, nk0, total_nwin, &U);
    }
    // ... and makes the filter's test itself where the pack is going to be the sums-only one and the genome gives every wave a few
    // runs (KGMA_PACK_TEST=0: never; KGMA_PACK_RUN: units per run; KGMA_PACK_TEST_MIN_UNITS: the gate, for tests).  Below the gate
    // the runs would leave waves idle, and the filter kernel on a small genome's sums costs next to nothing.
    const char *sp = getenv("KGMA_SPARSE_PACK"), *pt = getenv("KGMA_PACK_TEST");
    PackSums with_sums{ctx->d_Stab, ctx->k, ctx->kfv[0].Smax, ctx->n_cus};
    if (sums && g->d_planes == nullptr && g->n_contigs > 0 && !(sp && atoi(sp) == 0) && !(pt && atoi(pt) == 0)) {
        int run = PACK_TEST_RUN;
        if (const char *e = getenv("KGMA_PACK_RUN")) run = std::min(std::max(1, atoi(e)), 4096);
        const int64_t units = (g->total_words + 127) / 128;
        int64_t min_units = pack_sums_waves(ctx->n_cus) * run * PACK_TEST_MIN_RUNS;
        if (const char *e = getenv("KGMA_PACK_TEST_MIN_UNITS")) min_units = std::max<int64_t>(1, atoll(e));
        const int nblk = (nk0 + 14) / 16 + 1;
        if (units >= min_units && units < ((int64_t)1 << 29) && run <= 4096 && nblk >= 1 && nblk <= 63) {
            int64_t cap = 0;
            const int lrc = filter_reserve_list(ctx, &cap);
            if (lrc) return lrc;
            if (g->bsum_S_refs != ctx->refs_version || !g->d_bsum_S) {  // (ensure_bsum may run after the context's references changed)
                const size_t nb = ((size_t)1 << (2 * p.k)) * sizeof(int32_t);
                if (!g->d_bsum_S) HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&g->d_bsum_S), (size_t)4096 * sizeof(int32_t)));
                HIP_TRY(ctx, hipMemcpyAsync(g->d_bsum_S, ctx->d_Stab, nb, hipMemcpyDeviceToDevice, ctx->stream));
                g->bsum_S_refs = ctx->refs_version;
            }
            with_sums.test = true; with_sums.U = U; with_sums.nblk = nblk; with_sums.nk = nk0; with_sums.run = run; with_sums.cap = cap;
            ctx->ptest_U = U; ctx->ptest_cap = cap;
            ctx->ptest.tested = 1; ctx->ptest.run = run;
            ctx->ptest.units = units;
        }
    }
    if (sums && !with_sums.test && !g->d_bsum) {
        if (hipMalloc(reinterpret_cast<void **>(&g->d_bsum), (size_t)g->total_words * 4) != hipSuccess) {
            (void)hipGetLastError();
            g->d_bsum = nullptr; g->bsum_failed = true; sums = false;
        } else g->device_bytes += g->total_words * 4;
    }
    // ... and, on a genome without planes, leaves the 2-bit copy to the blocks the step reads (KGMA_SPARSE_PACK=0: never)
    const bool sparse = sums && g->d_planes == nullptr && !(sp && atoi(sp) == 0);
    return genome_repack(ctx, g, sums ? &with_sums : nullptr, sparse);
}

// Launches that keep different numbers of streams resident (one KFV: 32 per CU; four: 22): all launches share one
// stream table.  Its streams per CU, S, are chosen so that every launch runs at its OWN residency s in
// ceil(S / s) nearly full rounds (s = 22 and 32: S = 64 is 3 rounds of 22 and 2 of 32), weighing the launches by
// their cost; with one residency (or nothing to gain) S = s and there is one round.
void plan_natural_slots(ScanPlan &p)
{
    int s_max = 0;
    for (const LaunchGroup &L : p.groups) s_max = std::max(s_max, L.slots);
    if (s_max <= p.stream_nw) return;
    auto cost = [&](int S) {
        double c = 0;
        for (const LaunchGroup &L : p.groups) c += L.weight * (double)(((S + L.slots - 1) / L.slots) * L.slots) / (double)S;
        return c;
    };
    // (cutting every launch down to the smallest residency costs the others s / s_min; 0.9: fewer waves run a little faster each)
    double best = 0;
    for (const LaunchGroup &L : p.groups) best += L.weight * std::max(1.0, 0.9 * (double)L.slots / (double)p.stream_nw);
    int best_S = 0;
    for (int S = s_max; S <= 4 * s_max; S++)
        if (cost(S) < best * 0.99) { best = cost(S); best_S = S; }
    if (best_S > 0) { p.natural_slots = true; p.stream_nw = best_S; }
}

// Step 1: which kernel serves the scan, in which launches, at which residency.  Nothing here runs on the device but what these
// decisions need: the occupancy queries, overlap_setup and the pack a step left to this scan.
int plan_scan(kgma_ctx *ctx, kgma_genome *g, int32_t mode, uint32_t flags, ScanPlan &p)
{
    p.mode = mode;
    p.flags = flags;
    p.strobe = mode == KGMA_MODE_STROBE;
    p.want_dists = (flags & KGMA_F_RETURN_DISTS) != 0;
    const int k = p.k = ctx->k, m_used = p.m_used = mode == KGMA_MODE_SINGLE ? 1 : ctx->m;
    for (int j = 0; j < m_used; j++) p.maxws = std::max(p.maxws, ctx->kfv[(size_t)j].W);
    read_scan_env(p);
    const char *kenv = p.kernel_env;
    // ---- which kernel: the count-table stream kernel for k <= 7 (one wave per stream), the bit-sliced
    //      kernel for longer k-mers (their 4^k counters do not fit a wave's share of the LDS)
    // (measured, 400 Mb random sequence: k=6 one KFV 294 vs 172 Gbp/s; below k=5 the 64 transitions of
    // a step collide too often, and at k=7 the per-wave LDS share leaves too few waves)
    // Several KFVs: the 8-bit stream kernel takes the KFVs of ONE window size per launch (they share the k-mers, the
    // count table and the corrections), so the cluster engine's KFVs are grouped by window size for it; the bit-sliced
    // kernel groups up to 8 KFVs of up to 4 sizes.
    bool s8_all = k >= 5 && k <= 7 && !(kenv && !strcmp(kenv, "bitslice"));
    // (a KFV whose window has 384 ... 65535 k-mers at k = 5, 6, 7, or whose prefix leaves int32, takes the 16-bit counter form of the
    //  same kernel, which carries the prefix in 64 bits)
    auto c16_ok = [&](const KfvInfo &f) {
        return !f.fp && f.big_ok && stream8_c16_applies(k, (int)(f.W - k + 1), 1, f.N, f.Smax <= 32767, !f.fits32);
    };
    for (int j = 0; j < m_used && s8_all; j++) {
        const KfvInfo &f = ctx->kfv[(size_t)j];
        const int nkj = (int)(f.W - k + 1);
        s8_all = (!f.fp && f.fits32 && stream8_applies(k, nkj, 1, f.N, f.Smax <= 32767)) || c16_ok(f);
    }
    // The generic kernel (kgma_generic.hip; one KFV per launch) takes the whole scan when a KFV is served by nothing else: a general
    // Float64 KFV, a window of more than 2031 k-mers or a prefix beyond int32 where the 16-bit stream8 form does not apply
    // (k < 5, k > 7, S beyond int16 at k = 7, N >= 2^22).  KGMA_KERNEL=generic (testing): always.
    // k = 1 and k >= 11: only the generic kernel's 32-bit counter and wide hash forms serve them
    // (the strobemer kernel -- kgma_strobe.hip -- is a stream kernel of the same kind: one KFV, the same stream table and records)
    p.generic_all = p.strobe || (kenv && !strcmp(kenv, "generic")) || k == 1 || k >= KGMA_WIDE_MIN_K;
    for (int j = 0; j < m_used; j++) {
        const KfvInfo &f = ctx->kfv[(size_t)j];
        if (f.fp || ((f.W - k + 1 > KGMA_MAX_NK || !f.fits32) && !(s8_all && c16_ok(f)))) p.generic_all = true;
        p.generic_fp = p.generic_fp || f.fp;
    }
    if (p.generic_all) { for (int j = 0; j < m_used; j++) p.groups.push_back(describe_group(ctx, Group{ctx->kfv[(size_t)j].W, {j}}, true)); }
    else for (Group &gr : make_groups(ctx, mode, s8_all)) p.groups.push_back(describe_group(ctx, std::move(gr), false));
    p.use_stream = (k >= 5 && k <= 6) || (k == 7 && s8_all);   // k = 7: only the 8-bit kernel (S tables in global memory) beats the bit-sliced one
    for (const LaunchGroup &L : p.groups)
        if (L.gr.kfvs.size() != 1 && !L.s8) p.use_stream = false;   // (the 16-bit multi-KFV stream kernel lost to the bit-sliced one: 99 vs 112 Gbp/s)
    if (kenv) {
        if (!strcmp(kenv, "bitslice")) p.use_stream = false;
        if (!strcmp(kenv, "stream")) p.use_stream = k <= KGMA_STREAM_MAX_K;
    }
    if (p.generic_all) p.use_stream = true;            // (a stream kernel: same stream table, same records)
    const int prc = plan_deferred_pack(ctx, g, p);
    if (prc) return prc;
    p.eff_reserved = p.overlap ? std::max(ctx->reserved_cus, ctx->ov_cus) : ctx->reserved_cus;   // (the scan's streams are sized for the CUs it gets)
    p.stream_nw = 1 << 20;           // streams resident per CU (smallest over the launch groups)
    if (p.generic_all) {
        p.stream_nw = p.strobe ? strobe_slots_per_cu(ctx->st_s) : generic_slots_per_cu(k, p.generic_fp, (int)(p.maxws - k + 1));
        if (p.stream_nw < 1) return fail(ctx, KGMA_E_HIP, "the %s kernel cannot be launched (k = %d)", p.strobe ? "strobemer" : "generic", k);
    }
    if (p.use_stream && !p.generic_all)
        for (LaunchGroup &L : p.groups) {
            L.slots = stream_slots_per_cu(k, L.nk, L.nk_min, L.n_longer, (int)L.gr.kfvs.size(), L.n_sizes, L.s16, L.nmax, L.u8, L.n_plus2, L.need_wide);
            if (L.slots < 1) p.use_stream = false;
            p.stream_nw = std::min(p.stream_nw, L.slots);
            L.weight = 4.0 + (double)L.gr.kfvs.size();                  // (a launch costs about 55 + 13 per KFV, in arbitrary units)
        }
    if (p.use_stream && !p.generic_all && !p.minslots) plan_natural_slots(p);
    // (what the stream table was sized for: reserved CUs < 2^10, CUs < 2^14, streams per CU < 2^16 -- 64 bits, no packing games)
    p.geom_version = p.use_stream ? (p.generic_all ? 3u : 2u) + ((uint64_t)(uint32_t)p.eff_reserved << 4) + ((uint64_t)(uint32_t)ctx->n_cus << 16) + ((uint64_t)(uint32_t)p.stream_nw << 32) : 1u;
    bool s8 = p.use_stream;
    p.planes_needed = !p.use_stream;                   // every kernel but the 8-bit stream kernel reads the bit-plane copy of the genome
    for (const LaunchGroup &L : p.groups) { s8 = s8 && L.s8; p.planes_needed = p.planes_needed || !L.s8; }
    if (p.strobe) snprintf(p.kernel_name, sizeof p.kernel_name, "strobe_kernel<%d>", ctx->st_s);
    else snprintf(p.kernel_name, sizeof p.kernel_name, p.generic_all ? (p.generic_fp ? "gen_kernel<f64,%d>" : "gen_kernel<%d>") : s8 ? "stream8_kernel<%d>" : p.use_stream ? "stream_kernel<%d>" : "scan_kernel<%d>", k);   // (+ pos_kernel for multi-KFV groups)
    return KGMA_OK;
}

// Which windows a record of L residues evaluates (nwin) and how many of its residues the reference looks up on the way (looked;
// -1: it raises a BoundsError)
void record_windows_looked(const kgma_ctx *ctx, const ScanPlan &p, int64_t L, int64_t &nwin, int64_t &looked)
{
    const int k = p.k;
    nwin = 0; looked = 0;
    if (p.mode == KGMA_MODE_SINGLE) {
        const int64_t W = ctx->kfv[0].W;
        if (L >= W) { nwin = L - W + 1; looked = L; }   // GenomeMiner.jl:37-39,60
    } else if (p.strobe) {
        // StrobeGenomeMiner.jl:36,40,48-57: the first window (virtual window start 1) and one window per step i = 1 .. L - W - 1
        // (start i + 1); the residues looked up are the first window's and those of the strobemers up to the one at L - k - 1
        const int64_t W = ctx->kfv[0].W;
        if (L >= W) { nwin = std::max<int64_t>(L - W, 1); looked = std::max<int64_t>(W, L - 2); }
    } else if (L < k - 1) {
        looked = -1;                                                   // BoundsError, OmnGenomeMiner.jl:84-86
    } else {
        looked = k - 1;                                                // :84-86
        for (int j = 0; j < p.m_used; j++)
            if (L >= ctx->kfv[(size_t)j].W) looked = std::max(looked, ctx->kfv[(size_t)j].W);   // :61-82
        const int64_t n_iter = L - p.maxws - k + 2;                    // :89
        if (n_iter >= 1) { nwin = n_iter + 1; looked = std::max(looked, L - k + 2); }   // seq[i+ws], :97
    }
}

// windows per tile: fixed by the workgroup geometry for the bit-sliced kernel; for the stream
// kernel one wave owns one stream, so the stream length is chosen to give every wave slot of the
// chip (256 CUs x waves per workgroup) a whole number of equally long streams
int64_t stream_length(const kgma_ctx *ctx, const ScanPlan &p, int64_t total_nwin)
{
    const int k = p.k;
    const int64_t maxws = p.maxws;
    if (!p.use_stream) return (int64_t)scan_tile_stride_words((int)(maxws - k + 1)) * 32;
    const int64_t slots = (int64_t)std::max(1, ctx->n_cus - p.eff_reserved) * p.stream_nw;      // (kgma_set_reserved_cus; the pack / scan overlap)
    int64_t rounds = std::max<int64_t>(1, (total_nwin + slots * KGMA_STREAM_MAX_WINDOWS - 1) / (slots * KGMA_STREAM_MAX_WINDOWS));
    // Several rounds of shorter streams balance the CUs (the workgroups of a launch are handed out as earlier
    // ones finish; measured at GRCh38 size, one KFV: 5.72 ms with one round, 5.13 ms with three; 400 Mb: 0.752 / 0.704 ms;
    // 50.8 Mb: 0.118 ms with one round of 6.2 k windows, 0.124 with two, 0.135 with three), as long as a
    // stream stays long against its warm-up (n k-mers) and the S-table staging of its workgroup.
    {
        int64_t want = 3, min_windows = std::max<int64_t>(8192, 8 * (maxws - k + 1));   // (a stream's warm-up is its window's n k-mers)
        if (p.generic_all && !p.strobe && generic_count_mode(k, (int)(maxws - k + 1)) == 1) min_windows = std::max<int64_t>(min_windows, (int64_t)1 << (2 * k - 2));   // (and zeroing its global count table)
        if (p.rounds) want = p.rounds;                                 // experiments
        if (p.round_windows) min_windows = p.round_windows;
        rounds = std::max(rounds, std::min<int64_t>(want, total_nwin / (slots * min_windows)));
    }
    int64_t P = (total_nwin + slots * rounds - 1) / (slots * rounds);
    P = ((P + 63) / 64) * 64;
    // (a stream's warm-up is its window's n k-mers: at least 4 n windows per stream; streams start on 64-window boundaries)
    P = std::min<int64_t>(std::max<int64_t>(P, std::max<int64_t>(KGMA_STREAM_MIN_WINDOWS, std::min<int64_t>(((4 * (maxws - k + 1) + 63) / 64) * 64, 1 << 16))),
                          KGMA_STREAM_MAX_WINDOWS);
    // every record ends with a shorter stream: lengthen the streams until they fit the wave slots
    // again (one stream too many would cost a whole extra round on one CU)
    auto count_streams = [&](int64_t len) {
        int64_t n = 0;
        for (int64_t nwin : ctx->contig_nwin) n += (nwin + len - 1) / len;
        return n;
    };
    for (int it = 0; it < 64 && P < KGMA_STREAM_MAX_WINDOWS && count_streams(P) > slots * rounds; it++)
        P = std::min<int64_t>(((P + P / 128 + 63) / 64) * 64, KGMA_STREAM_MAX_WINDOWS);
    return P;
}

// ---- which windows each record evaluates (tile table), cached per (genome, mode, W, k, kernel) ----
bool stream_table_cached(const kgma_ctx *ctx, const kgma_genome *g, const ScanPlan &p)
{
    return ctx->tk_uid == g->uid && ctx->tk_mode == p.mode && ctx->tk_maxws == p.maxws && ctx->tk_k == p.k && ctx->tk_version == p.geom_version;
}

// Step 2: the stream (tile) table of the plan over the genome's records, on the host (kgma_scan_device uploads it)
void build_stream_table(kgma_ctx *ctx, const kgma_genome *g, const ScanPlan &p)
{
    const int64_t nc = g->n_contigs;
    ctx->contig_len.resize((size_t)nc);
    ctx->contig_nwin.assign((size_t)nc, 0);
    ctx->contig_looked.assign((size_t)nc, 0);
    ctx->contig_tile_base.assign((size_t)nc, -1);
    ctx->tiles.clear();
    int64_t dist_total = 0, bases = 0, windows = 0, total_nwin = 0;
    for (int64_t c = 0; c < nc; c++) {
        const int64_t L = g->cd[(size_t)c].len;
        ctx->contig_len[(size_t)c] = L;
        bases += L;
        record_windows_looked(ctx, p, L, ctx->contig_nwin[(size_t)c], ctx->contig_looked[(size_t)c]);
        total_nwin += ctx->contig_nwin[(size_t)c];
    }
    const int64_t P = stream_length(ctx, p, total_nwin);
    if (p.geom_debug)
        fprintf(stderr, "scan geometry: %s, %d CUs (%d reserved), %d streams per CU, %lld windows -> streams of %lld\n", p.use_stream ? "stream" : "bitslice",
                ctx->n_cus, ctx->reserved_cus, p.use_stream ? p.stream_nw : 0, (long long)total_nwin, (long long)P);
    const int64_t stride_words = P / 32;
    ctx->tile_windows = P;
    for (int64_t c = 0; c < nc; c++) {
        const int64_t nwin = ctx->contig_nwin[(size_t)c];
        if (nwin <= 0) continue;
        ctx->contig_tile_base[(size_t)c] = (int64_t)ctx->tiles.size();
        const int64_t nt = (nwin + P - 1) / P;
        for (int64_t t = 0; t < nt; t++) {
            TileDesc td;
            td.word_base = g->cd[(size_t)c].word_off + t * stride_words;
            td.win0 = t * P + 1;
            td.dist_base = dist_total + t * P - 1;
            td.n_valid = (int32_t)std::min<int64_t>(P, nwin - t * P);
            td.first_test = t == 0 ? 1 : 0;
            td.contig = (int32_t)c;
            td.pad = 0;
            ctx->tiles.push_back(td);
        }
        dist_total += nwin - 1;
        windows += nwin * p.m_used;
    }
    ctx->n_dists_per_kfv = dist_total;
    ctx->tk_bases = bases;
    ctx->tk_windows = windows;
    ctx->tk_uid = 0;   // set once the table is on the device
}

// errors the reference raises while walking the records, in record order
int check_records(kgma_ctx *ctx, const kgma_genome *g)
{
    for (int64_t c = 0; c < g->n_contigs; c++) {
        const int64_t looked = ctx->contig_looked[(size_t)c];
        if (looked < 0)
            return fail(ctx, KGMA_E_BOUNDS, "record %lld has %lld residues, fewer than k-1 (BoundsError, OmnGenomeMiner.jl:84-86)",
                        (long long)c, (long long)ctx->contig_len[(size_t)c]);
        const unsigned long long fb = g->first_bad[(size_t)c];
        if (fb != NO_BAD && (int64_t)fb <= looked)
            return fail(ctx, KGMA_E_BADBASE, "record %lld position %llu: residue is not one of A/C/G/T/N (KeyError, Consts.jl:22-28)",
                        (long long)c, fb);
    }
    return KGMA_OK;
}

// a genome without a single window: the records are still walked for the reference's errors
int scan_without_windows(kgma_ctx *ctx, kgma_genome *g, const ScanPlan &p)
{
    if (g->repack_deferred) {
        g->repack_deferred = false;
        const int prc = kgma_genome_repack(ctx, g);
        if (prc) return prc;
    }
    int rc = genome_sync(ctx, g);
    if (rc) return rc;
    rc = check_records(ctx, g);
    if (rc) return rc;
    ctx->D0.assign((size_t)ctx->m, -1);
    ctx->firstD.assign((size_t)ctx->m * (size_t)g->n_contigs, -1);
    ctx->dips.clear(); ctx->dip_argl.clear(); ctx->dip_aux.clear();
    ctx->att.clear(); ctx->chain_pair.clear(); ctx->firstF.clear(); ctx->dip_fmin.clear(); ctx->dip_fexit.clear();
    ctx->last_mode = p.mode;
    ctx->have_dists = p.want_dists;
    return KGMA_OK;
}

// The result block on the device and its pinned mirror share one layout: counters | D0 slots | aux | records (one memset, one
// download per scan; the mirror holds the first INLINE_RECS records)
constexpr size_t INLINE_RECS = 4096;
struct ResultBlock {
    uint8_t *base;
    int64_t d0_slots;
    unsigned int *n_recs() const { return reinterpret_cast<unsigned int *>(base); }
    unsigned int *aux_used() const { return reinterpret_cast<unsigned int *>(base + 4); }
    unsigned long long *n_att() const { return reinterpret_cast<unsigned long long *>(base + 8); }
    unsigned long long *n_cold() const { return reinterpret_cast<unsigned long long *>(base + 16); }
    int64_t *D0() const { return reinterpret_cast<int64_t *>(base + KGMA_RES_HDR); }
    uint8_t *aux() const { return base + KGMA_RES_HDR + d0_slots * 8; }
    DevRecord *recs() const { return reinterpret_cast<DevRecord *>(aux() + KGMA_AUX_BYTES); }
    static int64_t bytes(int64_t d0_slots, int64_t n_recs) { return KGMA_RES_HDR + d0_slots * 8 + KGMA_AUX_BYTES + n_recs * (int64_t)sizeof(DevRecord); }
};
inline ResultBlock device_results(const kgma_ctx *ctx) { return ResultBlock{ctx->d_res, ctx->res_d0_slots}; }
inline ResultBlock host_results(const kgma_ctx *ctx) { return ResultBlock{ctx->h_pin, ctx->res_d0_slots}; }

int res_reserve(kgma_ctx *ctx, int64_t d0_slots, int64_t recs)
{
    if (ctx->d_res && d0_slots <= ctx->res_d0_slots && recs <= (int64_t)ctx->rec_cap) return KGMA_OK;
    d0_slots = std::max(d0_slots, ctx->res_d0_slots);
    recs = std::max<int64_t>(recs, ctx->rec_cap);
    int64_t cap = 0;
    uint8_t *fresh = nullptr;
    int r2 = dev_reserve(ctx, fresh, cap, ResultBlock::bytes(d0_slots, recs));
    if (r2) return r2;
    if (ctx->d_res) { (void)hipFree(ctx->d_res); ctx->device_bytes -= ctx->res_bytes; }
    ctx->d_res = fresh; ctx->res_bytes = cap; ctx->res_d0_slots = d0_slots; ctx->rec_cap = (unsigned int)recs;
    ctx->counters_clean = false;                     // a fresh block is not zeroed
    return KGMA_OK;
}

// Step 3: room for the stream table, the result block, the distances and the pinned mirror
int reserve_results(kgma_ctx *ctx, const ScanPlan &p, int64_t n_tiles)
{
    int rc = dev_reserve(ctx, ctx->d_tiles, ctx->tiles_cap, n_tiles);
    if (rc) return rc;
    rc = res_reserve(ctx, n_tiles * ctx->m, std::max<int64_t>(ctx->rec_cap, 1 << 16));
    if (rc) return rc;
    if (p.want_dists)
        for (int j = 0; j < p.m_used; j++) {
            rc = dev_reserve(ctx, ctx->d_dist[(size_t)j], ctx->dist_cap[(size_t)j], std::max<int64_t>(1, ctx->n_dists_per_kfv));
            if (rc) return rc;
        }
    const size_t pin_need = (size_t)ResultBlock::bytes(ctx->res_d0_slots, INLINE_RECS);
    if (pin_need > ctx->h_pin_cap) {
        if (ctx->h_pin) (void)hipHostFree(ctx->h_pin);
        ctx->h_pin = nullptr; ctx->h_pin_cap = 0;
        HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->h_pin), pin_need + (pin_need >> 2), hipHostMallocDefault));
        ctx->h_pin_cap = pin_need + (pin_need >> 2);
        HIP_TRY(ctx, hipHostGetDevicePointer(reinterpret_cast<void **>(&ctx->h_pin_dev), ctx->h_pin, 0));
    }
    if (!ctx->d_done) {
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_done), 16));
        ctx->counters_clean = false;
    }
    return KGMA_OK;
}

// the table the exact kernel walks (the prefilter's candidate streams, or the regular one): its streams, D0 slots and records
struct ScanTables {
    int64_t n_tiles = 0;               // streams of the regular table
    int64_t n_scan = 0;                // streams of the table walked
    const TileDesc *d_scan_tiles = nullptr;
    bool filtered = false;
};

void bind_results(ScanArgs &a, const kgma_ctx *ctx, int64_t n_streams)
{
    const ResultBlock d = device_results(ctx);
    a.D0out = d.D0();                      // [KFV id - 1][tile]
    a.recs = d.recs();
    a.rec_count = d.n_recs();
    a.rec_cap = ctx->rec_cap;
    a.n_tiles = (int32_t)n_streams;
    a.n_att = d.n_att();
    a.n_cold = d.n_cold();
}

// the per-KFV part of a launch's parameters, shared by the scan and the chain kernel's launches (which add T / T_hi and
// chain_invN / chain_form)
void fill_group_params(const kgma_ctx *ctx, const std::vector<int> &kfvs, GroupParams &gp)
{
    const int k = ctx->k;
    for (size_t u = 0; u < kfvs.size(); u++) {
        const int j = kfvs[u];
        const KfvInfo &f = ctx->kfv[(size_t)j];
        const int32_t nkj = (int32_t)(f.W - k + 1);
        if (gp.n_sizes == 0 || gp.sizes[gp.n_sizes - 1] != nkj) gp.sizes[gp.n_sizes++] = nkj;   // ascending
        gp.nk_of[u] = nkj;
        gp.kfv_id[u] = j + 1;                                   // (the kernel finds the S table and the first-window slot by it)
        gp.N[u] = (int32_t)f.N;
        gp.sumS2[u] = f.sumS2;
        gp.inv_scale[u] = 2.0 * (double)k * (double)f.N * (double)f.N;
        if (u == 0) gp.s_fits_i16 = gp.s_fits_u8 = 1;
        if (f.Smax > 32767) gp.s_fits_i16 = 0;
        if (f.Smax > 255) gp.s_fits_u8 = 0;
    }
}

// the generic kernels' parameters for KFV j, shared by the scan and the chain: its table, the count mode of a window of nk_mode
// k-mers and the global count table where that mode needs one (`what`: "scan" / "chain", for the debug line)
int fill_gen_params(kgma_ctx *ctx, int j, int nk, int nk_mode, int32_t n_slots, bool fp, const char *what, GenParams &gg)
{
    const int k = ctx->k;
    const KfvInfo &f = ctx->kfv[(size_t)j];
    memset(&gg, 0, sizeof gg);
    gg.k = k; gg.nk = nk; gg.N = (int32_t)f.N; gg.kfv_id = j + 1; gg.fp = fp ? 1 : 0;
    gg.n_slots = n_slots;
    gg.sumR2 = f.sumR2; gg.SF = 1.0 / (double)k;
    if (f.sparse) {
        set_sparse_params(ctx, f, gg, fp);
    } else {
        const int64_t NBk = (int64_t)1 << (2 * k);
        gg.S = ctx->d_Stab + (size_t)j * (size_t)NBk;
        gg.R = ctx->d_Rtab ? ctx->d_Rtab + (size_t)j * (size_t)NBk : nullptr;
        if (fp && !gg.R) return fail(ctx, KGMA_E_STATE, "internal: no Float64 table for KFV %d", j + 1);
    }
    generic_set_mode(gg, nk_mode);
    if (getenv("KGMA_GEOM_DEBUG"))
        fprintf(stderr, "generic %s geometry: k %d, cmode %d, log2m %d, rebuild %d\n", what, k, gg.cmode, gg.hash_log2m, gg.hash_rebuild);
    if (gg.cmode == 1 || gg.cmode == 4) {
        const int rc = dev_reserve(ctx, ctx->d_gctab, ctx->gctab_cap, (int64_t)gg.n_slots * generic_ctab_dwords(gg));
        if (rc) return rc;
        gg.ctab = ctx->d_gctab;
    }
    return KGMA_OK;
}

int launch_group_strobe(kgma_ctx *ctx, const ScanPlan &p, const LaunchGroup &, const ScanTables &t, ScanArgs &a, const GroupParams &gp)
{
    const KfvInfo &f = ctx->kfv[0];
    StrobeParams sp;
    memset(&sp, 0, sizeof sp);
    sp.s = ctx->st_s; sp.w_min = ctx->st_wmin; sp.w_max = ctx->st_wmax;
    sp.nk = (int32_t)(f.W - p.k);                          // the strobemers that slide; the window's permanent one comes on top
    sp.N = (int32_t)f.N; sp.kfv_id = 1;
    sp.n_slots = (int32_t)((int64_t)std::max(1, ctx->n_cus - ctx->reserved_cus) * p.stream_nw);
    sp.T = f.T; sp.T_hi = f.T_hi; sp.sumS2 = f.sumS2; sp.inv_scale = gp.inv_scale[0];
    sp.S = ctx->d_Stab;
    strobe_zero_mask(ctx->st_q, sp.zero);
    bind_results(a, ctx, t.n_tiles);                       // (never filtered)
    HIP_TRY(ctx, launch_strobe(a, sp, ctx->stream));
    ctx->stats.n_launches++;
    return KGMA_OK;
}

int launch_group_generic(kgma_ctx *ctx, const ScanPlan &p, const LaunchGroup &L, const ScanTables &t, ScanArgs &a, const GroupParams &gp)
{
    const int j = L.gr.kfvs[0];
    const KfvInfo &f = ctx->kfv[(size_t)j];
    GenParams gg;
    // (one geometry for every launch of the scan: its longest window decides)
    const int rc = fill_gen_params(ctx, j, gp.nk, (int)(p.maxws - p.k + 1), (int32_t)((int64_t)std::max(1, ctx->n_cus - ctx->reserved_cus) * p.stream_nw),
                                   f.fp, "scan", gg);
    if (rc) return rc;
    gg.T = f.T; gg.T_hi = f.T_hi; gg.sumS2 = f.sumS2;
    gg.thr_lo = f.thr * (1.0 - std::ldexp(1.0, -ctx->band_log2)); gg.thr_hi = f.thr * (1.0 + std::ldexp(1.0, -ctx->band_log2));
    gg.inv_scale = gp.inv_scale[0];
    gg.tie_rel = 9.313225746154785e-10;
    bind_results(a, ctx, t.n_tiles);                       // (never filtered)
    HIP_TRY(ctx, launch_generic(a, gg, ctx->stream));
    ctx->stats.n_launches++;
    return KGMA_OK;
}

// several KFVs, k <= 7: two kernels (match loop -> per-window differences; window pass with the S
// tables in LDS), in chunks of tiles so that the difference buffer stays bounded (kgma_pos.hip)
int launch_group_two_kernel(kgma_ctx *ctx, const ScanPlan &p, const LaunchGroup &, const ScanTables &t, ScanArgs &a, const GroupParams &gp)
{
    const int64_t n_tiles = t.n_tiles;
    const int64_t P = ctx->tile_windows;
    const int64_t per_tile = (int64_t)gp.n_sizes * P;                 // int16 elements
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n_tiles, (((int64_t)2 << 30) / 2) / per_tile));
    const int rc = dev_reserve(ctx, ctx->d_diff, ctx->diff_cap, chunk * per_tile);
    if (rc) return rc;
    const int per_pass = std::max(1, pos_tables_per_pass(p.k));
    for (int64_t t0 = 0; t0 < n_tiles; t0 += chunk) {
        a.tile0 = (int32_t)t0;
        a.n_chunk_tiles = (int32_t)std::min<int64_t>(chunk, n_tiles - t0);
        for (int z = 0; z < gp.n_sizes; z++) a.diff[z] = ctx->d_diff + (int64_t)z * chunk * P;
        a.Stab = ctx->d_Stab;
        HIP_TRY(ctx, launch_scan(a, gp, ctx->stream));
        ScanArgs b = a;
        b.Stab = ctx->d_StabC;
        for (int j0 = 0; j0 < gp.n_kfv; j0 += per_pass)
            HIP_TRY(ctx, launch_pos(b, gp, j0, std::min(per_pass, gp.n_kfv - j0), ctx->stream));
        ctx->stats.n_launches++;
    }
    return KGMA_OK;
}

// one launch of the stream kernel or the bit-sliced one -- or, with a pack left to this scan, the overlapped (pack, scan) pairs
int launch_group_stream(kgma_ctx *ctx, kgma_genome *g, const ScanPlan &p, const LaunchGroup &, const ScanTables &t, ScanArgs &a, const GroupParams &gp)
{
    if (p.overlap && g->repack_deferred) {
        const int rc = launch_overlapped(ctx, g, a, gp, t.n_tiles);
        if (rc) return rc;
        ctx->stats.n_launches += ctx->ov_groups;
        return KGMA_OK;
    }
    HIP_TRY(ctx, p.use_stream ? launch_stream(a, gp, ctx->stream) : launch_scan(a, gp, ctx->stream));
    ctx->stats.n_launches++;
    return KGMA_OK;
}

// Step 4: the parameters of one launch group, and its launch by the kernel the plan chose
int launch_group(kgma_ctx *ctx, kgma_genome *g, const ScanPlan &p, const LaunchGroup &L, const ScanTables &t)
{
    const int k = p.k, n_kfv = (int)L.gr.kfvs.size();
    GroupParams gp;
    memset(&gp, 0, sizeof gp);
    ScanArgs a;
    memset(&a, 0, sizeof a);
    gp.n_kfv = n_kfv;
    gp.k = k;
    gp.nk = L.nk;                                                      // largest window of the launch
    gp.nk_min = L.nk_min;
    gp.nblocks = scan_nblocks(gp.nk);
    gp.stream_slots = p.use_stream && !p.natural_slots ? p.stream_nw : 0;
    gp.need_wide = L.need_wide ? 1 : 0;
    gp.debug_skip = p.debug_skip;
    fill_group_params(ctx, L.gr.kfvs, gp);
    for (int u = 0; u < n_kfv; u++) {
        const int j = L.gr.kfvs[(size_t)u];
        gp.T[u] = ctx->kfv[(size_t)j].T;
        gp.T_hi[u] = ctx->kfv[(size_t)j].T_hi;
        a.dist[u] = p.want_dists ? ctx->d_dist[(size_t)j] : nullptr;
    }
    a.planes = g->d_planes;
    a.inter = g->d_inter;
    a.tiles = t.d_scan_tiles;
    if (p.strobe) return launch_group_strobe(ctx, p, L, t, a, gp);
    if (p.generic_all) return launch_group_generic(ctx, p, L, t, a, gp);
    // all tables; the kernel indexes by KFV id.  The 16-bit stream kernel indexes k-mers as (hi bits << k) | lo bits,
    // the bit-sliced kernel and the 8-bit stream kernel by the 2-bit interleaved code (first base least significant)
    a.Stab = (p.use_stream && !L.s8) ? ctx->d_StabC : ctx->d_Stab;
    a.Sinter = nullptr;
    if (p.use_stream && L.s8 && k >= 7) {
        const int nv0 = stream8_variant(n_kfv);
        const int nv = nv0 == 3 ? 4 : nv0;                     // row width in int16 slots (the kernel variant's)
        const int rc = sinter_tables(ctx, L.gr.kfvs, nv, &a.Sinter, &a.Sbits);
        if (rc) return rc;
    }
    if (p.use_stream && stream8_state_words(k, n_kfv) > 0) {
        const int rc = dev_reserve(ctx, ctx->d_wstate, ctx->wstate_cap, t.n_tiles * stream8_state_words(k, n_kfv));
        if (rc) return rc;
        a.wave_state = ctx->d_wstate;
    }
    bind_results(a, ctx, t.n_scan);
    a.tile0 = 0;
    a.n_chunk_tiles = (int32_t)t.n_scan;
    a.tile_windows = ctx->tile_windows;
    // (measured, 400 Mb: k=7 with 8 KFVs 10.5 vs 16.3 ms; at k <= 6 the bit-sliced kernel's own position
    // phase, with one table at a time in LDS, is faster: 4.8 vs 7.5 ms at 5 KFVs.  KGMA_TWOKERNEL=1/0 forces)
    bool two_kernels = !p.use_stream && n_kfv >= 2 && k == KGMA_STREAM_MAX_K;
    if (p.twokernel >= 0) two_kernels = !p.use_stream && n_kfv >= 2 && k <= KGMA_STREAM_MAX_K && p.twokernel != 0;
    if (two_kernels) return launch_group_two_kernel(ctx, p, L, t, a, gp);
    return launch_group_stream(ctx, g, p, L, t, a, gp);
}

// the pack's time of a step whose pack this scan ran or waited for
void note_pack_time(kgma_ctx *ctx, kgma_genome *g)
{
    if (!g->pack_pending) return;
    float pms = 0;
    if (ctx->ov_groups > 0) {
        // (an overlapped step: the sums of the groups' kernel times -- the pack launches of all but the first group ran on
        //  a few CUs beside the scan, so their times are long and mostly hidden)
        for (int gi = 0; gi < ctx->ov_groups; gi++) { float t = 0; (void)hipEventElapsedTime(&t, ctx->ov_p0[gi], ctx->ov_p1[gi]); pms += t; }
    } else (void)hipEventElapsedTime(&pms, ctx->genome.evp0, ctx->genome.evp1);
    ctx->stats.pack_ms = pms;
    g->pack_pending = false;
}

// Step 5: the scan's time from the events, the records from the mirror (and, beyond its inline block, from the device), the
// streams' first distances on the host's lattice, and the dips stitched from the records
int collect_results(kgma_ctx *ctx, kgma_genome *g, const ScanPlan &p, const ScanTables &t, unsigned int n_recs)
{
    const int k = p.k;
    const int64_t nc = g->n_contigs, n_scan = t.n_scan;
    const ResultBlock h = host_results(ctx);
    float ms = 0;
    // (a scan whose filter ran: from the filter's launch to the end of the exact kernel -- filter, read-back, table, exact launch)
    (void)hipEventElapsedTime(&ms, ctx->fstats.ran ? ctx->evf0 : ctx->ev0, ctx->ev1);
    ctx->stats.overlap_ms = 0;
    if (ctx->ov_groups > 0) {
        // overlapped step: scan_ms = the sum of the scan launches' times (what the roofline is computed from), overlap_ms = the
        // wall time of the whole pack + scan region
        ctx->stats.overlap_ms = ms;
        ms = 0;
        for (int gi = 0; gi < ctx->ov_groups; gi++) { float tg = 0; (void)hipEventElapsedTime(&tg, ctx->ov_s0[gi], ctx->ov_s1[gi]); ms += tg; }
        ctx->ov_groups = 0;
    }
    ctx->stats.scan_ms = ms;
    int rc = check_records(ctx, g);
    if (rc) return rc;

    std::vector<DevRecord> recs((size_t)n_recs);
    const size_t n_inline = std::min<size_t>(n_recs, INLINE_RECS);
    if (n_inline) memcpy(recs.data(), h.recs(), n_inline * sizeof(DevRecord));
    if (n_recs > n_inline)
        HIP_TRY(ctx, hipMemcpy(recs.data() + n_inline, device_results(ctx).recs() + n_inline, ((size_t)n_recs - n_inline) * sizeof(DevRecord), hipMemcpyDeviceToHost));
    ctx->D0.assign(h.D0(), h.D0() + (size_t)n_scan * (size_t)ctx->m);
    for (int j = 0; j < p.m_used; j++) {
        // (Float64 KFV: the kernel wrote each stream's first distance as a double; the host works on the lattice)
        const KfvInfo &kf = ctx->kfv[(size_t)j];
        if (!kf.fp) continue;
        for (int64_t s = 0; s < n_scan; s++) {
            double dv;
            memcpy(&dv, &ctx->D0[(size_t)j * (size_t)n_scan + (size_t)s], sizeof dv);
            // (a first distance whose rounding noise went below zero -- the KFV is that window's counts up to noise -- is 0, as the
            //  kernel writes it for every later window; -1 in kgma_get_first_window means "record skipped")
            ctx->D0[(size_t)j * (size_t)n_scan + (size_t)s] = lattice_of(kf, k, dv < 0.0 ? 0.0 : dv);
        }
    }
    ctx->firstD.assign((size_t)ctx->m * (size_t)nc, -1);
    for (int j = 0; j < ctx->m; j++)
        for (int64_t c = 0; c < nc; c++) {
            const int64_t tb = t.filtered ? ctx->fcontig_tile_base[(size_t)c] : ctx->contig_tile_base[(size_t)c];   // (the record's first stream starts at its first window)
            if (tb >= 0) ctx->firstD[(size_t)j * (size_t)nc + (size_t)c] = ctx->D0[(size_t)j * (size_t)n_scan + (size_t)tb];
        }
    ctx->stats.n_at_threshold = (int64_t)*h.n_att();
    if (p.geom_debug) fprintf(stderr, "scan cold steps: %llu\n", *h.n_cold());
    ctx->aux_host = h.aux();
    ctx->aux_used = *h.aux_used();
    ctx->have_dists = p.want_dists;
    ctx->scan_filtered = t.filtered;
    rc = stitch_dips(ctx, recs);
    if (rc) return rc;
    ctx->last_mode = p.mode;
    ctx->stats.device_bytes = ctx->device_bytes + g->device_bytes;
    return KGMA_OK;
}

}  // namespace

extern "C" {

int kgma_scan_device(kgma_ctx *ctx, const kgma_genome *gc, int32_t mode, uint32_t flags)
{
    if (!ctx || !gc) return KGMA_E_ARG;
    kgma_genome *g = const_cast<kgma_genome *>(gc);   // only its pack bookkeeping is updated
    if (ctx->m == 0) return fail(ctx, KGMA_E_STATE, "kgma_set_refs has not been called");
    if (mode != KGMA_MODE_SINGLE && mode != KGMA_MODE_OMN && mode != KGMA_MODE_STROBE) return fail(ctx, KGMA_E_ARG, "unknown mode %d", mode);
    if ((mode == KGMA_MODE_STROBE) != ctx->strobe)
        return fail(ctx, KGMA_E_STATE, mode == KGMA_MODE_STROBE ? "a strobemer scan needs strobemer references (kgma_set_strobe_ref)"
                                                                : "the context holds strobemer references: a k-mer scan needs kgma_set_refs");
    (void)hipSetDevice(ctx->device);
    ScanPlan plan;
    int rc = plan_scan(ctx, g, mode, flags, plan);
    if (rc) return rc;
    memcpy(ctx->kernel_name, plan.kernel_name, sizeof ctx->kernel_name);

    ctx->dips.clear();
    ctx->hits.clear();
    ctx->have_dists = false;
    ctx->last_mode = -1;
    ctx->scan_filtered = false;
    memset(&ctx->fstats, 0, sizeof ctx->fstats);
    ctx->fentries.clear();
    if (plan.planes_needed) {
        rc = ensure_planes(ctx, g);
        if (rc != KGMA_OK) return rc;
    }

    const bool tiles_cached = stream_table_cached(ctx, g, plan);
    if (!tiles_cached) build_stream_table(ctx, g, plan);
    const int64_t n_tiles = (int64_t)ctx->tiles.size();
    if (n_tiles > 0x7FFFFFF0ll) return fail(ctx, KGMA_E_UNSUPPORTED, "too many tiles");
    ctx->stats.bases_scanned = ctx->tk_bases;
    ctx->stats.windows_scanned = ctx->tk_windows;
    ctx->stats.n_tiles = (int32_t)n_tiles;
    ctx->stats.n_launches = 0;
    ctx->stats.scan_ms = 0;
    ctx->stats.n_at_threshold = 0;
    ctx->stats.n_dips = ctx->stats.n_hits = ctx->stats.n_tie_flagged = 0;
    if (n_tiles == 0) return scan_without_windows(ctx, g, plan);

    rc = reserve_results(ctx, plan, n_tiles);
    if (rc) return rc;
    if (!tiles_cached) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_tiles, ctx->tiles.data(), (size_t)n_tiles * sizeof(TileDesc), hipMemcpyHostToDevice, ctx->stream));
        // the vector is pageable memory: the runtime stages it before returning, so it may be reused
        ctx->tk_uid = g->uid; ctx->tk_mode = mode; ctx->tk_maxws = plan.maxws; ctx->tk_k = plan.k; ctx->tk_version = plan.geom_version;
    }

    // ---- distance-bound prefilter: one integer KFV on the 8-bit count-table kernel at k = 5, 6, no distance output -- the exact
    //      kernel then walks the candidate stream table instead of the regular one (filter_candidate_table)
    ScanTables t;
    if (filter_wanted(ctx, plan, plan.overlap)) {
        rc = filter_candidate_table(ctx, g, (int)(ctx->kfv[0].W - plan.k + 1), n_tiles, &t.filtered);
        if (rc) return rc;
    }
    // every scan but the one over a sparse step's candidate streams reads the 2-bit copy anywhere: the filter does not apply, did
    // not run or fell back (one full pack, once: a fallback is remembered), or this is no step's scan at all
    // (an overlapped step packs every block itself, group by group beside its launches)
    if (!t.filtered && !(plan.overlap && g->repack_deferred)) {
        rc = ensure_inter(ctx, g);
        if (rc) return rc;
    }
    t.n_tiles = n_tiles;
    t.n_scan = t.filtered ? (int64_t)ctx->ftiles.size() : n_tiles;
    t.d_scan_tiles = t.filtered ? ctx->d_ftiles : ctx->d_tiles;

    unsigned int n_recs = 0;
    for (int attempt = 0;; attempt++) {
        if (attempt > 0) ctx->ov_groups = 0;                          // (a repeated scan is one plain launch)
        // (the previous scan's export_kernel normally left the counters at zero: no memset between steps)
        if (!ctx->counters_clean) {
            HIP_TRY(ctx, hipMemsetAsync(ctx->d_res, 0, KGMA_RES_HDR, ctx->stream));
            HIP_TRY(ctx, hipMemsetAsync(ctx->d_done, 0, 16, ctx->stream));
        }
        ctx->counters_clean = false;
        HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        ctx->stats.n_launches = 0;
        for (const LaunchGroup &L : plan.groups) {
            rc = launch_group(ctx, g, plan, L, t);
            if (rc) return rc;
        }
        HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        // last kernel: residues under tied minima are gathered on the device behind the scan (spares the host
        // a second round trip for the Float64 tie replay; skipped when the caller wants pure exact arithmetic),
        // then everything the host needs is written to the pinned mirror from inside the kernel (same layout:
        // counters | D0 slots | aux | first INLINE_RECS records; records beyond the inline block need a copy
        // afterwards, which only happens for dip-dense inputs) and the counters are reset: ONE synchronisation,
        // no copy-engine launch, no memset before the next scan
        HIP_TRY(ctx, launch_export(ctx->d_res, ctx->h_pin_dev, ctx->res_d0_slots, t.n_scan * (int64_t)ctx->m, ctx->rec_cap,
                                   (unsigned int)std::min<size_t>(INLINE_RECS, ctx->rec_cap), ((flags & KGMA_F_NO_TIE_RESOLVE) || plan.strobe) ? 0 : 1,
                                   t.d_scan_tiles, g->d_cd, g->d_ascii, ctx->d_Wtab, ctx->d_done, ctx->stream));
        HIP_TRY(ctx, sync_spin(ctx->stream));
        ctx->counters_clean = true;
        note_pack_time(ctx, g);
        n_recs = *host_results(ctx).n_recs();
        if (n_recs <= ctx->rec_cap) break;
        if (attempt >= 4) return fail(ctx, KGMA_E_OVERFLOW, "record buffer overflow (%u records)", n_recs);
        rc = res_reserve(ctx, n_tiles * ctx->m, (int64_t)n_recs + (n_recs >> 2) + 1024);
        if (rc) return rc;
    }
    return collect_results(ctx, g, plan, t, n_recs);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// Tie resolution.  Two situations are decided by Float64 rounding in the reference, not by the
// exact distances: (A) a dip whose exact minimum is attained at several separated windows -- the
// reference keeps the first window whose running Float64 value is strictly below all earlier ones
// (GenomeMiner.jl:82-87); (B) a dip whose exact minimum EQUALS the stale running minimum left by an
// earlier, suppressed dip (GenomeMiner.jl:93-103) -- whether `kmerDist < currminim` holds is then
// rounding noise.  Inside one binade every value of the chain is a multiple of the same ulp u, so
// d_{t+1} = d_t + round_u(inc_t): the DIFFERENCE between the chain values at two windows does not
// depend on the (unknown) low bits the chain carried in -- unless an addition lands exactly half
// way between two doubles or the chain changes binade on the way.  The resolver replays the
// reference's Float64 update (same operation order) from the window that set the running minimum
// to the last tied window, on the host, over the residues of that stretch only.  If no step was
// sensitive the outcome is what any IEEE-754 machine running the reference computes
// (KGMA_HIT_TIE_RESOLVED); otherwise exact arithmetic's choice is kept and KGMA_HIT_TIE is set.
// ------------------------------------------------------------------------------------------
namespace {

inline int res_code(uint8_t b)
{
    switch (b & 0xDF) {
    case 'A': return 0;
    case 'C': return 1;
    case 'G': return 2;
    default: return 3;      // T and N (validated earlier)
    }
}

struct TieResolver {
    kgma_ctx *ctx;
    const kgma_genome *g;
    std::vector<int32_t> cnt;
    std::vector<uint32_t> touched;
    std::vector<uint8_t> seqbuf;
    const uint8_t *pre = nullptr;        // residues under the tied stretch of every TIE-flagged dip (one gather)
    std::vector<int64_t> pre_off;        // per dip: offset into `pre`, or -1
    std::vector<const uint8_t *> pre_ptr; // per dip: residues gathered on the device behind the scan, or nullptr
    static constexpr int64_t MAX_SPAN = 1 << 22;
    static constexpr int64_t MAX_PREFETCH = (int64_t)256 << 20;
    std::unordered_map<uint32_t, int32_t> spcnt{};   // k >= 11: the window's counts (no 4^k table)

    // One gather launch + one download for all case-(A) dips (instead of a blocking copy per dip).
    void prefetch()
    {
        const size_t nd = ctx->dips.size();
        pre_off.assign(nd, -1);
        std::vector<int64_t> desc;
        int64_t total = 0;
        pre_ptr.assign(nd, nullptr);
        for (size_t i = 0; i < nd; i++) {
            const kgma_dip &d = ctx->dips[i];
            if (!(d.flags & KGMA_HIT_TIE) || ctx->kfv[(size_t)(d.kfv - 1)].fp) continue;
            const int64_t W = ctx->kfv[(size_t)(d.kfv - 1)].W;
            const int64_t span = ctx->dip_argl[i] - d.argmin;
            if (d.argmin < 1 || span < 0 || span > MAX_SPAN) continue;
            const int64_t nb = span + W;
            if (d.argmin - 1 + nb > g->cd[(size_t)d.contig].len) continue;
            // already gathered on the device behind the scan kernel?
            const int64_t ax = i < ctx->dip_aux.size() ? ctx->dip_aux[i] : -1;
            if (ax >= 0 && ctx->aux_host && ax + nb <= (int64_t)KGMA_AUX_BYTES && ax + nb <= (int64_t)((ctx->aux_used + 15u) & ~15u)) {
                pre_ptr[i] = ctx->aux_host + ax;
                continue;
            }
            if (total + nb > MAX_PREFETCH) continue;
            desc.push_back(g->cd[(size_t)d.contig].ascii_off + (d.argmin - 1));
            desc.push_back(total);
            desc.push_back(nb);
            pre_off[i] = total;
            total += nb;
        }
        if (desc.empty()) return;
        (void)hipSetDevice(ctx->device);
        const size_t desc_bytes = (desc.size() * sizeof(int64_t) + 255) & ~(size_t)255;
        const size_t need = desc_bytes + (size_t)total;
        bool ok = true;
        if (need > ctx->gath_cap) {
            if (ctx->h_gath) (void)hipHostFree(ctx->h_gath);
            if (ctx->d_gath) (void)hipFree(ctx->d_gath);
            ctx->h_gath = ctx->d_gath = nullptr; ctx->gath_cap = 0;
            const size_t cap = need + (need >> 1) + 65536;
            ok = hipHostMalloc(reinterpret_cast<void **>(&ctx->h_gath), cap, hipHostMallocDefault) == hipSuccess &&
                 hipMalloc(reinterpret_cast<void **>(&ctx->d_gath), cap) == hipSuccess;
            if (ok) ctx->gath_cap = cap;
        }
        if (ok) {
            memcpy(ctx->h_gath, desc.data(), desc.size() * sizeof(int64_t));
            ok = hipMemcpyAsync(ctx->d_gath, ctx->h_gath, desc_bytes, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
                 launch_gather_ranges(g->d_ascii, reinterpret_cast<const int64_t *>(ctx->d_gath), (int)(desc.size() / 3),
                                      ctx->d_gath + desc_bytes, ctx->stream) == hipSuccess &&
                 hipMemcpyAsync(ctx->h_gath + desc_bytes, ctx->d_gath + desc_bytes, (size_t)total, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
                 sync_spin(ctx->stream) == hipSuccess;
        }
        pre = ok ? ctx->h_gath + desc_bytes : nullptr;
        if (!ok) pre_off.assign(nd, -1);       // replay() falls back to its own copies
    }
    const uint8_t *prefetched(size_t dip_index) const
    {
        if (dip_index < pre_ptr.size() && pre_ptr[dip_index]) return pre_ptr[dip_index];
        return dip_index < pre_off.size() && pre_off[dip_index] >= 0 && pre ? pre + pre_off[dip_index] : nullptr;
    }

    struct Result { bool ok, sensitive, improved; int64_t pos; };
    int64_t n_calls = 0, n_fetches = 0, n_windows = 0;          // KGMA_TIE_DEBUG: what the replays cost
    double fetch_ms = 0;

    // Replays windows p_from .. cand_hi of record `contig` for KFV `kfv` (0-based).  The chain value
    // at p_from stands for the running minimum (exact value D_from).  Candidates are the windows in
    // [cand_lo, cand_hi] whose exact D equals Dmin.  With include_start the candidates must beat the
    // value at p_from (case B); otherwise p_from == cand_lo is itself the first candidate (case A).
    Result replay(int kfv, int64_t contig, int64_t p_from, int64_t D_from, int64_t cand_lo, int64_t cand_hi,
                  int64_t Dmin, bool include_start, const uint8_t *residues = nullptr)
    {
        Result r{false, true, false, cand_lo};
        if (!g && !ctx->fetch) return r;                    // no residues at hand (dips came from another GPU, no residue source set)
        const KfvInfo &f = ctx->kfv[(size_t)kfv];
        if (f.fp) return r;                                 // (a Float64 KFV has no exact lattice to replay on: its near ties stay flagged for the chain)
        // k = 1: no local decision either.  The replay starts from the exact distance as a stand-in for the reference's running value;
        // with four k-mers the increments are a handful of values repeated, their rounding errors add up instead of cancelling (1e-9
        // relative over 400 Mb), and the tied windows of a dip -- long plateaus of one exact distance on this coarse lattice -- are
        // ordered by exactly those low bits.  The ties stay flagged (KGMA_HIT_TIE) and KGMA_F_CHAIN_REPLAY decides them.
        if (ctx->k == 1) return r;
        const int k = ctx->k;
        const int64_t NB = (int64_t)1 << (2 * k);
        const uint64_t mask = (uint64_t)NB - 1;
        const int64_t W = f.W, N = f.N;
        if (p_from < 1 || cand_hi < p_from || cand_hi - p_from > MAX_SPAN) return r;
        const int64_t nbases = (cand_hi - p_from) + W;
        if (p_from - 1 + nbases > (g ? g->cd[(size_t)contig].len : ctx->contig_len[(size_t)contig])) return r;
        const uint8_t *seq = residues;
        n_calls++; n_windows += cand_hi - p_from;
        if (!seq) {
            const double tf0 = now_ms();
            n_fetches++;
            seqbuf.resize((size_t)nbases);
            if (g) {
                (void)hipSetDevice(ctx->device);
                if (hipMemcpy(seqbuf.data(), g->d_ascii + g->cd[(size_t)contig].ascii_off + (p_from - 1), (size_t)nbases,
                              hipMemcpyDeviceToHost) != hipSuccess) return r;
            } else if (ctx->fetch(ctx->fetch_user, (int32_t)contig, p_from, nbases, seqbuf.data()) != 0) {
                return r;                                   // the caller's residue source could not deliver
            }
            seq = seqbuf.data();
            fetch_ms += now_ms() - tf0;
        }
        if (!f.sparse && cnt.empty()) cnt.assign((size_t)NB, 0);
        spcnt.clear();
        auto C = [&](const uint64_t x) -> int32_t & { return f.sparse ? spcnt[(uint32_t)x] : cnt[(size_t)x]; };
        touched.clear();
        uint64_t km = 0;
        for (int64_t i = 0; i < W; i++) {
            km = ((km << 2) & mask) | (uint64_t)res_code(seq[(size_t)i]);
            if (i >= k - 1) { if (C(km)++ == 0) touched.push_back((uint32_t)km); }
        }
        uint64_t left = 0, right = 0;
        for (int64_t i = 0; i < k - 1; i++) left = (left << 2) | (uint64_t)res_code(seq[(size_t)i]);
        for (int64_t i = W - k + 1; i < W; i++) right = (right << 2) | (uint64_t)res_code(seq[(size_t)i]);
        const double SF = 1.0 / (double)k;
        const double scale = 2.0 * (double)k * (double)N * (double)N;
        int64_t D = D_from;
        double dist = (double)D / scale;            // grid-aligned stand-in for the chain value at p_from
        int e0;
        const double m0 = std::frexp(dist, &e0);
        bool sensitive = std::fabs(m0 - 0.5) < 1e-9 || std::fabs(m0 - 1.0) < 1e-9;   // chain may sit in the other binade
        double best = dist;
        bool improved = false;
        int64_t best_pos = p_from;
        bool consistent = true;
        for (int64_t s = p_from; s < cand_hi; s++) {     // roll window s -> s+1  (GenomeMiner.jl:60-77)
            const int64_t o = s - p_from;
            left = ((left << 2) & mask) | (uint64_t)res_code(seq[(size_t)(o + k - 1)]);
            right = ((right << 2) & mask) | (uint64_t)res_code(seq[(size_t)(o + W)]);
            if (left != right) {
                const int64_t cl = C(left), cr = C(right);
                double t = (double)(1 + cr);
                t = t + f.ref_at(left);
                t = t - f.ref_at(right);
                t = t - (double)cl;
                const double inc = SF * t;
                const double sum = dist + inc;
                const double bb = sum - dist;                          // TwoSum: exact error of the addition
                const double err = (dist - (sum - bb)) + (inc - bb);
                // exponent of the sum as frexp counts it, and half an ulp of its binade, from the bits (the distance is a
                // positive normal number; anything else is treated as rounding-sensitive)
                uint64_t sbits;
                memcpy(&sbits, &sum, sizeof sbits);
                const int ef = (int)((sbits >> 52) & 0x7FF);
                if (ef == 0 || ef == 0x7FF || (sbits >> 63)) sensitive = true;
                else {
                    const int es = ef - 1022;
                    const uint64_t hbits = (uint64_t)(ef - 53) << 52;          // 2^(es - 54)
                    double half_ulp;
                    memcpy(&half_ulp, &hbits, sizeof half_ulp);
                    if (ef <= 53 || std::fabs(err) == half_ulp || es != e0) sensitive = true;
                }
                dist = sum;
                D += 2 * N * N + 2 * N * ((f.S_at(left) - N * cl) - (f.S_at(right) - N * cr));
                if (C(right)++ == 0) touched.push_back((uint32_t)right);
                C(left)--;
            }
            const int64_t w = s + 1;
            if (w >= cand_lo) {
                if (D < Dmin) consistent = false;                      // the device minimum is exact: cannot happen
                if (D == Dmin && dist < best) { best = dist; best_pos = w; improved = true; }
            }
        }
        if (!f.sparse) for (uint32_t x : touched) cnt[(size_t)x] = 0;
        if (!consistent) return r;
        (void)include_start;
        r.ok = true; r.sensitive = sensitive; r.improved = improved; r.pos = best_pos;
        return r;
    }
};

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------------------
// scan: host replay of the hit state machine over the dips
// ------------------------------------------------------------------------------------------
// The reference's hit state machines (GenomeMiner.jl:82-104, OmnGenomeMiner.jl:113-156) over
// ctx->dips (sorted by record, KFV, start), ctx->firstD, ctx->contig_len / contig_nwin.  `g` may be
// NULL (dips gathered from other GPUs: kgma_replay_dips): ties that would need residues then stay flagged.
static int replay_hits(kgma_ctx *ctx, const kgma_genome *g, int32_t mode, int64_t buff, int64_t genome_pos0,
                       uint32_t flags, kgma_align_fn align, void *align_user)
{
    if (buff < 0) return fail(ctx, KGMA_E_ARG, "buff < 0");
    const bool resolve = !(flags & KGMA_F_NO_TIE_RESOLVE);
    TieResolver tr{ctx, g, {}, {}, {}, nullptr, {}, {}};
    if (resolve && g) tr.prefetch();
    int64_t n_resolved = 0, n_ambiguous = 0;
    const double t0 = now_ms();
    const int k = ctx->k;
    ctx->hits.clear();
    const int64_t nc = (int64_t)ctx->contig_len.size();
    size_t di = 0;   // dips are sorted by (contig, kfv, start)
    if (mode == KGMA_MODE_SINGLE) {
        const KfvInfo &f = ctx->kfv[0];
        const int64_t W = f.W;
        const double scale = 2.0 * (double)k * (double)f.N * (double)f.N;
        int64_t genome_pos = 0;                                         // GenomeMiner.jl:25
        for (int64_t c = 0; c < nc; c++) {
            const int64_t L = ctx->contig_len[(size_t)c];
            if (ctx->contig_nwin[(size_t)c] == 0) continue;            // L < W: :37-39
            const int64_t D1 = ctx->firstD[(size_t)c];
            int64_t CMI = 2, goal_ind = 0, currmin = D1;               // :57
            int64_t currmin_pos = 1;                                   // window whose value currminim holds
            bool stop = true;
            uint32_t cur_flags = 0;
            // a record decided by the Float64 chain replay compares the chain's values, like the reference
            const bool ch = !ctx->chain_pair.empty() && ctx->chain_pair[(size_t)c] != 0;
            double currmin_f = ch ? ctx->firstF[(size_t)c] : 0.0;
            while (di < ctx->dips.size() && ctx->dips[di].contig < c) di++;
            for (; di < ctx->dips.size() && ctx->dips[di].contig == c; di++) {
                kgma_dip &d = ctx->dips[di];
                bool improved = ch ? ctx->dip_fmin[di] < currmin_f : d.D_min < currmin;   // :83-87 (strict running minimum)
                int64_t best_pos = d.argmin;
                uint32_t dflags = d.flags;
                if (ch) {
                    // nothing to decide: argmin is the first window attaining the chain's minimum
                } else if (f.fp) {
                    // Float64 KFV: a minimum within rounding noise of the running minimum is flagged (exact order kept)
                    if (near_tie(f, d.D_min, currmin)) dflags |= KGMA_HIT_TIE;
                } else if (resolve && improved && (d.flags & KGMA_HIT_TIE)) {
                    // (A) several separated windows attain the dip's minimum
                    const TieResolver::Result r = tr.replay(0, c, d.argmin, d.D_min, d.argmin, ctx->dip_argl[di], d.D_min, false, tr.prefetched(di));
                    if (r.ok && !r.sensitive) {
                        best_pos = r.pos;
                        dflags = (dflags & ~(uint32_t)KGMA_HIT_TIE) | KGMA_HIT_TIE_RESOLVED;
                        n_resolved++;
                    } else n_ambiguous++;
                } else if (resolve && !improved && d.D_min == currmin) {
                    // (B) the dip's minimum equals the stale running minimum exactly
                    const TieResolver::Result r = tr.replay(0, c, currmin_pos, currmin, d.start, ctx->dip_argl[di], d.D_min, true);
                    if (r.ok && !r.sensitive) {
                        dflags |= KGMA_HIT_TIE_RESOLVED;
                        n_resolved++;
                        if (r.improved) { improved = true; best_pos = r.pos; }
                    } else { dflags |= KGMA_HIT_TIE; n_ambiguous++; }
                } else if (!resolve && !improved && d.D_min == currmin) {
                    dflags |= KGMA_HIT_TIE;
                }
                d.flags = dflags;
                if (improved) {
                    currmin = d.D_min;
                    if (ch) currmin_f = ctx->dip_fmin[di];
                    currmin_pos = best_pos;
                    d.argmin = best_pos;
                    CMI = best_pos + k - 2;                            // i_left of the best window
                    stop = false;
                    cur_flags = dflags;
                }
                if (d.exit_pos == 0) continue;                         // dip still open at the record end
                if (!stop) {                                           // :90-104
                    stop = true;
                    CMI += 1;
                    if (CMI > goal_ind) {
                        goal_ind = CMI + W - 1;
                        int64_t lo = std::max<int64_t>(CMI - buff, 1);
                        int64_t hi = std::min<int64_t>(CMI + W - 1 + buff, L);
                        if (align) align(align_user, (int32_t)c, 0, lo, hi, L, &lo, &hi);   // :96-99
                        kgma_hit h;
                        memset(&h, 0, sizeof h);
                        h.contig = (int32_t)c; h.kfv = 0; h.cmi = CMI; h.lo = lo; h.hi = hi;
                        h.genome_pos = genome_pos; h.D = currmin; h.dist = ch ? currmin_f : (double)currmin / scale;
                        h.flags = cur_flags | (d.flags & KGMA_HIT_AT_THRESHOLD);
                        ctx->hits.push_back(h);
                        currmin = d.D_exit;                            // :102
                        if (ch) currmin_f = ctx->dip_fexit[di];
                        currmin_pos = d.exit_pos;
                    }
                }
            }
            genome_pos += L;                                           // :106
        }
    } else {
        const int m = ctx->m;
        int64_t genome_pos = genome_pos0;                              // OmnGenomeMiner.jl:25
        std::vector<int64_t> curr_mins((size_t)m), CMIs((size_t)m);
        std::vector<char> stops((size_t)m);
        std::vector<uint32_t> cflags((size_t)m);
        std::vector<kgma_dip *> evs;
        std::vector<int64_t> min_pos((size_t)m, 1);
        std::vector<double> curr_mins_f((size_t)m, 0.0);
        std::vector<char> chj((size_t)m, 0);
        for (int64_t c = 0; c < nc; c++) {
            const int64_t L = ctx->contig_len[(size_t)c];
            while (di < ctx->dips.size() && ctx->dips[di].contig < c) di++;
            if (ctx->contig_nwin[(size_t)c] > 0) {
                int64_t prev_lo = 0, prev_hi = 0;                      // prev_hit_range = 0:0, :59
                for (int j = 0; j < m; j++) {                          // :61-82
                    curr_mins[(size_t)j] = ctx->firstD[(size_t)j * (size_t)nc + (size_t)c];
                    CMIs[(size_t)j] = 1; stops[(size_t)j] = 1; cflags[(size_t)j] = 0; min_pos[(size_t)j] = 1;
                    chj[(size_t)j] = !ctx->chain_pair.empty() && ctx->chain_pair[(size_t)j * (size_t)nc + (size_t)c] != 0;
                    curr_mins_f[(size_t)j] = chj[(size_t)j] ? ctx->firstF[(size_t)j * (size_t)nc + (size_t)c] : 0.0;
                }
                evs.clear();
                for (; di < ctx->dips.size() && ctx->dips[di].contig == c; di++) evs.push_back(&ctx->dips[di]);
                // per-KFV minimum updates happen inside the dip, exits are ordered by (iteration, KFV)
                std::stable_sort(evs.begin(), evs.end(), [](const kgma_dip *a, const kgma_dip *b) {
                    const int64_t ea = a->exit_pos ? a->exit_pos : INT64_MAX, eb = b->exit_pos ? b->exit_pos : INT64_MAX;
                    if (ea != eb) return ea < eb;
                    return a->kfv < b->kfv;
                });
                for (kgma_dip *dp : evs) {
                    kgma_dip &d = *dp;
                    const int j = d.kfv - 1;
                    const KfvInfo &f = ctx->kfv[(size_t)j];
                    const size_t dix = (size_t)(dp - ctx->dips.data());
                    const bool ch = chj[(size_t)j] != 0;
                    bool improved = ch ? ctx->dip_fmin[dix] < curr_mins_f[(size_t)j] : d.D_min < curr_mins[(size_t)j];    // :114-119
                    int64_t best_pos = d.argmin;
                    uint32_t dflags = d.flags;
                    if (ch) {
                        // decided by the Float64 chain replay
                    } else if (f.fp) {
                        if (near_tie(f, d.D_min, curr_mins[(size_t)j])) dflags |= KGMA_HIT_TIE;
                    } else if (resolve && improved && (d.flags & KGMA_HIT_TIE)) {
                        const TieResolver::Result r = tr.replay(j, c, d.argmin, d.D_min, d.argmin, ctx->dip_argl[dix], d.D_min, false, tr.prefetched(dix));
                        if (r.ok && !r.sensitive) {
                            best_pos = r.pos;
                            dflags = (dflags & ~(uint32_t)KGMA_HIT_TIE) | KGMA_HIT_TIE_RESOLVED;
                            n_resolved++;
                        } else n_ambiguous++;
                    } else if (resolve && !improved && d.D_min == curr_mins[(size_t)j]) {
                        const TieResolver::Result r = tr.replay(j, c, min_pos[(size_t)j], curr_mins[(size_t)j], d.start, ctx->dip_argl[dix], d.D_min, true);
                        if (r.ok && !r.sensitive) {
                            dflags |= KGMA_HIT_TIE_RESOLVED;
                            n_resolved++;
                            if (r.improved) { improved = true; best_pos = r.pos; }
                        } else { dflags |= KGMA_HIT_TIE; n_ambiguous++; }
                    } else if (!resolve && !improved && d.D_min == curr_mins[(size_t)j]) {
                        dflags |= KGMA_HIT_TIE;
                    }
                    d.flags = dflags;
                    if (improved) {
                        curr_mins[(size_t)j] = d.D_min;
                        if (ch) curr_mins_f[(size_t)j] = ctx->dip_fmin[dix];
                        min_pos[(size_t)j] = best_pos;
                        d.argmin = best_pos;
                        CMIs[(size_t)j] = best_pos - 1;                // i = window start - 1
                        stops[(size_t)j] = 0;
                        cflags[(size_t)j] = dflags;
                    }
                    if (d.exit_pos == 0) continue;
                    if (!stops[(size_t)j]) {                           // :122
                        stops[(size_t)j] = 1;
                        const int64_t CMI = CMIs[(size_t)j];
                        if (!(CMI >= prev_lo && CMI <= prev_hi)) {     // :126
                            int64_t lo = std::max<int64_t>(CMI - buff, 1);
                            int64_t hi = std::min<int64_t>(CMI + f.W - 1 + buff, L);
                            if (align) align(align_user, (int32_t)c, j + 1, lo, hi, L, &lo, &hi);   // :130-136
                            if (hi < prev_lo || lo > prev_hi) {        // :139
                                kgma_hit h;
                                memset(&h, 0, sizeof h);
                                h.contig = (int32_t)c; h.kfv = j + 1; h.cmi = CMI; h.lo = lo; h.hi = hi;
                                h.genome_pos = genome_pos; h.D = curr_mins[(size_t)j];
                                h.dist = ch ? curr_mins_f[(size_t)j] : (double)h.D / (2.0 * (double)k * (double)f.N * (double)f.N);
                                h.flags = cflags[(size_t)j] | (d.flags & KGMA_HIT_AT_THRESHOLD);
                                ctx->hits.push_back(h);
                                prev_lo = lo; prev_hi = hi;            // :152
                                curr_mins[(size_t)j] = d.D_exit;       // :153
                                if (ch) curr_mins_f[(size_t)j] = ctx->dip_fexit[dix];
                                min_pos[(size_t)j] = d.exit_pos;
                            }
                        }
                    }
                }
            }
            genome_pos += L;                                           // :159 (always)
        }
    }
    ctx->stats.n_hits = (int64_t)ctx->hits.size();
    ctx->stats.n_tie_flagged = 0;
    for (const kgma_dip &dd : ctx->dips) ctx->stats.n_tie_flagged += (dd.flags & KGMA_HIT_TIE) ? 1 : 0;
    (void)n_resolved; (void)n_ambiguous;
    ctx->stats.replay_ms = now_ms() - t0;
    if (getenv("KGMA_TIE_DEBUG"))
        fprintf(stderr, "tie resolver: %lld replays (%lld with their own residue download: %.2f ms), %lld windows walked; replay %.2f ms\n",
                (long long)tr.n_calls, (long long)tr.n_fetches, tr.fetch_ms, (long long)tr.n_windows, ctx->stats.replay_ms);
    return KGMA_OK;
}

// ------------------------------------------------------------------------------------------
// The chain on the device.  For the given (record, KFV) pairs the reference's running Float64 value is wanted at the
// windows of `iv`.  stream8_kernel<..., CHAIN> walks windows 1 .. last of every pair in streams of `T` transitions
// (same count table, same exact counts as the scan), forms each window's Float64 increment in the reference's
// operation order and reduces it chunk by chunk to what the host needs (kgma_device.h: ChainChunk); the host then
// walks each pair's chunks in order (kgma_chain.cpp: run_chain_walks) -- an integer add per regular chunk, hardware
// additions through the chunks that hold a wanted window or may change binade.  Pairs the kernel does not serve
// (k, window length, a KFV that is not RN(S * (1/N))) or whose walk fails a check are left to the host chain.
//
// The host control, per batch of pairs (ChainBatch): plan_chain_launches, plan_chain_streams and mark_hot_steps decide
// everything before the device is touched (ChainPlan); reserve_chain_buffers and run_chain_kernels size the buffers and
// launch (with the pool-regrowth retry); start_download lays out the pinned mirror and starts the copies; finish --
// first_windows, then the export or walk_pairs -- is the host part, run by chain_on_device on a worker while the next
// batch's device part runs.
// ------------------------------------------------------------------------------------------
static void reset_chain_stats(kgma_ctx *ctx)
{
    ctx->stats.chain_ms = 0; ctx->stats.n_chain_pairs = 0; ctx->stats.chain_windows = 0;
    ctx->stats.chain_device_pairs = 0; ctx->stats.chain_device_ms = 0; ctx->stats.chain_raw_steps = 0; ctx->stats.chain_max_drift = 0;
}

struct ChainPair {
    int32_t c, j;
    size_t d0, d1, a0, a1;                 // its dips / guard-band windows in ctx->dips / ctx->att
    std::vector<ChainInterval> iv;
    std::vector<double> val;
    int64_t last;
};

// What the device chains of one call add up to.  Two threads write it, each its own fields: the thread that runs the batches'
// device parts (plan, launches) the first line, the one that runs a batch's host part (ChainBatch::finish: chain_on_device's
// worker, or the same thread when nothing follows the batch) the second.
struct ChainDevInfo {
    int64_t chunks = 0; double setup_ms = 0, kernel_ms = 0; int attempts = 0;
    int64_t pairs = 0, windows = 0, raw_steps = 0, streams = 0; double copy_ms = 0, walk_ms = 0, max_drift = 0;
};

// The chain's switches, read once per entry (chain_decide, kgma_chain_values, kgma_chain_export) and never kept on the
// context: tests change them between calls on one context
struct ChainEnv {
    bool debug = false;                            // KGMA_CHAIN_DEBUG
    bool host_only = false;                        // KGMA_CHAIN=host (tests): chain_decide keeps every pair on the host chain
    int generic = -1;                              // KGMA_CHAIN_GENERIC (tests): 0 / 1 never / always the generic chain kernel; -1: not set
    int group = 1;                                 // KGMA_CHAIN_GROUP: KFVs per chain launch, 1 .. 4
    bool stream_set = false; int64_t stream = 0;   // KGMA_CHAIN_STREAM (experiments / tests): transitions per stream
    int64_t pool_units = 0;                        // KGMA_CHAIN_POOL_UNITS (tests: force the regrowth); 0: not set
    int64_t batch_windows = (int64_t)1 << 35;      // KGMA_CHAIN_BATCH_WINDOWS (tests): windows per device batch
    int64_t batch_bytes = (int64_t)2 << 30;        // KGMA_CHAIN_BATCH_MB (experiments): 2-bit codes per host batch
    int threads = 1;                               // KGMA_CHAIN_THREADS: host threads of the chains and walks, 1 .. 64
};

static ChainEnv read_chain_env()
{
    ChainEnv v;
    v.debug = getenv("KGMA_CHAIN_DEBUG") != nullptr;
    if (const char *e = getenv("KGMA_CHAIN")) v.host_only = !strcmp(e, "host");
    if (const char *e = getenv("KGMA_CHAIN_GENERIC")) v.generic = atoi(e);
    if (const char *e = getenv("KGMA_CHAIN_GROUP")) v.group = std::max(1, std::min(4, atoi(e)));
    if (const char *e = getenv("KGMA_CHAIN_STREAM")) { v.stream_set = true; v.stream = atoll(e); }
    if (const char *e = getenv("KGMA_CHAIN_POOL_UNITS")) v.pool_units = std::max<int64_t>(1, atoll(e));
    if (const char *e = getenv("KGMA_CHAIN_BATCH_WINDOWS")) v.batch_windows = std::max<int64_t>(1, atoll(e));
    if (const char *e = getenv("KGMA_CHAIN_BATCH_MB")) v.batch_bytes = std::max<int64_t>(1, atoll(e)) << 20;
    v.threads = (int)std::thread::hardware_concurrency();
    if (const char *e = getenv("KGMA_CHAIN_THREADS")) v.threads = atoi(e);
    v.threads = std::max(1, std::min(v.threads, 64));
    return v;
}

// which chain kernel serves a KFV: 1 = stream8_kernel<..., CHAIN> (k = 5, 6, 7, S/N KFVs in one of the two forms), 2 = the generic chain
// kernel (any k, any window, any KFV: it reads the caller's table), 0 = none (the host chain).  KGMA_CHAIN_GENERIC=0 / 1 (tests):
// never / always the generic one.
static int chain_kernel_for(const kgma_ctx *ctx, const KfvInfo &f, const ChainEnv &env)
{
    const int k = ctx->k, nk = (int)(f.W - k + 1);
    const bool s8 = !f.fp && (f.fits32 || f.big_ok) && chain_applies(k, nk, f.N, f.Smax <= 32767, !f.fits32) && f.ref_form >= 0 &&
                    chain_slots_per_cu(k, f.Smax <= 32767, 1, nk, !f.fits32) >= 1;
    if (s8 && env.generic != 1) return 1;
    if (env.generic == 0) return 0;
    return k >= 1 && k <= KGMA_MAX_K && nk >= 1 && nk <= KGMA_MAX_NK_WIDE && generic_chain_slots_per_cu(k, nk) >= 1 ? 2 : 0;
}

// 2 k N^2: a KFV's exact distance is D / chain_scale
static double chain_scale(int k, const KfvInfo &f)
{
    return 2.0 * (double)k * (double)f.N * (double)f.N;
}

// One host chain of KFV `f` over a record given as 2-bit codes: windows 1 .. last, sampled at `iv`
static ChainJob chain_job(const KfvInfo &f, int k, const uint32_t *packed, int64_t n_res, int64_t last, const ChainInterval *iv, size_t n_iv, double *out)
{
    ChainJob J;
    J.seq = nullptr; J.packed = packed; J.n_res = n_res; f.chain_ref(J);
    J.k = k; J.W = f.W; J.last_window = last; J.iv = iv; J.n_iv = n_iv; J.out = out; J.n_out = 0; J.ok = false;
    return J;
}

// the chain's value at window 1: kmer_count! + sqeuclidean of the first window (GenomeMiner.jl:42-47), on the host
static ChainJob first_window_job(const KfvInfo &f, int k, const uint32_t *packed, double *out)
{
    static const ChainInterval one{1, 1};
    return chain_job(f, k, packed, f.W, 1, &one, 1, out);
}

// ---- the plan of one batch: everything that is decided before the device is touched ----------------------------------
struct ChainLaunch { std::vector<int> kfvs; size_t t0, t1; int64_t T, chunk0, n_chunks; size_t d0_off; bool s16; };
struct PairStreams { size_t s0, s1; int64_t T; };                // into `streams` (per pair: its slot's chunk and D0 indices)

struct ChainPlan {
    bool generic = false;                                         // the generic chain kernel's batch (one KFV per launch)
    std::vector<ChainLaunch> launches;
    std::vector<TileDesc> tiles;
    std::vector<ChainStream> streams;
    std::vector<size_t> stream_d0;                                // index of each stream's first-window D in the downloaded array
    std::vector<PairStreams> ps;                                  // per pair of the batch
    int64_t n_chunks = 0, total_steps = 0;
    size_t d0_total = 0;
    // hot steps: every step that holds a transition into a wanted window, as one 64-bit mask per chunk that has any
    size_t hot_words = 0;
    std::vector<uint32_t> hot;                                    // [bit per chunk | hot chunks before each word]
    std::vector<uint64_t> hot_masks;                              // (never empty: one zero word when no chunk is hot)
    int64_t hot_steps = 0, hot_chunks = 0;

    int64_t n_tiles() const { return (int64_t)tiles.size(); }
    // (beyond these the batch is left to the host chain)
    bool fits() const { return n_tiles() <= 0x7FFFFFF0ll && n_chunks <= 0x7FFFFFF0ll && (int64_t)d0_total <= 0x7FFFFFF0ll; }
};

// ---- launch groups: the KFVs of one window size share the count table of a pass, so up to `maxg` of them that are
//      wanted on this batch CAN go into one launch (slots; a record's streams carry the mask of the slots it is flagged
//      for).  Measured, it does not pay: the flags are sparse (config 5: 268 of 800 (record, KFV) pairs, a record is
//      rarely wanted for two KFVs of one size), every slot costs its prefix sum in every step, and the 2-4 slot variants
//      spill 60-320 scalar registers -- config 4 (k = 6): chain kernels 16.0 ms with one KFV per launch, 18.8 ms with
//      two slots, 30.4 ms with four; a 20 Gb config-5 genome (k = 7): 145 ms against 191 ms with four slots.  So: one
//      KFV per launch; KGMA_CHAIN_GROUP=2..4 keeps the grouped form reachable for tests and for tie-dense inputs.
static void plan_chain_launches(const kgma_ctx *ctx, const ChainEnv &env, const std::vector<ChainPair> &pairs, const std::vector<size_t> &el, ChainPlan &plan)
{
    const int k = ctx->k;
    const int maxg = plan.generic ? 1 : env.group;                     // (the generic chain kernel walks one KFV)
    // KFVs wanted, by (k-mers per window, int16 tables)
    std::vector<int> kf;
    for (size_t u : el) kf.push_back(pairs[u].j);
    std::sort(kf.begin(), kf.end());
    kf.erase(std::unique(kf.begin(), kf.end()), kf.end());
    std::stable_sort(kf.begin(), kf.end(), [&](int a, int b) {
        const KfvInfo &fa = ctx->kfv[(size_t)a], &fb = ctx->kfv[(size_t)b];
        if (fa.W != fb.W) return fa.W < fb.W;
        return (fa.Smax <= 32767) > (fb.Smax <= 32767);
    });
    for (size_t i = 0; i < kf.size();) {
        const KfvInfo &f0 = ctx->kfv[(size_t)kf[i]];
        const bool s16 = f0.Smax <= 32767;
        size_t e = i + 1;
        while (!plan.generic && e < kf.size() && (int)(e - i) < (s16 ? maxg : 1) && ctx->kfv[(size_t)kf[e]].W == f0.W && (ctx->kfv[(size_t)kf[e]].Smax <= 32767) == s16 &&
               f0.fits32 && ctx->kfv[(size_t)kf[e]].fits32 && chain_slots_per_cu(k, s16, (int)(e - i) + 1, (int)(f0.W - k + 1), false) > 0)
            e++;
        ChainLaunch L;
        L.kfvs.assign(kf.begin() + (long)i, kf.begin() + (long)e);
        L.s16 = s16; L.t0 = L.t1 = 0; L.T = 0; L.chunk0 = L.n_chunks = 0; L.d0_off = 0;
        plan.launches.push_back(L);
        i = e;
    }
}

// Per launch: its records, the stream length, the stream table (tiles) and every pair's view of its record's streams
static void plan_chain_streams(const kgma_ctx *ctx, const kgma_genome *g, const ChainEnv &env, const std::vector<ChainPair> &pairs, const std::vector<size_t> &el,
                               ChainPlan &plan)
{
    const int k = ctx->k;
    std::vector<TileDesc> &tiles = plan.tiles;
    plan.ps.assign(el.size(), PairStreams{0, 0, 0});
    for (ChainLaunch &L : plan.launches) {
        const int nslots = (int)L.kfvs.size();
        const int nk = (int)(ctx->kfv[(size_t)L.kfvs[0]].W - k + 1);
        // the records of this launch: per record the slots wanted and the last window any of them wants
        struct LaunchRecord { int32_t c; uint32_t mask; int64_t last; };
        std::vector<LaunchRecord> recs;
        for (size_t u = 0; u < el.size(); u++) {
            const ChainPair &p = pairs[el[u]];
            const auto it = std::find(L.kfvs.begin(), L.kfvs.end(), p.j);
            if (it == L.kfvs.end()) continue;
            const uint32_t bit = 1u << (it - L.kfvs.begin());
            auto r = std::find_if(recs.begin(), recs.end(), [&](const LaunchRecord &x) { return x.c == p.c; });
            if (r == recs.end()) recs.push_back(LaunchRecord{p.c, bit, p.last});
            else { r->mask |= bit; r->last = std::max(r->last, p.last); }
        }
        std::sort(recs.begin(), recs.end(), [](const LaunchRecord &a, const LaunchRecord &b) { return a.c < b.c; });
        int64_t windows = 0;
        for (const LaunchRecord &r : recs) windows += r.last;
        // transitions per stream: about three rounds of streams over the chip, 64 | T (streams start on plane words), at most
        // 2^18 (the drift a stream may add stays far below the guard band)
        int64_t T;
        {
            const int64_t slots = (int64_t)std::max(1, ctx->n_cus) *
                                  (plan.generic ? generic_chain_slots_per_cu(k, nk) : chain_slots_per_cu(k, L.s16, nslots, nk, !ctx->kfv[(size_t)L.kfvs[0]].fits32));
            T = (windows + slots * 3 - 1) / (slots * 3);
            if (env.stream_set) T = env.stream;
            // (a stream's warm-up is its window's n k-mers: streams of at least 4 n transitions)
            T = std::min<int64_t>(std::max<int64_t>(((T + 63) / 64) * 64, std::max<int64_t>(1024, (((int64_t)4 * nk + 63) / 64) * 64)), (int64_t)1 << 18);
        }
        L.T = T;
        L.t0 = tiles.size();
        L.chunk0 = plan.n_chunks;
        int64_t local_chunks = 0;
        std::vector<std::pair<size_t, size_t>> rec_tiles(recs.size());
        for (size_t ri = 0; ri < recs.size(); ri++) {
            const LaunchRecord &r = recs[ri];
            rec_tiles[ri].first = tiles.size();
            for (int64_t win0 = 1; win0 < r.last; win0 += T) {
                TileDesc td;
                td.word_base = g->cd[(size_t)r.c].word_off + (win0 - 1) / 32;
                td.win0 = win0;
                td.dist_base = L.chunk0 + local_chunks;                // (chain launches: slot 0's chunk of the stream's first chunk)
                td.n_valid = (int32_t)std::min<int64_t>(T + 1, r.last - win0 + 1);
                td.first_test = (int32_t)r.mask;                       // (chain launches: the slots this record wants)
                td.contig = r.c;
                td.pad = 0;
                tiles.push_back(td);
                const int64_t nb = ((int64_t)td.n_valid + nk - 1 + 63) >> 6;
                local_chunks += (nb + KGMA_CHAIN_STEPS - 1) / KGMA_CHAIN_STEPS;
                plan.total_steps += nb * __builtin_popcount(r.mask);
            }
            rec_tiles[ri].second = tiles.size();
        }
        L.t1 = tiles.size();
        L.n_chunks = local_chunks;
        plan.n_chunks += local_chunks * nslots;
        L.d0_off = plan.d0_total;
        plan.d0_total += (size_t)ctx->m * (L.t1 - L.t0);              // the kernel indexes first-window D by [KFV][stream of the launch]
        // every pair's view of its record's streams: its own slot's chunk records and first-window D
        for (size_t u = 0; u < el.size(); u++) {
            const ChainPair &p = pairs[el[u]];
            const auto it = std::find(L.kfvs.begin(), L.kfvs.end(), p.j);
            if (it == L.kfvs.end()) continue;
            const int64_t slot = it - L.kfvs.begin();
            size_t ri = 0;
            while (recs[ri].c != p.c) ri++;
            plan.ps[u].s0 = plan.streams.size();
            plan.ps[u].T = T;
            for (size_t t = rec_tiles[ri].first; t < rec_tiles[ri].second; t++) {
                const TileDesc &td = tiles[t];
                if (td.win0 >= p.last) break;                           // (the record's streams go on for another slot)
                plan.streams.push_back(ChainStream{td.win0, td.dist_base + slot * L.n_chunks, 0, td.n_valid, 0});
                plan.stream_d0.push_back(L.d0_off + (size_t)p.j * (L.t1 - L.t0) + (t - L.t0));
            }
            plan.ps[u].s1 = plan.streams.size();
        }
    }
}

static void mark_hot_steps(const kgma_ctx *ctx, const std::vector<ChainPair> &pairs, const std::vector<size_t> &el, ChainPlan &plan)
{
    const int k = ctx->k;
    const size_t hot_words = plan.hot_words = (size_t)(plan.n_chunks + 31) / 32 + 1;
    plan.hot.assign(2 * hot_words, 0u);
    std::vector<std::pair<int64_t, uint64_t>> marks;                   // (chunk, step bit), in stream order per pair
    for (size_t u = 0; u < el.size(); u++) {
        const ChainPair &p = pairs[el[u]];
        const int nk = (int)(ctx->kfv[(size_t)p.j].W - k + 1);
        for (const ChainInterval &x : p.iv)
            for (int64_t w = std::max<int64_t>(x.lo, 2); w <= x.hi; w++) {
                const int64_t si = (w - 2) / plan.ps[u].T;
                const ChainStream &S = plan.streams[plan.ps[u].s0 + (size_t)si];
                const int64_t pos = (w - S.win0) + nk - 1;
                const int64_t cid = S.chunk_base + (pos >> (6 + KGMA_CHAIN_STEPS_LOG2));
                marks.emplace_back(cid, (uint64_t)1 << ((pos >> 6) & (KGMA_CHAIN_STEPS - 1)));
                // (jump to the step's last window: the windows of one step share the bit)
                const int64_t w_step_last = S.win0 + (pos | 63) - nk + 1;
                if (w_step_last > w) w = std::min(w_step_last, std::min<int64_t>(x.hi, S.win0 + S.n_valid - 1));
            }
    }
    std::sort(marks.begin(), marks.end());
    for (size_t i = 0; i < marks.size();) {
        uint64_t m = 0;
        size_t j = i;
        while (j < marks.size() && marks[j].first == marks[i].first) m |= marks[j++].second;
        plan.hot[(size_t)(marks[i].first >> 5)] |= 1u << (marks[i].first & 31);
        plan.hot_masks.push_back(m);
        plan.hot_steps += __builtin_popcountll(m);
        i = j;
    }
    uint32_t before = 0;
    for (size_t wd = 0; wd < hot_words; wd++) { plan.hot[hot_words + wd] = before; before += (uint32_t)__builtin_popcount(plan.hot[wd]); }
    plan.hot_chunks = (int64_t)plan.hot_masks.size();
    if (plan.hot_masks.empty()) plan.hot_masks.push_back(0);
}

// ---- the device part of one batch ---------------------------------------------------------------------------------------
// (everything but the pool, which run_chain_kernels sizes; `set`: the other set may still be on its way to the host)
static int reserve_chain_buffers(kgma_ctx *ctx, const ChainPlan &plan, ChainBufferSet &set)
{
    int rc = dev_reserve(ctx, ctx->d_ctiles, ctx->ctiles_cap, plan.n_tiles());
    if (rc) return rc;
    if (!ctx->chain_copy_stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->chain_copy_stream, hipStreamNonBlocking));
    rc = dev_reserve(ctx, set.chunks, set.chunks_cap, plan.n_chunks);
    if (rc) return rc;
    rc = dev_reserve(ctx, ctx->d_chot, ctx->chot_cap, (int64_t)plan.hot.size());
    if (rc) return rc;
    rc = dev_reserve(ctx, ctx->d_chmask, ctx->chmask_cap, (int64_t)plan.hot_masks.size());
    if (rc) return rc;
    rc = dev_reserve(ctx, set.D0, set.D0_cap, (int64_t)plan.d0_total);
    if (rc) return rc;
    if (!ctx->d_cctl) HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_cctl), 16));
    return KGMA_OK;
}

// One launch of the batch: the parameters of its KFVs, its slice of the stream table, the batch's output buffers
static int launch_chain_group(kgma_ctx *ctx, const kgma_genome *g, const ChainPlan &plan, const ChainLaunch &L, const ChainBufferSet &set, int64_t pool_units)
{
    const int k = ctx->k, nslots = (int)L.kfvs.size();
    GroupParams gp;
    memset(&gp, 0, sizeof gp);
    ScanArgs a;
    memset(&a, 0, sizeof a);
    gp.n_kfv = nslots; gp.k = k;
    gp.nk = gp.nk_min = (int32_t)(ctx->kfv[(size_t)L.kfvs[0]].W - k + 1);
    gp.need_wide = ctx->kfv[(size_t)L.kfvs[0]].fits32 ? 0 : 1;
    fill_group_params(ctx, L.kfvs, gp);
    // (a launch's KFVs have one window size and one S width; the chain kernels do not look at s_fits_u8)
    gp.n_sizes = 1; gp.sizes[0] = gp.nk;
    gp.s_fits_i16 = L.s16 ? 1 : 0;
    for (int u = 0; u < nslots; u++) {
        const KfvInfo &f = ctx->kfv[(size_t)L.kfvs[(size_t)u]];
        gp.chain_invN[u] = 1.0 / (double)f.N;
        gp.chain_form[u] = f.ref_form;
    }
    a.inter = g->d_inter;
    a.tiles = ctx->d_ctiles + L.t0;
    a.n_tiles = (int32_t)(L.t1 - L.t0);
    a.Stab = ctx->d_Stab;
    if (!plan.generic && k >= 7) {
        // k = 7: the kernel gathers S from global memory, one row of int16 slots per k-mer (the scan's compacted layout)
        const int nv = nslots == 3 ? 4 : nslots;                       // row width in int16 slots (the kernel variant's)
        const int rc = sinter_tables(ctx, L.kfvs, nv, &a.Sinter, &a.Sbits);
        if (rc) return rc;
    }
    if (!plan.generic && stream8_state_words(k, nslots) > 0) {
        const int rc = dev_reserve(ctx, ctx->d_wstate, ctx->wstate_cap, (int64_t)(L.t1 - L.t0) * stream8_state_words(k, nslots));
        if (rc) return rc;
        a.wave_state = ctx->d_wstate;
    }
    a.D0out = set.D0 + L.d0_off;                                       // [KFV][stream of this launch]
    a.n_chunk_tiles = a.n_tiles;
    a.chain.chunks = set.chunks;
    a.chain.pool = set.pool;
    a.chain.pool_cursor = ctx->d_cctl;
    a.chain.pool_cap = (unsigned int)pool_units;
    a.chain.hot = ctx->d_chot;
    a.chain.hot_prefix = ctx->d_chot + plan.hot_words;
    a.chain.hot_masks = ctx->d_chmask;
    a.chain.chunk_stride = L.n_chunks;
    a.chain.SF = 1.0 / (double)k;                                      // src/API.jl:86,204
    a.chain.guard = 1.862645149230957e-09;                             // 2^-29
    a.chain.guard_abs = 9.313225746154785e-10;                         // 2^-30 of the stream's first distance
    a.chain.status = ctx->d_cctl + 1;
    if (plan.generic) {
        GenParams gg;                                                  // (the chain walks the Float64 table whatever the KFV's form)
        const int rc = fill_gen_params(ctx, L.kfvs[0], gp.nk, gp.nk, (int32_t)((int64_t)std::max(1, ctx->n_cus) * generic_chain_slots_per_cu(k, gp.nk)), true, "chain", gg);
        if (rc) return rc;
        HIP_TRY(ctx, launch_generic_chain(a, gg, ctx->stream));
        return KGMA_OK;
    }
    HIP_TRY(ctx, launch_chain(a, gp, ctx->stream));
    return KGMA_OK;
}

// One batch of pairs on the device.  It owns what its host part needs -- the plan, the download layout, the list of its pairs --
// so that finish() can run on chain_on_device's worker after the frame that built the batch is gone: finish() touches what the
// batch owns, the pinned mirror of its buffer set (not reused before the worker is joined), the context's reference tables
// (constant during the call) and, of the caller's, `pairs` / `done` / `info` alone, which outlive the worker (chain_on_device
// joins it before it returns).  The worker and the launching thread write disjoint fields of `info` (ChainDevInfo) and disjoint
// elements of `done` and of the pairs' values.
struct ChainBatch {
    kgma_ctx *ctx; const kgma_genome *g; ChainEnv env;
    std::vector<ChainPair> &pairs; std::vector<char> &done; ChainDevInfo &info;
    std::vector<size_t> el;                        // the batch's pairs (indices into `pairs`)
    ChainBufferSet *set;                           // output buffers and pinned mirror of this batch
    bool export_only = false;                      // kgma_chain_export: the pair's material goes to the context, nothing is walked
    ChainPlan plan;
    int64_t pool_units = 0;                        // the pool the launches ran with, cut to what they used
    bool downloading = false;                      // start_download() ran: finish() is due
    // the download: [D0 per stream | chunk records | the used part of the pool | per record the residues of its first window]
    struct RecordSlice { int32_t c; size_t dw_off, dw; };
    std::vector<RecordSlice> recs;
    size_t off_D0 = 0, off_chunks = 0, off_raw = 0, off_first = 0;
    const uint8_t *pin = nullptr;
    hipStream_t copy_stream = nullptr;
    double t_copy0 = 0;

    ChainBatch(kgma_ctx *ctx_, const kgma_genome *g_, const ChainEnv &env_, std::vector<ChainPair> &pairs_, std::vector<char> &done_, ChainDevInfo &info_,
               std::vector<size_t> el_, int sel, bool generic)
        : ctx(ctx_), g(g_), env(env_), pairs(pairs_), done(done_), info(info_), el(std::move(el_)), set(&ctx_->cset[sel]) { plan.generic = generic; }

    int start_download();
    int finish();

private:
    bool first_windows(std::vector<double> &first) const;
    void export_pair(const std::vector<double> &first);
    void walk_pairs(const std::vector<double> &first);
};

// Upload the plan, launch every group, read the control words back; a launch that ran out of pool is repeated once with the
// pool it asked for.  *served = false with KGMA_OK: no room (or a batch beyond the pool's index range) -- the host chain
static int run_chain_kernels(ChainBatch &b, bool *served)
{
    kgma_ctx *ctx = b.ctx;
    const ChainPlan &plan = b.plan;
    ChainBufferSet &set = *b.set;
    ChainDevInfo &info = b.info;
    *served = false;
    // pool (16-byte units): 32 per raw step + up to KGMA_CHAIN_STEPS entries per detailed chunk.  The hot steps are
    // known; for the steps that go raw on a binade change there is room for one in a few hundred, and the launch is
    // repeated once with what it asked for if that was short
    const int64_t total_steps = plan.total_steps;
    const int64_t full_units = total_steps * 33 + plan.n_chunks + 64;  // every step raw
    const int64_t hot_units = plan.hot_steps * 32 + plan.hot_chunks * KGMA_CHAIN_STEPS;
    int64_t pool_units = hot_units + std::max<int64_t>(1 << 18, std::min<int64_t>(total_steps / 3, (int64_t)1 << 29));
    if (ctx->cpool_per_step > 0)                                       // (what the previous scans of this context needed, with a margin)
        pool_units = std::max(pool_units, hot_units + (int64_t)(1.25 * ctx->cpool_per_step * (double)total_steps) + (1 << 16));
    if (b.env.pool_units > 0) pool_units = b.env.pool_units;
    for (int attempt = 0;; attempt++) {
        info.attempts = std::max(info.attempts, attempt + 1);
        pool_units = std::min<int64_t>(pool_units, full_units);
        if (pool_units > 0xFFFFFFF0ll) return KGMA_OK;
        if (set.pool_cap < pool_units) {
            ChainChunk *fresh = nullptr;
            int64_t cap = 0;
            if (dev_reserve(ctx, fresh, cap, pool_units) != KGMA_OK) { ctx->err.clear(); (void)hipGetLastError(); return KGMA_OK; }   // no room: host chain
            if (set.pool) { (void)hipFree(set.pool); ctx->device_bytes -= set.pool_cap * (int64_t)sizeof(ChainChunk); }
            set.pool = fresh; set.pool_cap = cap;
        }
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_ctiles, plan.tiles.data(), (size_t)plan.n_tiles() * sizeof(TileDesc), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_chot, plan.hot.data(), plan.hot.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_chmask, plan.hot_masks.data(), plan.hot_masks.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_cctl, 0, 16, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        for (const ChainLaunch &L : plan.launches) {
            const int rc = launch_chain_group(ctx, b.g, plan, L, set, pool_units);
            if (rc) return rc;
        }
        HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        unsigned int ctl[4] = {0, 0, 0, 0};
        HIP_TRY(ctx, hipMemcpyAsync(ctl, ctx->d_cctl, 16, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, sync_spin(ctx->stream));
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
        info.kernel_ms += ms;
        if (b.env.debug)
            fprintf(stderr, "  chain batch: %zu pairs, %lld steps, %lld hot units, pool of %lld units, %u asked for%s, attempt %d, kernels %.2f ms\n", b.el.size(),
                    (long long)total_steps, (long long)hot_units, (long long)pool_units, ctl[0], (ctl[1] & 1u) ? " (ran out)" : "", attempt, ms);
        if (ctl[1] & 2u) return fail(ctx, KGMA_E_HIP, "internal: the chain kernel gave up on a stream (hash table of the window's k-mers)");
        if (!(ctl[1] & 1u)) {
            pool_units = std::min<int64_t>(pool_units, (int64_t)ctl[0]);
            // (the densest batch this context has seen: a launch that runs out of pool is a launch repeated)
            ctx->cpool_per_step = std::max(ctx->cpool_per_step, std::max(0.0, (double)(pool_units - hot_units)) / (double)std::max<int64_t>(1, total_steps));
            break;
        }
        if (attempt >= 1 || pool_units >= full_units) return KGMA_OK;                 // (cannot happen: the second pool is what the first launch asked for)
        pool_units = (int64_t)ctl[0] + (ctl[0] >> 4) + 4096;
    }
    b.pool_units = pool_units;
    *served = true;
    return KGMA_OK;
}

// ---- download: D0 per stream, chunk records, the used part of the raw pool; the pairs' first residues ----
int ChainBatch::start_download()
{
    t_copy0 = now_ms();
    size_t first_dw = 0;
    for (size_t u : el) {
        const ChainPair &p = pairs[u];
        const size_t dw = (size_t)((ctx->kfv[(size_t)p.j].W + 15) / 16);
        auto it = std::find_if(recs.begin(), recs.end(), [&](const RecordSlice &r) { return r.c == p.c; });
        if (it == recs.end()) recs.push_back(RecordSlice{p.c, 0, dw});
        else it->dw = std::max(it->dw, dw);
    }
    for (RecordSlice &r : recs) { r.dw_off = first_dw; first_dw += r.dw + 2; }
    off_D0 = 0; off_chunks = off_D0 + plan.d0_total * 8; off_raw = off_chunks + (size_t)plan.n_chunks * sizeof(ChainChunk);
    off_first = off_raw + (size_t)pool_units * sizeof(ChainChunk);
    const size_t pin_need = off_first + first_dw * 4 + 64;
    // (the mirror's previous user, two batches ago, has been joined)
    if (!grow_pinned(set->pin, set->pin_cap, pin_need, pin_need >> 2)) { (void)hipGetLastError(); return KGMA_OK; }
    uint8_t *const dst = set->pin;
    pin = dst;
    // (the launches have finished: the copies go to their own stream, and finish() waits for them, so that the next
    //  batch's launches -- into the other set of buffers -- run while this batch comes down)
    hipStream_t cs = copy_stream = ctx->chain_copy_stream;
    HIP_TRY(ctx, hipMemcpyAsync(dst + off_D0, set->D0, plan.d0_total * 8, hipMemcpyDeviceToHost, cs));
    HIP_TRY(ctx, hipMemcpyAsync(dst + off_chunks, set->chunks, (size_t)plan.n_chunks * sizeof(ChainChunk), hipMemcpyDeviceToHost, cs));
    if (pool_units > 0)
        HIP_TRY(ctx, hipMemcpyAsync(dst + off_raw, set->pool, (size_t)pool_units * sizeof(ChainChunk), hipMemcpyDeviceToHost, cs));
    for (const RecordSlice &r : recs)
        HIP_TRY(ctx, hipMemcpyAsync(dst + off_first + r.dw_off * 4, g->d_inter + 2 * g->cd[(size_t)r.c].word_off, r.dw * 4, hipMemcpyDeviceToHost, cs));
    downloading = true;
    return KGMA_OK;
}

// ---- host part: first windows and chunk walks (chain_on_device runs it on a worker when more batches follow) ----
int ChainBatch::finish()
{
    downloading = false;
    (void)hipSetDevice(ctx->device);
    if (hipStreamSynchronize(copy_stream) != hipSuccess) return (int)KGMA_E_HIP;
    info.copy_ms += now_ms() - t_copy0;
    const double tw0 = now_ms();
    std::vector<ChainStream> &streams = plan.streams;
    const int64_t *h_D0 = reinterpret_cast<const int64_t *>(pin + off_D0);
    for (size_t t = 0; t < streams.size(); t++) streams[t].D0 = h_D0[plan.stream_d0[t]];
    if (plan.generic) {
        // (the generic chain kernel reports each stream's first distance as a double: onto the KFV's integer lattice)
        for (size_t u = 0; u < el.size(); u++) {
            const KfvInfo &f = ctx->kfv[(size_t)pairs[el[u]].j];
            for (size_t t = plan.ps[u].s0; t < plan.ps[u].s1; t++) {
                double dv;
                memcpy(&dv, &streams[t].D0, sizeof dv);
                streams[t].D0 = lattice_of(f, ctx->k, dv);
            }
        }
    }
    std::vector<double> first(el.size(), 0.0);
    if (!first_windows(first)) return (int)KGMA_E_HIP;
    if (export_only) { export_pair(first); return KGMA_OK; }
    walk_pairs(first);
    info.streams += plan.n_tiles();
    info.walk_ms += now_ms() - tw0;
    return KGMA_OK;
}

bool ChainBatch::first_windows(std::vector<double> &first) const
{
    std::vector<ChainJob> jobs(el.size());
    for (size_t u = 0; u < el.size(); u++) {
        const ChainPair &p = pairs[el[u]];
        size_t off = 0;
        for (const RecordSlice &r : recs) if (r.c == p.c) off = r.dw_off;
        jobs[u] = first_window_job(ctx->kfv[(size_t)p.j], ctx->k, reinterpret_cast<const uint32_t *>(pin + off_first) + off, &first[u]);
    }
    run_chain_jobs(jobs.data(), jobs.size(), 1);
    for (size_t u = 0; u < el.size(); u++)
        if (!jobs[u].ok) return false;
    return true;
}

// (kgma_chain_export: one pair; its material goes to the caller, who walks it where the whole record's pieces meet)
void ChainBatch::export_pair(const std::vector<double> &first)
{
    ctx->cx_streams.assign(plan.streams.begin(), plan.streams.end());
    const ChainChunk *hc = reinterpret_cast<const ChainChunk *>(pin + off_chunks), *hp = reinterpret_cast<const ChainChunk *>(pin + off_raw);
    ctx->cx_chunks.assign(hc, hc + plan.n_chunks);
    ctx->cx_pool.assign(hp, hp + pool_units);
    ctx->cx_first = first.empty() ? 0.0 : first[0];
    for (size_t u = 0; u < el.size(); u++) done[el[u]] = 1;
    info.pairs += (int64_t)el.size();
    info.streams += plan.n_tiles();
}

void ChainBatch::walk_pairs(const std::vector<double> &first)
{
    const int k = ctx->k;
    std::vector<ChainWalkJob> walks(el.size());
    for (size_t u = 0; u < el.size(); u++) {
        ChainPair &p = pairs[el[u]];
        const KfvInfo &f = ctx->kfv[(size_t)p.j];
        ChainWalkJob &J = walks[u];
        J = ChainWalkJob{};
        J.first = first[u];
        J.scale = chain_scale(k, f);
        J.nk = (int)(f.W - k + 1);
        J.streams = plan.streams.data() + plan.ps[u].s0; J.n_streams = plan.ps[u].s1 - plan.ps[u].s0;
        J.chunks = reinterpret_cast<const ChainChunk *>(pin + off_chunks);
        J.pool = reinterpret_cast<const ChainChunk *>(pin + off_raw);
        J.pool_units = pool_units;
        J.iv = p.iv.data(); J.n_iv = p.iv.size(); J.out = p.val.data();
    }
    run_chain_walks(walks.data(), walks.size(), env.threads);
    for (size_t u = 0; u < el.size(); u++) {
        const ChainWalkJob &J = walks[u];
        const ChainPair &p = pairs[el[u]];
        info.max_drift = std::max(info.max_drift, J.max_drift);
        if (J.status != CHAIN_WALK_OK || J.n_out != (int64_t)p.val.size()) {
            if (env.debug)
                fprintf(stderr, "chain on the device: record %d KFV %d left to the host (status %d, %lld of %zu values, drift %.3g)\n", p.c,
                        p.j + 1, J.status, (long long)J.n_out, p.val.size(), J.max_drift);
            continue;
        }
        done[el[u]] = 1;
        info.pairs++;
        info.windows += p.last;
        info.raw_steps += J.raw_steps;
    }
}

// The device part of a batch, up to the start of its download; then its host part, unless the caller takes it (`defer`: the
// batch says whether one is due, ChainBatch::downloading).  A batch that does not fit is left as it is: the host chain.
static int run_chain_batch(ChainBatch &b, bool defer)
{
    kgma_ctx *ctx = b.ctx;
    const double ts0 = now_ms();
    plan_chain_launches(ctx, b.env, b.pairs, b.el, b.plan);
    plan_chain_streams(ctx, b.g, b.env, b.pairs, b.el, b.plan);
    if (!b.plan.fits()) return KGMA_OK;
    mark_hot_steps(ctx, b.pairs, b.el, b.plan);
    int rc = reserve_chain_buffers(ctx, b.plan, *b.set);
    if (rc) return rc;
    b.info.setup_ms += now_ms() - ts0;
    b.info.chunks += b.plan.n_chunks;
    bool served = false;
    rc = run_chain_kernels(b, &served);
    if (rc || !served) return rc;
    rc = b.start_download();
    if (rc || !b.downloading || defer) return rc;
    const int frc = b.finish();
    if (frc) return fail(ctx, frc, "internal: first window of a chained record");
    return KGMA_OK;
}

static int chain_on_device(kgma_ctx *ctx, const kgma_genome *g, const ChainEnv &env, std::vector<ChainPair> &pairs, std::vector<char> &done, ChainDevInfo &info)
{
    std::vector<size_t> el8, elg;
    for (size_t i = 0; i < pairs.size(); i++) {
        const ChainPair &p = pairs[i];
        if (p.last < 2) continue;
        const int which = chain_kernel_for(ctx, ctx->kfv[(size_t)p.j], env);
        if (which == 1) el8.push_back(i);
        else if (which == 2) elg.push_back(i);
    }
    if (el8.empty() && elg.empty()) return KGMA_OK;
    (void)hipSetDevice(ctx->device);
    {
        // a sparse step: the chain kernels and the download of the first windows' codes read these records of the 2-bit copy
        std::vector<int32_t> recs_read;
        for (const std::vector<size_t> *el : {&el8, &elg})
            for (const size_t i : *el) recs_read.push_back(pairs[i].c);
        const int prc = pack_record_blocks(ctx, const_cast<kgma_genome *>(g), std::move(recs_read));
        if (prc) return prc;
    }
    NumaBind numa(ctx);                      // (the pinned download buffers and the walking threads on the GPU's NUMA node: gigabytes come back on dense inputs)
    // batches of bounded size (2^35 windows: a chunk array of 128 MiB), in record order; the host part of a batch overlaps
    // the device part of the next, so what stays exposed is the LAST batch's host part: smaller batches, shorter tail
    // (config 5, 2.5e11 windows, 1.31 s of kernels: 1577 ms with 2^36, 1499 ms with 2^35, 1542 ms with 2^34)
    // The host part of a batch (first windows, chunk walks) runs on a worker while the device works on the next batch;
    // two sets of output buffers, each with its pinned mirror, alternate.  (At most one worker at a time: it is joined before
    // the next one starts.)
    struct Worker {
        std::thread th;
        int rc = KGMA_OK;
        int join() { if (th.joinable()) th.join(); const int r = rc; rc = KGMA_OK; return r; }
        ~Worker() { if (th.joinable()) th.join(); }
    } worker;
    int sel = 0;
    for (int pass = 0; pass < 2; pass++) {
        const std::vector<size_t> &el = pass == 0 ? el8 : elg;
        for (size_t u0 = 0; u0 < el.size();) {
            size_t u1 = u0;
            int64_t w = 0;
            while (u1 < el.size() && (u1 == u0 || w + pairs[el[u1]].last <= env.batch_windows)) w += pairs[el[u1++]].last;
            const bool more = u1 < el.size() || worker.th.joinable() || (pass == 0 && !elg.empty());
            const double tb0 = now_ms();
            auto batch = std::make_unique<ChainBatch>(ctx, g, env, pairs, done, info, std::vector<size_t>(el.begin() + (long)u0, el.begin() + (long)u1), sel, pass == 1);
            const int rc = run_chain_batch(*batch, more);
            const double tb1 = now_ms();
            const int wrc = worker.join();
            if (env.debug) fprintf(stderr, "  chain batch: device part %.2f ms, then %.2f ms waiting for the previous batch's host part\n", tb1 - tb0, now_ms() - tb1);
            if (rc) return rc;
            if (wrc) return fail(ctx, wrc, "internal: first window of a chained record");
            if (batch->downloading) {
                Worker *wk = &worker;
                worker.th = std::thread([wk, b = std::move(batch)]() { wk->rc = b->finish(); });
            }
            sel ^= 1;
            u0 = u1;
        }
    }
    const double tj0 = now_ms();
    const int wrc = worker.join();
    if (env.debug) fprintf(stderr, "  chain: %.2f ms waiting for the last batch's host part\n", now_ms() - tj0);
    if (wrc) return fail(ctx, wrc, "internal: first window of a chained record");
    return KGMA_OK;
}

// ------------------------------------------------------------------------------------------
// Float64 chain replay (KGMA_F_CHAIN_REPLAY): for the (record, KFV) pairs in which exact arithmetic leaves a
// decision to the rounding of the reference's running Float64 value, re-run that value from the record's
// first window (kgma_chain.cpp, host threads) and rebuild the pair's dips from the chain's values at the
// windows the device scan found -- every dip of the pair and every window inside the threshold guard band.
// A pair is selected when (1) one of its dips still carries KGMA_HIT_TIE after the local tie resolver or
// KGMA_HIT_AT_THRESHOLD, (2) it has a tested window inside the guard band, or (3) two of its dips (or a
// dip and the first window) have the same exact minimum -- the superset of "a dip's minimum equals the
// stale running minimum" (GenomeMiner.jl:93-103), which is only known once the hit state machine runs.
// Every other pair has no exact tie anywhere, so exact arithmetic and the chain decide alike.
// chain_decide, below, is the list of its phases.
// ------------------------------------------------------------------------------------------

// (A) ties inside one dip are decided where that is provably independent of the chain's history
// (no genome: kgma_replay_dips, residues through the source)
static void resolve_local_ties(kgma_ctx *ctx, const kgma_genome *g)
{
    TieResolver tr{ctx, g, {}, {}, {}, nullptr, {}, {}};
    if (g) tr.prefetch();
    for (size_t i = 0; i < ctx->dips.size(); i++) {
        kgma_dip &d = ctx->dips[i];
        if (!(d.flags & KGMA_HIT_TIE)) continue;
        const TieResolver::Result r = tr.replay(d.kfv - 1, d.contig, d.argmin, d.D_min, d.argmin, ctx->dip_argl[i], d.D_min, false,
                                                g ? tr.prefetched(i) : nullptr);
        if (r.ok && !r.sensitive) {
            d.argmin = r.pos;
            d.flags = (d.flags & ~(uint32_t)KGMA_HIT_TIE) | KGMA_HIT_TIE_RESOLVED;
        }
    }
}

// (cluster engine) does the widest candidate range of a dip meet that of another dip of its record?
static std::vector<char> mark_dips_meeting_others(const kgma_ctx *ctx, int64_t buff)
{
    std::vector<char> dip_meets_other(ctx->dips.size(), 0);
    struct Rg { int64_t lo, hi; size_t u; };
    std::vector<Rg> rg;
    size_t u0 = 0;
    const size_t ndp = ctx->dips.size();
    while (u0 < ndp) {
        size_t u1 = u0;
        rg.clear();
        while (u1 < ndp && ctx->dips[u1].contig == ctx->dips[u0].contig) {
            const kgma_dip &d = ctx->dips[u1];
            const int64_t W = ctx->kfv[(size_t)(d.kfv - 1)].W;
            rg.push_back(Rg{d.start - 1 - buff, d.end - 1 + W - 1 + buff, u1});     // CMI = best window - 1, anywhere in the dip
            u1++;
        }
        std::sort(rg.begin(), rg.end(), [](const Rg &a, const Rg &b) { return a.lo < b.lo; });
        int64_t reach = INT64_MIN;                                                 // farthest end among the ranges before
        for (size_t i = 0; i < rg.size(); i++) {
            if (reach >= rg[i].lo) dip_meets_other[rg[i].u] = 1;
            if (i + 1 < rg.size() && rg[i + 1].lo <= rg[i].hi) dip_meets_other[rg[i].u] = 1;
            reach = std::max(reach, rg[i].hi);
        }
        u0 = u1;
    }
    return dip_meets_other;
}

// Single engine: may a dip's minimum of pair `p` equal the running minimum?  The single engine's alignment does not feed back
// (GenomeMiner.jl:96-99): with no other tie in the pair its state machine is a function of the dips alone, so "a dip's minimum
// equals the running minimum" is found by running it (GenomeMiner.jl:82-104)
static bool single_engine_may_tie(const kgma_ctx *ctx, const ChainPair &p, int64_t firstD)
{
    const int k = ctx->k;
    const int64_t W = ctx->kfv[0].W;
    int64_t currmin = firstD, CMI = 2, goal_ind = 0;
    bool stop = true, need = false;
    for (size_t u = p.d0; u < p.d1 && !need; u++) {
        const kgma_dip &d = ctx->dips[u];
        if (near_tie(ctx->kfv[0], d.D_min, currmin)) need = true;
        if (d.D_min < currmin) { currmin = d.D_min; CMI = d.argmin + k - 2; stop = false; }
        if (d.exit_pos == 0 || stop) continue;
        stop = true;
        CMI += 1;
        if (CMI > goal_ind) { goal_ind = CMI + W - 1; currmin = d.D_exit; }
    }
    return need;
}

// Cluster engine: whether a hit is emitted (and the running minimum reset) depends on the alignment
// callback (OmnGenomeMiner.jl:126,139,152), so its state machine cannot be run ahead.  What can tie:
// a dip's minimum with the first window's value (curr_mins starts there, :73-74), or with the STALE
// minimum an earlier dip A of the same KFV left behind -- and a dip only leaves one when it is
// suppressed (:126 CMI in prev_hit_range, :139 aligned range not disjoint from it); the accepted hit's
// range is a sub-range of its candidate range max(CMI-buff,1) : CMI+ws-1+buff, so A can only be suppressed
// if its candidate range meets that of another dip of the record (any KFV).  Superset taken: equal minima
// A before B where A's widest possible candidate range meets another dip's.
static bool cluster_engine_may_tie(const kgma_ctx *ctx, const ChainPair &p, int64_t firstD, const std::vector<char> &dip_meets_other)
{
    const KfvInfo &fj = ctx->kfv[(size_t)p.j];
    bool need = false;
    for (size_t u = p.d0; u < p.d1 && !need; u++) need = near_tie(fj, ctx->dips[u].D_min, firstD);
    for (size_t u = p.d0; u < p.d1 && !need; u++) {
        if (!dip_meets_other[u]) continue;
        for (size_t v = u + 1; v < p.d1 && !need; v++) need = near_tie(fj, ctx->dips[v].D_min, ctx->dips[u].D_min);
    }
    return need;
}

// The pairs the chain decides: a merge over the dips and the guard-band windows (both in (record, KFV) order).
// why_count (KGMA_CHAIN_DEBUG): what selected them
static std::vector<ChainPair> select_chain_pairs(const kgma_ctx *ctx, int32_t mode, const std::vector<char> &dip_meets_other, int64_t why_count[5])
{
    std::vector<ChainPair> pairs;
    const int64_t nc = (int64_t)ctx->contig_len.size();
    size_t di = 0, ai = 0;
    const size_t nd = ctx->dips.size(), na = ctx->att.size();
    while (di < nd || ai < na) {
        int32_t c, j;
        const bool dip_first = di < nd && (ai >= na || ctx->dips[di].contig < ctx->att[ai].contig ||
                                           (ctx->dips[di].contig == ctx->att[ai].contig && ctx->dips[di].kfv - 1 <= ctx->att[ai].kfv));
        if (dip_first) { c = ctx->dips[di].contig; j = ctx->dips[di].kfv - 1; }
        else { c = ctx->att[ai].contig; j = ctx->att[ai].kfv; }
        ChainPair p{c, j, di, di, ai, ai, {}, {}, 0};
        while (p.d1 < nd && ctx->dips[p.d1].contig == c && ctx->dips[p.d1].kfv - 1 == j) p.d1++;
        while (p.a1 < na && ctx->att[p.a1].contig == c && ctx->att[p.a1].kfv == j) p.a1++;
        di = p.d1; ai = p.a1;
        bool need = p.a1 > p.a0;
        int why = need ? 1 : 0;
        for (size_t u = p.d0; u < p.d1; u++)
            if (ctx->dips[u].flags & (KGMA_HIT_TIE | KGMA_HIT_AT_THRESHOLD)) { need = true; if (!why) why = (ctx->dips[u].flags & KGMA_HIT_TIE) ? 2 : 3; }
        const int64_t firstD = ctx->firstD[(size_t)j * (size_t)nc + (size_t)c];
        if (!need) need = mode == KGMA_MODE_SINGLE ? single_engine_may_tie(ctx, p, firstD) : cluster_engine_may_tie(ctx, p, firstD, dip_meets_other);
        if (need && !why) why = 4;
        if (need) { why_count[why]++; pairs.push_back(std::move(p)); }
    }
    return pairs;
}

// ---- sample windows of every pair: its dips (start .. exit) and its guard-band windows (+ the next) ----
static int sample_pair_windows(kgma_ctx *ctx, std::vector<ChainPair> &pairs)
{
    for (ChainPair &p : pairs) {
        const int64_t nwin = ctx->contig_nwin[(size_t)p.c];
        std::vector<ChainInterval> iv;
        iv.push_back(ChainInterval{1, 1});
        for (size_t u = p.d0; u < p.d1; u++) {
            const kgma_dip &d = ctx->dips[u];
            iv.push_back(ChainInterval{d.start, d.exit_pos ? d.exit_pos : d.end});
        }
        for (size_t u = p.a0; u < p.a1; u++) iv.push_back(ChainInterval{ctx->att[u].pos, std::min<int64_t>(ctx->att[u].pos + 1, nwin)});
        std::sort(iv.begin(), iv.end(), [](const ChainInterval &a, const ChainInterval &b) { return a.lo < b.lo; });
        for (const ChainInterval &x : iv) {
            if (!p.iv.empty() && x.lo <= p.iv.back().hi + 1) p.iv.back().hi = std::max(p.iv.back().hi, x.hi);
            else p.iv.push_back(x);
        }
        int64_t n = 0;
        for (const ChainInterval &x : p.iv) n += x.hi - x.lo + 1;
        p.val.assign((size_t)n, 0.0);
        p.last = p.iv.back().hi;
        if (p.iv.front().lo < 1 || p.last > nwin) return fail(ctx, KGMA_E_HIP, "internal: chain replay window outside record %d", p.c);
    }
    return KGMA_OK;
}

// kgma_replay_dips: the residues are with the ranks that scanned them; the caller's source runs the chain there
// (kgma_chain_export per slice) and hands back the values at the wanted windows
static int chains_from_source(kgma_ctx *ctx, std::vector<ChainPair> &pairs, std::vector<char> &done, ChainDevInfo &dev)
{
    if (!ctx->chain_src) return fail(ctx, KGMA_E_STATE, "chain replay without a genome needs a chain source (kgma_set_chain_source)");
    std::vector<int32_t> pc(pairs.size()), pj(pairs.size());
    std::vector<int64_t> ivb(pairs.size() + 1, 0), lo, hi;
    size_t nv = 0;
    for (size_t i = 0; i < pairs.size(); i++) {
        pc[i] = pairs[i].c; pj[i] = pairs[i].j + 1;
        for (const ChainInterval &x : pairs[i].iv) { lo.push_back(x.lo); hi.push_back(x.hi); }
        ivb[i + 1] = (int64_t)lo.size();
        nv += pairs[i].val.size();
    }
    std::vector<double> vals(nv, 0.0);
    const int src = ctx->chain_src(ctx->chain_user, (int64_t)pairs.size(), pc.data(), pj.data(), ivb.data(), lo.data(), hi.data(), vals.data());
    if (src != 0) return fail(ctx, KGMA_E_STATE, "the chain source failed (status %d)", src);
    size_t off = 0;
    for (size_t i = 0; i < pairs.size(); i++) {
        std::copy(vals.begin() + (long)off, vals.begin() + (long)(off + pairs[i].val.size()), pairs[i].val.begin());
        off += pairs[i].val.size();
        done[i] = 1;
        dev.pairs++;
        dev.windows += pairs[i].last;
    }
    return KGMA_OK;
}

// ---- host chains, records in batches of bounded host memory; *windows: the windows chained are added ----
static int chains_on_host(kgma_ctx *ctx, const kgma_genome *g, const ChainEnv &env, const std::vector<ChainPair *> &hostp, int64_t *windows)
{
    const int k = ctx->k;
    (void)hipSetDevice(ctx->device);
    if (g && !hostp.empty()) {
        std::vector<int32_t> recs_read;                                // (a sparse step: the records whose codes come down)
        for (const ChainPair *p : hostp) recs_read.push_back(p->c);
        const int prc = pack_record_blocks(ctx, const_cast<kgma_genome *>(g), std::move(recs_read));
        if (prc) return prc;
    }
    size_t pi = 0;
    double copy_ms = 0, jobs_ms = 0;
    while (pi < hostp.size()) {
        // the records of this batch: their 2-bit codes (the device's interleaved copy: a quarter of the residue text)
        // are copied into one pinned buffer, kept by the context; all pairs of one record share its copy
        struct HostRecord { ChainBatch::RecordSlice codes; size_t p0, p1; int64_t need; };
        std::vector<HostRecord> recs;
        std::vector<ChainJob> jobs;
        int64_t bytes = 0;
        size_t pj = pi, total_dw = 0;
        while (pj < hostp.size() && (pj == pi || bytes < env.batch_bytes)) {
            const int32_t c = hostp[pj]->c;
            size_t pe = pj;
            int64_t need = 0;
            while (pe < hostp.size() && hostp[pe]->c == c) {
                need = std::max(need, ctx->kfv[(size_t)hostp[pe]->j].W + hostp[pe]->last - 1);
                pe++;
            }
            need = std::min(need, g->cd[(size_t)c].len);
            const size_t dw = (size_t)((need + 15) / 16);
            recs.push_back(HostRecord{{c, total_dw, dw}, pj, pe, need});
            total_dw += dw;
            bytes += (int64_t)dw * 4;
            pj = pe;
        }
        const double tc0 = now_ms();
        const size_t spare = (total_dw >> 3) + 1024;
        if (!grow_pinned(ctx->h_chain, ctx->chain_cap, total_dw, spare))
            return fail(ctx, KGMA_E_NOMEM, "chain replay: cannot allocate %zu bytes of pinned host memory", (total_dw + spare) * 4);
        for (const HostRecord &r : recs)
            if (hipMemcpyAsync(ctx->h_chain + r.codes.dw_off, g->d_inter + 2 * g->cd[(size_t)r.codes.c].word_off, r.codes.dw * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
                return fail(ctx, KGMA_E_HIP, "chain replay: cannot read record %d", r.codes.c);
        if (sync_spin(ctx->stream) != hipSuccess) return fail(ctx, KGMA_E_HIP, "chain replay: cannot read the records");
        copy_ms += now_ms() - tc0;
        for (const HostRecord &r : recs)
            for (size_t u = r.p0; u < r.p1; u++) {
                ChainPair &p = *hostp[u];
                jobs.push_back(chain_job(ctx->kfv[(size_t)p.j], k, ctx->h_chain + r.codes.dw_off, r.need, p.last, p.iv.data(), p.iv.size(), p.val.data()));
                *windows += p.last;
            }
        const double tj0 = now_ms();
        run_chain_jobs(jobs.data(), jobs.size(), env.threads);
        jobs_ms += now_ms() - tj0;
        for (size_t u = 0; u < jobs.size(); u++)
            if (!jobs[u].ok || jobs[u].n_out != (int64_t)hostp[pi + u]->val.size())
                return fail(ctx, KGMA_E_HIP, "internal: chain replay of record %d KFV %d failed", hostp[pi + u]->c, hostp[pi + u]->j + 1);
        pi = pj;
    }
    if (env.debug) fprintf(stderr, "chain replay: residues copied in %.1f ms, chains %.1f ms, %d threads\n", copy_ms, jobs_ms, env.threads);
    return KGMA_OK;
}

// The windows sampled are the ones whose EXACT distance is under (or within 2^-30 of) the threshold: that
// covers every window the reference's value can be under thr at only while the chain stays within 2^-30 of the
// exact distance.  Checked where both are known -- the first window and every dip's minimum (the device chain
// has checked every stream start too): a chain that drifted further is an error, never a silent miss.
// What the band has to cover is the value's ABSOLUTE error where the distance is near thr: the error is measured
// against max(exact distance, thr) -- at a dip's minimum the distance can be tiny (near-identical reference
// sequences: D_min of a few units) and an error inherited from windows of ordinary distances says nothing about
// the threshold there.  (The device chain's binade decisions have their own guard: kgma_device.h, ChainArgs.)
static double pair_drift(const kgma_ctx *ctx, const ChainPair &p)
{
    const KfvInfo &f = ctx->kfv[(size_t)p.j];
    const double scale = chain_scale(ctx->k, f);
    const int64_t nc = (int64_t)ctx->contig_len.size();
    auto value_at = [&](int64_t w) -> const double * {
        size_t off = 0;
        for (const ChainInterval &x : p.iv) {
            if (w >= x.lo && w <= x.hi) return &p.val[off + (size_t)(w - x.lo)];
            off += (size_t)(x.hi - x.lo + 1);
        }
        return nullptr;
    };
    double drift = 0;
    auto drifted = [&](int64_t w, int64_t D) {
        const double *v = value_at(w);
        if (!v || D < 0) return;
        const double exact = (double)D / scale, dr = std::fabs(*v - exact) / std::max(exact, f.thr > 0 ? f.thr : exact);
        if (!(dr >= 0)) return;
        drift = std::max(drift, dr);
    };
    drifted(1, ctx->firstD[(size_t)p.j * (size_t)nc + (size_t)p.c]);
    for (size_t u = p.d0; u < p.d1; u++) drifted(ctx->dips[u].argmin, ctx->dips[u].D_min);
    return drift;
}

// a dip with what the hit state machine wants beside it (ctx->dip_argl / dip_aux / dip_fmin / dip_fexit)
struct ChainDip { kgma_dip d; int64_t argl, aux; double fmin, fexit; };

// The dips of pair `p` as the chain's values draw them: the runs of windows under the threshold, appended to `all`
static int rebuild_pair_dips(kgma_ctx *ctx, const ChainPair &p, std::vector<ChainDip> &all)
{
    const KfvInfo &f = ctx->kfv[(size_t)p.j];
    const double scale = chain_scale(ctx->k, f);
    const int64_t nwin = ctx->contig_nwin[(size_t)p.c];
    bool in_run = false;
    ChainDip cur{};
    int64_t prev_w = 0;
    size_t vi = 0;
    auto close_run = [&](int64_t exit_pos, double fexit) {
        cur.d.exit_pos = exit_pos;
        cur.fexit = fexit;
        cur.d.D_exit = exit_pos ? (int64_t)std::llround(fexit * scale) : 0;
        cur.d.D_min = (int64_t)std::llround(cur.fmin * scale);
        cur.argl = cur.d.argmin;
        all.push_back(cur);
        in_run = false;
    };
    for (const ChainInterval &x : p.iv) {
        for (int64_t w = x.lo; w <= x.hi; w++, vi++) {
            const double v = p.val[vi];
            const bool under = w >= 2 && v < f.thr;            // GenomeMiner.jl:82 / OmnGenomeMiner.jl:113 (the first window is never tested)
            if (in_run && w != prev_w + 1)                     // a run never reaches the end of a sampled interval
                return fail(ctx, KGMA_E_HIP, "internal: chain replay lost the exit of a dip (record %d KFV %d window %lld)", p.c, p.j + 1, (long long)prev_w);
            if (under) {
                if (!in_run) {
                    in_run = true;
                    memset(&cur.d, 0, sizeof cur.d);
                    cur.d.contig = p.c; cur.d.kfv = p.j + 1; cur.d.start = w; cur.d.argmin = w;
                    cur.d.flags = KGMA_HIT_CHAIN;
                    cur.fmin = v; cur.aux = -1;
                } else if (v < cur.fmin) { cur.fmin = v; cur.d.argmin = w; }   // strict: the first window attaining the minimum
                cur.d.end = w;
            } else if (in_run) {
                close_run(w, v);
            }
            prev_w = w;
        }
    }
    if (in_run) {
        if (prev_w != nwin)
            return fail(ctx, KGMA_E_HIP, "internal: chain replay lost the exit of a dip (record %d KFV %d window %lld)", p.c, p.j + 1, (long long)prev_w);
        close_run(0, 0.0);                                         // still open at the record end: dropped by the state machine
    }
    return KGMA_OK;
}

// the dips no chain pair replaces, as they are
static std::vector<ChainDip> dips_outside_pairs(const kgma_ctx *ctx, const std::vector<ChainPair> &pairs)
{
    std::vector<ChainDip> all;
    all.reserve(ctx->dips.size() + 16);
    std::vector<char> replaced(ctx->dips.size(), 0);
    for (const ChainPair &p : pairs)
        for (size_t u = p.d0; u < p.d1; u++) replaced[u] = 1;
    for (size_t u = 0; u < ctx->dips.size(); u++)
        if (!replaced[u]) all.push_back(ChainDip{ctx->dips[u], ctx->dip_argl[u], ctx->dip_aux[u], 0.0, 0.0});
    return all;
}

static void store_chain_dips(kgma_ctx *ctx, std::vector<ChainDip> &all)
{
    std::stable_sort(all.begin(), all.end(), [](const ChainDip &a, const ChainDip &b) {
        if (a.d.contig != b.d.contig) return a.d.contig < b.d.contig;
        if (a.d.kfv != b.d.kfv) return a.d.kfv < b.d.kfv;
        return a.d.start < b.d.start;
    });
    const size_t n = all.size();
    ctx->dips.resize(n); ctx->dip_argl.resize(n); ctx->dip_aux.resize(n); ctx->dip_fmin.resize(n); ctx->dip_fexit.resize(n);
    for (size_t u = 0; u < n; u++) {
        ctx->dips[u] = all[u].d; ctx->dip_argl[u] = all[u].argl; ctx->dip_aux[u] = all[u].aux;
        ctx->dip_fmin[u] = all[u].fmin; ctx->dip_fexit[u] = all[u].fexit;
    }
    ctx->stats.n_dips = (int64_t)n;
}

// (*drift_out, when given: instead of failing on a chain that has drifted beyond the guard band's half width, the largest drift seen
//  is returned there with status CHAIN_DRIFT_RETRY, and kgma_scan repeats the scan with a band that covers it)
constexpr int CHAIN_DRIFT_RETRY = -77;
static int chain_decide(kgma_ctx *ctx, const kgma_genome *g, int32_t mode, int64_t buff, double *drift_out = nullptr)
{
    const double t0 = now_ms();
    const ChainEnv env = read_chain_env();
    const int m = ctx->m;
    const int64_t nc = (int64_t)ctx->contig_len.size();
    reset_chain_stats(ctx);
    resolve_local_ties(ctx, g);
    // ---- select the pairs ------------------------------------------------------------------
    int64_t why_count[5] = {0, 0, 0, 0, 0};
    const std::vector<char> dip_meets_other = mode == KGMA_MODE_OMN ? mark_dips_meeting_others(ctx, buff) : std::vector<char>(ctx->dips.size(), 0);
    std::vector<ChainPair> pairs = select_chain_pairs(ctx, mode, dip_meets_other, why_count);
    if (env.debug)
        fprintf(stderr, "chain replay: %zu pairs selected: %lld by a window in the threshold band, %lld by a dip with tied minima, %lld by a dip at the threshold, "
                "%lld by a minimum equal to the running / first / an earlier minimum\n", pairs.size(), (long long)why_count[1], (long long)why_count[2],
                (long long)why_count[3], (long long)why_count[4]);
    ctx->dip_fmin.assign(ctx->dips.size(), 0.0);
    ctx->dip_fexit.assign(ctx->dips.size(), 0.0);
    ctx->chain_pair.assign((size_t)m * (size_t)nc, 0);
    ctx->firstF.assign((size_t)m * (size_t)nc, 0.0);
    if (pairs.empty()) { ctx->stats.chain_ms = now_ms() - t0; return KGMA_OK; }
    int rc = sample_pair_windows(ctx, pairs);
    if (rc) return rc;

    // ---- the chains: on the device where its kernel applies, the rest (and whatever failed a check there) on the host ----
    std::vector<char> on_device(pairs.size(), 0);
    ChainDevInfo dev;
    const double t_selected = now_ms();
    if (!g) rc = chains_from_source(ctx, pairs, on_device, dev);
    else if (!env.host_only) rc = chain_on_device(ctx, g, env, pairs, on_device, dev);
    if (rc) return rc;
    ctx->stats.chain_device_pairs = dev.pairs;
    ctx->stats.chain_device_ms = dev.kernel_ms;
    ctx->stats.chain_raw_steps = dev.raw_steps;
    ctx->stats.chain_max_drift = dev.max_drift;
    if (env.debug) {
        fprintf(stderr, "chain replay: local tie pass + pair selection %.2f ms, device chains %.2f ms (wall)\n", t_selected - t0, now_ms() - t_selected);
        fprintf(stderr, "chain on the device: %lld of %zu pairs, %lld windows in %lld streams / %lld chunks, setup %.2f ms, kernels %.2f ms (%d attempt(s)), download %.2f ms, host walk %.2f ms, %lld raw steps, drift <= %.3g\n",
                (long long)dev.pairs, pairs.size(), (long long)dev.windows, (long long)dev.streams, (long long)dev.chunks, dev.setup_ms, dev.kernel_ms, dev.attempts,
                dev.copy_ms, dev.walk_ms, (long long)dev.raw_steps, dev.max_drift);
    }
    std::vector<ChainPair *> hostp;
    for (size_t i = 0; i < pairs.size(); i++)
        if (!on_device[i]) hostp.push_back(&pairs[i]);
    int64_t windows = dev.windows;
    rc = chains_on_host(ctx, g, env, hostp, &windows);
    if (rc) return rc;

    // ---- rebuild the dips of the chain pairs from the chain values ---------------------------
    const double limit = std::ldexp(1.0, -(ctx->band_log2 + 1));
    double worst_drift = 0;                                            // beyond the limit, over all pairs
    std::vector<ChainDip> all = dips_outside_pairs(ctx, pairs);
    for (const ChainPair &p : pairs) {
        ctx->chain_pair[(size_t)p.j * (size_t)nc + (size_t)p.c] = 1;
        ctx->firstF[(size_t)p.j * (size_t)nc + (size_t)p.c] = p.val[0];
        const double drift = pair_drift(ctx, p);
        ctx->stats.chain_max_drift = std::max(ctx->stats.chain_max_drift, drift);
        if (drift > limit) {
            if (!drift_out)
                return fail(ctx, KGMA_E_STATE, "chain replay: the running Float64 value of record %d KFV %d has drifted %.3g (relative to max(distance, thr)) from the "
                            "exact distance; the threshold guard band (2^-%d) no longer covers it", p.c, p.j + 1, drift, ctx->band_log2);
            worst_drift = std::max(worst_drift, drift);
        }
        rc = rebuild_pair_dips(ctx, p, all);
        if (rc) return rc;
    }
    if (worst_drift > 0) { *drift_out = worst_drift; return CHAIN_DRIFT_RETRY; }
    store_chain_dips(ctx, all);
    ctx->stats.n_chain_pairs = (int64_t)pairs.size();
    ctx->stats.chain_windows = windows;
    ctx->stats.chain_ms = now_ms() - t0;
    if (env.debug) fprintf(stderr, "chain replay: %.2f ms in all\n", ctx->stats.chain_ms);
    return KGMA_OK;
}

// Device scan + (KGMA_F_CHAIN_REPLAY) the chain replay, with the replay's drift policy: the scan samples the reference's running
// value at the windows whose exact distance is below or within 2^-band_log2 of thr.  If the replayed value turns out further than
// half of that from the exact distances (long records, values accumulated at large distances), the band no longer provably holds
// every window the reference may see below thr: the scan is repeated with a band that covers four times the drift measured (more
// windows sampled, more raw steps in the chain kernel), up to twice; only a drift beyond 2^-10 fails (KGMA_E_STATE).
static int scan_and_decide(kgma_ctx *ctx, const kgma_genome *g, int32_t mode, int64_t buff, uint32_t flags)
{
    auto set_band = [&](int b) {
        ctx->band_log2 = b;
        for (int j = 0; j < ctx->m; j++) threshold_band(ctx->kfv[(size_t)j].thr, ctx->k, ctx->kfv[(size_t)j].N, &ctx->kfv[(size_t)j].T, &ctx->kfv[(size_t)j].T_hi, b);
    };
    int rc = KGMA_OK, rescans = 0;
    for (;;) {
        rc = kgma_scan_device(ctx, g, mode, flags);
        if (rc) break;
        reset_chain_stats(ctx);
        if ((flags & KGMA_F_CHAIN_REPLAY) && !(flags & KGMA_F_NO_TIE_RESOLVE)) {
            double drift = 0;
            rc = chain_decide(ctx, g, mode, buff, &drift);
            if (rc == CHAIN_DRIFT_RETRY) {
                const int b = (int)std::floor(-std::log2(drift)) - 2;        // 2^-(b + 1) >= 2 x the drift
                if (rescans >= 2 || b < 10 || b >= ctx->band_log2) {
                    rc = fail(ctx, KGMA_E_STATE, "chain replay: the running Float64 value has drifted %.3g (relative to max(distance, thr)) from the exact "
                              "distances; a guard band of 2^-%d does not cover it%s", drift, ctx->band_log2, rescans >= 2 ? " (after two repeated scans)" : "");
                    break;
                }
                set_band(b);
                rescans++;
                continue;
            }
        }
        break;
    }
    ctx->stats.chain_band_log2 = ctx->band_log2;
    ctx->stats.chain_rescans = rescans;
    if (ctx->band_log2 != ctx->band_log2_default) set_band(ctx->band_log2_default);   // (the dips carry their flags: the replay below does not read the band)
    return rc;
}

int kgma_scan(kgma_ctx *ctx, const kgma_genome *g, int32_t mode, int64_t buff, int64_t genome_pos0,
              uint32_t flags, kgma_align_fn align, void *align_user)
{
    if (!ctx) return KGMA_E_ARG;
    if (mode == KGMA_MODE_STROBE) {
        if (align) return fail(ctx, KGMA_E_UNSUPPORTED, "the strobemer scan aligns on the device: kgma_strobe_scan takes the consensus");
        return kgma_strobe_scan(ctx, g, buff, flags, nullptr, 0, 0, 0, 0);
    }
    const int rc = scan_and_decide(ctx, g, mode, buff, flags);
    if (rc) return rc;
    return replay_hits(ctx, g, mode, buff, genome_pos0, flags, align, align_user);
}

// The caller's window intervals as a request for one pair: sorted, disjoint, inside 1 .. bound.  false: they are not
static bool pair_of_intervals(int64_t contig, int32_t kfv, const int64_t *win_lo, const int64_t *win_hi, int64_t n_intervals, int64_t bound, ChainPair &p)
{
    p.c = (int32_t)contig; p.j = kfv - 1; p.d0 = p.d1 = p.a0 = p.a1 = 0;
    p.last = 0;                                                        // (here: the last window wanted)
    for (int64_t i = 0; i < n_intervals; i++) {
        if (win_lo[i] < 1 || win_hi[i] < win_lo[i] || win_lo[i] <= p.last || win_hi[i] > bound) return false;
        p.iv.push_back(ChainInterval{win_lo[i], win_hi[i]});
        p.last = win_hi[i];
    }
    return true;
}

int kgma_chain_values(kgma_ctx *ctx, const kgma_genome *g, int64_t contig, int32_t kfv, const int64_t *win_lo, const int64_t *win_hi,
                      int64_t n_intervals, double *out, int64_t cap, int64_t *n_out)
{
    if (ctx && ctx->strobe) return fail(ctx, KGMA_E_UNSUPPORTED, "%s is not served for strobemer references (kgma_set_strobe_ref)", __func__);
    if (!ctx || !g || !win_lo || !win_hi || !n_out || n_intervals < 1) return KGMA_E_ARG;
    if (ctx->m == 0) return fail(ctx, KGMA_E_STATE, "kgma_set_refs has not been called");
    if (kfv < 1 || kfv > ctx->m || contig < 0 || contig >= g->n_contigs) return fail(ctx, KGMA_E_ARG, "no such record / KFV");
    const KfvInfo &f = ctx->kfv[(size_t)(kfv - 1)];
    const int64_t L = g->cd[(size_t)contig].len, nwin = L - f.W + 1;
    std::vector<ChainPair> pairs(1);
    ChainPair &p = pairs[0];
    if (!pair_of_intervals(contig, kfv, win_lo, win_hi, n_intervals, nwin, p)) return fail(ctx, KGMA_E_ARG, "window intervals must be sorted, disjoint and inside the record");
    const int64_t prev = p.last;
    int64_t total = 0;
    for (const ChainInterval &x : p.iv) total += x.hi - x.lo + 1;
    *n_out = total;
    if (!out) return KGMA_OK;
    if (cap < total) return KGMA_E_ARG;
    {
        kgma_genome *gm = const_cast<kgma_genome *>(g);
        const int src = genome_sync(ctx, gm);
        if (src) return src;
        const unsigned long long fb = g->first_bad[(size_t)contig];
        if (fb != NO_BAD && (int64_t)fb <= f.W + prev - 1)
            return fail(ctx, KGMA_E_BADBASE, "record %lld position %llu: residue is not one of A/C/G/T/N (KeyError, Consts.jl:22-28)", (long long)contig, fb);
    }
    p.val.assign((size_t)total, 0.0);
    {
        const int irc = ensure_inter(ctx, const_cast<kgma_genome *>(g));   // (no step's reader: the whole copy)
        if (irc) return irc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));               // (the blocking copy below does not wait for the context's stream)
    }
    if (prev == 1) {
        // only window 1 is wanted: its value is the first window's kmer_count! + sqeuclidean (GenomeMiner.jl:42-47), formed on the
        // host from the window's 2-bit codes like the first value of every device chain
        const size_t dw = (size_t)((f.W + 15) / 16) + 2;
        std::vector<uint32_t> codes(dw, 0u);
        HIP_TRY(ctx, hipMemcpy(codes.data(), g->d_inter + 2 * g->cd[(size_t)contig].word_off, dw * 4, hipMemcpyDeviceToHost));
        ChainJob J = first_window_job(f, ctx->k, codes.data(), out);
        run_chain_jobs(&J, 1, 1);
        return J.ok && J.n_out == 1 ? KGMA_OK : fail(ctx, KGMA_E_HIP, "internal: first window of record %lld", (long long)contig);
    }
    std::vector<char> done(1, 0);
    ChainDevInfo info;
    const int rc = chain_on_device(ctx, g, read_chain_env(), pairs, done, info);
    if (rc) return rc;
    if (!done[0])
        return fail(ctx, KGMA_E_UNSUPPORTED, "no chain kernel served this request (KGMA_CHAIN / KGMA_CHAIN_GENERIC switched them off, the buffers did not fit, or the walk failed a drift check)");
    memcpy(out, p.val.data(), (size_t)total * sizeof(double));
    ctx->stats.chain_device_pairs = info.pairs; ctx->stats.chain_device_ms = info.kernel_ms;
    ctx->stats.chain_raw_steps = info.raw_steps; ctx->stats.chain_max_drift = info.max_drift;
    return KGMA_OK;
}

// windows a record of L residues contributes (GenomeMiner.jl:37-39,60 / OmnGenomeMiner.jl:89)
static int64_t record_windows(const kgma_ctx *ctx, int32_t mode, int64_t L)
{
    if (mode == KGMA_MODE_SINGLE) {
        const int64_t W = ctx->kfv[0].W;
        return L >= W ? L - W + 1 : 0;
    }
    int64_t maxws = 0;
    for (int j = 0; j < ctx->m; j++) maxws = std::max(maxws, ctx->kfv[(size_t)j].W);
    const int64_t n_iter = L - maxws - ctx->k + 2;
    return n_iter >= 1 ? n_iter + 1 : 0;
}

// Ties inside a dip (several windows attain its minimum) do not depend on the hit state machine: they
// can be decided where the residues are.  Called by a rank before it ships its dips (kgma_replay_dips).
int kgma_resolve_ties_local(kgma_ctx *ctx, const kgma_genome *g)
{
    if (ctx && ctx->strobe) return fail(ctx, KGMA_E_UNSUPPORTED, "%s is not served for strobemer references (kgma_set_strobe_ref)", __func__);
    if (!ctx || !g) return KGMA_E_ARG;
    if (ctx->last_mode < 0) return fail(ctx, KGMA_E_STATE, "no scan has been run");
    resolve_local_ties(ctx, g);
    return KGMA_OK;
}

// ------------------------------------------------------------------------------------------
// kgma_scan_aligned: the scan with the re-alignment of hits done ON THE DEVICE, in batches.
//   single engine (GenomeMiner.jl:96-99): the alignment does not feed back, so the hits of the scan are
//     re-aligned in one batch afterwards;
//   cluster engine (OmnGenomeMiner.jl:126-153): the aligned range feeds the overlap checks, but the range that
//     gets aligned depends only on a dip's best window (CMI) and its KFV -- so EVERY dip's candidate range
//     max(CMI - buff, 1) : min(CMI + ws - 1 + buff, L) is aligned speculatively in one batch per KFV right after
//     the scan, and the hit state machine looks the results up where the reference calls pairalign.  A range that
//     was not speculated (a tie decided differently during the replay) is aligned by the host restatement.
// ------------------------------------------------------------------------------------------
namespace {

struct AlignKey {
    int32_t contig, kfv; int64_t lo, hi;
    bool operator<(const AlignKey &o) const
    {
        if (contig != o.contig) return contig < o.contig;
        if (kfv != o.kfv) return kfv < o.kfv;
        if (lo != o.lo) return lo < o.lo;
        return hi < o.hi;
    }
};

// cigar_to_UnitRange (src/Alignment.jl:13-30), quirks included: the LAST operation is dropped from the sum, `lower` is the
// length of the FIRST operation whatever its type
void cigar_range(const char *cigar, int64_t *first, int64_t *last)
{
    int64_t curr = 0, count = 0, sum = 0, lower = 0;
    const size_t n = strlen(cigar);
    for (size_t i = 1; i <= n; i++) {
        if (i == n) break;
        const char ch = cigar[i - 1];
        if (ch >= '0' && ch <= '9') curr = curr * 10 + (ch - '0');
        else { count++; if (count == 1) lower = curr; sum += curr; curr = 0; }
    }
    *first = lower + 1; *last = sum;
}

struct AlignedScan {
    kgma_ctx *ctx; const kgma_genome *g;
    const uint8_t *const *cons; const int64_t *cons_len; int32_t go, ge;
    std::map<AlignKey, std::pair<int64_t, int64_t>> table;
    bool failed = false;
};

void aligned_cb(void *user, int32_t contig, int32_t kfv, int64_t lo, int64_t hi, int64_t L, int64_t *out_lo, int64_t *out_hi)
{
    AlignedScan *A = static_cast<AlignedScan *>(user);
    kgma_ctx *ctx = A->ctx;
    int64_t first = 1, last = hi - lo + 1;
    auto it = A->table.find(AlignKey{contig, kfv, lo, hi});
    if (it != A->table.end()) {
        first = it->second.first; last = it->second.second;
        ctx->n_align_device++;
    } else {
        // not speculated: align on the host (the library's restatement of BioAlignments' semi-global affine alignment)
        const int j = kfv > 0 ? kfv - 1 : 0;
        const int64_t n = hi - lo + 1;
        std::vector<uint8_t> seg((size_t)std::max<int64_t>(n, 1));
        std::vector<char> cig((size_t)(2 * (A->cons_len[j] + n) + 16));
        int64_t score = 0;
        if (n < 1 || hipMemcpy(seg.data(), A->g->d_ascii + A->g->cd[(size_t)contig].ascii_off + (lo - 1), (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
            kgma_host_semiglobal_cigar(A->cons[j], A->cons_len[j], seg.data(), n, A->go, A->ge, cig.data(), (int64_t)cig.size(), &score) != KGMA_OK) {
            A->failed = true;
        } else {
            cigar_range(cig.data(), &first, &last);
        }
        ctx->n_align_host++;
    }
    ctx->aligns.push_back(kgma_alignment{contig, kfv, lo, hi, first, last});
    *out_lo = std::max<int64_t>(1, lo + first - 1);                   // Alignment.jl:46 / OmnGenomeMiner.jl:133-136
    *out_hi = std::min<int64_t>(lo + last - 1, L);
}

}  // namespace

int kgma_scan_aligned(kgma_ctx *ctx, const kgma_genome *g, int32_t mode, int64_t buff, int64_t genome_pos0, uint32_t flags,
                      const uint8_t *const *consensus, const int64_t *consensus_len, int32_t gap_open_score, int32_t gap_extend_score)
{
    if (ctx && ctx->strobe) return fail(ctx, KGMA_E_UNSUPPORTED, "%s is not served for strobemer references (kgma_set_strobe_ref)", __func__);
    if (!ctx || !g) return KGMA_E_ARG;
    if (!consensus || !consensus_len) return fail(ctx, KGMA_E_ARG, "null consensus");
    if (buff < 0) return fail(ctx, KGMA_E_ARG, "buff < 0");
    const int m_used = mode == KGMA_MODE_SINGLE ? 1 : ctx->m;
    // (an empty consensus is only an error once there is something to align against it, as in the reference, where
    //  ac_gma_testing!'s default consensus_refseq fails inside pairalign at the first hit, not before)
    for (int j = 0; j < m_used; j++)
        if (consensus_len[j] < 0 || consensus_len[j] > KGMA_ALIGN_MAX_CONSENSUS || (consensus_len[j] > 0 && !consensus[j]))
            return fail(ctx, KGMA_E_UNSUPPORTED, "consensus %d: %lld residues", j + 1, (long long)consensus_len[j]);
    ctx->aligns.clear();
    ctx->n_align_device = ctx->n_align_host = 0;
    int rc = scan_and_decide(ctx, g, mode, buff, flags);
    if (rc) return rc;
    if ((flags & KGMA_F_CHAIN_REPLAY) && !(flags & KGMA_F_NO_TIE_RESOLVE)) {
        // (decided by the chain replay)
    } else if (!(flags & KGMA_F_NO_TIE_RESOLVE)) {
        rc = kgma_resolve_ties_local(ctx, g);                          // the dips' best windows are final before they are aligned
        if (rc) return rc;
    }
    if (mode == KGMA_MODE_SINGLE) {
        // GenomeMiner.jl:96-99: align the hits' ranges (consensus[1:windowsize], Alignment.jl:42) in one batch
        rc = replay_hits(ctx, g, mode, buff, genome_pos0, flags, nullptr, nullptr);
        if (rc) return rc;
        const int64_t nh = (int64_t)ctx->hits.size();
        if (nh == 0) return KGMA_OK;
        const int64_t W = ctx->kfv[0].W;
        const int64_t cl = std::min<int64_t>(consensus_len[0], W);
        if (cl < 1) return fail(ctx, KGMA_E_UNSUPPORTED, "consensus 1 is empty and %lld hits are to be aligned against it", (long long)nh);
        // (segments beyond the device aligner's rows -- windows of more than ~8000 residues -- are aligned by the host restatement)
        std::vector<int32_t> hc;
        std::vector<int64_t> lo, hi, which, first((size_t)nh), last((size_t)nh);
        int64_t n_host = 0;
        for (int64_t i = 0; i < nh; i++) {
            const kgma_hit &h = ctx->hits[(size_t)i];
            const int64_t n = h.hi - h.lo + 1;
            if (n >= 1 && n <= KGMA_ALIGN_MAX_SEGMENT) { hc.push_back(h.contig); lo.push_back(h.lo); hi.push_back(h.hi); which.push_back(i); continue; }
            std::vector<uint8_t> seg((size_t)std::max<int64_t>(n, 1));
            std::vector<char> cig((size_t)(2 * (cl + std::max<int64_t>(n, 0)) + 16));
            int64_t score = 0, f1 = 1, l1 = n;
            if (n < 1 || hipMemcpy(seg.data(), g->d_ascii + g->cd[(size_t)h.contig].ascii_off + (h.lo - 1), (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
                kgma_host_semiglobal_cigar(consensus[0], cl, seg.data(), n, gap_open_score, gap_extend_score, cig.data(), (int64_t)cig.size(), &score) != KGMA_OK)
                return fail(ctx, KGMA_E_HIP, "host fallback alignment of hit %lld failed", (long long)i);
            cigar_range(cig.data(), &f1, &l1);
            first[(size_t)i] = f1; last[(size_t)i] = l1;
            n_host++;
        }
        if (!which.empty()) {
            std::vector<int64_t> f2(which.size()), l2(which.size());
            rc = kgma_align_hits_device(ctx, g, consensus[0], cl, gap_open_score, gap_extend_score, (int64_t)which.size(), hc.data(), lo.data(), hi.data(),
                                        f2.data(), l2.data(), nullptr);
            if (rc) return rc;
            for (size_t u = 0; u < which.size(); u++) { first[(size_t)which[u]] = f2[u]; last[(size_t)which[u]] = l2[u]; }
        }
        ctx->n_align_host = n_host;
        for (int64_t i = 0; i < nh; i++) {
            kgma_hit &h = ctx->hits[(size_t)i];
            const int64_t L = ctx->contig_len[(size_t)h.contig];
            ctx->aligns.push_back(kgma_alignment{h.contig, 0, h.lo, h.hi, first[(size_t)i], last[(size_t)i]});
            const int64_t l0 = h.lo;
            h.lo = std::max<int64_t>(1, l0 + first[(size_t)i] - 1);
            h.hi = std::min<int64_t>(l0 + last[(size_t)i] - 1, L);
        }
        ctx->n_align_device = nh - n_host;
        return KGMA_OK;
    }
    // cluster engine: speculate every dip's candidate range, one device batch per KFV
    AlignedScan A{ctx, g, consensus, consensus_len, gap_open_score, gap_extend_score, {}, false};
    {
        std::vector<std::vector<AlignKey>> jobs((size_t)ctx->m);
        for (const kgma_dip &d : ctx->dips) {
            if (d.exit_pos == 0) continue;                            // open at the record end: never a hit
            const int j = d.kfv - 1;
            const int64_t L = ctx->contig_len[(size_t)d.contig];
            const int64_t CMI = d.argmin - 1;                         // OmnGenomeMiner.jl:117
            const int64_t lo = std::max<int64_t>(CMI - buff, 1), hi = std::min<int64_t>(CMI + ctx->kfv[(size_t)j].W - 1 + buff, L);
            if (hi < lo || hi - lo + 1 > KGMA_ALIGN_MAX_SEGMENT) continue;   // (the replay falls back to the host for it)
            jobs[(size_t)j].push_back(AlignKey{d.contig, d.kfv, lo, hi});
        }
        for (int j = 0; j < ctx->m; j++) {
            std::vector<AlignKey> &v = jobs[(size_t)j];
            std::sort(v.begin(), v.end());
            v.erase(std::unique(v.begin(), v.end(), [](const AlignKey &a, const AlignKey &b) { return !(a < b) && !(b < a); }), v.end());
            const int64_t n = (int64_t)v.size();
            if (n == 0) continue;
            if (consensus_len[j] < 1) return fail(ctx, KGMA_E_UNSUPPORTED, "consensus %d is empty and %lld candidate ranges are to be aligned against it", j + 1, (long long)n);
            std::vector<int32_t> hc((size_t)n);
            std::vector<int64_t> lo((size_t)n), hi((size_t)n), first((size_t)n), last((size_t)n);
            for (int64_t i = 0; i < n; i++) { hc[(size_t)i] = v[(size_t)i].contig; lo[(size_t)i] = v[(size_t)i].lo; hi[(size_t)i] = v[(size_t)i].hi; }
            rc = kgma_align_hits_device(ctx, g, consensus[j], consensus_len[j], gap_open_score, gap_extend_score, n, hc.data(), lo.data(),
                                        hi.data(), first.data(), last.data(), nullptr);
            if (rc) return rc;
            for (int64_t i = 0; i < n; i++) A.table[v[(size_t)i]] = std::make_pair(first[(size_t)i], last[(size_t)i]);
        }
    }
    rc = replay_hits(ctx, g, mode, buff, genome_pos0, flags, aligned_cb, &A);
    if (rc) return rc;
    if (A.failed) return fail(ctx, KGMA_E_HIP, "host fallback alignment failed");
    return KGMA_OK;
}

// ------------------------------------------------------------------------------------------
// The strobemer engine's host half (StrobeGenomeMiner.jl:46-91, Alignment.jl:83-111).  The hit state machine is the single
// engine's over the dips, with CMI = the best window's step i (virtual window start - 1) and with the score gate of process_hit!
// applied AFTER the machine has run: the gate returns before append_hit!, but goal_ind and currminim are updated by the caller
// whether or not the hit was kept, so alignment never feeds back.  Candidates first, one alignment batch, then the gate.
// ------------------------------------------------------------------------------------------
namespace {

// The reference's sequential Float64 loop over one record (KGMA_F_CHAIN_REPLAY): residues -> randstrobe bins -> first window summed
// left to right -> the running update in the reference's operation order.  The exact integer D is carried along for kgma_hit.D.
// This file is compiled with -ffp-contract=off: every rounding below is the reference's.
void strobe_float_record(const kgma_ctx *ctx, const uint8_t *res, int64_t L, int64_t c, int64_t buff, int64_t genome_pos, std::vector<kgma_hit> &out)
{
    const KfvInfo &f = ctx->kfv[0];
    const int s = ctx->st_s, w_min = ctx->st_wmin, w_max = ctx->st_wmax, k = ctx->k;
    const int64_t q = ctx->st_q, W = f.W, N = f.N;
    const int64_t NB = (int64_t)1 << (4 * s);
    const int64_t n_items = std::max<int64_t>(W - k + 1, L - k - 1);  // strobemers the loop reads
    std::vector<uint8_t> code((size_t)L);
    for (int64_t i = 0; i < L; i++) { const int cd = res_code(res[i]); code[(size_t)i] = (uint8_t)(cd < 0 ? 0 : cd); }   // (a residue the reference never looks up)
    const int64_t n_s = L - s + 1;
    std::vector<uint32_t> smer((size_t)n_s);
    for (int64_t i = 0; i < n_s; i++) {
        uint32_t v = 0;
        for (int j = 0; j < s; j++) v = (v << 2) | code[(size_t)(i + j)];
        smer[(size_t)i] = v;
    }
    std::vector<uint32_t> bin((size_t)n_items);
    for (int64_t p = 0; p < n_items; p++) {
        const uint32_t first = smer[(size_t)p];
        uint32_t second = smer[(size_t)(p + w_min - 1)];
        for (int o = w_min; o <= w_max; o++) {                         // Strobemers.jl:52-60: the last offset of score 0, else w_min
            const uint32_t cand = smer[(size_t)(p + o - 1)];
            if ((int64_t)(first + cand) % q == 0) second = cand;
        }
        bin[(size_t)p] = (first << (2 * s)) | second;
    }
    std::vector<double> cur((size_t)NB, 0.0);
    std::vector<int64_t> ci((size_t)NB, 0);
    for (int64_t p = 0; p <= W - k; p++) { cur[bin[(size_t)p]] += 1.0; ci[bin[(size_t)p]] += 1; }
    double acc = 0.0;
    int64_t D = 0;
    for (int64_t x = 0; x < NB; x++) {
        const double d = f.ref[(size_t)x] - cur[(size_t)x];
        acc += d * d;
        const int64_t e = f.S[(size_t)x] - N * ci[(size_t)x];
        D += e * e;
    }
    double kd = (1.0 / (double)(2 * k)) * acc;                          // StrobeGenomeMiner.jl:43
    const double SF = 1.0 / (double)k;                                  // :137
    const double thr = f.thr;
    int64_t CMI = 2, goal_ind = 0, curD = D;
    bool stop = true;
    double currminim = kd;
    for (int64_t i = 1; i <= L - W - 1; i++) {
        const uint32_t l = bin[(size_t)(i - 1)], r = bin[(size_t)(i - 1 + W - k)];
        if (l != r) {
            double t = 1.0 + cur[r];                                   // :60-62, left to right
            t = t + f.ref[l];
            t = t - f.ref[r];
            t = t - cur[l];
            kd += SF * t;
            D += 2 * N * (f.S[l] - f.S[r] - N * (ci[l] - 1 - ci[r]));
            cur[l] -= 1.0; cur[r] += 1.0;
            ci[l] -= 1; ci[r] += 1;
        }
        if (kd < thr) {
            if (kd < currminim) { currminim = kd; curD = D; CMI = i; stop = false; }
        } else if (!stop) {
            stop = true;
            CMI += 1;
            if (CMI > goal_ind) {
                goal_ind = CMI + W - 1;
                kgma_hit h;
                memset(&h, 0, sizeof h);
                h.contig = (int32_t)c; h.kfv = 0; h.cmi = CMI;
                h.lo = std::max<int64_t>(CMI - buff, 1); h.hi = std::min<int64_t>(CMI + W - 1 + buff, L);
                h.genome_pos = genome_pos; h.D = curD; h.dist = currminim; h.flags = KGMA_HIT_CHAIN;
                out.push_back(h);
                currminim = kd; curD = D;
            }
        }
    }
}

// candidates of every record: the dip machine on exact integers, or (chain) the Float64 replay for the records that need it
int strobe_candidates(kgma_ctx *ctx, const kgma_genome *g, int64_t buff, uint32_t flags)
{
    const bool chain = (flags & KGMA_F_CHAIN_REPLAY) && !(flags & KGMA_F_NO_TIE_RESOLVE);
    const double t0 = now_ms();
    const KfvInfo &f = ctx->kfv[0];
    const int64_t W = f.W;
    const double scale = 2.0 * (double)ctx->k * (double)f.N * (double)f.N;
    const int64_t nc = (int64_t)ctx->contig_len.size();
    reset_chain_stats(ctx);
    ctx->stats.chain_band_log2 = ctx->band_log2; ctx->stats.chain_rescans = 0;
    ctx->hits.clear();
    size_t di = 0, ai = 0;
    int64_t genome_pos = 0;                                            // StrobeGenomeMiner.jl:24
    std::vector<kgma_hit> rec_hits;
    std::vector<uint8_t> res;
    double chain_ms = 0;
    for (int64_t c = 0; c < nc; c++) {
        const int64_t L = ctx->contig_len[(size_t)c];
        if (ctx->contig_nwin[(size_t)c] == 0) continue;                // L < W: :36 (genome_pos does not advance)
        const int64_t D1 = ctx->firstD[(size_t)c];
        int64_t CMI = 2, goal_ind = 0, currmin = D1;                   // :46
        bool stop = true, flagged = false;
        uint32_t cur_flags = 0;
        rec_hits.clear();
        while (di < ctx->dips.size() && ctx->dips[di].contig < c) di++;
        for (; di < ctx->dips.size() && ctx->dips[di].contig == c; di++) {
            kgma_dip &d = ctx->dips[di];
            const bool improved = d.D_min < currmin;                   // :73-77 (strict running minimum)
            if (!improved && d.D_min == currmin) d.flags |= KGMA_HIT_TIE;   // equal to the stale running minimum: rounding decides in the reference
            if (d.flags & (KGMA_HIT_TIE | KGMA_HIT_AT_THRESHOLD)) flagged = true;
            if (improved) {
                currmin = d.D_min;
                CMI = d.argmin - 1;                                    // the step i whose window starts at i + 1
                stop = false;
                cur_flags = d.flags;
            }
            if (d.exit_pos == 0) continue;                             // dip still open at the record end
            if (!stop) {                                               // :80-90
                stop = true;
                CMI += 1;
                if (CMI > goal_ind) {
                    goal_ind = CMI + W - 1;
                    kgma_hit h;
                    memset(&h, 0, sizeof h);
                    h.contig = (int32_t)c; h.kfv = 0; h.cmi = CMI;
                    h.lo = std::max<int64_t>(CMI - buff, 1); h.hi = std::min<int64_t>(CMI + W - 1 + buff, L);
                    h.genome_pos = genome_pos; h.D = currmin; h.dist = (double)currmin / scale;
                    h.flags = cur_flags | (d.flags & KGMA_HIT_AT_THRESHOLD);
                    rec_hits.push_back(h);
                    currmin = d.D_exit;                                // :88
                }
            }
        }
        while (ai < ctx->att.size() && ctx->att[ai].contig < c) ai++;
        if (ai < ctx->att.size() && ctx->att[ai].contig == c) flagged = true;   // a tested window inside the threshold band
        if (chain && flagged && g) {
            const double t1 = now_ms();
            res.resize((size_t)L);
            const int frc = kgma_genome_fetch(ctx, g, c, 1, L, res.data());
            if (frc) return frc;
            rec_hits.clear();
            strobe_float_record(ctx, res.data(), L, c, buff, genome_pos, rec_hits);
            ctx->stats.n_chain_pairs++;
            ctx->stats.chain_windows += std::max<int64_t>(L - W, 1);
            chain_ms += now_ms() - t1;
        }
        ctx->hits.insert(ctx->hits.end(), rec_hits.begin(), rec_hits.end());
        genome_pos += L;                                               // :92
    }
    ctx->stats.chain_ms = chain_ms;
    ctx->stats.n_tie_flagged = 0;
    for (const kgma_dip &dd : ctx->dips) ctx->stats.n_tie_flagged += (dd.flags & KGMA_HIT_TIE) ? 1 : 0;
    ctx->stats.replay_ms = now_ms() - t0 - chain_ms;
    return KGMA_OK;
}

}  // namespace

int kgma_strobe_scan(kgma_ctx *ctx, const kgma_genome *g, int64_t buff, uint32_t flags, const uint8_t *consensus, int64_t consensus_len,
                     int32_t gap_open_score, int32_t gap_extend_score, int64_t score_threshold)
{
    if (!ctx || !g) return KGMA_E_ARG;
    if (buff < 0) return fail(ctx, KGMA_E_ARG, "buff < 0");
    if (consensus && (consensus_len < 0 || consensus_len > KGMA_ALIGN_MAX_CONSENSUS))
        return fail(ctx, KGMA_E_UNSUPPORTED, "consensus: %lld residues", (long long)consensus_len);
    ctx->aligns.clear();
    ctx->n_align_device = ctx->n_align_host = 0;
    int rc = kgma_scan_device(ctx, g, KGMA_MODE_STROBE, flags);
    if (rc) return rc;
    rc = strobe_candidates(ctx, g, buff, flags);
    if (rc) return rc;
    const int64_t nh = (int64_t)ctx->hits.size();
    if (consensus && nh > 0) {
        // process_hit! (Alignment.jl:91-106): pairalign against consensus[1:windowsize], the score gate, cigar_to_UnitRange
        const int64_t cl = std::min<int64_t>(consensus_len, ctx->kfv[0].W);
        if (cl < 1) return fail(ctx, KGMA_E_UNSUPPORTED, "the consensus is empty and %lld candidates are to be aligned against it", (long long)nh);
        std::vector<int32_t> hc;
        std::vector<int64_t> lo, hi, which, first((size_t)nh), last((size_t)nh), score((size_t)nh);
        int64_t n_host = 0;
        for (int64_t i = 0; i < nh; i++) {
            const kgma_hit &h = ctx->hits[(size_t)i];
            const int64_t n = h.hi - h.lo + 1;
            if (n >= 1 && n <= KGMA_ALIGN_MAX_SEGMENT) { hc.push_back(h.contig); lo.push_back(h.lo); hi.push_back(h.hi); which.push_back(i); continue; }
            // (segments beyond the device aligner's rows: the host restatement)
            std::vector<uint8_t> seg((size_t)std::max<int64_t>(n, 1));
            std::vector<char> cig((size_t)(2 * (cl + std::max<int64_t>(n, 0)) + 16));
            int64_t sc = 0, f1 = 1, l1 = n;
            if (n < 1 || hipMemcpy(seg.data(), g->d_ascii + g->cd[(size_t)h.contig].ascii_off + (h.lo - 1), (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
                kgma_host_semiglobal_cigar(consensus, cl, seg.data(), n, gap_open_score, gap_extend_score, cig.data(), (int64_t)cig.size(), &sc) != KGMA_OK)
                return fail(ctx, KGMA_E_HIP, "host alignment of candidate %lld failed", (long long)i);
            cigar_range(cig.data(), &f1, &l1);
            first[(size_t)i] = f1; last[(size_t)i] = l1; score[(size_t)i] = sc;
            n_host++;
        }
        if (!which.empty()) {
            std::vector<int64_t> f2(which.size()), l2(which.size()), s2(which.size());
            rc = kgma_align_hits_device(ctx, g, consensus, cl, gap_open_score, gap_extend_score, (int64_t)which.size(), hc.data(), lo.data(), hi.data(),
                                        f2.data(), l2.data(), s2.data());
            if (rc) return rc;
            for (size_t u = 0; u < which.size(); u++) { first[(size_t)which[u]] = f2[u]; last[(size_t)which[u]] = l2[u]; score[(size_t)which[u]] = s2[u]; }
        }
        ctx->n_align_host = n_host;
        ctx->n_align_device = nh - n_host;
        std::vector<kgma_hit> kept;
        for (int64_t i = 0; i < nh; i++) {
            kgma_hit h = ctx->hits[(size_t)i];
            if (score[(size_t)i] < score_threshold) continue;          // Alignment.jl:96-98
            const int64_t L = ctx->contig_len[(size_t)h.contig];
            ctx->aligns.push_back(kgma_alignment{h.contig, 0, h.lo, h.hi, first[(size_t)i], last[(size_t)i]});
            const int64_t l0 = h.lo;
            h.lo = std::max<int64_t>(1, l0 + first[(size_t)i] - 1);
            h.hi = std::min<int64_t>(l0 + last[(size_t)i] - 1, L);
            kept.push_back(h);
        }
        ctx->hits.swap(kept);
    }
    ctx->stats.n_hits = (int64_t)ctx->hits.size();
    return KGMA_OK;
}

int kgma_get_alignments(kgma_ctx *ctx, kgma_alignment *out, int64_t cap, int64_t *n, int64_t *n_device, int64_t *n_host)
{
    if (!ctx || !n) return KGMA_E_ARG;
    *n = (int64_t)ctx->aligns.size();
    if (n_device) *n_device = ctx->n_align_device;
    if (n_host) *n_host = ctx->n_align_host;
    if (!out) return KGMA_OK;
    if (cap < *n) return fail(ctx, KGMA_E_ARG, "kgma_get_alignments: capacity %lld < %lld", (long long)cap, (long long)*n);
    if (*n) memcpy(out, ctx->aligns.data(), (size_t)*n * sizeof(kgma_alignment));
    return KGMA_OK;
}

int kgma_set_residue_source(kgma_ctx *ctx, kgma_fetch_fn fn, void *user)
{
    if (!ctx) return KGMA_E_ARG;
    ctx->fetch = fn; ctx->fetch_user = user;
    return KGMA_OK;
}

int kgma_get_dip_last_min(kgma_ctx *ctx, int64_t *out, int64_t cap, int64_t *n)
{
    if (!ctx || !n) return KGMA_E_ARG;
    *n = (int64_t)ctx->dip_argl.size();
    if (!out) return KGMA_OK;
    if (cap < *n) return fail(ctx, KGMA_E_ARG, "kgma_get_dip_last_min: capacity too small");
    if (*n) memcpy(out, ctx->dip_argl.data(), (size_t)*n * sizeof(int64_t));
    return KGMA_OK;
}

// Hit state machine over dips that were found elsewhere (other GPUs of a sharded scan): record lengths,
// the D of every record's first window per KFV ([m][n_records], -1 for skipped records), and the dips
// in whole-record coordinates, sorted by (record, KFV, start).  Needs kgma_set_refs only.
int kgma_replay_dips(kgma_ctx *ctx, int32_t mode, int64_t buff, int64_t genome_pos0, uint32_t flags, int64_t n_records,
                     const int64_t *record_len, const int64_t *first_D, const kgma_dip *dips, const int64_t *dip_last_min,
                     int64_t n_dips, kgma_align_fn align, void *align_user)
{
    if (ctx && ctx->strobe) return fail(ctx, KGMA_E_UNSUPPORTED, "%s is not served for strobemer references (kgma_set_strobe_ref)", __func__);
    if (!ctx || n_records < 0 || n_dips < 0 || (n_records && (!record_len || !first_D)) || (n_dips && (!dips || !dip_last_min)))
        return KGMA_E_ARG;
    if (ctx->m == 0) return fail(ctx, KGMA_E_STATE, "kgma_set_refs has not been called");
    if (mode != KGMA_MODE_SINGLE && mode != KGMA_MODE_OMN) return fail(ctx, KGMA_E_ARG, "unknown mode %d", mode);
    ctx->contig_len.assign(record_len, record_len + n_records);
    ctx->contig_nwin.assign((size_t)n_records, 0);
    for (int64_t c = 0; c < n_records; c++) ctx->contig_nwin[(size_t)c] = record_windows(ctx, mode, record_len[c]);
    ctx->firstD.assign(first_D, first_D + (size_t)ctx->m * (size_t)n_records);
    ctx->dips.assign(dips, dips + n_dips);
    ctx->dip_argl.assign(dip_last_min, dip_last_min + n_dips);
    ctx->dip_aux.assign((size_t)n_dips, -1);
    ctx->att.swap(ctx->att_next);                                      // (kgma_set_att; empty otherwise)
    ctx->att_next.clear();
    for (const kgma_ctx::AttWin &a : ctx->att)
        if (a.contig < 0 || a.contig >= n_records || a.kfv < 0 || a.kfv >= ctx->m) return fail(ctx, KGMA_E_ARG, "kgma_set_att: window of record %d / KFV %d", a.contig, a.kfv + 1);
    ctx->chain_pair.clear(); ctx->firstF.clear(); ctx->dip_fmin.clear(); ctx->dip_fexit.clear();
    for (int64_t i = 1; i < n_dips; i++) {
        const kgma_dip &a = dips[i - 1], &b = dips[i];
        const bool ordered = a.contig < b.contig || (a.contig == b.contig && (a.kfv < b.kfv || (a.kfv == b.kfv && a.start < b.start)));
        if (!ordered) return fail(ctx, KGMA_E_ARG, "kgma_replay_dips: dips are not sorted by (record, KFV, start) at %lld", (long long)i);
    }
    for (int64_t i = 0; i < n_dips; i++)
        if (dips[i].contig < 0 || dips[i].contig >= n_records || dips[i].kfv < 1 || dips[i].kfv > ctx->m)
            return fail(ctx, KGMA_E_ARG, "kgma_replay_dips: dip %lld refers to record %d / KFV %d", (long long)i, dips[i].contig, dips[i].kfv);
    ctx->tiles.clear();
    ctx->scan_filtered = false;
    ctx->contig_tile_base.assign((size_t)n_records, -1);
    ctx->tk_uid = 0;            // the scan's cached tile geometry is gone: the next scan rebuilds it
    ctx->have_dists = false;
    ctx->last_mode = mode;
    ctx->stats.n_dips = n_dips;
    reset_chain_stats(ctx);
    if ((flags & KGMA_F_CHAIN_REPLAY) && !(flags & KGMA_F_NO_TIE_RESOLVE) && ctx->chain_src) {
        const int rc = chain_decide(ctx, nullptr, mode, buff);
        if (rc) return rc;
    }
    return replay_hits(ctx, nullptr, mode, buff, genome_pos0, flags, align, align_user);
}

int kgma_kfv_scale(kgma_ctx *ctx, int32_t kfv, double *scale, int64_t *n_refs)
{
    if (!ctx || !scale) return KGMA_E_ARG;
    if (kfv < 1 || kfv > ctx->m) return fail(ctx, KGMA_E_ARG, "no such KFV");
    const KfvInfo &f = ctx->kfv[(size_t)(kfv - 1)];
    *scale = 2.0 * (double)ctx->k * (double)f.N * (double)f.N;
    if (n_refs) *n_refs = f.N;
    return KGMA_OK;
}

int kgma_kfv_is_float(kgma_ctx *ctx, int32_t kfv, int32_t *is_float)
{
    if (!ctx || !is_float) return KGMA_E_ARG;
    if (kfv < 1 || kfv > ctx->m) return fail(ctx, KGMA_E_ARG, "no such KFV");
    *is_float = ctx->kfv[(size_t)(kfv - 1)].fp ? 1 : 0;
    return KGMA_OK;
}

int kgma_set_chain_source(kgma_ctx *ctx, kgma_chain_fn fn, void *user)
{
    if (!ctx) return KGMA_E_ARG;
    ctx->chain_src = fn; ctx->chain_user = user;
    return KGMA_OK;
}

int kgma_get_att(kgma_ctx *ctx, int32_t *contig, int32_t *kfv, int64_t *pos, int64_t cap, int64_t *n)
{
    if (!ctx || !n) return KGMA_E_ARG;
    *n = (int64_t)ctx->att.size();
    if (!contig && !kfv && !pos) return KGMA_OK;
    if (!contig || !kfv || !pos || cap < *n) return fail(ctx, KGMA_E_ARG, "kgma_get_att: capacity %lld < %lld", (long long)cap, (long long)*n);
    for (int64_t i = 0; i < *n; i++) { contig[i] = ctx->att[(size_t)i].contig; kfv[i] = ctx->att[(size_t)i].kfv + 1; pos[i] = ctx->att[(size_t)i].pos; }
    return KGMA_OK;
}

int kgma_set_att(kgma_ctx *ctx, const int32_t *contig, const int32_t *kfv, const int64_t *pos, int64_t n)
{
    if (!ctx || n < 0 || (n && (!contig || !kfv || !pos))) return KGMA_E_ARG;
    ctx->att_next.clear();
    for (int64_t i = 0; i < n; i++) ctx->att_next.push_back(kgma_ctx::AttWin{contig[i], kfv[i] - 1, pos[i]});
    std::sort(ctx->att_next.begin(), ctx->att_next.end(), [](const kgma_ctx::AttWin &a, const kgma_ctx::AttWin &b) {
        if (a.contig != b.contig) return a.contig < b.contig;
        if (a.kfv != b.kfv) return a.kfv < b.kfv;
        return a.pos < b.pos;
    });
    return KGMA_OK;
}

int kgma_chain_export(kgma_ctx *ctx, const kgma_genome *g, int64_t contig, int32_t kfv, int64_t last_window, const int64_t *win_lo,
                      const int64_t *win_hi, int64_t n_intervals, int64_t *n_streams, int64_t *n_chunks, int64_t *pool_units, double *first)
{
    if (ctx && ctx->strobe) return fail(ctx, KGMA_E_UNSUPPORTED, "%s is not served for strobemer references (kgma_set_strobe_ref)", __func__);
    if (!ctx || !g || !n_streams || !n_chunks || !pool_units || !first || n_intervals < 0 || (n_intervals && (!win_lo || !win_hi))) return KGMA_E_ARG;
    if (ctx->m == 0) return fail(ctx, KGMA_E_STATE, "kgma_set_refs has not been called");
    if (kfv < 1 || kfv > ctx->m || contig < 0 || contig >= g->n_contigs) return fail(ctx, KGMA_E_ARG, "no such record / KFV");
    const KfvInfo &f = ctx->kfv[(size_t)(kfv - 1)];
    const int64_t nwin = g->cd[(size_t)contig].len - f.W + 1;
    if (last_window < 2 || last_window > nwin) return fail(ctx, KGMA_E_ARG, "last window %lld outside 2 ... %lld", (long long)last_window, (long long)nwin);
    std::vector<ChainPair> pairs(1);
    ChainPair &p = pairs[0];
    if (!pair_of_intervals(contig, kfv, win_lo, win_hi, n_intervals, last_window, p)) return fail(ctx, KGMA_E_ARG, "window intervals must be sorted, disjoint and <= the last window");
    p.last = last_window;
    {
        kgma_genome *gm = const_cast<kgma_genome *>(g);
        const int src = genome_sync(ctx, gm);
        if (src) return src;
    }
    const ChainEnv env = read_chain_env();
    const int which = chain_kernel_for(ctx, f, env);
    if (which == 0) return fail(ctx, KGMA_E_UNSUPPORTED, "no chain kernel serves this KFV");
    std::vector<char> done(1, 0);
    ChainDevInfo info;
    (void)hipSetDevice(ctx->device);
    {
        // (a rank's part of a sharded step's chain: the record's blocks, like the step's own chain)
        const int prc = pack_record_blocks(ctx, const_cast<kgma_genome *>(g), std::vector<int32_t>(1, (int32_t)contig));
        if (prc) return prc;
    }
    ChainBatch batch(ctx, g, env, pairs, done, info, std::vector<size_t>(1, 0), 0, which == 2);
    batch.export_only = true;
    const int rc = run_chain_batch(batch, false);
    if (rc) return rc;
    if (!done[0]) return fail(ctx, KGMA_E_NOMEM, "the chain kernel's buffers do not fit");
    *n_streams = (int64_t)ctx->cx_streams.size(); *n_chunks = (int64_t)ctx->cx_chunks.size(); *pool_units = (int64_t)ctx->cx_pool.size();
    *first = ctx->cx_first;
    return KGMA_OK;
}

int kgma_chain_export_copy(kgma_ctx *ctx, int64_t *win0, int32_t *n_valid, int64_t *chunk_base, int64_t *D0, void *chunks, void *pool)
{
    if (!ctx || !win0 || !n_valid || !chunk_base || !D0 || !chunks) return KGMA_E_ARG;
    for (size_t i = 0; i < ctx->cx_streams.size(); i++) {
        win0[i] = ctx->cx_streams[i].win0; n_valid[i] = ctx->cx_streams[i].n_valid; chunk_base[i] = ctx->cx_streams[i].chunk_base; D0[i] = ctx->cx_streams[i].D0;
    }
    if (!ctx->cx_chunks.empty()) memcpy(chunks, ctx->cx_chunks.data(), ctx->cx_chunks.size() * sizeof(ChainChunk));
    if (pool && !ctx->cx_pool.empty()) memcpy(pool, ctx->cx_pool.data(), ctx->cx_pool.size() * sizeof(ChainChunk));
    return KGMA_OK;
}

// ------------------------------------------------------------------------------------------
// threshold calibration: distances of chosen windows of a genome and of mutated copies of sequences (the working form of
// src/DistanceTesting.jl; kernels: kgma_calib.hip)
// ------------------------------------------------------------------------------------------
constexpr int64_t CALIB_TAB_DWORDS = (int64_t)1 << 24;   // calib_grid(k, ...) x 4^k counters at k = 8, 9, 10: 64 MiB

// The checks both entry points make of the context and the KFV; *fo: the KFV.
static int calib_kfv(kgma_ctx *ctx, const char *what, int32_t kfv, const KfvInfo **fo)
{
    if (ctx->strobe) return fail(ctx, KGMA_E_STATE, "%s: the context holds a strobemer reference (kgma_set_strobe_ref); call kgma_set_refs first", what);
    if (ctx->m < 1) return fail(ctx, KGMA_E_STATE, "%s: no references (call kgma_set_refs first)", what);
    if (kfv < 1 || kfv > ctx->m) return fail(ctx, KGMA_E_ARG, "%s: no such KFV: %d (1 ... %d)", what, kfv, ctx->m);
    if (ctx->k > 10) return fail(ctx, KGMA_E_UNSUPPORTED, "%s: k = %d: references at k >= 11 are kept sparse; this call serves 1 <= k <= 10", what, ctx->k);
    *fo = &ctx->kfv[(size_t)(kfv - 1)];
    return KGMA_OK;
}

// What both share behind their checks: the KFV's tables, the counter table, one launch between the context's events, the
// download.  a: text, item_off, n_items (> 0) and the source's own fields are set.  *bad: first_bad as the kernel left it.
static int calib_launch(kgma_ctx *ctx, const char *what, int source, CalibArgs &a, const KfvInfo &f, int32_t kfv, int64_t *D_out,
                        double *dist_out, unsigned long long *bad)
{
    const int k = ctx->k;
    const int64_t NB = (int64_t)1 << (2 * k), n = a.n_items;
    int rc;
    if ((rc = dev_reserve(ctx, ctx->d_cbD, ctx->cbD_cap, n))) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_cbdist, ctx->cbdist_cap, n))) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_cbbad, ctx->cbbad_cap, 1))) return rc;
    if (k > 7 && !ctx->d_cbtab) {
        if ((rc = dev_reserve(ctx, ctx->d_cbtab, ctx->cbtab_cap, CALIB_TAB_DWORDS))) return rc;
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_cbtab, 0, (size_t)CALIB_TAB_DWORDS * 4, ctx->stream));
    }
    const int grid = calib_grid(k, n, ctx->n_cus);
    if (k > 7 && (int64_t)grid * NB > CALIB_TAB_DWORDS) return fail(ctx, KGMA_E_STATE, "%s: internal error: counter table too small", what);
    a.k = k; a.fp = f.fp ? 1 : 0;
    a.S = ctx->d_Stab + (size_t)(kfv - 1) * (size_t)NB;
    a.R = ctx->d_Rtab + (size_t)(kfv - 1) * (size_t)NB;
    a.N = f.N; a.sumS2 = f.sumS2;
    a.scale = 2.0 * (double)k * (double)f.N * (double)f.N;
    a.half_inv_k = 1.0 / (double)(2 * k);
    a.scratch = ctx->d_cbtab; a.D_out = ctx->d_cbD; a.dist_out = ctx->d_cbdist; a.first_bad = ctx->d_cbbad;
    *bad = NO_BAD;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_cbbad, bad, 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    HIP_TRY(ctx, launch_calib(a, source, grid, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(bad, ctx->d_cbbad, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (dist_out) HIP_TRY(ctx, hipMemcpyAsync(dist_out, ctx->d_cbdist, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (D_out && !f.fp) HIP_TRY(ctx, hipMemcpyAsync(D_out, ctx->d_cbD, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<double> tmp;
    if (D_out && f.fp && !dist_out) {
        tmp.resize((size_t)n);
        HIP_TRY(ctx, hipMemcpyAsync(tmp.data(), ctx->d_cbdist, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    ctx->stats.scan_ms = ms;
    ctx->stats.n_launches = 1;
    snprintf(ctx->kernel_name, sizeof ctx->kernel_name, "calib_kernel<%s,%s,%s>", source == 0 ? "window" : "mutation",
             k <= 7 ? "lds" : "global", f.fp ? "f64" : "int");
    if (D_out && f.fp && *bad == NO_BAD) {
        // the header's D of a Float64 KFV: the distance on the host's integer lattice (lattice_of)
        const double *d = dist_out ? dist_out : tmp.data();
        for (int64_t i = 0; i < n; i++) D_out[i] = (int64_t)std::llround(d[i] * a.scale);
    }
    return KGMA_OK;
}

// KGMA_E_BADBASE of the window calls.  bad: the smallest byte offset of a bad residue the requested windows looked up; its record is
// the one it lies in.
static int window_bad(kgma_ctx *ctx, const kgma_genome *g, unsigned long long bad)
{
    int64_t c = 0;
    for (int64_t r = 0; r < g->n_contigs; r++)
        if (g->cd[(size_t)r].len > 0 && g->cd[(size_t)r].ascii_off <= (int64_t)bad &&
            (int64_t)bad < g->cd[(size_t)r].ascii_off + g->cd[(size_t)r].len) c = r;
    return fail(ctx, KGMA_E_BADBASE, "record %lld position %lld: residue is not one of A/C/G/T/N (KeyError, Consts.jl:22-28)", (long long)c,
                (long long)((int64_t)bad - g->cd[(size_t)c].ascii_off + 1));
}

int kgma_window_dists(kgma_ctx *ctx, const kgma_genome *g, int32_t kfv, int64_t n, const int32_t *contig, const int64_t *start,
                      int64_t *D_out, double *dist_out)
{
    if (!ctx || !g) return KGMA_E_ARG;
    const KfvInfo *fp_ = nullptr;
    int rc = calib_kfv(ctx, "kgma_window_dists", kfv, &fp_);
    if (rc) return rc;
    const KfvInfo &f = *fp_;
    if (n < 0 || (n > 0 && (!contig || !start))) return fail(ctx, KGMA_E_ARG, "kgma_window_dists: null argument or n < 0");
    std::vector<int64_t> off((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const int64_t c = contig[i];
        if (c < 0 || c >= g->n_contigs) return fail(ctx, KGMA_E_ARG, "kgma_window_dists: window %lld: no record %lld", (long long)i, (long long)c);
        const ContigDesc &d = g->cd[(size_t)c];
        if (start[i] < 1 || start[i] > d.len - f.W + 1)
            return fail(ctx, KGMA_E_ARG, "kgma_window_dists: window %lld: residues %lld .. %lld do not lie inside record %lld of %lld residues",
                        (long long)i, (long long)start[i], (long long)(start[i] + f.W - 1), (long long)c, (long long)d.len);
        off[(size_t)i] = d.ascii_off + (start[i] - 1);
    }
    ctx->stats.scan_ms = 0;
    ctx->stats.n_launches = 0;
    if (n == 0) return KGMA_OK;
    (void)hipSetDevice(ctx->device);
    if ((rc = dev_reserve(ctx, ctx->d_cboff, ctx->cboff_cap, n))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_cboff, off.data(), (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    CalibArgs a;
    memset(&a, 0, sizeof a);
    a.text = g->d_ascii; a.item_off = ctx->d_cboff; a.n_items = n; a.W = f.W;
    unsigned long long bad = NO_BAD;
    if ((rc = calib_launch(ctx, "kgma_window_dists", 0, a, f, kfv, D_out, dist_out, &bad))) return rc;
    if (bad != NO_BAD) return window_bad(ctx, g, bad);
    return KGMA_OK;
}

// What kgma_mutation_dists and kgma_strobe_mutation_dists share behind the check of their references: the argument checks (a
// sequence of len residues holds len - k + 1 `unit`s), the uploads and the mutation source's fields of `a`.  off: the sequences'
// offsets from the first one's; empty: there is nothing to launch.
struct MutationUpload { std::vector<int64_t> off; std::vector<uint64_t> P; bool empty = true; };   // (what the copies read lives until the launch's synchronise)
static int mutation_source(kgma_ctx *ctx, const char *what, const char *unit, const KfvInfo &f, const uint8_t *seqs, const int64_t *offsets,
                           int64_t n_seqs, const double *rates, int32_t n_rates, int32_t n_trials, uint64_t seed, CalibArgs &a,
                           MutationUpload &u)
{
    std::vector<int64_t> &off = u.off;
    std::vector<uint64_t> &P = u.P;
    u.empty = true;
    if (n_seqs < 0 || !offsets || !rates) return fail(ctx, KGMA_E_ARG, "%s: null argument or n_seqs < 0", what);
    if (n_rates < 1 || n_trials < 1) return fail(ctx, KGMA_E_ARG, "%s: n_rates = %d, n_trials = %d (both at least 1)", what, n_rates, n_trials);
    P.assign((size_t)n_rates, 0);
    for (int32_t r = 0; r < n_rates; r++) {
        if (!std::isfinite(rates[r]) || rates[r] < 0.0 || rates[r] > 1.0)
            return fail(ctx, KGMA_E_ARG, "%s: rates[%d] = %g is not in [0, 1]", what, r, rates[r]);
        P[(size_t)r] = (uint64_t)std::floor(std::ldexp(rates[r], 53));
    }
    for (int64_t i = 0; i < n_seqs; i++) {
        if (offsets[i + 1] < offsets[i]) return fail(ctx, KGMA_E_ARG, "%s: offsets[%lld] > offsets[%lld]", what, (long long)i, (long long)(i + 1));
        const int64_t nk = std::max<int64_t>(offsets[i + 1] - offsets[i] - ctx->k + 1, 0);
        if (!f.fp && (__int128)f.sumS2 + (__int128)f.N * f.N * nk * (__int128)nk >= ((__int128)1 << 61))
            return fail(ctx, KGMA_E_UNSUPPORTED, "%s: sequence %lld: N = %lld with %lld %s exceeds the int64 range of the device path", what,
                        (long long)i, (long long)f.N, (long long)nk, unit);
        if (f.fp && nk > ((int64_t)1 << 31))
            return fail(ctx, KGMA_E_UNSUPPORTED, "%s: sequence %lld: %lld %s exceed the 32-bit counters", what, (long long)i, (long long)nk, unit);
    }
    const __int128 n_items128 = (__int128)n_seqs * n_rates * n_trials;
    if (n_items128 > ((__int128)1 << 28)) return fail(ctx, KGMA_E_UNSUPPORTED, "%s: %lld x %d x %d distances in one call", what, (long long)n_seqs, n_rates, n_trials);
    ctx->stats.scan_ms = 0;
    ctx->stats.n_launches = 0;
    if (n_seqs == 0) return KGMA_OK;
    const int64_t base = offsets[0], bytes = offsets[n_seqs] - base;
    if (bytes > 0 && !seqs) return fail(ctx, KGMA_E_ARG, "%s: null argument", what);
    off.resize((size_t)n_seqs + 1);
    for (int64_t i = 0; i <= n_seqs; i++) off[(size_t)i] = offsets[i] - base;
    (void)hipSetDevice(ctx->device);
    int rc;
    if ((rc = dev_reserve(ctx, ctx->d_cboff, ctx->cboff_cap, n_seqs + 1))) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_cbtext, ctx->cbtext_cap, bytes))) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_cbP, ctx->cbP_cap, n_rates))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_cboff, off.data(), off.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    if (bytes) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_cbtext, seqs + base, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_cbP, P.data(), P.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    memset(&a, 0, sizeof a);
    a.text = ctx->d_cbtext; a.item_off = ctx->d_cboff; a.n_items = (int64_t)n_items128;
    a.n_rates = n_rates; a.n_trials = n_trials; a.seed = seed; a.P = ctx->d_cbP;
    u.empty = false;
    return KGMA_OK;
}

static int mutation_bad(kgma_ctx *ctx, const std::vector<int64_t> &off, unsigned long long bad)
{
    const int64_t si = (int64_t)(std::upper_bound(off.begin(), off.end(), (int64_t)bad) - off.begin()) - 1;
    return fail(ctx, KGMA_E_BADBASE, "sequence %lld position %lld: residue is not one of A/C/G/T (mutation_dict has no other key, DistanceTesting.jl:38-42)",
                (long long)si, (long long)((int64_t)bad - off[(size_t)si] + 1));
}

int kgma_mutation_dists(kgma_ctx *ctx, int32_t kfv, const uint8_t *seqs, const int64_t *offsets, int64_t n_seqs, const double *rates,
                        int32_t n_rates, int32_t n_trials, uint64_t seed, int64_t *D_out, double *dist_out)
{
    if (!ctx) return KGMA_E_ARG;
    const KfvInfo *fp_ = nullptr;
    int rc = calib_kfv(ctx, "kgma_mutation_dists", kfv, &fp_);
    if (rc) return rc;
    const KfvInfo &f = *fp_;
    CalibArgs a;
    MutationUpload u;
    if ((rc = mutation_source(ctx, "kgma_mutation_dists", "k-mers", f, seqs, offsets, n_seqs, rates, n_rates, n_trials, seed, a, u)) || u.empty)
        return rc;
    unsigned long long bad = NO_BAD;
    if ((rc = calib_launch(ctx, "kgma_mutation_dists", 1, a, f, kfv, D_out, dist_out, &bad))) return rc;
    if (bad != NO_BAD) return mutation_bad(ctx, u.off, bad);
    return KGMA_OK;
}

// ---- the same two calls for the strobemer engine's reference (kgma_set_strobe_ref; kernel: strobe_calib_kernel) ----
static int strobe_calib_ref(kgma_ctx *ctx, const char *what)
{
    if (!ctx->strobe || ctx->m < 1)
        return fail(ctx, KGMA_E_STATE, "%s: the context holds no strobemer reference (call kgma_set_strobe_ref first)", what);
    return KGMA_OK;
}

// What both share behind their checks, as calib_launch: the reference's table and parameters, one launch between the context's
// events, the download.  a.c: text, item_off, n_items (> 0) and the source's own fields are set; a.rec_off for the window source.
static int strobe_calib_launch(kgma_ctx *ctx, int source, StrobeCalibArgs &a, int64_t *D_out, double *dist_out, unsigned long long *bad)
{
    const KfvInfo &f = ctx->kfv[0];
    const int64_t n = a.c.n_items;
    int rc;
    if ((rc = dev_reserve(ctx, ctx->d_cbD, ctx->cbD_cap, n))) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_cbdist, ctx->cbdist_cap, n))) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_cbbad, ctx->cbbad_cap, 1))) return rc;
    a.s = ctx->st_s; a.w_min = ctx->st_wmin; a.w_max = ctx->st_wmax;
    strobe_zero_mask(ctx->st_q, a.zero);
    a.c.k = ctx->k;
    a.c.S = ctx->d_Stab;
    a.c.N = f.N; a.c.sumS2 = f.sumS2;
    a.c.scale = 2.0 * (double)ctx->k * (double)f.N * (double)f.N;      // = kgma_kfv_scale: what the strobemer scan divides by
    a.c.D_out = ctx->d_cbD; a.c.dist_out = ctx->d_cbdist; a.c.first_bad = ctx->d_cbbad;
    *bad = NO_BAD;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_cbbad, bad, 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    HIP_TRY(ctx, launch_strobe_calib(a, source, calib_grid(1, n, ctx->n_cus), ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(bad, ctx->d_cbbad, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (dist_out) HIP_TRY(ctx, hipMemcpyAsync(dist_out, ctx->d_cbdist, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (D_out) HIP_TRY(ctx, hipMemcpyAsync(D_out, ctx->d_cbD, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    ctx->stats.scan_ms = ms;
    ctx->stats.n_launches = 1;
    snprintf(ctx->kernel_name, sizeof ctx->kernel_name, "strobe_calib_kernel<%s,%d>", source == 0 ? "window" : "mutation", ctx->st_s);
    return KGMA_OK;
}

int kgma_strobe_window_dists(kgma_ctx *ctx, const kgma_genome *g, int64_t n, const int32_t *contig, const int64_t *start, int64_t *D_out,
                             double *dist_out)
{
    if (!ctx || !g) return KGMA_E_ARG;
    int rc = strobe_calib_ref(ctx, "kgma_strobe_window_dists");
    if (rc) return rc;
    const int64_t W = ctx->kfv[0].W;
    if (n < 0 || (n > 0 && (!contig || !start))) return fail(ctx, KGMA_E_ARG, "kgma_strobe_window_dists: null argument or n < 0");
    // [window offsets | offsets of the windows' records]
    std::vector<int64_t> off((size_t)(2 * n));
    for (int64_t i = 0; i < n; i++) {
        const int64_t c = contig[i];
        if (c < 0 || c >= g->n_contigs) return fail(ctx, KGMA_E_ARG, "kgma_strobe_window_dists: window %lld: no record %lld", (long long)i, (long long)c);
        const ContigDesc &d = g->cd[(size_t)c];
        if (d.len < W)
            return fail(ctx, KGMA_E_ARG, "kgma_strobe_window_dists: window %lld: record %lld of %lld residues is shorter than the window (%lld): the scan skips it",
                        (long long)i, (long long)c, (long long)d.len, (long long)W);
        if (start[i] < 1 || start[i] > std::max<int64_t>(1, d.len - W))
            return fail(ctx, KGMA_E_ARG, "kgma_strobe_window_dists: window %lld: start %lld is not one of 1 .. %lld, the window starts of record %lld of %lld residues",
                        (long long)i, (long long)start[i], (long long)std::max<int64_t>(1, d.len - W), (long long)c, (long long)d.len);
        off[(size_t)i] = d.ascii_off + (start[i] - 1);
        off[(size_t)(n + i)] = d.ascii_off;
    }
    ctx->stats.scan_ms = 0;
    ctx->stats.n_launches = 0;
    if (n == 0) return KGMA_OK;
    (void)hipSetDevice(ctx->device);
    if ((rc = dev_reserve(ctx, ctx->d_cboff, ctx->cboff_cap, 2 * n))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_cboff, off.data(), off.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    StrobeCalibArgs a;
    memset(&a, 0, sizeof a);
    a.c.text = g->d_ascii; a.c.item_off = ctx->d_cboff; a.rec_off = ctx->d_cboff + n; a.c.n_items = n; a.c.W = W;
    unsigned long long bad = NO_BAD;
    if ((rc = strobe_calib_launch(ctx, 0, a, D_out, dist_out, &bad))) return rc;
    if (bad != NO_BAD) return window_bad(ctx, g, bad);
    return KGMA_OK;
}

int kgma_strobe_mutation_dists(kgma_ctx *ctx, const uint8_t *seqs, const int64_t *offsets, int64_t n_seqs, const double *rates,
                               int32_t n_rates, int32_t n_trials, uint64_t seed, int64_t *D_out, double *dist_out)
{
    if (!ctx) return KGMA_E_ARG;
    int rc = strobe_calib_ref(ctx, "kgma_strobe_mutation_dists");
    if (rc) return rc;
    StrobeCalibArgs a;
    memset(&a, 0, sizeof a);
    MutationUpload u;
    if ((rc = mutation_source(ctx, "kgma_strobe_mutation_dists", "strobemers", ctx->kfv[0], seqs, offsets, n_seqs, rates, n_rates, n_trials, seed,
                              a.c, u)) || u.empty)
        return rc;
    unsigned long long bad = NO_BAD;
    if ((rc = strobe_calib_launch(ctx, 1, a, D_out, dist_out, &bad))) return rc;
    if (bad != NO_BAD) return mutation_bad(ctx, u.off, bad);
    return KGMA_OK;
}

// ------------------------------------------------------------------------------------------
// results
// ------------------------------------------------------------------------------------------
int kgma_get_hits(kgma_ctx *ctx, kgma_hit *out, int64_t cap, int64_t *n)
{
    return ctx ? copy_out(ctx, "kgma_get_hits", ctx->hits, out, cap, n) : KGMA_E_ARG;
}

int kgma_get_dips(kgma_ctx *ctx, kgma_dip *out, int64_t cap, int64_t *n)
{
    return ctx ? copy_out(ctx, "kgma_get_dips", ctx->dips, out, cap, n) : KGMA_E_ARG;
}

int kgma_get_first_window(kgma_ctx *ctx, int32_t kfv, int64_t *out, int64_t cap, int64_t *n)
{
    if (!ctx || !n) return KGMA_E_ARG;
    if (ctx->last_mode < 0) return fail(ctx, KGMA_E_STATE, "no scan has been run");
    const int m_scanned = ctx->last_mode == KGMA_MODE_SINGLE ? 1 : ctx->m;      // the single engine evaluates KFV 1 only
    if (kfv < 1 || kfv > m_scanned) return fail(ctx, KGMA_E_ARG, "kfv %d out of range (the last scan evaluated %d KFV(s))", kfv, m_scanned);
    const int64_t nc = (int64_t)ctx->contig_len.size();
    *n = nc;
    if (!out) return KGMA_OK;
    if (cap < nc) return fail(ctx, KGMA_E_ARG, "kgma_get_first_window: capacity too small");
    for (int64_t c = 0; c < nc; c++) out[c] = ctx->firstD[(size_t)(kfv - 1) * (size_t)nc + (size_t)c];
    return KGMA_OK;
}

int kgma_get_dists(kgma_ctx *ctx, int32_t kfv, double *out, int64_t cap, int64_t *n)
{
    if (!ctx || !n) return KGMA_E_ARG;
    if (ctx->last_mode < 0 || !ctx->have_dists) return fail(ctx, KGMA_E_STATE, "the last scan did not keep distances (KGMA_F_RETURN_DISTS)");
    const int m_used = ctx->last_mode == KGMA_MODE_SINGLE ? 1 : ctx->m;
    if (kfv < 1 || kfv > m_used) return fail(ctx, KGMA_E_ARG, "kfv %d out of range", kfv);
    *n = ctx->n_dists_per_kfv;
    if (!out) return KGMA_OK;
    if (cap < *n) return fail(ctx, KGMA_E_ARG, "kgma_get_dists: capacity too small");
    (void)hipSetDevice(ctx->device);
    if (*n) HIP_TRY(ctx, hipMemcpy(out, ctx->d_dist[(size_t)(kfv - 1)], (size_t)*n * sizeof(double), hipMemcpyDeviceToHost));
    return KGMA_OK;
}

int kgma_get_filter_stats(kgma_ctx *ctx, kgma_filter_stats *out)
{
    if (!ctx || !out) return KGMA_E_ARG;
    *out = ctx->fstats;
    return KGMA_OK;
}

int kgma_get_pack_test_stats(kgma_ctx *ctx, kgma_pack_test_stats *out)
{
    if (!ctx || !out) return KGMA_E_ARG;
    *out = ctx->ptest;
    return KGMA_OK;
}

int kgma_get_block_sums(kgma_ctx *ctx, const kgma_genome *g, int64_t contig, int64_t first_block, int64_t n, uint32_t *out)
{
    if (!ctx || !g) return KGMA_E_ARG;
    if (g->bsum_state == KGMA_BSUM_NONE || g->bsum_k == 0) return fail(ctx, KGMA_E_STATE, "kgma_get_block_sums: no step has put block sums into this genome's pack");
    if (contig < 0 || contig >= g->n_contigs || first_block < 0 || n < 0 || (!out && n > 0)) return fail(ctx, KGMA_E_ARG, "kgma_get_block_sums: bad argument");
    const ContigDesc &d = g->cd[(size_t)contig];
    if (first_block + n > 2 * ((d.len + 31) / 32)) return fail(ctx, KGMA_E_ARG, "kgma_get_block_sums: blocks outside the record");
    if (n == 0) return KGMA_OK;
    (void)hipSetDevice(ctx->device);
    {
        const int brc = ensure_bsum(ctx, const_cast<kgma_genome *>(g), true);   // (a step whose pack tested left them to be written)
        if (brc) return brc;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint16_t> tmp((size_t)n);
    HIP_TRY(ctx, hipMemcpy(tmp.data(), g->d_bsum + 2 * d.word_off + first_block, (size_t)n * sizeof(uint16_t), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; i++) out[i] = tmp[(size_t)i];
    return KGMA_OK;
}

int kgma_get_filter_candidates(kgma_ctx *ctx, int32_t *contig, int64_t *granule, int64_t cap, int64_t *n)
{
    if (!ctx || !n) return KGMA_E_ARG;
    int64_t need = 0;
    for (const FilterEntry &e : ctx->fentries) need += __builtin_popcountll(e.mask);
    *n = need;
    if (!contig || !granule) return KGMA_OK;
    if (cap < need) return KGMA_E_ARG;
    int64_t i = 0;
    for (const FilterEntry &e : ctx->fentries)
        for (uint64_t m = e.mask; m; m &= m - 1) { contig[i] = e.contig; granule[i] = (int64_t)e.gbase + __builtin_ctzll(m); i++; }
    return KGMA_OK;
}

int kgma_get_stats(kgma_ctx *ctx, kgma_stats *out)
{
    if (!ctx || !out) return KGMA_E_ARG;
    *out = ctx->stats;
    return KGMA_OK;
}

}  // extern "C"
