// lzani_hip.hip -- the C-ABI of include/lzani.h: the context, the run driver (check_rows ... run_rows_impl) and the entry
// points.  gfx950 (MI355X) only.
//
// The kernels (all integer / bit work; no MFMA by design) live in the headers included below:
//   lzani_kernels_index.h   k_pack, k_kmers, k_idx_*   genomes -> packed texts, k-mer words, anchor indexes
//   lzani_kernels_cand.h    k_pm_build, k_pm_cand   dense rows: presence matrix of a group of references -> per-pair candidate bitmaps
//   lzani_kernels_pairs.h   DevWave, k_pairs   the pair kernel
//   lzani_kernels_prefilter.h   k_pf_*   the k-mer prefilter: shared k-mer counts of all genome pairs
//   lzani_kernels_outfilter.h   k_of_kept   the output filter: the pairs of a finished result buffer of which a TSV line passes
//   lzani_kernels_cluster.h     k_cl_*   the cluster stage: single linkage, greedy clustering, greedy set cover and complete linkage of the kept pairs
//   lzani_kernels_regions.h     k_rg_*   the alignment-region stage: the regions of the entries that pass the alignment's rule, in file order
//   lzani_block.h           block_sum, block_rank, block_scan_step   what a block's threads work out together (index, prefilter)
// The algorithm itself (PairMachine and its building blocks, shared with the host model of the tests) is
// lzani_core.h; sizes and the parameter envelope are lzani_layout.h.  The pure decisions are free of HIP: those of a run
// (batches, queues, the split rule, the bytes of a slab slot) in lzani_run_plan.h, which pair kernel a launch takes (the
// table of the instantiations, choose_pair_kernel) in lzani_pair_dispatch.h, those of a genome set (the set-level
// switches, the form of the index, footprints, the block plan, residency, the slot count of the slabs) in lzani_set_plan.h,
// those of an out-of-core run (the order of its tiles, their local tables, the tables of an upload) in lzani_tile_plan.h.
// Device memory and events have one owner each, lzani_devmem.h.  Seven layers of the host side are files of their own,
// included at fixed places below:
//   lzani_index.h       the index stage: genome upload, slabs, k-mer words, join lists, the index build, its test hooks
//   lzani_dense.h       the dense-row stage of a run: candidate bitmaps from the presence matrix, the split of few, long pairs
//   lzani_ooc.h         genome sets larger than the device: block plan, block uploads, the tiled run
//   lzani_prefilter.h   the k-mer prefilter's host stage: slice and pass plans, the pass / tile driver, its entry points
//   lzani_kept.h        the output filter's host stage: a run whose results stay on the device, only the kept pairs come back
//   lzani_regions.h     the alignment-region stage's host side: a run with the region sink on the device, the stage, the fetch in pieces
//   lzani_cluster.h     the cluster stage's host side: the edges of the kept results, the run, its entry points
//   lzani_multi.h       the multi-GPU layer
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <optional>
#include <string>
#include <type_traits>
#include <variant>
#include <vector>

#include "../../include/lzani.h"

__device__ int g_guard_trip = 0;   // see LZ_GUARD_TRIP in lzani_core.h
#ifdef LZANI_STAMPS
__device__ unsigned long long g_stamp_acc[8];
#endif
#ifdef LZANI_CHAIN_STATS
__device__ unsigned long long g_chain_stats[24];
#endif
#ifdef LZANI_PHASE_TIME
__device__ unsigned long long g_phase_time[4];
#endif
#ifdef LZANI_PATH_STATS
__device__ unsigned long long g_path_stats[36];
#endif

int lzani_sort_segments(const unsigned long long* in, unsigned long long* out, size_t seg_len, size_t n_seg, int begin_bit, int end_bit,
                        void* tmp, size_t* tmp_bytes, hipStream_t stream);
int lzani_sort_keys(const unsigned long long* in, unsigned long long* out, size_t n, int begin_bit, int end_bit,
                    void* tmp, size_t* tmp_bytes, hipStream_t stream);      // lzani_sort.hip (the engine's own radix sort)

#include "lzani_core.h"
#include "lzani_layout.h"
#include "lzani_tables.h"
#include "lzani_kernels_index.h"
#include "lzani_kernels_cand.h"
#include "lzani_kernels_pairs.h"
#include "lzani_kernels_split.h"
#include "lzani_kernels_prefilter.h"
#include "lzani_kernels_outfilter.h"
#include "lzani_kernels_cluster.h"
#include "lzani_kernels_regions.h"
#include "lzani_rtc.h"
#include "lzani_devmem.h"
#include "lzani_run_plan.h"
#include "lzani_pair_dispatch.h"
#include "lzani_set_plan.h"
#include "lzani_tile_plan.h"

// ============================================================================================
// Host side of the C-ABI
// ============================================================================================
using namespace lzani;

// What the last run did (lzani_get_timing, lzani_get_layout, lzani_debug_kernel_launches): reset at its start; an
// out-of-core run sums its tiles' records.
struct RunRecord {
    lzani_timing tm{};
    u32 batches = 0;
    // launches of k_pairs_blk; pair-kernel launches fed by candidate bitmaps, with tickets longest pair first, by a run-time
    // compiled kernel; presence matrices made by k_pm_from_index; batches whose pairs several waves each scanned, their segments
    int blk_launches = 0, pm_launches = 0, lpt_launches = 0, rtc_launches = 0, pmfi_launches = 0, split_launches = 0;
    int pmc_launches = 0;         // k_pm_cand launches (a group of more than 32,768 queries takes several)
    u64 split_items = 0;
    // the split's repair loop (lzani_debug_split_stats): pairs cut, the most rounds of a batch, items listed to resume, pairs
    // given up (all cuts disabled, scanned whole by segment 0), void stitches by cause (lzani_core.h: split_stitch)
    u64 split_cut = 0, split_resumed = 0, split_given_up = 0, split_void[6] = {};
    u32 split_rounds = 0;
    u64 klaunch[PK_COUNT] = {};   // the launch record: launches per pair-kernel instantiation (PAIR_KERNELS)

    RunRecord& operator+=(const RunRecord& o)
    {
        tm.index_ms += o.tm.index_ms; tm.pairs_ms += o.tm.pairs_ms; tm.cand_ms += o.tm.cand_ms; tm.kmers_ms += o.tm.kmers_ms;
        tm.pair_launches += o.tm.pair_launches; tm.index_launches += o.tm.index_launches; tm.cand_launches += o.tm.cand_launches;
        tm.pairs += o.tm.pairs;
        batches += o.batches;
        blk_launches += o.blk_launches; pm_launches += o.pm_launches; lpt_launches += o.lpt_launches; pmfi_launches += o.pmfi_launches;
        split_launches += o.split_launches; split_items += o.split_items; rtc_launches += o.rtc_launches; pmc_launches += o.pmc_launches;
        split_cut += o.split_cut; split_resumed += o.split_resumed; split_given_up += o.split_given_up;
        split_rounds = std::max(split_rounds, o.split_rounds);
        for (int x = 0; x < 6; ++x) split_void[x] += o.split_void[x];
        for (int x = 0; x < PK_COUNT; ++x) klaunch[x] += o.klaunch[x];
        return *this;
    }
};

// ---- the context, grouped by lifetime; every group owns its device memory (lzani_devmem.h), so that dropping a group
// ---- is assigning a fresh one

// The device tables of a genome set (kernels see them as a GenomeTab); out-of-core: of the resident region.
struct GenomeTables {
    DevMem<u64> t2, nm, nmoff;
    DevMem<int> L, hasN;
    DevMem<u32> kmL, kmS;         // k-mer arrays (fast path: mal, msl <= 15), 64 entries per nm word
};

// Join form of candidate detection (long genomes): per-genome k-mer lists sorted by bucket.  A group of its own inside the
// genome set: the lists of an out-of-core run belong to one tile's local genome table and are released between tiles.
struct JoinLists {
    bool ready = false;
    DevMem<unsigned long long> keys;      // sorted
    DevMem<u64> koff;                     // per genome: offset of its forward positions (n + 1)
    DevMem<u64> soff;                     // per genome: offset of its sorted valid keys (n + 1)
    DevMem<u32> cnt;
    std::vector<u64> h_koff;
};

// lzani_set_genomes -> the next one.
struct GenomeSet {
    u32 n = 0;
    std::vector<int> L;
    std::vector<u64> nmoff;
    int Tmax = 0;
    IndexGeom geo{};
    GenomeTables tab;
    u64 total_nm = 0;
    bool kmers_ready = false;
    bool all_nfree = false;       // no genome holds an N: the NFREE kernel instantiation applies
    u64 dir_stride = 0, ent_stride = 0;
    SetLayout lay;                // the form of the anchor index, chosen per set (set_layout_of)
    int blk_fold = -1;            // k_pairs_blk: LDS filter = global filter folded 2^blk_fold times (-1: not decided yet, -2: does not fit)
    JoinLists jl;
    DevMem<unsigned char> d_jtmp; // radix-sort scratch (join lists, the sort-based index build, ticket order)

    // Out-of-core genome sets (lzani_ooc.h): the set stays on the host and the runs go tile by tile over
    // (reference block, query block).  n / L describe the whole set at all times -- a tile's run is given its local
    // table as a RunGenomes -- and the device tables above the resident region (two halves, A and B, of half_words
    // packed words each).
    u64 mem_limit = 0;            // the limit applied to this set (0: automatic mode kept it in-core)
    bool ooc = false;
    std::vector<uint8_t> h_codes;                 // host copy of the set's codes, genome after genome
    std::vector<u64> h_codeoff;
    std::vector<int> h_hasN;                      // per genome: a code >= 4
    std::vector<u32> blk_first;                   // block b = genomes [blk_first[b], blk_first[b + 1])
    std::vector<u64> blk_bytes;                   // genome-table footprint of every block (ooc_genome_bytes)
    u64 half_words = 0;                           // packed words of one half (the largest block's)
    u32 half_genomes = 0;                         // genomes of the largest block
    int half_block[2] = {-1, -1};                 // the block each half holds (-1: none)
    int half_a = 0;                               // which half is A (the reference block's)
    DevMem<uint8_t> d_stage;                      // 1 B per base of the largest block
    DevMem<u64> d_up_tab;                         // an upload's code offsets and word offsets (2 x half_genomes)
    DevMem<int> d_up_L;                           // ... lengths, and N flags written by k_pack (2 x half_genomes)
};

// The genome table of one run, count and lengths: the set's own (run_genomes_of) or, out-of-core, a tile's local one
// (lzani_tile_plan.h).  run_rows_impl and everything below it go by this, never by gs.n / gs.L.
struct RunGenomes { u32 n; const int* L; };

// The index slabs: grown by ensure_slabs, dropped with the genome set.
struct IndexSlabs {
    u32 slots = 0;
    int index_build = -1;         // the form the last build_indexes took: LZANI_INDEX_BUILD_LDS / _ATOMICS / _SORT (test hooks)
    DevMem<u32> d_dirz, d_ent;
    DevMem<u32> d_bk, d_tw;       // bucket tables and their tag words
    DevMem<u32> d_fl;             // presence filters (probe form with tag words), or one all-ones word
    DevMem<u32> d_status;         // per slot: the LDS index build left this slot to the global-atomics kernels
    // sort-based index build: keys of the batch's references, unsorted / sorted, per-slot counts and starts
    DevMem<unsigned long long> d_ikeys_in, d_ikeys;
    DevMem<u32> d_icnt;
    DevMem<u64> d_ibase;
};

// Candidate scratch of dense rows (lzani_dense.h): grown by plan_bitmaps / choose_split_lpt / run_split, dropped with the
// genome set or when the matrix, the pair table or the bitmaps cannot be had.
struct CandScratch {
    DevMem<u32> d_pm;             // the presence matrix of one group: 2^pm_bits rows of PM_GROUP bits
    DevMem<u32> d_pm_cbits;       // candidate bitmaps of a batch's pairs
    DevMem<u32> d_pm_pidx;        // rows with query lists: pair of (query, slot of the group), query flags + list + count behind it
    DevMem<u32> d_lpt_cnt;        // batches of few, long pairs: candidates per pair ...
    DevMem<unsigned long long> d_lpt_keys;        // ... then the ticket keys unsorted / sorted (two per pair)
    // few, long pairs by several waves each (run_split): per segment its checkpoint and its result, the work lists of this
    // round and the next; the counters; per pair: finished, cut into segments
    DevMem<SplitStart> d_sp_cuts;
    DevMem<SplitOut> d_sp_outs;
    DevMem<u32> d_sp_work, d_sp_next, d_sp_cnt;
    DevMem<unsigned char> d_sp_done, d_sp_heavy;
};

// The k-mer prefilter (lzani_prefilter, lzani_kernels_prefilter.h): lzani_set_genomes -> the next one.  The results stay
// until the next prefilter; the workspace is released when the stage ends.
struct PrefilterTile {
    u32 r0 = 0, r1 = 0;           // rows of the count matrix the tile held
    DevMem<u32> ids, shared;      // the kept entries of those rows, row after row
};
struct PrefilterWork {
    DevMem<u64> cbase;            // per genome: number of its first chunk of PF_CHUNK forward positions (n + 1)
    DevMem<u32> blkcnt;           // per chunk: windows kept
    DevMem<u64> blkoff;           // ... their exclusive prefix: where a chunk's keys go, in both key passes
    DevMem<u32> ucnt;             // per PF_CHUNK elements of a sorted array: elements that differ from their predecessor
    DevMem<u64> uoff;
    DevMem<unsigned long long> ka, kb;            // keys, sorted keys / dictionary, rank keys / postings, in turn
    DevMem<unsigned char> tmp;    // radix-sort scratch
    DevMem<u32> runoff;           // per rank: its first posting (distinct k-mers + 1)
    DevMem<u32> runsplit;         // cross form, per rank: its first posting of a query (distinct k-mers + 1)
    DevMem<u32> mat;              // one row tile of the count matrix, rows x n (cross form: rows x n_query)
    DevMem<u32> rowcnt;
    DevMem<u64> rowoff;
    // sparse counting: the pair table in place of mat
    DevMem<unsigned long long> sp_keys;           // per slot: a << 32 | b, all ones where it is free
    DevMem<u32> sp_cnt;           // ... and the pair's count
    DevMem<u32> sp_ctl;           // slots in use, the overflow word
    DevMem<u32> sp_bcnt;          // per PF_CHUNK slots: the kept ones
    DevMem<u64> sp_boff;
    DevMem<unsigned long long> sp_kin, sp_kout;   // a tile's kept keys in table order / sorted
    DevMem<unsigned char> sp_tmp; // radix-sort scratch of the kept keys
};
struct Prefilter {
    bool done = false;
    u32 n = 0;                            // genomes of the prefilter that made the result (lzani_prefilter_codes: not gs.n)
    bool streamed = false;                // made by lzani_prefilter_codes: sinfo holds
    bool cross = false;                   // made by a cross call: cinfo holds
    lzani_prefilter_cross_info cinfo{};
    lzani_prefilter_info info{};
    lzani_prefilter_stream_info sinfo{};
    lzani_prefilter_pass_info pinfo{};
    lzani_prefilter_sparse_info spinfo{}; // all zero unless the pair table counted
    bool limited = false;                 // lzani_prefilter_limit cut the result: linfo holds, and one tile covers all rows
    lzani_prefilter_limit_info linfo{};
    std::vector<u32> bin_lo;              // the pass plan: pass p holds the bins bin_lo[p] .. bin_lo[p + 1]
    DevMem<u32> kmers_of;                 // |K(g)|
    std::vector<u64> row_off;             // CSR of the kept pairs (n + 1)
    std::vector<PrefilterTile> tiles;     // in row order
    PrefilterWork work;
};

// The output filter's result (lzani_kept.h): a kept call -> the next one, or lzani_set_genomes.
struct Kept {
    bool done = false;
    u32 n = 0;                            // the genomes of the call
    lzani_kept_info info{};
    DevMem<u32> rec;                      // 9 words a kept pair (lzani_kept_pair)
};

// The ordered regions of the alignment output (lzani_regions.h): a regions call -> the next one, or lzani_set_genomes.  (The
// name Regions is the pair machine's, lzani_core.h.)
struct AlignedRegions {
    bool done = false;
    lzani_regions_info info{};
    DevMem<lzani_region> rec;             // info.kept records, in file order
};

// The cluster stage's state (lzani_cluster.h): lzani_cluster_begin -> the next one, or lzani_set_genomes.
struct Cluster {
    bool begun = false, ran = false;      // ran: rep_of and cluster_of are those of the edges as they are
    lzani_cluster_info info{};
    // the last run's own info where its algorithm (info.algo) has one: set cover, complete linkage or Leiden
    std::variant<std::monostate, lzani_cluster_cover_info, lzani_cluster_link_info, lzani_cluster_leiden_info> specific;
    DevMem<u32> len;                     // the reported lengths (n)
    DevMem<lzani_cluster_edge> edges;     // info.edges of them, a < b; grown geometrically
    DevMem<u32> rep_of, cluster_of;       // of the last run (n each)
    bool from_level = false;              // made by lzani_cluster_level: `level` holds
    lzani_cluster_level_info level{};
};

// The record store of the cluster levels (lzani_cluster.h): lzani_cluster_store_begin -> the next one, or lzani_set_genomes.
struct ClusterStore {
    bool begun = false;
    lzani_cluster_store_info info{};
    DevMem<u32> len;                      // the reported lengths (n)
    DevMem<u32> rec;                      // 9 words a record (lzani_kept_pair), info.records of them; grown geometrically
};

// Residency counters of the last run (lzani_get_residency).
struct Residency { u32 tiles = 0; u64 uploads = 0, peak = 0; double upload_ms = 0; };

struct lzani_ctx {
    // create -> destroy
    Params P;
    int dev = 0;
    hipStream_t stream = nullptr;
    std::vector<DevEvent> events;      // EV per batch of a run, made as the runs need them and used again
    int n_cus = 256;
    std::string err;
    StreamSpan km_span;
    bool km_timed = false;        // the last run made the k-mer words (km_span holds their stamps)
    double join_ms_pending = 0;   // ... and / or the join lists: their time, added to that run's kmers_ms
    DevMem<unsigned long long> d_cursor;
    DevMem<u32> d_blkctr;         // k_pairs_blk: one pair counter per block
    std::vector<std::pair<const void*, size_t>> lds_limits;     // the dynamic-LDS limit this context gave a kernel (raise_lds)
    // pair kernels compiled at run time for this context's parameters (lzani_rtc.h); none for the two ahead-of-time tuples
    lzani_rtc::State rtc;
    std::string arch;             // the device's gfx target, as hipRTC wants it
    u64 pairs_seen = 0;           // directed pairs this context has been asked for so far (a run-time compile must pay)
    void* comm = nullptr;         // ncclComm_t of lzani_comm_init (one process per GPU), lzani_multi.h
    u32 n_ranks = 1, rank = 0;
    u64 mem_req = 0;              // lzani_set_genome_memory: applies at the next lzani_set_genomes; 0 = automatic
    double leiden_resolution = CL_LEIDEN_RESOLUTION;      // lzani_set_cluster_leiden: the parameters of the later Leiden runs
    int leiden_iterations = CL_LEIDEN_ITERATIONS;
    int pf_counting = LZANI_PF_COUNTING_AUTO;     // lzani_set_prefilter_counting: the accumulator of the later prefilter calls
    u64 region_cap = 0;           // lzani_set_region_capacity: the first capacity of the later lzani_run_rows_aligned calls; 0 = automatic

    GenomeSet gs;
    IndexSlabs sl;
    CandScratch cs;
    Prefilter pf;
    Kept kept;
    AlignedRegions rg;
    Cluster cl;
    ClusterStore cls;
    // the last run
    RunRecord run;
    Residency res;
};

namespace {

bool trace_on()
{
    static int on = -1;
    if (on < 0) { const char* e = getenv("LZANI_TRACE"); on = (e && *e && *e != '0') ? 1 : 0; }
    return on == 1;
}
#define TRACE(...) do { if (trace_on()) { fprintf(stderr, "[lzani] " __VA_ARGS__); fputc('\n', stderr); fflush(stderr); } } while (0)

int fail(lzani_ctx* c, int code, const std::string& msg)
{
    if (c) c->err = msg;
    return code;
}

#define HIPCHK(c, call)                                                                               \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail(c, e_ == hipErrorOutOfMemory ? LZANI_ERR_NOMEM : LZANI_ERR_DEVICE,            \
                        std::string(#call) + ": " + hipGetErrorString(e_));                           \
    } while (0)

// The one place that raises a kernel's dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize): lds_limit is what
// this context last gave the kernel (0: the default), raise_lds calls the runtime only where that is below `bytes`.
size_t& lds_limit(lzani_ctx* c, const void* fn)
{
    for (auto& e : c->lds_limits) if (e.first == fn) return e.second;
    c->lds_limits.emplace_back(fn, 0);
    return c->lds_limits.back().second;
}
template <class K>
int raise_lds(lzani_ctx* c, K* kernel, size_t bytes)
{
    const void* fn = reinterpret_cast<const void*>(kernel);
    size_t& have = lds_limit(c, fn);
    if (bytes <= have) return LZANI_OK;
    HIPCHK(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    have = bytes;
    return LZANI_OK;
}

// The engine's radix sort (lzani_sort.hip) of n_seg segments of seg_len keys by the bits [begin_bit, end_bit), on the
// context's stream.  sort_scratch_bytes: its size query.  sort_keys: the query, `scratch` grown to what it asks for -- sync:
// behind the stream's queued work, which may still be using it -- and the sort.  `what` names the caller's sort in the message.
int sort_scratch_bytes(lzani_ctx* c, size_t seg_len, size_t n_seg, int begin_bit, int end_bit, const char* what, size_t& need)
{
    if (lzani_sort_segments(nullptr, nullptr, seg_len, n_seg, begin_bit, end_bit, nullptr, &need, c->stream) != 0)
        return fail(c, LZANI_ERR_DEVICE, std::string(what) + " (size query) failed");
    return LZANI_OK;
}
int sort_keys(lzani_ctx* c, DevMem<unsigned char>& scratch, const unsigned long long* in, unsigned long long* out, size_t seg_len, size_t n_seg,
              int begin_bit, int end_bit, const char* what, bool sync)
{
    size_t need = 0;
    if (int rc = sort_scratch_bytes(c, seg_len, n_seg, begin_bit, end_bit, what, need)) return rc;
    if (need > scratch.capacity()) {
        if (sync) HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, scratch.alloc(need));
    }
    size_t have = scratch.capacity();
    const int e = lzani_sort_segments(in, out, seg_len, n_seg, begin_bit, end_bit, scratch, &have, c->stream);
    if (e != 0) return fail(c, LZANI_ERR_DEVICE, std::string(what) + " failed: " + hipGetErrorString((hipError_t)e));
    return LZANI_OK;
}

// The run path's switches (experiments and tests), read where a Knobs is made: at the start of every run (tests change them
// between the runs of one context).  Empty: not set, the run's own rule decides.
struct Knobs {
    bool pm = !env_is("LZANI_PM", '0');                                     // 0: no candidate bitmaps
    std::optional<int> pm_min_rows = env_int("LZANI_PM_MIN_ROWS");
    std::optional<u64> pm_max_bytes = env_u64("LZANI_PM_MAX_BYTES");         // the candidate bitmaps of a batch
    std::optional<u64> pm_min_share = env_u64("LZANI_PM_MIN_SHARE");         // pairs per query and group of rows (query lists)
    bool pm_fail_cbits = env_is("LZANI_PM_FAIL_CBITS", '1');                // tests: the bitmaps cannot be had
    std::optional<bool> pm_from_index = env_flag("LZANI_PM_FROM_INDEX");
    u32 blocks_per_cu = (u32)std::max(1, std::min(8, env_int("LZANI_BLOCKS_PER_CU").value_or(8)));   // occupancy experiments
    std::optional<bool> block_kernel = env_flag("LZANI_BLOCK_KERNEL");
    u64 rtc_min_pairs = env_u64("LZANI_RTC_MIN_PAIRS").value_or(2000000ull);
    std::optional<bool> lpt = env_flag("LZANI_LPT"), split = env_flag("LZANI_SPLIT");
    u64 split_s = (u64)std::max(2, env_int("LZANI_SPLIT_S").value_or(64));   // segments per pair
    int split_seglen = env_int("LZANI_SPLIT_SEGLEN").value_or(0);           // > 0: the segment length instead
    bool split_all = !env_is("LZANI_SPLIT_ALL", '0');                       // 0: cut only the pairs with many candidates
    u32 split_thr = (u32)env_u64("LZANI_SPLIT_THR").value_or(0);             // ... or with this many
    std::optional<int> split_give_up = env_int("LZANI_SPLIT_GIVE_UP");       // rounds before a pair's cuts are given up (empty: 6 + S / 4)
    bool lds_index = !env_is("LZANI_NO_LDS_INDEX", '1');
    int lds_index_max_dirbits = env_int("LZANI_LDS_INDEX_MAX_DIRBITS").value_or(19);
};

}  // namespace

#include "lzani_index.h"

namespace {

struct RegionSink { lzani_region* d_regions; unsigned long long* d_count; unsigned long long capacity; };

// The tuples the pair kernels fold into their code ahead of time: 1 = the defaults, 2 = the long-genome parameters
// (--mal 15 --msl 9 --reg 60, BASELINE configs[3]; the hand-written null chain included, bitmap, join and split forms),
// 0 = any other (the generic kernel, or one compiled at run time).
int defp_select(const Params& q)
{
    if (q.mrd != 40 || q.mqd != 40 || q.aw != 15 || q.am != 7 || q.ar != 3) return 0;
    return (q.mal == 11 && q.msl == 7 && q.reg == 35) ? 1 : (q.mal == 15 && q.msl == 9 && q.reg == 60) ? 2 : 0;
}

// Launch record: launches per row of PAIR_KERNELS (lzani_pair_dispatch.h), counted per context for the last run
// (lzani_debug_kernel_launches).  The kernels' host addresses in row order, from the lists the table is made of (the rows
// of the run-time compiled kernel have none: its function belongs to a module, lzani_rtc.h).
#define LZANI_PK_PAIRS_FN(F, N, D, A, B, C) reinterpret_cast<const void*>(k_pairs<F, N, D, A, B, C>),
#define LZANI_PK_BLK_FN(N, D) reinterpret_cast<const void*>(k_pairs_blk<N, D>),
#define LZANI_PK_SPLIT_FN(N, D, M) reinterpret_cast<const void*>(k_split<N, D, M>),
#define LZANI_PK_RTC_FN(N, C) nullptr,
const void* const PAIR_KERNEL_FN[PK_COUNT] = {
    LZANI_PK_PAIRS_ROWS(LZANI_PK_PAIRS_FN) LZANI_PK_BLK_ROWS(LZANI_PK_BLK_FN) LZANI_PK_SPLIT_ROWS(LZANI_PK_SPLIT_FN)
    LZANI_PK_RTC_ROWS(LZANI_PK_RTC_FN)
};

// The one launch of a pair kernel, on the context's stream: the kernel of the row -- `rtc`: the module function of a
// run-time compiled row -- and, where the launch was taken, its count in the launch record.
hipError_t launch_row(lzani_ctx* c, int row, dim3 gd, dim3 bd, void** args, size_t lds = 0, hipFunction_t rtc = nullptr)
{
    const hipError_t e = PAIR_KERNELS[row].kind == PK_RTC ? hipModuleLaunchKernel(rtc, gd.x, 1, 1, bd.x, 1, 1, 0, c->stream, args, nullptr)
                                                          : hipLaunchKernel(PAIR_KERNEL_FN[row], gd, bd, args, lds, c->stream);
    if (e == hipSuccess) c->run.klaunch[row] += 1;
    return e;
}

// What a run's rows hold beyond their checks: the pairs and, for query lists, whether a row names a query twice and how
// many queries the groups of PM_GROUP consecutive rows involve (what the candidate form goes by).
struct RowFacts { u64 n_pairs = 0; bool lists_dup = false; u64 lists_involved = 0; };

// The checks of a run's rows (n_rows > 0) against the genome set; the query ids in one pass.
int check_rows(lzani_ctx* c, const RunGenomes& g, u32 n_rows, const u32* ref_ids, const u64* row_off, const u32* query_ids, RowFacts& f)
{
    for (u32 k = 0; k < n_rows; ++k) {
        if (ref_ids[k] >= g.n) return fail(c, LZANI_ERR_ARG, "lzani_run_rows: reference id out of range");
        if (row_off[k + 1] < row_off[k]) return fail(c, LZANI_ERR_ARG, "lzani_run_rows: row_off not monotone");
        if (!query_ids && row_off[k + 1] - row_off[k] != (u64)g.n - 1)
            return fail(c, LZANI_ERR_ARG, "lzani_run_rows: dense row must have n-1 queries");
    }
    if (row_off[0] != 0) return fail(c, LZANI_ERR_ARG, "lzani_run_rows: row_off[0] must be 0");
    f.n_pairs = row_off[n_rows];
    if (query_ids) {
        std::vector<u32> in_row(g.n, 0xFFFFFFFFu), in_group(g.n, 0xFFFFFFFFu);
        for (u32 k = 0; k < n_rows; ++k)
            for (u64 e = row_off[k]; e < row_off[k + 1]; ++e) {
                const u32 q = query_ids[e];
                if (q >= g.n) return fail(c, LZANI_ERR_ARG, "lzani_run_rows: query id out of range");
                f.lists_dup |= in_row[q] == k;
                in_row[q] = k;
                if (in_group[q] != k / PM_GROUP) { in_group[q] = k / PM_GROUP; ++f.lists_involved; }
            }
    }
    return LZANI_OK;
}

// The candidate form of a run, the geometry of its candidate bitmaps and its batches: decided once, before the first launch.
struct RunPlan {
    // candidates from the presence matrix of a group of references (dense rows), from the join of sorted k-mer lists (long
    // genomes), or neither: a probe per query position
    bool pm = false, use_join = false;
    int Lmax = 0;                 // the longest genome
    int pm_bits = 0;              // the presence matrix: 2^pm_bits rows of pm_group bits
    u32 pm_group = PM_GROUP, pm_tiles = 0;
    u64 cb_words = 0;             // 32-bit words of one pair's candidate bitmap
    std::vector<u32> bstart;      // batch b: rows [bstart[b], bstart[b + 1])
};

struct CandSink;                                  // lzani_dense.h

// What the batches of one run share: its rows and queues on the device, the launch geometry, the kernels of its tuple.
struct RunCtx {
    lzani_ctx* c;
    RunGenomes g;                                            // the genome table of the run
    const Knobs& k;
    const RunPlan& p;
    const RegionSink* rs; const u64* row_off; const u32* query_ids; int* d_out;     // the call's arguments
    const u32 *d_ref, *d_q, *d_qorder;                       // their device copies, the queues
    const u64 *d_off, *d_qcum;
    u32 max_blocks; int dsel;                                // the launch geometry, defp_select of the tuple
    unsigned long long* d_cbits;                             // join form: one candidate bitmap per resident wave
    u64 cbits_stride;
    lzani_rtc::Kernel* rtc_k;                                // the tuple's run-time compiled kernel, if any
    std::vector<u32> grp_seen = {}; u32 grp_stamp = 0;       // (query lists + candidate bitmaps) the group a query was last seen in
    CandSink* sink = nullptr;                                // test hook only (lzani_debug_run_candidates)
};

// Batch b: rows [k0, k0 + rows), pairs [e0, e1), its queues' bounds (QueuePlan::qb); the split / LPT choice of its pair launch.
struct Batch { u32 b, k0, rows; u64 e0, e1; const u32* qb; u32 split_S = 0; int split_seglen = 0; bool lpt = false; };

}  // namespace

#include "lzani_dense.h"

namespace {

// The plan of a run: candidate bitmaps where the rows qualify and their buffers can be had, else the probe / join form;
// batches of as many consecutive rows as there are index slabs (and, with bitmaps, as their pairs' bitmaps may take).
int plan_run(lzani_ctx* c, const RunGenomes& g, const Knobs& k, const RowFacts& f, u32 n_rows, const u64* row_off, bool lists, bool regions, RunPlan& p)
{
    for (u32 x = 0; x < g.n; ++x) p.Lmax = std::max(p.Lmax, g.L[x]);
    // rows of the presence matrix: one per k-mer (exact: the mixer is a bijection on the key bits) where the genomes fill a fair
    // part of the key space, else the hash's top bits -- 2^9 rows per text position keep the false candidates below 0.2 % of the
    // query positions, and a group's matrix is cleared and built in proportion to the genomes, not to 4^mal
    p.pm_bits = std::min(std::min(c->gs.geo.kb, 30), ceil_log2((u64)std::max(c->gs.Tmax, 1)) + 9);
    int rc = plan_bitmaps(c, g, k, f, n_rows, row_off, lists, regions, p);
    if (rc || p.pm) return rc;
    p.use_join = c->gs.lay.join_mode;
    if (p.use_join) { rc = ensure_join(c, g); if (rc) return rc; }          // (before the slabs are sized: they take 60 % of what is left)
    rc = ensure_slabs(c, n_rows);
    if (rc) return rc;
    cut_batches(n_rows, row_off, c->sl.slots, ~0ull, p.bstart);
    return LZANI_OK;
}

// The largest LDS copy of the presence filter that leaves k_pairs_blk (kf) two blocks per CU, decided once per genome set
// (blk_fold -2: none does, the wave kernel takes these rows too).
bool blk_fits(lzani_ctx* c, const void* kf)
{
    if (c->gs.blk_fold == -1) {
        for (int fold = 0; fold <= 4 && c->gs.blk_fold < 0; ++fold) {
            const size_t l = (size_t)(BLK_WAVES * SEED_LDS_WORDS + std::max<u64>(c->gs.lay.fl_stride >> fold, 1)) * 4;
            if (hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l) != hipSuccess) { (void)hipGetLastError(); continue; }
            lds_limit(c, kf) = l;                      // (what the kernel has now: the launch's raise_lds finds the fold settled on)
            int nb = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kf, 64 * BLK_WAVES, l) == hipSuccess && nb >= 2) c->gs.blk_fold = fold;
        }
        (void)hipGetLastError();
        if (c->gs.blk_fold < 0) c->gs.blk_fold = -2;
    }
    return c->gs.blk_fold >= 0;
}

// The batch's pair launch: the arguments, the facts of the launch, its kernel (choose_pair_kernel); a tuple compiled at
// run time goes first where the choice offers its kernel.
int launch_pairs(RunCtx& r, const Batch& bt, bool blk_rows, const DevEvent* ev)
{
    lzani_ctx* c = r.c;
    const bool tickets = bt.lpt && bt.split_S < 2;
    PairArgs pa;
    pa.G = gtab(c);
    pa.P = c->P; pa.geo = c->gs.geo;
    pa.dirz = c->sl.d_dirz; pa.ent = c->sl.d_ent;
    pa.dir_stride = c->gs.dir_stride; pa.ent_stride = c->gs.ent_stride;
    pa.bk = c->sl.d_bk; pa.bk_stride = c->gs.lay.bk_stride;
    pa.tw = c->sl.d_tw; pa.tw_stride = c->gs.lay.tw_stride;
    pa.fl = c->sl.d_fl; pa.fl_stride = c->gs.lay.fl_stride; pa.fmask = c->gs.lay.fmask;
    pa.ref_ids = r.d_ref + bt.k0; pa.row_off = r.d_off + bt.k0; pa.query_ids = r.d_q;
    pa.out = r.d_out; pa.cursor = c->d_cursor;
    pa.qorder = r.d_qorder + bt.k0; pa.qcum = r.d_qcum + bt.k0 + bt.b;
    for (int x = 0; x <= NQUEUES; ++x) pa.qb[x] = bt.qb[x];
    pa.skeys = r.cbits_stride ? c->gs.jl.keys : nullptr; pa.soff = c->gs.jl.soff; pa.scnt = c->gs.jl.cnt;
    pa.cbits = r.d_cbits; pa.cbits_stride = r.cbits_stride; pa.cb_e0 = 0;
    if (r.p.pm) { pa.cbits = reinterpret_cast<unsigned long long*>(c->cs.d_pm_cbits.get()); pa.cbits_stride = r.p.cb_words / 2; pa.cb_e0 = bt.e0; }
    pa.reg_out = r.rs ? r.rs->d_regions : nullptr; pa.reg_count = r.rs ? r.rs->d_count : nullptr; pa.reg_cap = r.rs ? r.rs->capacity : 0;
    pa.torder = tickets ? c->cs.d_lpt_keys + (bt.e1 - bt.e0) : nullptr;
    c->run.lpt_launches += tickets ? 1 : 0;
    HIPCHK(c, hipMemsetAsync(c->d_cursor, 0, NQUEUES * sizeof(unsigned long long), c->stream));
    const u64 waves = bt.e1 - bt.e0;
    const dim3 gd((u32)std::min<u64>((waves + 3) / 4, r.max_blocks)), bd(256);
    HIPCHK(c, hipEventRecord(ev[2], c->stream));
    PairFacts f;
    f.regions = r.rs != nullptr; f.fast = c->gs.tab.kmL != nullptr; f.tw = pa.tw != nullptr;
    f.pm = r.p.pm; f.split = bt.split_S >= 2; f.join = pa.skeys != nullptr;
    f.nfree = c->gs.all_nfree; f.dsel = r.dsel; f.rtc = r.rtc_k != nullptr;
    // Probe form, dense rows of hundreds of pairs: blocks of 16 waves with the reference's presence filter in LDS
    // (k_pairs_blk).  The rows a kmer-db filter leaves hold related pairs, where most positions pass the filter:
    // BASELINE configs[4] at full size is 6 % slower this way; LZANI_BLOCK_KERNEL=1/0 overrides.
    const void* kf = PAIR_KERNEL_FN[pair_blk_row(f.nfree, f.dsel)];
    f.blk = blk_rows && f.fast && f.tw && !f.join && blk_fits(c, kf);
    if (f.blk && !c->d_blkctr) HIPCHK(c, c->d_blkctr.alloc((size_t)c->n_cus * 2));
    const PairChoice ch = choose_pair_kernel(f);
    const PairKernelDesc& d = PAIR_KERNELS[ch.row];
    int rc = LZANI_OK;
    if (d.kind == PK_SPLIT) rc = run_split(r, bt, pa, ch.row);           // few, long pairs: several waves a pair
    else if (d.kind == PK_BLK) {
        u32 fw = (u32)std::max<u64>(c->gs.lay.fl_stride >> c->gs.blk_fold, 1), fold = (u32)c->gs.blk_fold;
        const size_t lds = (size_t)(BLK_WAVES * SEED_LDS_WORDS + fw) * 4;
        rc = raise_lds(c, kf, lds);              // (a no-op after blk_fits, which recorded the fold it settled on)
        if (rc) return rc;
        pa.fmask = c->gs.lay.fmask >> c->gs.blk_fold;
        c->run.blk_launches += 1;
        const dim3 gb((u32)std::min<u64>((waves + BLK_CHUNK_MIN - 1) / BLK_CHUNK_MIN, (u64)c->n_cus * 2)), bb(64 * BLK_WAVES);
        u32* blkctr = c->d_blkctr.get();
        void* kargs[] = {&pa, &fw, &fold, &blkctr};
        HIPCHK(c, launch_row(c, ch.row, gb, bb, kargs, lds));
    } else {
        c->run.pm_launches += d.cand == 2 ? 1 : 0;          // dense rows: candidate bitmaps made ahead (k_pm_cand)
        void* kargs[] = {&pa};
        bool by_rtc = false;
        if (ch.rtc_row >= 0) {
            by_rtc = launch_row(c, ch.rtc_row, gd, bd, kargs, 0, r.rtc_k->fn) == hipSuccess;
            if (by_rtc) c->run.rtc_launches += 1; else (void)hipGetLastError();
        }
        if (!by_rtc) HIPCHK(c, launch_row(c, ch.row, gd, bd, kargs));
    }
    if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev[3], c->stream));
    return LZANI_OK;
}

constexpr int EV = 5;                             // stamps per batch: index begin / end, pairs begin / end, candidates end

// One batch: index build, split / LPT choice, candidate stage, pair launch -- stream work only, stamped into ev.
int run_batch(RunCtx& r, Batch bt, const DevEvent* ev)
{
    lzani_ctx* c = r.c;
    const RunPlan& p = r.p;
    TRACE("batch %u rows [%u,%u) pairs [%llu,%llu) slots=%u pm=%d", bt.b, bt.k0, bt.k0 + bt.rows, (unsigned long long)bt.e0, (unsigned long long)bt.e1, c->sl.slots, (int)p.pm);
    HIPCHK(c, hipEventRecord(ev[0], c->stream));
    // rows for k_pairs_blk (launch_pairs): dense, hundreds of pairs each, probe form with tag words and a filter
    const bool blk_rows = !p.pm && !r.rs && c->gs.tab.kmL && c->gs.lay.tw_stride && !c->gs.lay.join_mode && c->gs.lay.fl_stride && bt.e1 > bt.e0 &&
                          (bt.e1 - bt.e0) / bt.rows >= 128 && r.k.block_kernel.value_or(r.query_ids == nullptr);
    int rc = build_indexes(c, r.k, r.d_ref + bt.k0, bt.rows, blk_rows, !p.pm);
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(ev[1], c->stream));
    if (p.pm && bt.e1 > bt.e0) {
        rc = choose_split_lpt(r, bt);
        if (!rc) rc = candidate_stage(r, bt);
        if (rc) return rc;
    }
    if (r.sink && p.pm && bt.e1 > bt.e0) { rc = sink_candidates(r, bt); if (rc) return rc; }
    HIPCHK(c, hipEventRecord(ev[4], c->stream));
    if (bt.e1 > bt.e0) {
        rc = launch_pairs(r, bt, blk_rows, ev);
        if (rc) return rc;
        c->run.tm.pair_launches += 1;
    }
    c->run.tm.pairs += bt.e1 - bt.e0;
    return LZANI_OK;
}

// The counters of diagnostic builds (-DLZANI_STAMPS and the like), printed and cleared after every run.
int report_diagnostics(lzani_ctx* c, u64 n_pairs)
{
#ifdef LZANI_STAMPS
    {
        unsigned long long acc[8];
        HIPCHK(c, hipMemcpyFromSymbol(acc, HIP_SYMBOL(g_stamp_acc), sizeof acc));
        unsigned long long tot = 0;
        for (int k = 0; k < 8; ++k) tot += acc[k];
        fprintf(stderr, "[lzani stamps] pairs=%llu total_cycles/pair=%.0f shares:", (unsigned long long)n_pairs, (double)tot / (double)n_pairs);
        const char* nm[8] = {"setup", "null_chain", "refill", "event", "find_event", "ext_fwd", "tail", "-"};
        for (int k = 0; k < 8; ++k) fprintf(stderr, " %s=%.1f%%", nm[k], 100.0 * (double)acc[k] / (double)tot);
        fprintf(stderr, "\n");
        unsigned long long z[8] = {0};
        HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_acc), z, sizeof z));
    }
#endif
#ifdef LZANI_PHASE_TIME
    {
        unsigned long long acc[4], z[4] = {0};
        HIPCHK(c, hipMemcpyFromSymbol(acc, HIP_SYMBOL(g_phase_time), sizeof acc));
        if (acc[3])
            fprintf(stderr, "[lzani phase] pairs=%llu, s_memtime ticks per pair: whole pair %.0f, inside the null chain %.0f (%.1f %%), inside refill %.0f (%.1f %%)\n",
                    acc[3], (double)acc[0] / acc[3], (double)acc[1] / acc[3], 100.0 * acc[1] / acc[0], (double)acc[2] / acc[3], 100.0 * acc[2] / acc[0]);
        HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(g_phase_time), z, sizeof z));
    }
#endif
#ifdef LZANI_PATH_STATS
    {
        unsigned long long acc[36], z[36] = {0};
        HIPCHK(c, hipMemcpyFromSymbol(acc, HIP_SYMBOL(g_path_stats), sizeof acc));
#define LZ_SLOT_NAME(k, name) name,
        const char* const slot[36] = {LZ_PATH_SLOTS(LZ_SLOT_NAME)};      // (lzani_kernels_pairs.h: the names' one home)
#undef LZ_SLOT_NAME
        const char* const* const nm = slot;
        fprintf(stderr, "[lzani paths] pairs=%llu, per pair:", (unsigned long long)n_pairs);
        for (int k = 0; k < 24; ++k) fprintf(stderr, " %s=%.1f;", nm[k], (double)acc[k] / (double)n_pairs);
        const char* const* const wn = slot + 24;
        fprintf(stderr, "\n[lzani paths] stretch chain exits per pair:");
        for (int k = 1; k < 10; ++k) fprintf(stderr, " %s=%.1f;", wn[k], (double)acc[24 + k] / (double)n_pairs);
        fprintf(stderr, "\n[lzani paths raw]");                          // the totals themselves, one line per run (tests/path_cover.py)
        for (int k = 0; k < 36; ++k) fprintf(stderr, " %llu", acc[k]);
        fprintf(stderr, "\n");
        HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(g_path_stats), z, sizeof z));
    }
#endif
#ifdef LZANI_CHAIN_STATS
    {
        unsigned long long acc[24], z[24] = {0};
        HIPCHK(c, hipMemcpyFromSymbol(acc, HIP_SYMBOL(g_chain_stats), sizeof acc));
#define LZ_SLOT_NAME(k, name) name,
        const char* const nm[24] = {LZ_CHAIN_SLOTS(LZ_SLOT_NAME)};       // (lzani_kernels_pairs.h: the names' one home)
#undef LZ_SLOT_NAME
        fprintf(stderr, "[lzani chain] pairs=%llu per pair:", (unsigned long long)n_pairs);
        for (int k = 0; k < 8; ++k) fprintf(stderr, " %s=%.1f", nm[k], (double)acc[k] / (double)n_pairs);
        fprintf(stderr, "\n[lzani chain] wave cycles per pair: after exit_nothing=%.0f after round_done=%.0f after exit_event=%.0f inside the chain=%.0f\n",
                (double)acc[8] / (double)n_pairs, (double)acc[9] / (double)n_pairs, (double)acc[10] / (double)n_pairs, (double)acc[11] / (double)n_pairs);
        fprintf(stderr, "[lzani chain] events found but not null, per pair: close=%.1f region kept or none open=%.1f no forward record=%.1f backward side=%.1f\n",
                (double)acc[12] / (double)n_pairs, (double)acc[13] / (double)n_pairs, (double)acc[14] / (double)n_pairs, (double)acc[15] / (double)n_pairs);
        fprintf(stderr, "[lzani chain] exit_seed by the test that handed the round back, per pair: anchor's own step=%.1f no window position=%.1f several=%.1f text end=%.1f long seed=%.1f other=%.1f; event known, commit left=%.1f\n",
                (double)acc[16] / (double)n_pairs, (double)acc[17] / (double)n_pairs, (double)acc[18] / (double)n_pairs, (double)acc[19] / (double)n_pairs,
                (double)acc[20] / (double)n_pairs, (double)acc[21] / (double)n_pairs, (double)acc[22] / (double)n_pairs);
        fprintf(stderr, "[lzani chain raw]");
        for (int k = 0; k < 24; ++k) fprintf(stderr, " %llu", acc[k]);
        fprintf(stderr, "\n");
        HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(g_chain_stats), z, sizeof z));
    }
#endif
    return LZANI_OK;
}

// The end of a run: the one host wait, the loop guards, the event timings.
int finish_run(lzani_ctx* c, u64 n_pairs, const lzani_rtc::Kernel* rtc_k, const std::vector<u32>& bstart, const u64* row_off)
{
    HIPCHK(c, hipStreamSynchronize(c->stream));       // the one host wait of the call
    TRACE("pairs done");
    const int rc = report_diagnostics(c, n_pairs);
    if (rc) return rc;
    int trip = 0;
    HIPCHK(c, hipMemcpyFromSymbol(&trip, HIP_SYMBOL(g_guard_trip), sizeof(int)));
    if (rtc_k && c->run.rtc_launches) {          // (a code object of its own has a loop guard of its own)
        int t2 = 0, zero = 0;
        HIPCHK(c, hipMemcpyDtoH(&t2, rtc_k->guard, sizeof(int)));
        if (t2) { HIPCHK(c, hipMemcpyHtoD(rtc_k->guard, &zero, sizeof(int))); if (!trip) trip = t2; }
    }
    if (trip) {
        int zero = 0;
        HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(g_guard_trip), &zero, sizeof(int)));
        return fail(c, LZANI_ERR_DEVICE, "pair kernel: loop guard " + std::to_string(trip) + " tripped (corrupt index or text)");
    }
    lzani_timing& tm = c->run.tm;
    if (c->km_timed) {
        float ms = 0;
        HIPCHK(c, c->km_span.elapsed(ms));
        tm.kmers_ms = ms;
    }
    tm.kmers_ms += c->join_ms_pending;
    c->join_ms_pending = 0;
    for (size_t b = 0; b + 1 < bstart.size(); ++b) {
        const DevEvent* ev = c->events.data() + (size_t)EV * b;
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
        tm.index_ms += ms;
        HIPCHK(c, hipEventElapsedTime(&ms, ev[1], ev[4]));
        tm.cand_ms += ms;
        if (row_off[bstart[b + 1]] > row_off[bstart[b]]) {         // (a batch with pairs: its pair launch)
            HIPCHK(c, hipEventElapsedTime(&ms, ev[2], ev[3]));
            tm.pairs_ms += ms;
        }
    }
    return LZANI_OK;
}

RunGenomes run_genomes_of(const lzani_ctx* c) { return RunGenomes{c->gs.n, c->gs.L.data()}; }     // the set's own table

// A run of rows on the resident genomes, whose table is g: check, plan, queues and uploads, then the batches back to back
// on the stream, then one wait.
int run_rows_impl(lzani_ctx* c, const RunGenomes& g, u32 n_rows, const u32* ref_ids, const u64* row_off, const u32* query_ids,
                  int* d_out, const RegionSink* rs = nullptr, CandSink* sink = nullptr, RunPlan* plan_out = nullptr)
{
    if (!g.n) return fail(c, LZANI_ERR_STATE, "lzani_run_rows: no genomes set");
    c->run = RunRecord{};
    const Knobs k{};
    if (n_rows == 0) return LZANI_OK;
    RowFacts rf;
    int rc = check_rows(c, g, n_rows, ref_ids, row_off, query_ids, rf);
    const u64 n_pairs = rf.n_pairs;
    if (rc || n_pairs == 0) return rc;

    HIPCHK(c, hipSetDevice(c->dev));
    // (the k-mer words and the join lists are made by the first run after lzani_set_genomes -- inside its timed index
    // stage, reported as kmers_ms -- and kept: they depend on the genome set and the parameters only)
    c->km_timed = false;
    rc = ensure_kmers(c);
    if (rc) return rc;
    RunPlan p;
    rc = plan_run(c, g, k, rf, n_rows, row_off, query_ids != nullptr, rs != nullptr, p);
    if (rc) return rc;
    if (plan_out) *plan_out = p;

    // Everything the batches need from the host -- row tables and the per-XCD work queues of every batch -- is prepared and
    // uploaded before the first launch, so the batches follow each other on the stream without a host round trip in between.
    const u32 n_batches = (u32)p.bstart.size() - 1;
    c->run.batches = n_batches;
    const auto [qorder, qcum, qb] = plan_queues(n_rows, row_off, p.bstart, NQUEUES);
    DevMem<u32> d_ref, d_q, d_qorder;
    DevMem<u64> d_off, d_qcum;
    HIPCHK(c, d_qorder.alloc(n_rows));
    HIPCHK(c, d_qcum.alloc(qcum.size()));
    HIPCHK(c, d_ref.alloc(n_rows));
    HIPCHK(c, d_off.alloc((size_t)n_rows + 1));
    HIPCHK(c, hipMemcpyAsync(d_ref, ref_ids, (size_t)n_rows * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_off, row_off, (size_t)(n_rows + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_qorder, qorder.data(), qorder.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_qcum, qcum.data(), qcum.size() * 8, hipMemcpyHostToDevice, c->stream));
    if (query_ids) {
        HIPCHK(c, d_q.alloc(n_pairs));
        HIPCHK(c, hipMemcpyAsync(d_q, query_ids, (size_t)n_pairs * 4, hipMemcpyHostToDevice, c->stream));
    }
    while (c->events.size() < (size_t)EV * n_batches) {       // read back after the one sync
        DevEvent e;
        HIPCHK(c, e.create());
        c->events.push_back(std::move(e));
    }
    const u32 max_blocks = (u32)c->n_cus * k.blocks_per_cu;
    DevMem<unsigned long long> d_cbits;                      // join form: one candidate bitmap per resident wave
    u64 cbits_stride = 0;
    if (p.use_join && !rs) {
        cbits_stride = (u64)((p.Lmax + c->P.mrd) >> 6) + 8;
        HIPCHK(c, d_cbits.alloc((size_t)max_blocks * 4 * cbits_stride));
    }
    // Any other parameter tuple: the same kernel compiled for it the first time this context needs it (lzani_rtc.h) -- the
    // eight ints folded into the code, the hand-written null chain included where the tuple is inside what the chain is
    // written for (chain_params_ok).  Built (or loaded from the disk cache) here, ahead of the stream's first stamp.
    // A compile takes 2-3 s and the folded kernel saves ~0.13 s per million pairs of 40 kbp: a code object that is not in
    // the disk cache yet is built once the context has been asked for LZANI_RTC_MIN_PAIRS pairs in all (default 2 M: the
    // first such run loses a second or two, every later run and every later process wins).
    const int dsel = defp_select(c->P), cand = pair_cand(p.pm, p.use_join, c->sl.d_tw != nullptr);
    lzani_rtc::Kernel* rtc_k = nullptr;
    c->pairs_seen += n_pairs;
    if (!dsel && !rs && c->gs.tab.kmL && c->sl.d_bk && lzani_rtc::enabled() && cand >= 0) {
        rtc_k = lzani_rtc::get(c->rtc, c->P, c->gs.all_nfree, cand, c->arch.c_str(), c->pairs_seen >= k.rtc_min_pairs);
        if (!rtc_k && c->rtc.failed) TRACE("run-time compile unavailable (%s): the generic kernel runs", c->rtc.log.c_str());
    }

    RunCtx r{c, g, k, p, rs, row_off, query_ids, d_out, d_ref, d_q, d_qorder, d_off, d_qcum, max_blocks, dsel, d_cbits, cbits_stride, rtc_k};
    r.sink = sink;
    for (u32 b = 0; b < n_batches; ++b) {
        const u32 k0 = p.bstart[b], k1 = p.bstart[b + 1];
        rc = run_batch(r, Batch{b, k0, k1 - k0, row_off[k0], row_off[k1], qb.data() + (size_t)b * (NQUEUES + 1)}, c->events.data() + (size_t)EV * b);
        if (rc) return rc;
    }
    return finish_run(c, n_pairs, rtc_k, p.bstart, row_off);
}

}  // namespace

#include "lzani_ooc.h"

namespace {

// The one fork of the run entry points: tile by tile for an out-of-core set -- results to d_out (device) and / or h_out
// (host) -- else one run on the set's own table, whose results go to d_out or, where the caller gave a host buffer, to
// *d_res, made here for the caller to copy out (null with a null h_out).  Sets the tile count of lzani_get_residency.
int run_rows_any(lzani_ctx* c, u32 n_rows, const u32* ref_ids, const u64* row_off, const u32* query_ids,
                 int* d_out, lzani_result* h_out, DevMem<lzani_result>* d_res, const RegionSink* rs)
{
    if (c->gs.ooc) return run_rows_tiled(c, n_rows, ref_ids, row_off, query_ids, d_out, h_out, rs);
    const u64 n_pairs = n_rows ? row_off[n_rows] : 0;
    if (h_out && n_pairs) { HIPCHK(c, d_res->alloc(n_pairs)); d_out = (int*)d_res->get(); }
    const int rc = run_rows_impl(c, run_genomes_of(c), n_rows, ref_ids, row_off, query_ids, d_out, rs);
    c->res.tiles = rc == LZANI_OK && n_pairs ? 1 : 0;
    return rc;
}

}  // namespace

#include "lzani_prefilter.h"
#include "lzani_prefilter_limit.h"
#include "lzani_kept.h"
#include "lzani_regions.h"
#include "lzani_cluster.h"

extern "C" {

static void comm_release(lzani_ctx* c);      // lzani_multi.h

void lzani_default_params(lzani_params* p)
{
    p->min_anchor_len = 11; p->min_seed_len = 7; p->max_dist_in_ref = 40; p->max_dist_in_query = 40;
    p->min_region_len = 35; p->approx_window = 15; p->approx_mismatches = 7; p->approx_run_len = 3;
}

int lzani_create(const lzani_params* p, int device_id, lzani_ctx** out)
{
    if (!p || !out) return LZANI_ERR_ARG;
    *out = nullptr;
    const Params P = params_of(*p);
    if (!params_supported(P)) return LZANI_ERR_PARAMS;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return LZANI_ERR_DEVICE;
    lzani_ctx* c = new (std::nothrow) lzani_ctx();
    if (!c) return LZANI_ERR_NOMEM;
    c->P = P;
    c->dev = device_id;
    bool ok = hipSetDevice(device_id) == hipSuccess && hipStreamCreate(&c->stream) == hipSuccess;
    if (ok) {                                                  // the queue cursors: the one buffer a context is made with
        const hipError_t e = c->d_cursor.alloc(NQUEUES);
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); lzani_destroy(c); return LZANI_ERR_NOMEM; }
        ok = e == hipSuccess;
    }
    if (ok) {
        hipDeviceProp_t prop;
        ok = hipGetDeviceProperties(&prop, device_id) == hipSuccess;
        if (ok) { c->n_cus = prop.multiProcessorCount; c->arch = prop.gcnArchName; }
    }
    if (!ok) { lzani_destroy(c); return LZANI_ERR_DEVICE; }
    *out = c;
    return LZANI_OK;
}

void lzani_destroy(lzani_ctx* c)
{
    if (!c) return;
    hipSetDevice(c->dev);
    comm_release(c);
    lzani_rtc::release(c->rtc);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

const char* lzani_last_error(const lzani_ctx* c) { return c ? c->err.c_str() : "null context"; }

int lzani_set_genomes(lzani_ctx* c, uint32_t n, const uint8_t* const* codes, const uint32_t* len)
{
    if (!c) return LZANI_ERR_ARG;
    if (!n || !codes || !len) return fail(c, LZANI_ERR_ARG, "lzani_set_genomes: empty input");
    HIPCHK(c, hipSetDevice(c->dev));
    c->gs = GenomeSet{};
    c->sl = IndexSlabs{};
    c->cs = CandScratch{};
    c->pf = Prefilter{};
    c->kept = Kept{};
    c->rg = AlignedRegions{};
    c->cl = Cluster{};
    c->cls = ClusterStore{};
    c->res = Residency{};
    c->gs.L.resize(n);
    c->gs.nmoff.resize(n);
    std::vector<u64> codeoff(n);
    u64 total_codes = 0, total_nm = 0;
    int Lmax = 0;
    for (u32 g = 0; g < n; ++g) {
        if (len[g] > 0x3FFFFFFFu - 3u * (u32)c->P.mrd)
            return fail(c, LZANI_ERR_ARG, "lzani_set_genomes: sequence too long for 32-bit text positions");
        if (len[g] && !codes[g]) return fail(c, LZANI_ERR_ARG, "lzani_set_genomes: null sequence");
        c->gs.L[g] = (int)len[g];
        Lmax = std::max(Lmax, c->gs.L[g]);
        codeoff[g] = total_codes; total_codes += len[g];
        c->gs.nmoff[g] = total_nm; total_nm += text_wordsN(ref_text_len(c->gs.L[g], c->P.mrd));
    }
    c->gs.Tmax = ref_text_len(Lmax, c->P.mrd);
    c->gs.geo = index_geometry(c->gs.Tmax, c->P.mal);
    c->gs.dir_stride = ((u64)1 << c->gs.geo.dirbits) + 1;
    c->gs.ent_stride = (u64)c->gs.Tmax;
    c->gs.total_nm = total_nm;
    const SetKnobs k{};
    c->gs.lay = set_layout_of(c->P, c->gs.geo, c->gs.Tmax, n, k);
    // Residency: the whole set in HBM (upload_genomes, on every genome), or blocks of it kept on the host and uploaded by
    // the runs (lzani_ooc.h).  Automatic mode (limit 0) keeps every set in-core that can be had in-core: its tables, the
    // staging copy and one index slab within the free memory.
    u64 limit = c->mem_req;
    if (!limit) {
        size_t free_b = 0, total_b = 0;
        HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
        if (k.free_bytes) free_b = std::min<size_t>(free_b, (size_t)*k.free_bytes);
        limit = auto_genome_limit(genome_table_bytes(total_nm, kmer_words_of(c->P)), total_codes, slot_bytes(c->gs).total(), free_b);
    }
    std::vector<u64> bytes;
    std::string msg;
    const int nb = plan_blocks_impl(n, len, c->P, limit, k, c->gs.blk_first, bytes, msg);
    if (nb < 0) return fail(c, c->mem_req ? nb : LZANI_ERR_NOMEM, "lzani_set_genomes: " + msg);
    if (nb > 1) {
        c->gs.blk_bytes = bytes;
        c->gs.mem_limit = limit;
        return ooc_set_genomes(c, n, codes, len);
    }
    c->gs.mem_limit = c->mem_req;
    c->res.peak = bytes[0];
    c->gs.blk_first.clear();
    return upload_genomes(c, n, codes, len, codeoff, total_codes);
}

int lzani_run_rows_device(lzani_ctx* c, uint32_t n_rows, const uint32_t* ref_ids, const uint64_t* row_off,
                          const uint32_t* query_ids, void* d_out)
{
    if (!c) return LZANI_ERR_ARG;
    if (!ref_ids || !row_off || (!d_out && n_rows && row_off[n_rows]))
        return fail(c, LZANI_ERR_ARG, "lzani_run_rows_device: null argument");
    return run_rows_any(c, n_rows, ref_ids, row_off, query_ids, (int*)d_out, nullptr, nullptr, nullptr);
}

int lzani_run_rows(lzani_ctx* c, uint32_t n_rows, const uint32_t* ref_ids, const uint64_t* row_off,
                   const uint32_t* query_ids, lzani_result* out)
{
    if (!c) return LZANI_ERR_ARG;
    if (!ref_ids || !row_off) return fail(c, LZANI_ERR_ARG, "lzani_run_rows: null argument");
    const u64 n_pairs = n_rows ? row_off[n_rows] : 0;
    if (n_pairs && !out) return fail(c, LZANI_ERR_ARG, "lzani_run_rows: null output");
    HIPCHK(c, hipSetDevice(c->dev));
    DevMem<lzani_result> d_res;
    int rc = run_rows_any(c, n_rows, ref_ids, row_off, query_ids, nullptr, out, &d_res, nullptr);
    if (rc == LZANI_OK && d_res) {
        hipError_t e = hipMemcpy(out, d_res.get(), n_pairs * sizeof(lzani_result), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(c, LZANI_ERR_DEVICE, std::string("copy results: ") + hipGetErrorString(e));
    }
    return rc;
}

int lzani_run_rows_regions(lzani_ctx* c, uint32_t n_rows, const uint32_t* ref_ids, const uint64_t* row_off,
                           const uint32_t* query_ids, lzani_result* out, lzani_region* regions,
                           uint64_t capacity, uint64_t* n_regions)
{
    if (!c) return LZANI_ERR_ARG;
    if (!ref_ids || !row_off || !n_regions || (capacity && !regions))
        return fail(c, LZANI_ERR_ARG, "lzani_run_rows_regions: null argument");
    const u64 n_pairs = n_rows ? row_off[n_rows] : 0;
    if (n_pairs && !out) return fail(c, LZANI_ERR_ARG, "lzani_run_rows_regions: null output");
    *n_regions = 0;
    HIPCHK(c, hipSetDevice(c->dev));
    DevMem<lzani_result> d_res;
    DevMem<lzani_region> d_regions;
    DevMem<unsigned long long> d_count;
    HIPCHK(c, d_regions.alloc(capacity));
    HIPCHK(c, d_count.alloc(1));
    HIPCHK(c, hipMemset(d_count.get(), 0, sizeof(unsigned long long)));
    RegionSink rs{d_regions.get(), d_count.get(), capacity};
    int rc = run_rows_any(c, n_rows, ref_ids, row_off, query_ids, nullptr, out, &d_res, &rs);
    if (rc == LZANI_OK) {
        unsigned long long cnt = 0;
        hipError_t e = hipMemcpy(&cnt, rs.d_count, sizeof cnt, hipMemcpyDeviceToHost);
        if (e == hipSuccess && d_res) e = hipMemcpy(out, d_res.get(), n_pairs * sizeof(lzani_result), hipMemcpyDeviceToHost);
        if (e == hipSuccess && cnt && capacity)
            e = hipMemcpy(regions, rs.d_regions, std::min<uint64_t>(cnt, capacity) * sizeof(lzani_region), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(c, LZANI_ERR_DEVICE, std::string("copy regions: ") + hipGetErrorString(e));
        *n_regions = cnt;
    }
    return rc;
}

int lzani_get_timing(const lzani_ctx* c, lzani_timing* t)
{
    if (!c || !t) return LZANI_ERR_ARG;
    *t = c->run.tm;
    return LZANI_OK;
}

int lzani_get_layout(const lzani_ctx* c, lzani_layout_info* o)
{
    if (!c || !o) return LZANI_ERR_ARG;
    o->key_bits = c->gs.geo.kb; o->dir_bits = c->gs.geo.dirbits; o->pos_bits = c->gs.geo.posbits; o->tag_mask = c->gs.geo.tagmask;
    o->kmer_words = c->gs.tab.kmL != nullptr;
    o->bucket_table = c->gs.lay.bk_stride != 0; o->tag_words = c->gs.lay.tw_stride != 0;
    o->n_free = c->gs.all_nfree;
    o->slots = c->sl.slots; o->batches_last_run = c->run.batches;
    o->bytes_per_slot = slot_bytes(c->gs).tables;           // (without the keys of the sort-based build)
    o->bytes_genomes = genome_table_bytes(c->gs.total_nm, c->gs.tab.kmL != nullptr);
    o->join_lists = c->gs.lay.join_mode; o->block_launches = c->run.blk_launches; o->bitmap_launches = c->run.pm_launches; o->rtc_launches = c->run.rtc_launches;
    o->lpt_launches = c->run.lpt_launches; o->matrix_from_index = c->run.pmfi_launches;
    o->split_launches = c->run.split_launches; o->split_segments = c->run.split_items;
    return LZANI_OK;
}

int lzani_get_rtc_info(const lzani_ctx* c, lzani_rtc_info* o)
{
    if (!c || !o) return LZANI_ERR_ARG;
    o->folded_ahead_of_time = defp_select(c->P) != 0;
    o->null_chain = chain_params_ok(c->P);
    o->kernels_built = c->rtc.built; o->kernels_from_cache = c->rtc.from_cache; o->kernels_failed = c->rtc.failed;
    o->reserved_ = 0;
    o->build_ms = c->rtc.compile_ms;
    return LZANI_OK;
}

int lzani_debug_kernel_launches(const lzani_ctx* c, uint64_t* counts, uint32_t cap)
{
    if (!c || (!counts && cap)) return LZANI_ERR_ARG;
    for (u32 i = 0; i < cap && i < (u32)PK_COUNT; ++i) counts[i] = c->run.klaunch[i];
    return (int)PK_COUNT;
}

int lzani_debug_split_stats(const lzani_ctx* c, lzani_split_stats* o)
{
    if (!c || !o) return LZANI_ERR_ARG;
    o->pairs_cut = c->run.split_cut; o->rounds = c->run.split_rounds; o->resumed = c->run.split_resumed; o->given_up = c->run.split_given_up;
    for (int k = 0; k < 6; ++k) o->voids[k] = c->run.split_void[k];
    return LZANI_OK;
}

int lzani_set_genome_memory(lzani_ctx* c, uint64_t bytes)
{
    if (!c) return LZANI_ERR_ARG;
    c->mem_req = bytes;
    return LZANI_OK;
}

int lzani_plan_blocks(uint32_t n, const uint32_t* len, const lzani_params* p, uint64_t limit, uint32_t* block_of)
{
    if (!p || !len || !n) return LZANI_ERR_ARG;
    const Params P = params_of(*p);
    if (!params_supported(P)) return LZANI_ERR_PARAMS;
    std::vector<u32> first;
    std::vector<u64> bytes;
    std::string msg;
    const int nb = plan_blocks_impl(n, len, P, limit, SetKnobs{}, first, bytes, msg);
    if (nb > 0 && block_of)
        for (int b = 0; b < nb; ++b) std::fill(block_of + first[b], block_of + first[b + 1], (uint32_t)b);
    return nb;
}

int lzani_get_residency(const lzani_ctx* c, lzani_residency_info* o)
{
    if (!c || !o) return LZANI_ERR_ARG;
    o->limit = c->gs.mem_limit;
    o->blocks = c->gs.ooc ? (uint32_t)c->gs.blk_first.size() - 1 : (c->gs.n ? 1u : 0u);
    o->tiles = c->res.tiles;
    o->block_uploads = c->res.uploads;
    o->peak_resident_bytes = c->res.peak;
    o->host_bytes = c->gs.h_codes.size();
    o->upload_ms = c->res.upload_ms;
    return LZANI_OK;
}

// Test hook: the allocation fault of lzani_devmem.h.  Needs no context and calls no runtime.
int lzani_debug_alloc_fault(uint64_t first, uint64_t count, uint64_t* seen)
{
    if (first && !count) return LZANI_ERR_ARG;
    const uint64_t before = alloc_fault_arm(first, count);
    if (seen) *seen = before;
    return LZANI_OK;
}

const char* lzani_debug_kernel_name(uint32_t id)
{
    return id < (u32)PK_COUNT ? PAIR_KERNELS[id].name : nullptr;
}

int64_t lzani_debug_rtc_compile(const lzani_params* p, int nfree, int cand, const char* arch, char* log, uint64_t log_cap)
{
    if (!p || !arch || cand < 0 || cand > 2) return LZANI_ERR_ARG;
    const Params P = params_of(*p);
    if (!params_supported(P) || P.mal > 15 || P.msl > 15) return LZANI_ERR_PARAMS;
    std::string lg;
    const size_t n = lzani_rtc::compile_only(P, nfree != 0, cand, arch, lg);
    if (log && log_cap) { snprintf(log, (size_t)log_cap, "%s", lg.c_str()); }
    return n ? (int64_t)n : (int64_t)LZANI_ERR_DEVICE;
}

// Test hook: the engine's radix sort (lzani_sort.hip) on host keys -- n_seg segments of seg_len keys, each sorted on its own by
// the bits [begin_bit, end_bit), stably.
int lzani_debug_sort_segments(lzani_ctx* c, const uint64_t* keys, uint64_t* out, uint64_t seg_len, uint32_t n_seg, int begin_bit, int end_bit)
{
    if (!c || !keys || !out) return LZANI_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    const size_t n = (size_t)seg_len * n_seg;
    if (n == 0) return LZANI_OK;
    if (begin_bit < 0 || end_bit > 64 || end_bit < begin_bit) return fail(c, LZANI_ERR_ARG, "lzani_debug_sort_segments: bad arguments");
    DevMem<unsigned long long> d_in, d_out;
    DevMem<unsigned char> d_tmp;
    HIPCHK(c, d_in.alloc(n));
    HIPCHK(c, d_out.alloc(n));
    HIPCHK(c, hipMemcpy(d_in.get(), keys, n * 8, hipMemcpyHostToDevice));
    if (int rc = sort_keys(c, d_tmp, d_in.get(), d_out.get(), seg_len, n_seg, begin_bit, end_bit, "lzani_debug_sort_segments: sort", false)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, d_out.get(), n * 8, hipMemcpyDeviceToHost));
    return LZANI_OK;
}

// Test hook: lzani_run_rows with the candidate bitmaps of every batch copied out on the way (CandSink).
int lzani_debug_run_candidates(lzani_ctx* c, uint32_t n_rows, const uint32_t* ref_ids, const uint64_t* row_off,
                               const uint32_t* query_ids, lzani_result* out, uint64_t words, uint32_t* cbits,
                               uint32_t* pcount, lzani_cand_plan* plan)
{
    if (!c) return LZANI_ERR_ARG;
    if (!ref_ids || !row_off || !plan) return fail(c, LZANI_ERR_ARG, "lzani_debug_run_candidates: null argument");
    if (c->gs.ooc) return fail(c, LZANI_ERR_STATE, "lzani_debug_run_candidates: the genomes are not resident (out-of-core set)");
    const u64 n_pairs = n_rows ? row_off[n_rows] : 0;
    if (n_pairs && !out) return fail(c, LZANI_ERR_ARG, "lzani_debug_run_candidates: null output");
    HIPCHK(c, hipSetDevice(c->dev));
    if (pcount) std::fill(pcount, pcount + n_pairs, 0xFFFFFFFFu);
    DevMem<lzani_result> d_out;
    if (n_pairs) HIPCHK(c, d_out.alloc(n_pairs));
    CandSink sink{cbits, words, pcount, 0};
    RunPlan p;
    int rc = run_rows_impl(c, run_genomes_of(c), n_rows, ref_ids, row_off, query_ids, (int*)d_out.get(), nullptr, &sink, &p);
    if (rc == LZANI_OK && n_pairs) {
        hipError_t e = hipMemcpy(out, d_out.get(), n_pairs * sizeof(lzani_result), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(c, LZANI_ERR_DEVICE, std::string("copy results: ") + hipGetErrorString(e));
    }
    if (rc) return rc;
    plan->pm = p.pm; plan->pm_bits = p.pm ? p.pm_bits : 0; plan->rshift = p.pm ? c->gs.geo.kb - p.pm_bits : 0;
    plan->pm_group = p.pm ? p.pm_group : 0;
    plan->cb_words = p.pm ? p.cb_words : 0;
    plan->batches = c->run.batches;
    plan->from_index_launches = (uint32_t)c->run.pmfi_launches;
    plan->cand_launches = (uint32_t)c->run.pmc_launches;
    plan->counted_batches = sink.counted_batches;
    return LZANI_OK;
}

}  // extern "C"

#include "lzani_multi.h"
