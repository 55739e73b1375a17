// lzani_hip.hip -- the C-ABI of include/lzani.h: context, device memory, launches.  gfx950 (MI355X) only.
//
// The kernels (all integer / bit work; no MFMA by design) live in two headers included below:
//   lzani_kernels_index.h   k_pack, k_kmers, k_idx_*   genomes -> packed texts, k-mer words, anchor indexes
//   lzani_kernels_cand.h    k_pm_build, k_pm_cand   dense rows: presence matrix of a group of references -> per-pair candidate bitmaps
//   lzani_kernels_pairs.h   DevWave, k_pairs   the pair kernel
//   lzani_kernels_prefilter.h   k_pf_*   the k-mer prefilter: shared k-mer counts of all genome pairs
// The algorithm itself (PairMachine and its building blocks, shared with the host model of the tests) is
// lzani_core.h; sizes and the parameter envelope are lzani_layout.h; the pure decisions of a run (batches, queues, the
// split rule, the bytes of a slab slot) are lzani_run_plan.h, free of HIP.  Four layers of the host side are files of their
// own, included at fixed places below:
//   lzani_dense.h       the dense-row stage of a run: candidate bitmaps from the presence matrix, the split of few, long pairs
//   lzani_ooc.h         genome sets larger than the device: block plan, block uploads, the tiled run
//   lzani_prefilter.h   the k-mer prefilter's host stage: slice and pass plans, the pass / tile driver, its entry points
//   lzani_multi.h       the multi-GPU layer
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <optional>
#include <string>
#include <type_traits>
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
#include "lzani_rtc.h"
#include "lzani_devmem.h"
#include "lzani_run_plan.h"

// ============================================================================================
// Host side of the C-ABI
// ============================================================================================
using namespace lzani;

// Launch record: one entry per pair-kernel instantiation the dispatch of run_rows_impl can launch, counted per context
// for the last run (lzani_debug_kernel_launches).  The names follow one grammar a test can build from the dispatch rules:
//   pairs fast=F nfree=N defp=D aln=A bk=B cand=C   k_pairs<F, N, D, A, B, C>
//   pairs_blk nfree=N defp=D                        k_pairs_blk<N, D>
//   split nfree=N defp=D mode=M                     k_split<N, D, M>
//   rtc nfree=N cand=C                              the run-time compiled kernel (lzani_rtc.h), DEFP 9
// An instantiation added to the dispatch needs a row here (count_launch refuses to compile without one) and a cell in
// tests/test_gpu_instantiations.py.
enum PairKernelKind { PK_PAIRS, PK_BLK, PK_SPLIT, PK_RTC };
struct PairKernelDesc { const char* name; int kind, fast, nfree, defp, aln, bk, cand, mode; };
constexpr PairKernelDesc PAIR_KERNELS[] = {
    {"pairs fast=0 nfree=0 defp=0 aln=1 bk=0 cand=0", PK_PAIRS, 0, 0, 0, 1, 0, 0, 0},
    {"pairs fast=1 nfree=0 defp=0 aln=1 bk=1 cand=0", PK_PAIRS, 1, 0, 0, 1, 1, 0, 0},
    {"pairs fast=1 nfree=0 defp=0 aln=1 bk=0 cand=0", PK_PAIRS, 1, 0, 0, 1, 0, 0, 0},
    {"pairs fast=0 nfree=0 defp=0 aln=0 bk=0 cand=0", PK_PAIRS, 0, 0, 0, 0, 0, 0, 0},
    {"pairs fast=1 nfree=0 defp=0 aln=0 bk=1 cand=2", PK_PAIRS, 1, 0, 0, 0, 1, 2, 0},
    {"pairs fast=1 nfree=0 defp=1 aln=0 bk=1 cand=2", PK_PAIRS, 1, 0, 1, 0, 1, 2, 0},
    {"pairs fast=1 nfree=0 defp=2 aln=0 bk=1 cand=2", PK_PAIRS, 1, 0, 2, 0, 1, 2, 0},
    {"pairs fast=1 nfree=1 defp=0 aln=0 bk=1 cand=2", PK_PAIRS, 1, 1, 0, 0, 1, 2, 0},
    {"pairs fast=1 nfree=1 defp=1 aln=0 bk=1 cand=2", PK_PAIRS, 1, 1, 1, 0, 1, 2, 0},
    {"pairs fast=1 nfree=1 defp=2 aln=0 bk=1 cand=2", PK_PAIRS, 1, 1, 2, 0, 1, 2, 0},
    {"pairs fast=1 nfree=0 defp=0 aln=0 bk=1 cand=1", PK_PAIRS, 1, 0, 0, 0, 1, 1, 0},
    {"pairs fast=1 nfree=0 defp=1 aln=0 bk=1 cand=1", PK_PAIRS, 1, 0, 1, 0, 1, 1, 0},
    {"pairs fast=1 nfree=0 defp=2 aln=0 bk=1 cand=1", PK_PAIRS, 1, 0, 2, 0, 1, 1, 0},
    {"pairs fast=1 nfree=1 defp=0 aln=0 bk=1 cand=1", PK_PAIRS, 1, 1, 0, 0, 1, 1, 0},
    {"pairs fast=1 nfree=1 defp=1 aln=0 bk=1 cand=1", PK_PAIRS, 1, 1, 1, 0, 1, 1, 0},
    {"pairs fast=1 nfree=1 defp=2 aln=0 bk=1 cand=1", PK_PAIRS, 1, 1, 2, 0, 1, 1, 0},
    {"pairs fast=1 nfree=0 defp=0 aln=0 bk=1 cand=0", PK_PAIRS, 1, 0, 0, 0, 1, 0, 0},
    {"pairs fast=1 nfree=0 defp=1 aln=0 bk=1 cand=0", PK_PAIRS, 1, 0, 1, 0, 1, 0, 0},
    {"pairs fast=1 nfree=1 defp=0 aln=0 bk=1 cand=0", PK_PAIRS, 1, 1, 0, 0, 1, 0, 0},
    {"pairs fast=1 nfree=1 defp=1 aln=0 bk=1 cand=0", PK_PAIRS, 1, 1, 1, 0, 1, 0, 0},
    {"pairs fast=1 nfree=0 defp=0 aln=0 bk=0 cand=0", PK_PAIRS, 1, 0, 0, 0, 0, 0, 0},
    {"pairs fast=1 nfree=0 defp=1 aln=0 bk=0 cand=0", PK_PAIRS, 1, 0, 1, 0, 0, 0, 0},
    {"pairs fast=1 nfree=1 defp=0 aln=0 bk=0 cand=0", PK_PAIRS, 1, 1, 0, 0, 0, 0, 0},
    {"pairs fast=1 nfree=1 defp=1 aln=0 bk=0 cand=0", PK_PAIRS, 1, 1, 1, 0, 0, 0, 0},
    {"pairs_blk nfree=0 defp=0", PK_BLK, 1, 0, 0, 0, 1, 0, 0},
    {"pairs_blk nfree=0 defp=1", PK_BLK, 1, 0, 1, 0, 1, 0, 0},
    {"pairs_blk nfree=1 defp=0", PK_BLK, 1, 1, 0, 0, 1, 0, 0},
    {"pairs_blk nfree=1 defp=1", PK_BLK, 1, 1, 1, 0, 1, 0, 0},
    {"split nfree=0 defp=0 mode=0", PK_SPLIT, 1, 0, 0, 0, 1, 2, 0},
    {"split nfree=0 defp=0 mode=1", PK_SPLIT, 1, 0, 0, 0, 1, 2, 1},
    {"split nfree=0 defp=1 mode=0", PK_SPLIT, 1, 0, 1, 0, 1, 2, 0},
    {"split nfree=0 defp=1 mode=1", PK_SPLIT, 1, 0, 1, 0, 1, 2, 1},
    {"split nfree=0 defp=2 mode=0", PK_SPLIT, 1, 0, 2, 0, 1, 2, 0},
    {"split nfree=0 defp=2 mode=1", PK_SPLIT, 1, 0, 2, 0, 1, 2, 1},
    {"split nfree=1 defp=0 mode=0", PK_SPLIT, 1, 1, 0, 0, 1, 2, 0},
    {"split nfree=1 defp=0 mode=1", PK_SPLIT, 1, 1, 0, 0, 1, 2, 1},
    {"split nfree=1 defp=1 mode=0", PK_SPLIT, 1, 1, 1, 0, 1, 2, 0},
    {"split nfree=1 defp=1 mode=1", PK_SPLIT, 1, 1, 1, 0, 1, 2, 1},
    {"split nfree=1 defp=2 mode=0", PK_SPLIT, 1, 1, 2, 0, 1, 2, 0},
    {"split nfree=1 defp=2 mode=1", PK_SPLIT, 1, 1, 2, 0, 1, 2, 1},
    {"rtc nfree=0 cand=0", PK_RTC, 1, 0, 9, 0, 1, 0, 0},
    {"rtc nfree=0 cand=1", PK_RTC, 1, 0, 9, 0, 1, 1, 0},
    {"rtc nfree=0 cand=2", PK_RTC, 1, 0, 9, 0, 1, 2, 0},
    {"rtc nfree=1 cand=0", PK_RTC, 1, 1, 9, 0, 1, 0, 0},
    {"rtc nfree=1 cand=1", PK_RTC, 1, 1, 9, 0, 1, 1, 0},
    {"rtc nfree=1 cand=2", PK_RTC, 1, 1, 9, 0, 1, 2, 0},
};
constexpr int PK_COUNT = (int)(sizeof PAIR_KERNELS / sizeof PAIR_KERNELS[0]);
// the row of an instantiation; -1 = none
constexpr int pk_id(int kind, int fast, int nfree, int defp, int aln, int bk, int cand, int mode)
{
    for (int i = 0; i < PK_COUNT; ++i) {
        const PairKernelDesc& d = PAIR_KERNELS[i];
        if (d.kind == kind && d.fast == fast && d.nfree == nfree && d.defp == defp && d.aln == aln && d.bk == bk && d.cand == cand && d.mode == mode)
            return i;
    }
    return -1;
}
// the rows of the run-time compiled kernel: PK_RTC_N0_C0 + 3 * nfree + cand
constexpr int PK_RTC_N0_C0 = pk_id(PK_RTC, 1, 0, 9, 0, 1, 0, 0);
static_assert(PK_RTC_N0_C0 >= 0 && pk_id(PK_RTC, 1, 0, 9, 0, 1, 2, 0) == PK_RTC_N0_C0 + 2 && pk_id(PK_RTC, 1, 1, 9, 0, 1, 0, 0) == PK_RTC_N0_C0 + 3 &&
              pk_id(PK_RTC, 1, 1, 9, 0, 1, 2, 0) == PK_RTC_N0_C0 + 5, "the rtc rows of PAIR_KERNELS are out of order");

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
    u64 klaunch[PK_COUNT] = {};   // the launch record: launches per pair-kernel instantiation (PAIR_KERNELS)

    RunRecord& operator+=(const RunRecord& o)
    {
        tm.index_ms += o.tm.index_ms; tm.pairs_ms += o.tm.pairs_ms; tm.cand_ms += o.tm.cand_ms; tm.kmers_ms += o.tm.kmers_ms;
        tm.pair_launches += o.tm.pair_launches; tm.index_launches += o.tm.index_launches; tm.cand_launches += o.tm.cand_launches;
        tm.pairs += o.tm.pairs;
        batches += o.batches;
        blk_launches += o.blk_launches; pm_launches += o.pm_launches; lpt_launches += o.lpt_launches; pmfi_launches += o.pmfi_launches;
        split_launches += o.split_launches; split_items += o.split_items; rtc_launches += o.rtc_launches; pmc_launches += o.pmc_launches;
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
    u32 n = 0, n_pending = 0;     // n_pending: genome count while lzani_set_genomes is still at work
    std::vector<int> L;
    std::vector<u64> nmoff;
    int Tmax = 0;
    IndexGeom geo{};
    GenomeTables tab;
    u64 total_nm = 0;
    bool kmers_ready = false;
    bool all_nfree = false;       // no genome holds an N: the NFREE kernel instantiation applies
    // the form of the anchor index, chosen per set (choose_index_form)
    u64 dir_stride = 0, ent_stride = 0;
    u64 bk_stride = 0;            // bucket tables
    u64 tw_stride = 0;            // tag words of the bucket tables (tag bits <= 7)
    u64 fl_stride = 0;            // presence filters: words per slot; 0 = no filter (one all-ones word)
    u32 fmask = 31;
    bool join_mode = false;
    bool sort_build = false;      // sort-based index build (large directories)
    u32 max_slots = 65535;        // gridDim.y limit; LZANI_MAX_SLOTS lowers it (tests force the multi-batch path)
    int blk_fold = -1;            // k_pairs_blk: LDS filter = global filter folded 2^blk_fold times (-1: not decided yet, -2: does not fit)
    JoinLists jl;
    DevMem<unsigned char> d_jtmp; // radix-sort scratch (join lists, the sort-based index build, ticket order)

    // Out-of-core genome sets (lzani_ooc.h): the set stays on the host and the runs go tile by tile over
    // (reference block, query block).  Outside a run n / L describe the whole set; the device tables above then
    // describe the resident region (two halves, A and B, of half_words packed words each).
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
    std::vector<u32> bin_lo;              // the pass plan: pass p holds the bins bin_lo[p] .. bin_lo[p + 1]
    DevMem<u32> kmers_of;                 // |K(g)|
    std::vector<u64> row_off;             // CSR of the kept pairs (n + 1)
    std::vector<PrefilterTile> tiles;     // in row order
    PrefilterWork work;
};

// Residency counters of the last run (lzani_get_residency).
struct Residency { u32 tiles = 0; u64 uploads = 0, peak = 0; double upload_ms = 0; };

struct lzani_ctx {
    // create -> destroy
    Params P;
    int dev = 0;
    hipStream_t stream = nullptr;
    std::vector<hipEvent_t> events;    // four per batch of a run (index begin/end, pairs begin/end)
    int n_cus = 256;
    std::string err;
    hipEvent_t ev_km[2] = {nullptr, nullptr};
    bool km_timed = false;        // the last run made the k-mer words (ev_km holds their stamps)
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
    int pf_counting = LZANI_PF_COUNTING_AUTO;     // lzani_set_prefilter_counting: the accumulator of the later prefilter calls

    GenomeSet gs;
    IndexSlabs sl;
    CandScratch cs;
    Prefilter pf;
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

// Per-genome k-mer words exist for mal, msl <= 15 (the fast path).
bool kmer_words_of(const Params& P) { return P.mal <= 15 && P.msl <= 15; }

// An LZANI_* switch: whether it is set and begins with ch; its number (atoi / strtoull); empty where it is not set.
bool env_is(const char* name, char ch) { const char* v = getenv(name); return v && *v == ch; }
std::optional<bool> env_flag(const char* name) { const char* v = getenv(name); return v ? std::optional<bool>(*v == '1') : std::nullopt; }
std::optional<int> env_int(const char* name) { const char* v = getenv(name); return v ? std::optional<int>(atoi(v)) : std::nullopt; }
std::optional<u64> env_u64(const char* name) { const char* v = getenv(name); return v ? std::optional<u64>(strtoull(v, nullptr, 10)) : std::nullopt; }

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

struct IndexForm { u64 bk_stride, tw_stride; bool join_mode; };

// Bucket table, tag words and the join form of a genome set of n genomes with this geometry (environment overrides
// included): what choose_index_form lays out, and what the block plan of an out-of-core set (lzani_ooc.h) counts.
IndexForm index_form_of(const Params& P, const IndexGeom& geo, u32 n)
{
    IndexForm f;
    int tagbits = 0;
    while (tagbits < 32 && ((geo.tagmask >> tagbits) & 1u)) ++tagbits;
    const bool exact = geo.tagmask == (u32)lowmask(geo.kb - geo.dirbits);
    const int max_dirbits = env_int("LZANI_BK_MAX_DIRBITS").value_or(26);
    // bucket table (+ tag words): wherever the sentinels cannot be real entries; 20 B per bucket more per slot
    // (LZANI_NO_BUCKETS, LZANI_NO_TAGWORDS: experiments / test_index_forms)
    f.bk_stride = (kmer_words_of(P) && exact && geo.dirbits <= max_dirbits && tagbits + geo.posbits <= 30 && !env_is("LZANI_NO_BUCKETS", '1'))
                      ? ((u64)4 << geo.dirbits) : 0;
    f.tw_stride = (f.bk_stride && tagbits <= 7 && !env_is("LZANI_NO_TAGWORDS", '1')) ? ((u64)1 << geo.dirbits) : 0;
    // Join form of candidate detection: where the tag words of one reference exceed what an L2 holds by far, a random
    // probe per query position costs one HBM line each; the query's k-mer list sorted by bucket turns the probes into
    // two streams (DevWave::join).  Needs the anchor queue (tag words, seed window <= 128) and keys of 64 bits.
    const u64 min_bytes = env_u64("LZANI_JOIN_MIN_BYTES").value_or(8ull << 20);
    const int gbits = ceil_log2((u64)n + 1);                          // the all-ones genome number is the invalid key's
    f.join_mode = f.tw_stride && f.tw_stride * 4 >= min_bytes && P.mqd + P.mrd <= 128 &&
                  gbits + geo.kb + geo.posbits <= 64 && !env_is("LZANI_NO_JOIN", '1');
    return f;
}

// The form of the anchor index (bucket table, tag words) is a property of the genome set and the parameters:
// decided once per lzani_set_genomes, so the strides of the slabs never change under an allocation.
void choose_index_form(lzani_ctx* c)
{
    {
        const IndexForm f = index_form_of(c->P, c->gs.geo, c->gs.n_pending);
        c->gs.bk_stride = f.bk_stride;
        c->gs.tw_stride = f.tw_stride;
        c->gs.join_mode = f.join_mode;
    }
    // Sort-based index build where the directory is beyond the LDS-staged build (2^19 buckets): keys of 64 bits with up
    // to 16 bits of slot number (LZANI_SORT_INDEX_MIN_DIRBITS=0, tests: at every size)
    c->gs.sort_build = kmer_words_of(c->P) && c->gs.geo.dirbits >= env_int("LZANI_SORT_INDEX_MIN_DIRBITS").value_or(20) &&
                    c->gs.geo.kb + c->gs.geo.posbits <= 60 && !env_is("LZANI_NO_SORT_INDEX", '1');
    // Presence filter in front of the tag-word probes (probe form only; k_pairs_blk keeps the reference's in LDS): ~3 bits
    // per text position, at most 2^18 bits (genomes up to ~128 kbp); beyond, one all-ones word passes everything
    {
        const int fmax = env_int("LZANI_FILTER_MAX_BITS").value_or(18);      // 2^18 bits = 32 KB of LDS per block of 16 waves
        const int fbits = std::min(ceil_log2((u64)std::max(c->gs.Tmax, 1024)) + 1, fmax);
        const bool on = c->gs.tw_stride && !c->gs.join_mode && ceil_log2((u64)std::max(c->gs.Tmax, 1024)) <= fmax && !env_is("LZANI_NO_FILTER", '1');
        c->gs.fl_stride = on ? ((u64)1 << fbits) / 32 : 0;
        c->gs.blk_fold = -1;
        c->gs.fmask = on ? (u32)((1u << fbits) - 1u) : 31u;
    }
    const int ms = env_int("LZANI_MAX_SLOTS").value_or(0);
    c->gs.max_slots = ms > 0 ? (u32)std::min(65535, ms) : 65535u;
    if (c->gs.sort_build)                                  // the slot number shares the 64-bit key with hash and position
        c->gs.max_slots = (u32)std::min<u64>(c->gs.max_slots, (1ull << std::min(16, 64 - c->gs.geo.kb - c->gs.geo.posbits)) - 1);
}

// The bytes of one index slab slot of the set (lzani_run_plan.h): the tables, and the keys of the sort-based build.
SlabBytes slot_bytes(const GenomeSet& gs)
{
    return slab_bytes_per_slot(gs.dir_stride, gs.ent_stride, gs.bk_stride, gs.tw_stride, gs.fl_stride, gs.sort_build, (u64)gs.Tmax);
}

int ensure_slabs(lzani_ctx* c, u32 want_rows)
{
    const size_t per_slot = (size_t)slot_bytes(c->gs).total();
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    size_t have = c->sl.slots * per_slot;
    size_t budget = (size_t)((free_b + have) * 0.6);
    u32 slots = (u32)std::min<size_t>(std::min<u32>(want_rows, c->gs.max_slots), std::max<size_t>(1, budget / per_slot));
    if (slots <= c->sl.slots) return LZANI_OK;
    c->sl = IndexSlabs{};                              // released first: two generations need not fit
    IndexSlabs s;
    HIPCHK(c, s.d_dirz.alloc((size_t)slots * c->gs.dir_stride));
    HIPCHK(c, s.d_ent.alloc((size_t)slots * c->gs.ent_stride));
    if (c->gs.bk_stride) HIPCHK(c, s.d_bk.alloc((size_t)slots * c->gs.bk_stride));
    if (c->gs.tw_stride) HIPCHK(c, s.d_tw.alloc((size_t)slots * c->gs.tw_stride));
    if (c->gs.tw_stride) {
        HIPCHK(c, s.d_fl.alloc((size_t)slots * c->gs.fl_stride));
        if (!c->gs.fl_stride) HIPCHK(c, hipMemset(s.d_fl, 0xFF, 4));
    }
    HIPCHK(c, s.d_status.alloc(slots));
    if (c->gs.sort_build) {
        HIPCHK(c, s.d_ikeys_in.alloc((size_t)slots * c->gs.Tmax));
        HIPCHK(c, s.d_ikeys.alloc((size_t)slots * c->gs.Tmax));
        HIPCHK(c, s.d_icnt.alloc(slots));
        HIPCHK(c, s.d_ibase.alloc(slots));
    }
    s.slots = slots;
    c->sl = std::move(s);
    return LZANI_OK;
}

GenomeTab gtab(const lzani_ctx* c)
{
    const GenomeTables& t = c->gs.tab;
    return GenomeTab{t.t2, t.nm, t.nmoff, t.L, t.kmL, t.kmS, t.hasN};
}

// Join form: the k-mer list of every genome as a query, sorted by (genome, bucket) -- k_join_keys + the radix sort of lzani_sort.hip,
// once per run, behind k_kmers (it is part of the path's work like the k-mer words it is made from).
// the resident part of the join lists (the sorted keys: 8 B per forward position), allocated before the index slabs are
// sized so that those see what is really left
int alloc_join_lists(lzani_ctx* c)
{
    const u32 n = c->gs.n;
    if (c->gs.jl.keys) return LZANI_OK;
    JoinLists jl;                                        // (moved into the set whole, or not at all)
    jl.h_koff.assign((size_t)n + 1, 0);
    for (u32 g = 0; g < n; ++g) jl.h_koff[g + 1] = jl.h_koff[g] + (u64)c->gs.L[g];
    HIPCHK(c, jl.koff.alloc((size_t)n + 1));
    HIPCHK(c, jl.soff.alloc((size_t)n + 1));
    HIPCHK(c, jl.cnt.alloc(n));
    HIPCHK(c, jl.keys.alloc(jl.h_koff[n]));
    HIPCHK(c, hipMemcpyAsync(jl.koff, jl.h_koff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    c->gs.jl = std::move(jl);
    return LZANI_OK;
}

int build_join_lists(lzani_ctx* c)
{
    const u32 n = c->gs.n;
    int rc0 = alloc_join_lists(c);
    if (rc0) return rc0;
    // the unsorted keys live for the duration of the sort only (as much again as the lists themselves)
    DevMem<unsigned long long> keys_in;
    HIPCHK(c, keys_in.alloc(c->gs.jl.h_koff[n]));
    int Lmax = 0;
    for (u32 g = 0; g < n; ++g) Lmax = std::max(Lmax, c->gs.L[g]);
    // An invalid key is all ones; the sort looks at the bits [posbits, shift_g + gbits) only, so no real genome number may
    // be all ones in gbits bits, or its keys with the all-ones hash would be indistinguishable from the invalid keys of
    // the genomes before it (found by the fuzz at n = 4: genome 3 lost the k-mers of its last bucket)
    const int shift_g = c->gs.geo.kb + c->gs.geo.posbits, gbits = ceil_log2((u64)n + 1);
    HIPCHK(c, hipMemsetAsync(c->gs.jl.cnt, 0, (size_t)n * 4, c->stream));
    for (u32 g0 = 0; g0 < n && Lmax > 0; g0 += 32768) {
        const u32 cnt = std::min<u32>(32768, n - g0);
        GenomeTab G = gtab(c);
        G.nmoff += g0; G.L += g0;
        // (the genome number of the key is global: the kernel adds g0 through the offset tables it is given)
        hipLaunchKernelGGL(k_join_keys, dim3((Lmax + 4095) / 4096, cnt), dim3(256), 0, c->stream, G, c->gs.jl.koff + g0, keys_in,
                           c->gs.jl.cnt + g0, shift_g, c->gs.geo.posbits, Lmax, g0);
    }
    HIPCHK(c, hipGetLastError());
    std::vector<u32> valid(n);
    HIPCHK(c, hipMemcpyAsync(valid.data(), c->gs.jl.cnt, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // sort in groups of whole genomes below 2^30 keys; invalid keys (all ones) end up behind the group's valid ones
    std::vector<u64> soff((size_t)n + 1, 0);
    for (u32 g0 = 0; g0 < n;) {
        u32 g1 = g0;
        u64 keys = 0;
        while (g1 < n && (g1 == g0 || keys + (u64)c->gs.L[g1] <= (1ull << 30))) keys += (u64)c->gs.L[g1++];
        if (keys > 0x7FFFFFF0ull) return fail(c, LZANI_ERR_ARG, "join lists: a genome of more than 2^31 positions");
        u64 at = c->gs.jl.h_koff[g0];
        for (u32 g = g0; g < g1; ++g) { soff[g] = at; at += valid[g]; }
        if (g1 == n) soff[n] = at;
        if (keys)
            if (int rc = sort_keys(c, c->gs.d_jtmp, keys_in + c->gs.jl.h_koff[g0], c->gs.jl.keys + c->gs.jl.h_koff[g0], keys, 1, c->gs.geo.posbits, shift_g + gbits,
                                   "join lists: radix sort", false))
                return rc;
        g0 = g1;
    }
    // (a genome's list ends after its valid keys -- d_jcnt -- not where the next list begins: between two groups sit the
    // invalid keys of the first)
    HIPCHK(c, hipMemcpyAsync(c->gs.jl.soff, soff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));        // (before keys_in is released)
    c->run.tm.index_launches += 2;
    return LZANI_OK;
}

// Per-genome k-mer words (and, for long genomes, the sorted join lists made from them): once per genome set, by the
// first run after lzani_set_genomes -- before its index slabs are sized, so that the slabs see what the lists and the
// sort's temporaries have left -- and kept for the runs that follow (they depend on the genomes and the parameters
// only).  Timed on their own (lzani_timing.kmers_ms).
int ensure_kmers(lzani_ctx* c)
{
    if (!c->gs.tab.kmL || c->gs.kmers_ready) return LZANI_OK;
    HIPCHK(c, hipEventRecord(c->ev_km[0], c->stream));
    for (u32 g0 = 0; g0 < c->gs.n; g0 += 32768) {
        u32 cnt = std::min<u32>(32768, c->gs.n - g0);
        GenomeTab G = gtab(c);
        G.nmoff += g0; G.L += g0;
        hipLaunchKernelGGL(k_kmers, dim3((c->gs.Tmax + 255) / 256, cnt), dim3(256), 0, c->stream,
                           G, c->gs.tab.kmL, c->gs.tab.kmS, c->P.mal, c->P.msl, c->P.mrd, c->gs.Tmax);
    }
    HIPCHK(c, hipGetLastError());
    c->run.tm.index_launches += 1;
    HIPCHK(c, hipEventRecord(c->ev_km[1], c->stream));
    c->gs.kmers_ready = true;
    c->km_timed = true;
    return LZANI_OK;
}

// The sorted join lists of a long-genome set (join form of candidate detection): made by the first run that needs them
// -- dense rows take their candidates from the presence matrix instead -- and kept like the k-mer words they are made
// from; their time is part of that run's kmers_ms.
int ensure_join(lzani_ctx* c)
{
    if (!c->gs.join_mode || c->gs.jl.ready) return LZANI_OK;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPCHK(c, hipEventCreate(&e0));
    hipError_t e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipEventRecord(e0, c->stream);
    int rc = e == hipSuccess ? build_join_lists(c) : fail(c, LZANI_ERR_DEVICE, std::string("join lists: ") + hipGetErrorString(e));
    if (rc == LZANI_OK) {
        float ms = 0;
        if (hipEventRecord(e1, c->stream) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess)
            c->join_ms_pending = ms;
        c->gs.jl.ready = true;
    }
    hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    return rc;
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
    bool lds_index = !env_is("LZANI_NO_LDS_INDEX", '1');
    int lds_index_max_dirbits = env_int("LZANI_LDS_INDEX_MAX_DIRBITS").value_or(19);
};

// Index build of `rows` references (device list d_ref_ids) into slots 0..rows-1.
// with_tw = false: the sort-based build leaves the tag words out (a batch whose pairs read candidate bitmaps never probes them:
// 8.6 GB less to write per 128 x 5 Mbp references)
int build_indexes(lzani_ctx* c, const Knobs& k, const u32* d_ref_ids, u32 rows, bool with_filter = true, bool with_tw = true)
{
    IdxArgs ia;
    ia.G = gtab(c);
    ia.ref_ids = d_ref_ids;
    ia.dirz = c->sl.d_dirz; ia.ent = c->sl.d_ent;
    ia.dir_stride = c->gs.dir_stride; ia.ent_stride = c->gs.ent_stride;
    ia.mal = c->P.mal; ia.mrd = c->P.mrd; ia.geo = c->gs.geo; ia.todo = nullptr;
    const u32 nb = 1u << c->gs.geo.dirbits;
    { int rc = ensure_kmers(c); if (rc) return rc; }
    if (c->gs.fl_stride && with_filter) {              // (only the block kernel reads it)
        HIPCHK(c, hipMemsetAsync(c->sl.d_fl, 0, (size_t)rows * c->gs.fl_stride * 4, c->stream));
        hipLaunchKernelGGL(k_idx_filter, dim3((u32)std::min<u64>(((u64)c->gs.Tmax + 255) / 256, 64), rows), dim3(256), 0, c->stream,
                           ia, c->sl.d_fl, c->gs.fl_stride, c->gs.fmask, c->gs.Tmax);
        c->run.tm.index_launches += 1;
    }
    if (c->gs.sort_build) {
        c->sl.index_build = LZANI_INDEX_BUILD_SORT;
        // keys -> radix sort, every slot a segment of its own (lzani_sort.hip) -> the tables in one streaming pass.  A key is
        // hash || position; a position without a k-mer is all ones and sorts behind the slot's keys by the one bit above the hash.
        const int shift_slot = c->gs.geo.kb + c->gs.geo.posbits;
        const u64 Tm = (u64)c->gs.Tmax;
        const u32 group = 1;
        HIPCHK(c, hipMemsetAsync(c->sl.d_icnt, 0, (size_t)rows * 4, c->stream));
        hipLaunchKernelGGL(k_idx_keys, dim3((u32)((Tm + 4095) / 4096), rows), dim3(256), 0, c->stream, ia, c->sl.d_ikeys_in, c->sl.d_icnt, c->gs.Tmax, shift_slot);
        if (int rc = sort_keys(c, c->gs.d_jtmp, c->sl.d_ikeys_in, c->sl.d_ikeys, Tm, rows, c->gs.geo.posbits, shift_slot + 1, "index build: radix sort", true)) return rc;
        hipLaunchKernelGGL(k_idx_base, dim3((rows + 255) / 256), dim3(256), 0, c->stream, c->sl.d_icnt, c->sl.d_ibase, rows, group, Tm);
        hipLaunchKernelGGL(k_idx_from_sorted, dim3((u32)std::min<u64>((Tm + 255) / 256, 8192), rows), dim3(256), 0, c->stream,
                           ia, c->sl.d_ikeys, c->sl.d_icnt, c->sl.d_ibase, c->sl.d_bk, with_tw ? c->sl.d_tw : nullptr, c->gs.bk_stride, c->gs.tw_stride);
        HIPCHK(c, hipGetLastError());
        c->run.tm.index_launches += 4;
        return LZANI_OK;
    }
    const bool lds_build = c->gs.tab.kmL && c->gs.geo.dirbits <= k.lds_index_max_dirbits && k.lds_index;
    c->sl.index_build = lds_build ? LZANI_INDEX_BUILD_LDS : LZANI_INDEX_BUILD_ATOMICS;
    // blocks per slot of the global-atomics kernels: the whole range when they build every slot, a handful when
    // they only pick up what k_idx_build left (usually nothing)
    const u32 gx_pos = lds_build ? 16u : (u32)((c->gs.Tmax + 255) / 256), gx_bkt = lds_build ? 16u : (nb + 255) / 256;
    dim3 gp(gx_pos, rows);
    if (lds_build) {
        // one block per reference, everything through LDS; a slot that does not fit (status != 0) falls through
        // to the global-atomics kernels below, which skip every other slot
        const size_t lds = (size_t)(IDX_RANGE / 2 + IDX_STAGE) * 4;
        { int rc = raise_lds(c, k_idx_build, lds); if (rc) return rc; }
        HIPCHK(c, hipMemsetAsync(c->sl.d_status, 0, (size_t)rows * 4, c->stream));
        hipLaunchKernelGGL(k_idx_build, dim3(rows), dim3(1024), lds, c->stream, ia, c->sl.d_bk, c->sl.d_tw, c->gs.bk_stride, c->gs.tw_stride, c->sl.d_status);
        ia.todo = c->sl.d_status;
        hipLaunchKernelGGL(k_idx_zero, dim3(gx_bkt, rows), dim3(256), 0, c->stream, c->sl.d_dirz, c->gs.dir_stride, nb, ia.todo);
    } else HIPCHK(c, hipMemsetAsync(c->sl.d_dirz, 0, (size_t)rows * c->gs.dir_stride * 4, c->stream));
    hipLaunchKernelGGL(k_idx_count, gp, dim3(256), 0, c->stream, ia, c->gs.Tmax);
    hipLaunchKernelGGL(k_idx_scan, dim3(rows), dim3(1024), 0, c->stream, c->sl.d_dirz, c->gs.dir_stride, nb, ia.todo);
    hipLaunchKernelGGL(k_idx_fill, gp, dim3(256), 0, c->stream, ia, c->gs.Tmax);
    hipLaunchKernelGGL(k_idx_sort, dim3(gx_bkt, rows), dim3(256), 0, c->stream,
                       c->sl.d_dirz, c->sl.d_ent, c->gs.dir_stride, c->gs.ent_stride, nb, ia.todo, 0);
    if (c->sl.d_bk)
        hipLaunchKernelGGL(k_idx_buckets, dim3(gx_bkt, rows), dim3(256), 0, c->stream,
                           c->sl.d_dirz, c->sl.d_ent, c->sl.d_bk, c->sl.d_tw, c->gs.dir_stride, c->gs.ent_stride, c->gs.bk_stride, c->gs.tw_stride,
                           nb, c->gs.geo.posbits, ia.todo);
    HIPCHK(c, hipGetLastError());
    c->run.tm.index_launches += 4;
    return LZANI_OK;
}

struct RegionSink { lzani_region* d_regions; unsigned long long* d_count; unsigned long long capacity; };

// The tuples the pair kernels fold into their code ahead of time: 1 = the defaults, 2 = the long-genome parameters
// (--mal 15 --msl 9 --reg 60, BASELINE configs[3]; the hand-written null chain included, bitmap, join and split forms),
// 0 = any other (the generic kernel, or one compiled at run time).
int defp_select(const Params& q)
{
    if (q.mrd != 40 || q.mqd != 40 || q.aw != 15 || q.am != 7 || q.ar != 3) return 0;
    return (q.mal == 11 && q.msl == 7 && q.reg == 35) ? 1 : (q.mal == 15 && q.msl == 9 && q.reg == 60) ? 2 : 0;
}

// The pair kernels of one form for the run-time (nfree, dsel): f(NFREE, DEFP) with both as std::integral_constant.  The forms
// with ND = 3 have an instantiation per dsel; those with ND = 2 none for the long-genome tuple, which runs their DEFP 0.
template <int ND, class F>
void with_nfree_defp(bool nf, int dsel, F&& f)
{
    auto by_defp = [&](auto N) {
        if (dsel == 1) f(N, std::integral_constant<int, 1>{});
        else if (dsel == 2) f(N, std::integral_constant<int, ND == 3 ? 2 : 0>{});
        else f(N, std::integral_constant<int, 0>{});
    };
    if (nf) by_defp(std::true_type{}); else by_defp(std::false_type{});
}

// One launch in the launch record; a launch of an instantiation without a row in PAIR_KERNELS does not compile.
template <int KIND, int F, int N, int D, int A, int B, int C, int M = 0>
void count_launch(RunRecord& r)
{
    constexpr int id = pk_id(KIND, F, N, D, A, B, C, M);
    static_assert(id >= 0, "a pair kernel without a row in PAIR_KERNELS");
    r.klaunch[id] += 1;
}

template <bool F, bool N, int D, bool A, bool B, int C>
void launch_k_pairs(lzani_ctx* c, dim3 gd, dim3 bd, const PairArgs& pa)
{
    hipLaunchKernelGGL((k_pairs<F, N, D, A, B, C>), gd, bd, 0, c->stream, pa);
    count_launch<PK_PAIRS, F, N, D, A, B, C>(c->run);
}

// What a run's rows hold beyond their checks: the pairs and, for query lists, whether a row names a query twice and how
// many queries the groups of PM_GROUP consecutive rows involve (what the candidate form goes by).
struct RowFacts { u64 n_pairs = 0; bool lists_dup = false; u64 lists_involved = 0; };

// The checks of a run's rows (n_rows > 0) against the genome set; the query ids in one pass.
int check_rows(lzani_ctx* c, u32 n_rows, const u32* ref_ids, const u64* row_off, const u32* query_ids, RowFacts& f)
{
    for (u32 k = 0; k < n_rows; ++k) {
        if (ref_ids[k] >= c->gs.n) return fail(c, LZANI_ERR_ARG, "lzani_run_rows: reference id out of range");
        if (row_off[k + 1] < row_off[k]) return fail(c, LZANI_ERR_ARG, "lzani_run_rows: row_off not monotone");
        if (!query_ids && row_off[k + 1] - row_off[k] != (u64)c->gs.n - 1)
            return fail(c, LZANI_ERR_ARG, "lzani_run_rows: dense row must have n-1 queries");
    }
    if (row_off[0] != 0) return fail(c, LZANI_ERR_ARG, "lzani_run_rows: row_off[0] must be 0");
    f.n_pairs = row_off[n_rows];
    if (query_ids) {
        std::vector<u32> in_row(c->gs.n, 0xFFFFFFFFu), in_group(c->gs.n, 0xFFFFFFFFu);
        for (u32 k = 0; k < n_rows; ++k)
            for (u64 e = row_off[k]; e < row_off[k + 1]; ++e) {
                const u32 q = query_ids[e];
                if (q >= c->gs.n) return fail(c, LZANI_ERR_ARG, "lzani_run_rows: query id out of range");
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
    const Knobs& k;
    const RunPlan& p;
    const RegionSink* rs; const u64* row_off; const u32* query_ids; int* d_out;     // the call's arguments
    const u32 *d_ref, *d_q, *d_qorder;                       // their device copies, the queues
    const u64 *d_off, *d_qcum;
    u32 max_blocks; int dsel;                                // the launch geometry, defp_select of the tuple
    unsigned long long* d_cbits;                             // join form: one candidate bitmap per resident wave
    u64 cbits_stride;
    lzani_rtc::Kernel* rtc_k; int rtc_id;                    // the tuple's run-time compiled kernel, if any, and its row of the launch record
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
int plan_run(lzani_ctx* c, const Knobs& k, const RowFacts& f, u32 n_rows, const u64* row_off, bool lists, bool regions, RunPlan& p)
{
    for (u32 g = 0; g < c->gs.n; ++g) p.Lmax = std::max(p.Lmax, c->gs.L[g]);
    // rows of the presence matrix: one per k-mer (exact: the mixer is a bijection on the key bits) where the genomes fill a fair
    // part of the key space, else the hash's top bits -- 2^9 rows per text position keep the false candidates below 0.2 % of the
    // query positions, and a group's matrix is cleared and built in proportion to the genomes, not to 4^mal
    p.pm_bits = std::min(std::min(c->gs.geo.kb, 30), ceil_log2((u64)std::max(c->gs.Tmax, 1)) + 9);
    int rc = plan_bitmaps(c, k, f, n_rows, row_off, lists, regions, p);
    if (rc || p.pm) return rc;
    p.use_join = c->gs.join_mode;
    if (p.use_join) { rc = ensure_join(c); if (rc) return rc; }          // (before the slabs are sized: they take 60 % of what is left)
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
            const size_t l = (size_t)(BLK_WAVES * SEED_LDS_WORDS + std::max<u64>(c->gs.fl_stride >> fold, 1)) * 4;
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

// The batch's pair launch: the run's form picks the kernel, (nfree, dsel) its template arguments; a tuple compiled at run
// time goes first where it has a kernel of the form.
int launch_pairs(RunCtx& r, const Batch& bt, bool blk_rows, hipEvent_t* ev)
{
    lzani_ctx* c = r.c;
    const bool tickets = bt.lpt && bt.split_S < 2;
    PairArgs pa;
    pa.G = gtab(c);
    pa.P = c->P; pa.geo = c->gs.geo;
    pa.dirz = c->sl.d_dirz; pa.ent = c->sl.d_ent;
    pa.dir_stride = c->gs.dir_stride; pa.ent_stride = c->gs.ent_stride;
    pa.bk = c->sl.d_bk; pa.bk_stride = c->gs.bk_stride;
    pa.tw = c->sl.d_tw; pa.tw_stride = c->gs.tw_stride;
    pa.fl = c->sl.d_fl; pa.fl_stride = c->gs.fl_stride; pa.fmask = c->gs.fmask;
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
    const bool fast = c->gs.tab.kmL != nullptr, tw = pa.tw != nullptr, nf = c->gs.all_nfree;
    auto rtc_launch = [&]() -> bool {
        if (!r.rtc_k) return false;
        void* kargs[] = {&pa};
        if (hipModuleLaunchKernel(r.rtc_k->fn, gd.x, 1, 1, bd.x, 1, 1, 0, c->stream, kargs, nullptr) != hipSuccess) { (void)hipGetLastError(); return false; }
        c->run.rtc_launches += 1;
        c->run.klaunch[r.rtc_id] += 1;
        return true;
    };
    // Probe form, dense rows of hundreds of pairs: blocks of 16 waves with the reference's presence filter in LDS
    // (k_pairs_blk).  The rows a kmer-db filter leaves hold related pairs, where most positions pass the filter:
    // BASELINE configs[4] at full size is 6 % slower this way; LZANI_BLOCK_KERNEL=1/0 overrides.
    const void* kf = nullptr;
    with_nfree_defp<2>(nf, r.dsel, [&](auto N, auto D) { kf = reinterpret_cast<const void*>(k_pairs_blk<N, D>); });
    const bool use_blk = blk_rows && fast && tw && !pa.skeys && blk_fits(c, kf);
    if (use_blk && !c->d_blkctr) HIPCHK(c, c->d_blkctr.alloc((size_t)c->n_cus * 2));
    int rc = LZANI_OK;
    if (r.rs) {                                   // alignment output: one generic instantiation per index form
        if (!fast) launch_k_pairs<false, false, 0, true, false, 0>(c, gd, bd, pa);
        else if (tw) launch_k_pairs<true, false, 0, true, true, 0>(c, gd, bd, pa);
        else launch_k_pairs<true, false, 0, true, false, 0>(c, gd, bd, pa);
    } else if (!fast) launch_k_pairs<false, false, 0, false, false, 0>(c, gd, bd, pa);
    else if (r.p.pm && bt.split_S >= 2) {            // few, long pairs: several waves a pair
        rc = run_split(r, bt, pa, [&](SplitArgs& sa, int mode, u32 items) {
            const dim3 gs((u32)std::min<u64>(((u64)items + 3) / 4, r.max_blocks)), bs4(256);
            sa.n_work = items;
            with_nfree_defp<3>(nf, r.dsel, [&](auto N, auto D) {
                if (mode == 0) { hipLaunchKernelGGL((k_split<N, D, 0>), gs, bs4, 0, c->stream, sa); count_launch<PK_SPLIT, true, N, D, false, true, 2, 0>(c->run); }
                else { hipLaunchKernelGGL((k_split<N, D, 1>), gs, bs4, 0, c->stream, sa); count_launch<PK_SPLIT, true, N, D, false, true, 2, 1>(c->run); }
            });
        });
    } else if (r.p.pm) {                          // dense rows: candidate bitmaps made ahead (k_pm_cand)
        c->run.pm_launches += 1;
        if (!rtc_launch()) with_nfree_defp<3>(nf, r.dsel, [&](auto N, auto D) { launch_k_pairs<true, N, D, false, true, 2>(c, gd, bd, pa); });
    } else if (tw && pa.skeys) {                  // long genomes: candidates by the join
        if (!rtc_launch()) with_nfree_defp<3>(nf, r.dsel, [&](auto N, auto D) { launch_k_pairs<true, N, D, false, true, 1>(c, gd, bd, pa); });
    } else if (use_blk) {
        const u32 fw = (u32)std::max<u64>(c->gs.fl_stride >> c->gs.blk_fold, 1);
        const size_t lds = (size_t)(BLK_WAVES * SEED_LDS_WORDS + fw) * 4;
        rc = raise_lds(c, kf, lds);              // (a no-op after blk_fits, which recorded the fold it settled on)
        if (rc) return rc;
        pa.fmask = c->gs.fmask >> c->gs.blk_fold;
        c->run.blk_launches += 1;
        const dim3 gb((u32)std::min<u64>((waves + BLK_CHUNK_MIN - 1) / BLK_CHUNK_MIN, (u64)c->n_cus * 2)), bb(64 * BLK_WAVES);
        with_nfree_defp<2>(nf, r.dsel, [&](auto N, auto D) {
            hipLaunchKernelGGL((k_pairs_blk<N, D>), gb, bb, lds, c->stream, pa, fw, (u32)c->gs.blk_fold, c->d_blkctr);
            count_launch<PK_BLK, true, N, D, false, true, 0>(c->run);
        });
    } else if (tw) {
        if (!rtc_launch()) with_nfree_defp<2>(nf, r.dsel, [&](auto N, auto D) { launch_k_pairs<true, N, D, false, true, 0>(c, gd, bd, pa); });
    } else with_nfree_defp<2>(nf, r.dsel, [&](auto N, auto D) { launch_k_pairs<true, N, D, false, false, 0>(c, gd, bd, pa); });
    if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev[3], c->stream));
    return LZANI_OK;
}

constexpr int EV = 5;                             // stamps per batch: index begin / end, pairs begin / end, candidates end

// One batch: index build, split / LPT choice, candidate stage, pair launch -- stream work only, stamped into ev.
int run_batch(RunCtx& r, Batch bt, hipEvent_t* ev)
{
    lzani_ctx* c = r.c;
    const RunPlan& p = r.p;
    TRACE("batch %u rows [%u,%u) pairs [%llu,%llu) slots=%u pm=%d", bt.b, bt.k0, bt.k0 + bt.rows, (unsigned long long)bt.e0, (unsigned long long)bt.e1, c->sl.slots, (int)p.pm);
    HIPCHK(c, hipEventRecord(ev[0], c->stream));
    // rows for k_pairs_blk (launch_pairs): dense, hundreds of pairs each, probe form with tag words and a filter
    const bool blk_rows = !p.pm && !r.rs && c->gs.tab.kmL && c->gs.tw_stride && !c->gs.join_mode && c->gs.fl_stride && bt.e1 > bt.e0 &&
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
        const char* nm[24] = {"find_event calls", "fe: seed straight from the chain's round", "fe: common call, plain candidate", "fe: light rounds", "fe: light round hit",
                              "fe: light round without a hit", "fe: merge loop hit", "fe: jump to a plain candidate", "stretch calls", "stretch: not applicable",
                              "stretch: no seed step", "stretch: anchor before the seed", "stretch: seed event", "stretch: ... with the masks", "stretch: sum of seed steps",
                              "refills", "chain: nothing", "chain: round done", "chain: event found", "chain: seed event known", "events", "close events", "extension chunks", "stretch chain: events committed"};
        fprintf(stderr, "[lzani paths] pairs=%llu, per pair:", (unsigned long long)n_pairs);
        for (int k = 0; k < 24; ++k) fprintf(stderr, " %s=%.1f;", nm[k], (double)acc[k] / (double)n_pairs);
        const char* wn[12] = {"-", "text end", "no seed step", "several window positions", "seed bounds", "match of 64+", "anchor before the seed", "tag in two slots / overflow",
                              "anchor elsewhere", "extension runs on", "-", "-"};
        fprintf(stderr, "\n[lzani paths] stretch chain exits per pair:");
        for (int k = 1; k < 10; ++k) fprintf(stderr, " %s=%.1f;", wn[k], (double)acc[24 + k] / (double)n_pairs);
        fprintf(stderr, "\n");
        HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(g_path_stats), z, sizeof z));
    }
#endif
#ifdef LZANI_CHAIN_STATS
    {
        unsigned long long acc[24], z[24] = {0};
        HIPCHK(c, hipMemcpyFromSymbol(acc, HIP_SYMBOL(g_chain_stats), sizeof acc));
        const char* nm[8] = {"chain_calls", "commits", "exit_nothing", "exit_seed", "exit_not_plain", "exit_event", "events_general", "refills"};
        fprintf(stderr, "[lzani chain] pairs=%llu per pair:", (unsigned long long)n_pairs);
        for (int k = 0; k < 8; ++k) fprintf(stderr, " %s=%.1f", nm[k], (double)acc[k] / (double)n_pairs);
        fprintf(stderr, "\n[lzani chain] wave cycles per pair: after exit_nothing=%.0f after round_done=%.0f after exit_event=%.0f inside the chain=%.0f\n",
                (double)acc[8] / (double)n_pairs, (double)acc[9] / (double)n_pairs, (double)acc[10] / (double)n_pairs, (double)acc[11] / (double)n_pairs);
        fprintf(stderr, "[lzani chain] events found but not null, per pair: close=%.1f region kept or none open=%.1f no forward record=%.1f backward side=%.1f\n",
                (double)acc[12] / (double)n_pairs, (double)acc[13] / (double)n_pairs, (double)acc[14] / (double)n_pairs, (double)acc[15] / (double)n_pairs);
        fprintf(stderr, "[lzani chain] exit_seed by the test that handed the round back, per pair: anchor's own step=%.1f no window position=%.1f several=%.1f text end=%.1f long seed=%.1f other=%.1f; event known, commit left=%.1f\n",
                (double)acc[16] / (double)n_pairs, (double)acc[17] / (double)n_pairs, (double)acc[18] / (double)n_pairs, (double)acc[19] / (double)n_pairs,
                (double)acc[20] / (double)n_pairs, (double)acc[21] / (double)n_pairs, (double)acc[22] / (double)n_pairs);
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
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev_km[0], c->ev_km[1]));
        tm.kmers_ms = ms;
    }
    tm.kmers_ms += c->join_ms_pending;
    c->join_ms_pending = 0;
    for (size_t b = 0; b + 1 < bstart.size(); ++b) {
        hipEvent_t* ev = c->events.data() + (size_t)EV * b;
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

// A run of rows on the resident genome set: check, plan, queues and uploads, then the batches back to back on the stream,
// then one wait.
int run_rows_impl(lzani_ctx* c, u32 n_rows, const u32* ref_ids, const u64* row_off, const u32* query_ids,
                  int* d_out, const RegionSink* rs = nullptr, CandSink* sink = nullptr, RunPlan* plan_out = nullptr)
{
    if (!c->gs.n) return fail(c, LZANI_ERR_STATE, "lzani_run_rows: no genomes set");
    c->run = RunRecord{};
    const Knobs k{};
    if (n_rows == 0) return LZANI_OK;
    RowFacts rf;
    int rc = check_rows(c, n_rows, ref_ids, row_off, query_ids, rf);
    const u64 n_pairs = rf.n_pairs;
    if (rc || n_pairs == 0) return rc;

    HIPCHK(c, hipSetDevice(c->dev));
    // (the k-mer words and the join lists are made by the first run after lzani_set_genomes -- inside its timed index
    // stage, reported as kmers_ms -- and kept: they depend on the genome set and the parameters only)
    c->km_timed = false;
    rc = ensure_kmers(c);
    if (rc) return rc;
    RunPlan p;
    rc = plan_run(c, k, rf, n_rows, row_off, query_ids != nullptr, rs != nullptr, p);
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
        hipEvent_t e;
        HIPCHK(c, hipEventCreate(&e));
        c->events.push_back(e);
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
    const int dsel = defp_select(c->P), cand = p.pm ? 2 : (p.use_join && c->sl.d_tw) ? 1 : c->sl.d_tw ? 0 : -1;
    const int rtc_id = PK_RTC_N0_C0 + 3 * (int)c->gs.all_nfree + cand;      // (its row of the launch record)
    lzani_rtc::Kernel* rtc_k = nullptr;
    c->pairs_seen += n_pairs;
    if (!dsel && !rs && c->gs.tab.kmL && c->sl.d_bk && lzani_rtc::enabled() && cand >= 0) {
        rtc_k = lzani_rtc::get(c->rtc, c->P, c->gs.all_nfree, cand, c->arch.c_str(), c->pairs_seen >= k.rtc_min_pairs);
        if (!rtc_k && c->rtc.failed) TRACE("run-time compile unavailable (%s): the generic kernel runs", c->rtc.log.c_str());
    }

    RunCtx r{c, k, p, rs, row_off, query_ids, d_out, d_ref, d_q, d_qorder, d_off, d_qcum, max_blocks, dsel, d_cbits, cbits_stride, rtc_k, rtc_id};
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
#include "lzani_prefilter.h"

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
    Params P{p->min_anchor_len, p->min_seed_len, p->max_dist_in_ref, p->max_dist_in_query,
             p->min_region_len, p->approx_window, p->approx_mismatches, p->approx_run_len};
    if (!params_supported(P)) return LZANI_ERR_PARAMS;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return LZANI_ERR_DEVICE;
    lzani_ctx* c = new (std::nothrow) lzani_ctx();
    if (!c) return LZANI_ERR_NOMEM;
    c->P = P;
    c->dev = device_id;
    bool ok = hipSetDevice(device_id) == hipSuccess && hipStreamCreate(&c->stream) == hipSuccess &&
              c->d_cursor.alloc(NQUEUES) == hipSuccess;
    if (ok) ok = hipEventCreate(&c->ev_km[0]) == hipSuccess && hipEventCreate(&c->ev_km[1]) == hipSuccess;
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
    for (auto& e : c->events) if (e) hipEventDestroy(e);
    for (auto& e : c->ev_km) if (e) hipEventDestroy(e);
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
    c->gs.n_pending = n;
    choose_index_form(c);
    // Residency: the whole set in HBM (step (b) below, on every genome), or blocks of it kept on the host and uploaded by
    // the runs (lzani_ooc.h).  Automatic mode (limit 0) keeps every set in-core that can be had in-core: its tables, the
    // staging copy and one index slab within the free memory.
    {
        const bool kmers = kmer_words_of(c->P);
        u64 limit = c->mem_req;
        if (!limit) {
            size_t free_b = 0, total_b = 0;
            HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
            if (const char* fb = getenv("LZANI_FREE_BYTES")) free_b = std::min<size_t>(free_b, (size_t)strtoull(fb, nullptr, 10));   // tests: the automatic trigger
            const u64 tables = total_nm * (16 + 8) + (kmers ? total_nm * 64 * 8 : 0);
            const u64 per_slot = slot_bytes(c->gs).total();
            if (tables + total_codes > free_b || tables + per_slot > free_b) limit = free_b / 2;     // (half for the genomes, half for slabs and bitmaps)
        }
        std::vector<u64> bytes;
        std::string msg;
        const int nb = plan_blocks_impl(n, len, c->P, limit, c->gs.blk_first, bytes, msg);
        if (nb < 0) return fail(c, c->mem_req ? nb : LZANI_ERR_NOMEM, "lzani_set_genomes: " + msg);
        if (nb > 1) {
            c->gs.blk_bytes = bytes;
            c->gs.mem_limit = limit;
            return ooc_set_genomes(c, n, codes, len);
        }
        c->gs.mem_limit = c->mem_req;
        c->res.peak = bytes[0];
        c->gs.blk_first.clear();
    }

    DevMem<uint8_t> d_codes;
    DevMem<u64> d_codeoff;
    HIPCHK(c, d_codes.alloc(total_codes));
    HIPCHK(c, d_codeoff.alloc(n));
    {
        GenomeTables t;                                       // (moved into the set whole, or not at all)
        HIPCHK(c, t.t2.alloc(total_nm * 2));
        HIPCHK(c, t.nm.alloc(total_nm));
        HIPCHK(c, t.nmoff.alloc(n));
        HIPCHK(c, t.L.alloc(n));
        HIPCHK(c, t.hasN.alloc(n));
        HIPCHK(c, hipMemset(t.hasN, 0, (size_t)n * 4));
        if (c->P.mal <= 15 && c->P.msl <= 15) {
            HIPCHK(c, t.kmL.alloc(total_nm * 64));
            HIPCHK(c, t.kmS.alloc(total_nm * 64));
        }
        c->gs.tab = std::move(t);
    }
    // The caller's sequences are separate host buffers: they go up through two pinned 64 MB staging buffers, the
    // copy of one overlapping the fill of the other (the 4 GB of config 5 take as long as the PCIe link needs).
    {
        const u64 chunk = 64ull << 20;
        PinMem<uint8_t> pin[2];
        hipEvent_t done[2] = {nullptr, nullptr};
        hipError_t e = hipSuccess;
        for (int k = 0; k < 2 && e == hipSuccess; ++k) {
            e = pin[k].alloc(chunk);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&done[k], hipEventDisableTiming);
        }
        u64 at = 0;                                               // codes staged so far
        u32 g = 0; u64 goff = 0;                                  // next genome / offset inside it
        for (int k = 0; e == hipSuccess && at < total_codes; k ^= 1) {
            e = hipEventSynchronize(done[k]);                     // the previous copy out of this buffer (no-op the first time)
            u64 fill = 0;
            while (g < n && fill < chunk) {
                const u64 take = std::min<u64>(chunk - fill, (u64)len[g] - goff);
                if (take) memcpy(pin[k] + fill, codes[g] + goff, take);
                fill += take; goff += take;
                if (goff == len[g]) { ++g; goff = 0; }
            }
            if (e == hipSuccess) e = hipMemcpyAsync(d_codes.get() + at, pin[k], fill, hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) e = hipEventRecord(done[k], c->stream);
            at += fill;
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        for (int k = 0; k < 2; ++k) if (done[k]) hipEventDestroy(done[k]);
        if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? LZANI_ERR_NOMEM : LZANI_ERR_DEVICE, std::string("staging the sequences: ") + hipGetErrorString(e));
    }
    HIPCHK(c, hipMemcpy(d_codeoff, codeoff.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->gs.tab.nmoff, c->gs.nmoff.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->gs.tab.L, c->gs.L.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    c->gs.n = n;
    size_t maxblk = text_wordsN(c->gs.Tmax);
    // gridDim.y is limited to 65535: pack in slices of genomes
    for (u32 g0 = 0; g0 < n; g0 += 32768) {
        u32 cnt = std::min<u32>(32768, n - g0);
        hipLaunchKernelGGL(k_pack, dim3((u32)((maxblk + 127) / 128), cnt), dim3(128), 0, c->stream,
                           d_codes.get(), d_codeoff.get() + g0, c->gs.tab.t2, c->gs.tab.nm, c->gs.tab.nmoff + g0, c->gs.tab.L + g0, c->gs.tab.hasN + g0, c->P.mrd, cnt);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    {
        std::vector<int> hn(n);
        HIPCHK(c, hipMemcpy(hn.data(), c->gs.tab.hasN, (size_t)n * 4, hipMemcpyDeviceToHost));
        c->gs.all_nfree = std::all_of(hn.begin(), hn.end(), [](int v) { return v == 0; });
    }
    TRACE("set_genomes: n=%u Tmax=%d dirbits=%d posbits=%d tagmask=%x", n, c->gs.Tmax, c->gs.geo.dirbits, c->gs.geo.posbits, c->gs.geo.tagmask);
    return LZANI_OK;
}

int lzani_run_rows_device(lzani_ctx* c, uint32_t n_rows, const uint32_t* ref_ids, const uint64_t* row_off,
                          const uint32_t* query_ids, void* d_out)
{
    if (!c) return LZANI_ERR_ARG;
    if (!ref_ids || !row_off || (!d_out && n_rows && row_off[n_rows]))
        return fail(c, LZANI_ERR_ARG, "lzani_run_rows_device: null argument");
    if (c->gs.ooc) return run_rows_tiled(c, n_rows, ref_ids, row_off, query_ids, (int*)d_out, nullptr, nullptr);
    const int rc = run_rows_impl(c, n_rows, ref_ids, row_off, query_ids, (int*)d_out);
    c->res.tiles = rc == LZANI_OK && n_rows && row_off[n_rows] ? 1 : 0;
    return rc;
}

int lzani_run_rows(lzani_ctx* c, uint32_t n_rows, const uint32_t* ref_ids, const uint64_t* row_off,
                   const uint32_t* query_ids, lzani_result* out)
{
    if (!c) return LZANI_ERR_ARG;
    if (!ref_ids || !row_off) return fail(c, LZANI_ERR_ARG, "lzani_run_rows: null argument");
    const u64 n_pairs = n_rows ? row_off[n_rows] : 0;
    if (n_pairs && !out) return fail(c, LZANI_ERR_ARG, "lzani_run_rows: null output");
    HIPCHK(c, hipSetDevice(c->dev));
    if (c->gs.ooc) return run_rows_tiled(c, n_rows, ref_ids, row_off, query_ids, nullptr, out, nullptr);     // (host scatter)
    DevMem<lzani_result> d_out;
    if (n_pairs) HIPCHK(c, d_out.alloc(n_pairs));
    int rc = run_rows_impl(c, n_rows, ref_ids, row_off, query_ids, (int*)d_out.get());
    c->res.tiles = rc == LZANI_OK && n_pairs ? 1 : 0;
    if (rc == LZANI_OK && n_pairs) {
        hipError_t e = hipMemcpy(out, d_out.get(), n_pairs * sizeof(lzani_result), hipMemcpyDeviceToHost);
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
    DevMem<lzani_result> d_out;
    DevMem<lzani_region> d_regions;
    DevMem<unsigned long long> d_count;
    if (n_pairs && !c->gs.ooc) HIPCHK(c, d_out.alloc(n_pairs));      // (out-of-core: tile by tile)
    HIPCHK(c, d_regions.alloc(capacity));
    HIPCHK(c, d_count.alloc(1));
    HIPCHK(c, hipMemset(d_count.get(), 0, sizeof(unsigned long long)));
    RegionSink rs{d_regions.get(), d_count.get(), capacity};
    int rc;
    if (c->gs.ooc) rc = run_rows_tiled(c, n_rows, ref_ids, row_off, query_ids, nullptr, out, &rs);
    else {
        rc = run_rows_impl(c, n_rows, ref_ids, row_off, query_ids, (int*)d_out.get(), &rs);
        c->res.tiles = rc == LZANI_OK && n_pairs ? 1 : 0;
    }
    if (rc == LZANI_OK) {
        unsigned long long cnt = 0;
        hipError_t e = hipMemcpy(&cnt, rs.d_count, sizeof cnt, hipMemcpyDeviceToHost);
        if (e == hipSuccess && n_pairs && !c->gs.ooc) e = hipMemcpy(out, d_out.get(), n_pairs * sizeof(lzani_result), hipMemcpyDeviceToHost);
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
    o->bucket_table = c->gs.bk_stride != 0; o->tag_words = c->gs.tw_stride != 0;
    o->n_free = c->gs.all_nfree;
    o->slots = c->sl.slots; o->batches_last_run = c->run.batches;
    o->bytes_per_slot = slot_bytes(c->gs).tables;           // (without the keys of the sort-based build)
    o->bytes_genomes = c->gs.total_nm * (16 + 8) + (c->gs.tab.kmL ? c->gs.total_nm * 64 * 8 : 0);
    o->join_lists = c->gs.join_mode; o->block_launches = c->run.blk_launches; o->bitmap_launches = c->run.pm_launches; o->rtc_launches = c->run.rtc_launches;
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

int lzani_set_genome_memory(lzani_ctx* c, uint64_t bytes)
{
    if (!c) return LZANI_ERR_ARG;
    c->mem_req = bytes;
    return LZANI_OK;
}

int lzani_plan_blocks(uint32_t n, const uint32_t* len, const lzani_params* p, uint64_t limit, uint32_t* block_of)
{
    if (!p || !len || !n) return LZANI_ERR_ARG;
    Params P{p->min_anchor_len, p->min_seed_len, p->max_dist_in_ref, p->max_dist_in_query,
             p->min_region_len, p->approx_window, p->approx_mismatches, p->approx_run_len};
    if (!params_supported(P)) return LZANI_ERR_PARAMS;
    std::vector<u32> first;
    std::vector<u64> bytes;
    std::string msg;
    const int nb = plan_blocks_impl(n, len, P, limit, first, bytes, msg);
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

const char* lzani_debug_kernel_name(uint32_t id)
{
    return id < (u32)PK_COUNT ? PAIR_KERNELS[id].name : nullptr;
}

int64_t lzani_debug_rtc_compile(const lzani_params* p, int nfree, int cand, const char* arch, char* log, uint64_t log_cap)
{
    if (!p || !arch || cand < 0 || cand > 2) return LZANI_ERR_ARG;
    Params P{p->min_anchor_len, p->min_seed_len, p->max_dist_in_ref, p->max_dist_in_query,
             p->min_region_len, p->approx_window, p->approx_mismatches, p->approx_run_len};
    if (!params_supported(P) || P.mal > 15 || P.msl > 15) return LZANI_ERR_PARAMS;
    std::string lg;
    const size_t n = lzani_rtc::compile_only(P, nfree != 0, cand, arch, lg);
    if (log && log_cap) { snprintf(log, (size_t)log_cap, "%s", lg.c_str()); }
    return n ? (int64_t)n : (int64_t)LZANI_ERR_DEVICE;
}

int lzani_debug_get_index(lzani_ctx* c, uint32_t id, uint64_t* t2, uint64_t* nm, uint32_t* dirz,
                          uint32_t* ent, uint32_t* n_ent, uint32_t* geom)
{
    if (!c) return LZANI_ERR_ARG;
    if (!c->gs.n || id >= c->gs.n) return fail(c, LZANI_ERR_ARG, "lzani_debug_get_index: bad id");
    if (c->gs.ooc) return fail(c, LZANI_ERR_STATE, "lzani_debug_get_index: the genome is not resident (out-of-core set)");
    HIPCHK(c, hipSetDevice(c->dev));
    int rc = ensure_slabs(c, 1);
    if (rc) return rc;
    DevMem<u32> d_ref;
    HIPCHK(c, d_ref.alloc(1));
    HIPCHK(c, hipMemcpy(d_ref.get(), &id, 4, hipMemcpyHostToDevice));
    rc = build_indexes(c, Knobs{}, d_ref, 1);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int T = ref_text_len(c->gs.L[id], c->P.mrd);
    size_t wn = text_wordsN(T);
    if (nm) HIPCHK(c, hipMemcpy(nm, c->gs.tab.nm + c->gs.nmoff[id], wn * 8, hipMemcpyDeviceToHost));
    if (t2) HIPCHK(c, hipMemcpy(t2, c->gs.tab.t2 + 2 * c->gs.nmoff[id], wn * 16, hipMemcpyDeviceToHost));
    std::vector<u32> d(c->gs.dir_stride);
    HIPCHK(c, hipMemcpy(d.data(), c->sl.d_dirz, c->gs.dir_stride * 4, hipMemcpyDeviceToHost));
    u32 ne = d[c->gs.dir_stride - 1];
    if (dirz) memcpy(dirz, d.data(), c->gs.dir_stride * 4);
    if (ent && ne) HIPCHK(c, hipMemcpy(ent, c->sl.d_ent, (size_t)ne * 4, hipMemcpyDeviceToHost));
    if (n_ent) *n_ent = ne;
    if (geom) { geom[0] = c->gs.geo.kb; geom[1] = c->gs.geo.dirbits; geom[2] = c->gs.geo.posbits; geom[3] = c->gs.geo.tagmask; }
    return LZANI_OK;
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

// Test hook: the index slabs of one batch of `rows` reference ids, built by the run's own build_indexes into slots 0 .. rows-1.
int lzani_debug_index_slab(lzani_ctx* c, uint32_t rows, const uint32_t* ref_ids, int with_filter, int with_tw,
                           lzani_slab_info* info, uint32_t* dirz, uint32_t* ent, uint32_t* bk, uint32_t* tw, uint32_t* fl,
                           uint32_t* status)
{
    if (!c) return LZANI_ERR_ARG;
    if (!c->gs.n || !rows || !ref_ids || !info) return fail(c, LZANI_ERR_ARG, "lzani_debug_index_slab: bad arguments");
    if (c->gs.ooc) return fail(c, LZANI_ERR_STATE, "lzani_debug_index_slab: the genomes are not resident (out-of-core set)");
    for (u32 k = 0; k < rows; ++k)
        if (ref_ids[k] >= c->gs.n) return fail(c, LZANI_ERR_ARG, "lzani_debug_index_slab: reference id out of range");
    HIPCHK(c, hipSetDevice(c->dev));
    int rc = ensure_slabs(c, rows);
    if (rc) return rc;
    if (c->sl.slots < rows) return fail(c, LZANI_ERR_ARG, "lzani_debug_index_slab: more rows than index slabs");
    DevMem<u32> d_ref;
    HIPCHK(c, d_ref.alloc(rows));
    HIPCHK(c, hipMemcpy(d_ref.get(), ref_ids, (size_t)rows * 4, hipMemcpyHostToDevice));
    rc = build_indexes(c, Knobs{}, d_ref, rows, with_filter != 0, with_tw != 0);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    info->key_bits = c->gs.geo.kb; info->dir_bits = c->gs.geo.dirbits; info->pos_bits = c->gs.geo.posbits; info->tag_mask = c->gs.geo.tagmask;
    info->filter_mask = c->gs.fmask;
    info->build = c->sl.index_build;
    info->dir_stride = c->gs.dir_stride; info->ent_stride = c->gs.ent_stride; info->bk_stride = c->gs.bk_stride;
    // (what this build wrote: the sort build leaves the tag words out without with_tw, every build the filter without with_filter)
    info->tw_stride = (c->sl.index_build != LZANI_INDEX_BUILD_SORT || with_tw) ? c->gs.tw_stride : 0;
    info->fl_stride = with_filter ? c->gs.fl_stride : 0;
    const size_t r = rows;
    if (dirz) HIPCHK(c, hipMemcpy(dirz, c->sl.d_dirz, r * c->gs.dir_stride * 4, hipMemcpyDeviceToHost));
    if (ent) HIPCHK(c, hipMemcpy(ent, c->sl.d_ent, r * c->gs.ent_stride * 4, hipMemcpyDeviceToHost));
    if (bk && info->bk_stride) HIPCHK(c, hipMemcpy(bk, c->sl.d_bk, r * info->bk_stride * 4, hipMemcpyDeviceToHost));
    if (tw && info->tw_stride) HIPCHK(c, hipMemcpy(tw, c->sl.d_tw, r * info->tw_stride * 4, hipMemcpyDeviceToHost));
    if (fl && info->fl_stride) HIPCHK(c, hipMemcpy(fl, c->sl.d_fl, r * info->fl_stride * 4, hipMemcpyDeviceToHost));
    if (status) {
        if (c->sl.index_build == LZANI_INDEX_BUILD_LDS) HIPCHK(c, hipMemcpy(status, c->sl.d_status, r * 4, hipMemcpyDeviceToHost));
        else memset(status, 0, r * 4);
    }
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
    int rc = run_rows_impl(c, n_rows, ref_ids, row_off, query_ids, (int*)d_out.get(), nullptr, &sink, &p);
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
