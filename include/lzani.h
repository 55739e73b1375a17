/*
 * lzani.h -- C ABI of the MI355X LZ-ANI pair engine (liblzani_hip.so).
 *
 * This is the drop-in boundary for LZ-ANI's one data-parallel hot path: the worker loop of
 * CLZMatcher::do_matching (/root/reference/src/lz_matcher.cpp:172-277) and everything it calls
 * in CParser (/root/reference/src/parser.h:237-253, parser.cpp:16-783).  A host that owns
 * FASTA ingest, filtering and TSV output (the reference's CLZMatcher, or this repo's own
 * `lz-ani` binary) hands over genomes as reservoir symbol codes and rows of directed pairs,
 * and receives one results_t per pair.  Plain pointers and sizes only; no HIP, torch or C++
 * types cross the boundary.  INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions: every function returns LZANI_OK (0) or a negative error code and never calls
 * exit(); lzani_last_error() gives the message.  A context is bound to one GPU, is blocking
 * and not re-entrant (the reference's per-thread CParser has the same property, parser.h:25-56).
 * Outputs are written only on success.
 *
 * Results are bit-identical to the reference's for every parameter set with max_dist_in_query <=
 * max_dist_in_ref (all defaults and published settings).  Above that the reference reads beyond the end
 * of its reference text (undefined behaviour); this engine treats positions outside a text as never
 * matching, deterministically.
 */
#ifndef LZANI_H
#define LZANI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LZANI_OK             0
#define LZANI_ERR_ARG       -1   /* NULL / out-of-range argument                           */
#define LZANI_ERR_PARAMS    -2   /* LZ parameters outside the supported envelope           */
#define LZANI_ERR_DEVICE    -3   /* HIP runtime error (message in lzani_last_error)        */
#define LZANI_ERR_STATE     -4   /* call order violated (e.g. run before set_genomes)      */
#define LZANI_ERR_NOMEM     -5   /* host or device allocation failed                       */

/* The eight integers CParser reads from CParams (/root/reference/src/params.h:34-48;
 * CLI: -a/--mal -s/--msl -r/--mrd -q/--mqd -g/--reg --aw --am --ar, lz-ani.cpp:210-249). */
typedef struct lzani_params {
    int32_t min_anchor_len;     /* mal, default 11 */
    int32_t min_seed_len;       /* msl, default 7  */
    int32_t max_dist_in_ref;    /* mrd, default 40 */
    int32_t max_dist_in_query;  /* mqd, default 40 */
    int32_t min_region_len;     /* reg, default 35 */
    int32_t approx_window;      /* aw,  default 15 */
    int32_t approx_mismatches;  /* am,  default 7  */
    int32_t approx_run_len;     /* ar,  default 3  */
} lzani_params;

/* results_t (/root/reference/src/defs.h:48-65): what CParser::calc_stats returns. */
typedef struct lzani_result {
    int32_t sym_in_matches;     /* TSV nt_match    */
    int32_t sym_in_literals;    /* TSV nt_mismatch */
    int32_t no_components;      /* TSV num_alns    */
} lzani_result;

/* Device-side timing of the last lzani_run_rows* call, measured with HIP events on the
 * context's own stream (what bench.py reports as the roofline numerator/denominator). */
typedef struct lzani_timing {
    double   index_ms;          /* sum over batches: per-reference index build kernels      */
    double   pairs_ms;          /* sum over batches: the pair kernel                        */
    uint32_t pair_launches;     /* number of pair-kernel launches (= batches)               */
    uint32_t index_launches;    /* number of index-build kernel launches                    */
    uint64_t pairs;             /* directed pairs processed                                 */
    double   cand_ms;           /* sum over batches: presence matrix + candidate bitmaps of dense rows (0 otherwise) */
    double   kmers_ms;          /* per-genome k-mer words (+ join lists): made by the first run after
                                 * lzani_set_genomes and kept; 0 in the runs that found them ready; not part of index_ms */
    uint32_t cand_launches;     /* kernel launches of the candidate stage                   */
    uint32_t reserved_;
} lzani_timing;

/* One region of CParser::calc_regions / get_parsing (/root/reference/src/parser.cpp:786-837,
 * region_t in defs.h:67-153): what --out-alignment prints (lz_matcher.cpp:102-169).  `pair` is the
 * CSR position of the directed pair the region belongs to. */
typedef struct lzani_region {
    uint64_t pair;
    int32_t  ref_start, ref_end, seq_start, seq_end, num_matches, num_mismatches;
} lzani_region;

typedef struct lzani_ctx lzani_ctx;

void lzani_default_params(lzani_params *p);

/* Replaces CParser::CParser(const CParams&) (parser.h:237-241), once per GPU instead of once
 * per thread.  device_id is the HIP device ordinal.  LZANI_ERR_NOMEM where the context's one device buffer cannot be
 * had, LZANI_ERR_DEVICE for every other failure of the device; *out is NULL then and nothing is left allocated. */
int lzani_create(const lzani_params *p, int device_id, lzani_ctx **out);
void lzani_destroy(lzani_ctx *ctx);
const char *lzani_last_error(const lzani_ctx *ctx);

/* Replaces the seq_view hand-over of prepare_reference / prepare_data (parser.cpp:16-50;
 * lz_matcher.cpp:207-221): all n genomes at once, one symbol per byte in the reservoir's
 * codes (A0 C1 G2 T3, anything >= 4 is N; seq_reservoir.h:241-248).  The engine packs them to
 * 2 bit + N mask on the device and keeps them resident; caller buffers may be freed on return.
 * Ids used below are indices into this table (the reference's reordered sequence ids).
 * The call drops the genome set there was and everything made from it -- index slabs, candidate scratch, prefilter, kept,
 * regions and cluster results -- before it allocates.  LZANI_ERR_NOMEM, in-core or out-of-core, therefore leaves the context
 * without a genome set: every call that needs one returns LZANI_ERR_STATE until a lzani_set_genomes succeeds, and one
 * with the same arguments may be tried again on the same context. */
int lzani_set_genomes(lzani_ctx *ctx, uint32_t n, const uint8_t *const *codes, const uint32_t *len);

/* Genome sets larger than the device (out-of-core).  The genome-memory limit of a context (bytes of genome tables:
 * packed texts, N masks, k-mer words, join lists) applies at its next lzani_set_genomes; 0 (the default) is automatic.
 * A set that does not fit stays on the host (1 B per base) and is cut, in id order, into contiguous blocks of at most
 * limit / 2 bytes of tables each (lzani_plan_blocks); two blocks are resident at a time, and every lzani_run_rows* call
 * runs tile by tile over (reference block, query block) with results bit-identical to the in-core run.  Automatic
 * mode keeps a set in-core unless its tables, its 1 B/base staging copy or one index slab do not fit the free device
 * memory; it then applies half of the free memory as the limit.  An explicit limit below twice the footprint of the
 * largest genome makes lzani_set_genomes fail with LZANI_ERR_ARG.  For an out-of-core set lzani_get_layout's
 * bytes_genomes is the resident region and n_free describes the whole set; lzani_debug_get_index returns
 * LZANI_ERR_STATE. */
int lzani_set_genome_memory(lzani_ctx *ctx, uint64_t bytes);

/* The block plan as a pure host function (no GPU): block_of[g] (may be NULL) for the n genomes of lengths len under
 * the given limit; returns the number of blocks (limit 0: one), or LZANI_ERR_ARG / LZANI_ERR_PARAMS. */
int lzani_plan_blocks(uint32_t n, const uint32_t *len, const lzani_params *p, uint64_t limit, uint32_t *block_of);

/* Residency of the current genome set and the last run.  A run takes its reference blocks in ascending order (block
 * i to half A: nothing to do if A holds it, the halves trade places if B holds it, else one upload), and for each its
 * query blocks: i itself, then the block B holds, then the others ascending (one upload each unless B holds it). */
typedef struct lzani_residency_info {
    uint64_t limit;                 /* the genome-memory limit applied to the set (0: automatic, in-core)            */
    uint32_t blocks;                /* 1: the whole set is resident                                                   */
    uint32_t tiles;                 /* tiles of the last run (an in-core run: 1)                                      */
    uint64_t block_uploads;         /* block uploads of the last run                                                  */
    uint64_t peak_resident_bytes;   /* largest genome-table footprint resident at once (in-core: the whole set's)     */
    uint64_t host_bytes;            /* the host copy of the set's codes; 0 when in-core                               */
    double   upload_ms;             /* device time of the last run's block uploads (packing + k-mer words)            */
} lzani_residency_info;
int lzani_get_residency(const lzani_ctx *ctx, lzani_residency_info *info);

/* Replaces the body of the do_matching worker (lz_matcher.cpp:196-255) for n_rows reference
 * rows given in CSR form: row k has reference ref_ids[k] and queries
 * query_ids[row_off[k] .. row_off[k+1]).  query_ids == NULL means the dense row "every id !=
 * ref, ascending" (row_off[k+1]-row_off[k] must then be n-1), i.e. lz_matcher.cpp:214-233;
 * a non-NULL list is the filtered case (234-250).  out is CSR-aligned (out[e] belongs to
 * query_ids[e]) in host memory: out[e] = calc_stats() of parse(query = query_ids[e], ref = ref_ids[k]).
 * LZANI_ERR_NOMEM (every lzani_run_rows* form): `out` is unspecified, the genome set and the results of the other stages
 * (prefilter, kept, cluster) are as they were, and the same call may be made again.  What the run path keeps between runs
 * -- index slabs, candidate scratch, join lists -- may have been released; the next run makes it anew.  Where only the
 * buffers of a faster form cannot be had (presence matrix, pair table, candidate bitmaps, the slabs sized for them, the
 * longest-pair-first order), the run takes the form that needs none of them and succeeds with the same results;
 * lzani_get_layout's bitmap_launches, or lpt_launches and split_launches, of that run are then 0. */
int lzani_run_rows(lzani_ctx *ctx, uint32_t n_rows, const uint32_t *ref_ids, const uint64_t *row_off,
                   const uint32_t *query_ids, lzani_result *out);

/* Same, but the results stay in device memory: d_out is a device pointer (this context's GPU)
 * to row_off[n_rows] lzani_result records, e.g. the shard buffer handed to an RCCL gather. */
int lzani_run_rows_device(lzani_ctx *ctx, uint32_t n_rows, const uint32_t *ref_ids, const uint64_t *row_off,
                          const uint32_t *query_ids, void *d_out);

/* lzani_run_rows plus the per-pair regions (replaces parser.get_parsing() in the worker, lz_matcher.cpp:
 * 222-223, 241-242).  Up to `capacity` regions are written to `regions` (host memory) in no particular
 * order -- sort by (pair, length desc, seq_start) for the reference's per-pair order; *n_regions receives
 * the number found, which may exceed capacity (then call again with a larger buffer). */
int lzani_run_rows_regions(lzani_ctx *ctx, uint32_t n_rows, const uint32_t *ref_ids, const uint64_t *row_off,
                           const uint32_t *query_ids, lzani_result *out, lzani_region *regions,
                           uint64_t capacity, uint64_t *n_regions);

int lzani_get_timing(const lzani_ctx *ctx, lzani_timing *t);

/* What the context laid out in HBM for the current genome set (after lzani_set_genomes), and how the last
 * lzani_run_rows* call was batched.  The reference has no counterpart (its tables are private members of
 * CParser, parser.h:25-56); tests and the bench use it to assert which index form / batch path really ran. */
typedef struct lzani_layout_info {
    int32_t  key_bits, dir_bits, pos_bits;  /* anchor index geometry: 2*mal, log2(buckets), bits of a text position */
    uint32_t tag_mask;                      /* tag bits stored in an entry                                            */
    int32_t  kmer_words;                    /* 1: per-genome k-mer words exist (mal, msl <= 15)                      */
    int32_t  bucket_table, tag_words;       /* 1: the index slabs carry a bucket table / tag words                   */
    int32_t  n_free;                        /* 1: no genome holds an N (NFREE kernel instantiation)                  */
    uint32_t slots;                         /* index slabs allocated = reference rows per batch                      */
    uint32_t batches_last_run;              /* batches of the last run                                               */
    uint64_t bytes_per_slot;                /* HBM bytes of one index slab                                           */
    uint64_t bytes_genomes;                 /* HBM bytes of packed texts + N masks + k-mer words                     */
    int32_t  join_lists;                    /* 1: candidates come from a join with per-genome sorted k-mer lists (long genomes) */
    int32_t  block_launches;                /* pair-kernel launches of the last run by blocks of 16 waves with the
                                             * reference's presence filter in LDS (probe form, rows of >= 128 pairs) */
    int32_t  bitmap_launches;               /* pair-kernel launches of the last run fed by per-pair candidate bitmaps
                                             * (dense rows: presence matrix of the batch's references)                 */
    int32_t  rtc_launches;                  /* pair-kernel launches of the last run by a kernel compiled at run time for
                                             * this context's parameters (lzani_get_rtc_info)                          */
    int32_t  lpt_launches;                  /* pair-kernel launches of the last run that handed their tickets out longest pair
                                             * first (batches of few, long pairs; placement only)                      */
    int32_t  matrix_from_index;             /* presence matrices of the last run made from the batch's anchor indexes
                                             * (long genomes: no global atomics) instead of one atomicOr per text position */
    int32_t  split_launches;                /* batches of the last run whose pairs were scanned by several waves each (few, long
                                             * pairs: checkpoints, segments, stitch -- csrc/lzani_kernels_split.h)           */
    int32_t  reserved_;
    uint64_t split_segments;                /* segments run for them in all, the ones run again included                    */
} lzani_layout_info;
int lzani_get_layout(const lzani_ctx *ctx, lzani_layout_info *info);

/* The reference reads its eight LZ parameters at run time and has one speed for all of them (lz-ani.cpp:205-260,
 * parser.h:31).  Here the pair kernel folds them into its code: ahead of time for the defaults and for
 * --mal 15 --msl 9 --reg 60, and for every other tuple (with mal, msl <= 15) by compiling the same kernel source
 * with hipRTC the first time the context runs rows -- a few seconds once, then a code object cached on disk
 * ($LZANI_RTC_CACHE, else $XDG_CACHE_HOME/lzani_rtc, else ~/.cache/lzani_rtc; LZANI_RTC=0 turns run-time compilation
 * off).  If that fails the generic kernel runs; results are the same either way. */
typedef struct lzani_rtc_info {
    int32_t folded_ahead_of_time;   /* 1: the context's tuple is one of the two compiled ahead of time (nothing to build) */
    int32_t null_chain;             /* 1: the tuple is inside what the hand-scheduled null chain is written for            */
    int32_t kernels_built;          /* kernels of this context made ready at run time so far (compiled or loaded)          */
    int32_t kernels_from_cache;     /* ... of which came from the disk cache                                               */
    int32_t kernels_failed;         /* attempts that fell back to the generic kernel                                       */
    int32_t reserved_;
    double  build_ms;               /* host time spent building / loading them                                             */
} lzani_rtc_info;
int lzani_get_rtc_info(const lzani_ctx *ctx, lzani_rtc_info *info);
/* Test hook (needs no GPU): compiles the pair kernel for a parameter tuple the way a context would (nfree: genomes
 * without N; cand: 0 probe, 1 join, 2 candidate bitmaps) for the gfx target `arch` and returns the size of the code
 * object, or a negative error code with the compiler's messages in `log`. */
int64_t lzani_debug_rtc_compile(const lzani_params *p, int nfree, int cand, const char *arch, char *log, uint64_t log_cap);
/* Test hooks: the launch record.  Every pair-kernel instantiation the engine can launch (the ones compiled ahead of
 * time and the run-time compiled kernel per (nfree, cand)) has a fixed id and name; lzani_debug_kernel_launches copies
 * the launches per id of the context's last run (up to cap entries) and returns the size of the table;
 * lzani_debug_kernel_name returns the name of an id, NULL past the end (needs no context and no GPU).  Names:
 * "pairs fast=F nfree=N defp=D aln=A bk=B cand=C", "pairs_blk nfree=N defp=D", "split nfree=N defp=D mode=M",
 * "rtc nfree=N cand=C". */
int lzani_debug_kernel_launches(const lzani_ctx *ctx, uint64_t *counts, uint32_t cap);
const char *lzani_debug_kernel_name(uint32_t id);
/* Test hook: the repair loop of the split path (a pair scanned by several waves) in the context's last run, summed over
 * its split batches.  A stitch that does not get through finds one void segment; before the give-up round
 * (6 + S / 4 rounds, or LZANI_SPLIT_GIVE_UP) the void segment's cut is disabled and the segment that handed over to it is
 * resumed; in the give-up round, or where nothing can be retried, every cut of the pair is disabled and its segment 0
 * scans it whole. */
typedef struct {
    uint64_t pairs_cut;             /* pairs that were cut into segments (the others: scanned whole by their segment 0)    */
    uint64_t rounds;                /* rounds of segments + stitch: the most of any batch                                  */
    uint64_t resumed;               /* segments listed to resume                                                           */
    uint64_t given_up;              /* pairs whose cuts were all disabled                                                  */
    uint64_t voids[6];              /* void stitches by cause: 0 a look-back cut short, 1 kept by the segment / dropped by
                                       the true scan, 2 the other way round, 3 the true floor above what the segment's
                                       look-backs hold for, 4 kept on a guess and cut short, 5 a broken chain              */
} lzani_split_stats;
int lzani_debug_split_stats(const lzani_ctx *ctx, lzani_split_stats *stats);

/* ---- K-mer prefilter: the filter rows without a kmer-db file --------------------------------------------
 * The reference takes its filtered rows from a text file written by kmer-db (CFilter::load_filter).  This stage makes
 * them from the resident genome set: the number of shared canonical k-mers of every unordered genome pair, and the
 * pairs that pass a threshold.  Exact integer arithmetic, 8 <= k <= 31:
 *   window value   v(p) = sum over j < k of code[p + j] * 4^j (first symbol least significant), defined where no
 *                  symbol of the window is N; rc(p) is the same sum over the window's reverse complement
 *   canonical      canon(p) = min(v(p), rc(p))
 *   sampling       a canonical k-mer x is kept iff splitmix64(x) <= sample_max (UINT64_MAX keeps all), with
 *                  x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB;
 *                  x ^= x >> 31  (mod 2^64)
 *   K(g)           the set of kept canonical k-mers of genome g; shared(a, b) = |K(a) & K(b)|
 *   kept pairs     a < b with shared >= max(min_shared, 1) and (double)shared / (double)min(|K(a)|, |K(b)|) >= min_ratio
 * K-mer passes: the workspace is 24 B per kept window (keys, sorted keys, radix scratch) and a pass of the pipeline holds
 * fewer than 2^32 windows, so the stage runs in as many passes over disjoint classes of k-mers as that takes.  shared and
 * |K(g)| are sums over k-mers: every pass adds into the same counts, and the results are those of one pass, bit for bit.
 *   hash           h(x) = splitmix64(x), the hash of the sampling rule
 *   bin            bin(x) = (h(x) >> 20) & 4095: 4,096 bins, from the hash's low half (sampling by h <= sample_max does not
 *                  skew them)
 *   pass plan      P >= 1 contiguous bin ranges [lo_p, hi_p) that cover 0 .. 4096 in order; pass p works on exactly the
 *                  kept canonical k-mers with lo_p <= bin(x) < hi_p
 *   forced plan    LZANI_PREFILTER_PASSES=<P>, 1 <= P <= 4096 (else LZANI_ERR_ARG): lo_p = floor(4096 * p / P)
 *   automatic      from the histogram of the kept windows per bin over the whole set, greedy from bin 0: a pass takes bins
 *                  while its sum of windows stays <= cap.  cap = min(2^32 - 17, B / 24) -- 2^32 - 17 keys is what one sort
 *                  call takes -- with B a quarter of the free device memory at the time of the call;
 *                  LZANI_PREFILTER_MAX_WINDOWS=<w> replaces cap (a test and bench hook).  A single bin above cap:
 *                  LZANI_ERR_ARG, the message names the bin's windows -- the one case where the answer is a lower
 *                  sample_max.  (A forced plan is not held to cap, only to 2^32 - 17 windows per pass.)
 *   one pass       where the whole set's kept windows are <= cap and no plan is forced (or P = 1 is): no histogram is
 *                  taken, and the count matrix's tiles are worked over the one set of postings
 *   several        tile outer, pass inner: every (tile, pass) rebuilds the pass's postings and adds them into the tile,
 *                  T * P' key pipelines for T tiles and P' passes that hold a window; |K(g)| is complete after the first
 *                  tile's passes.  The workspace is that of the fullest pass, allocated once; the tile is sized behind it
 *   key sweeps     W = 1 where no window is kept (the count of the whole set); 3 with one pass (count, canonical k-mers,
 *                  rank keys); 2 + 3 * T * P' with several (the count of the whole set, the histogram, three per pipeline)
 * The count matrix is worked in tiles of rows sized by a workspace budget (half of the device memory free when the tile is
 * allocated: behind the postings, or behind the passes' workspace; LZANI_PREFILTER_TILE_ROWS=<rows> forces the tile height).  The genome tables, k-mer words, index slabs and compiled
 * kernels of the context are left as they are.  Out-of-core genome sets (lzani_set_genome_memory) are out of scope
 * here (LZANI_ERR_STATE): lzani_prefilter_codes below serves them.  LZANI_ERR_NOMEM where the workspace of the fullest
 * pass or a one-row matrix tile does not fit; after an error the context holds no prefilter result and is otherwise
 * unchanged. */
typedef struct lzani_prefilter_info {
    int32_t  k; uint32_t tiles;                                /* tiles: row tiles of the count matrix                */
    uint64_t positions, distinct_kmers, postings, entries;     /* valid sampled windows, distinct k-mers, (k-mer, genome) pairs, kept pairs */
    double   keys_ms, sort_ms, count_ms, compact_ms;           /* HIP events on the context's stream: k-mer extraction; the two
                                                                * sorts with dictionary and postings; the count matrix; the kept
                                                                * entries of its rows                                  */
} lzani_prefilter_info;
/* Runs the stage on the resident genome set; results stay in the context until the next prefilter / set_genomes. */
int lzani_prefilter(lzani_ctx *ctx, int k, uint64_t sample_max, uint32_t min_shared, double min_ratio, uint64_t *n_entries);
/* kmers_of[n] = |K(g)|; row_off[n+1], ids[], shared[]: CSR of the kept pairs a < b (row a, ids ascending).  Any may be NULL. */
int lzani_prefilter_fetch(lzani_ctx *ctx, uint32_t *kmers_of, uint64_t *row_off, uint32_t *ids, uint32_t *shared);
/* LZANI_ERR_STATE without a prefilter result, like the fetch. */
int lzani_get_prefilter_info(const lzani_ctx *ctx, lzani_prefilter_info *info);
/* The k-mer passes of the last prefilter (either entry point).  positions, distinct_kmers and postings of
 * lzani_prefilter_info are the sums over the passes of one tile -- the classes are disjoint, so the one-pass values --
 * and its *_ms fields sum everything that ran, the histogram sweep apart (hist_ms). */
typedef struct lzani_prefilter_pass_info {
    uint32_t passes, key_sweeps;          /* passes of the plan; key sweeps run in all (histogram included) */
    uint64_t cap, largest_pass;           /* windows a pass may hold; windows of the fullest pass            */
    uint64_t workspace_bytes;             /* ka + kb + radix scratch as allocated                            */
    double   hist_ms;                     /* the histogram sweep (0 when P == 1 without one)                 */
} lzani_prefilter_pass_info;
/* LZANI_ERR_STATE without a prefilter result. */
int lzani_get_prefilter_pass_info(const lzani_ctx *ctx, lzani_prefilter_pass_info *info);
/* bin_lo[passes + 1] of the last prefilter (may be NULL); returns passes or a negative error */
int lzani_prefilter_pass_plan(const lzani_ctx *ctx, uint32_t *bin_lo);
/* the plan rule as a pure host function (no GPU): hist[4096], cap, forced (0: automatic) -> bin_lo (may be NULL; up to
 * 4097 entries), returns P or LZANI_ERR_ARG (a bin above cap; forced above 4096).  A forced plan reads neither hist nor cap. */
int lzani_plan_passes(const uint64_t *hist, uint64_t cap, uint32_t forced, uint32_t *bin_lo);

/* The prefilter for genome sets larger than the device: the same definitions and the same results as lzani_prefilter, but
 * the n genomes are given here, as host symbol codes in the convention of lzani_set_genomes, and need not be (and are
 * not made) the context's genome set.  The stage reads genomes only where it extracts keys, so they stay in host memory
 * at 1 B per base and pass through one staging buffer on the device, slice by slice; no genome tables are built.  A
 * genome set the context holds, in-core or out-of-core -- its tables, resident halves and the blocks they hold, k-mer
 * words, index slabs, compiled kernels -- is left as it is.  The result replaces any earlier prefilter result, is read
 * with lzani_prefilter_fetch / lzani_get_prefilter_info (sized by this call's n) and lasts until the next prefilter or
 * lzani_set_genomes.  Caller buffers are read only during the call.
 *   slices   genomes in id order, contiguous runs: a new slice starts where the next genome would take the slice's sum of
 *            len above slice_bytes (genomes of length 0 join the current slice).  slice_bytes 0 is automatic:
 *            min(sum len, max(longest genome, free device memory / 8)); LZANI_PREFILTER_SLICE_BYTES=<bytes> overrides the
 *            argument.  A genome longer than the slice size: LZANI_ERR_ARG (the message names the minimum).
 *   sweeps   every key sweep of every k-mer pass (W of them, see "key sweeps" above) goes over all slices, and the sweeps
 *            alternate: up, down, up, ...; the slice the staging buffer holds is not copied again.  S slices:
 *            W * (S - 1) + 1 copies -- 3 S - 2 with one pass, S where no window is kept.  The staging buffer stays
 *            until the last sweep of the last tile, so with several passes the matrix tile is sized beside it.
 * LZANI_ERR_ARG for n == 0, NULL pointers, k outside 8 .. 31, a negative or NaN ratio, a sequence too long for 32-bit
 * positions; LZANI_ERR_NOMEM where the staging buffer or the workspace does not fit: the context then holds no prefilter
 * result and is otherwise unchanged. */
int lzani_prefilter_codes(lzani_ctx *ctx, uint32_t n, const uint8_t *const *codes, const uint32_t *len,
                          int k, uint64_t sample_max, uint32_t min_shared, double min_ratio,
                          uint64_t slice_bytes, uint64_t *n_entries);
/* The slice plan as a pure host function (no GPU): slice_of[g] (may be NULL) under the given slice size; returns the
 * number of slices (slice_bytes 0: one), or LZANI_ERR_ARG (no genomes, a genome longer than slice_bytes). */
int lzani_plan_slices(uint32_t n, const uint32_t *len, uint64_t slice_bytes, uint32_t *slice_of);
typedef struct lzani_prefilter_stream_info {
    uint32_t slices, slice_uploads;      /* slices of the plan; host-to-device slice copies made            */
    uint64_t staged_bytes, stage_bytes;  /* bytes copied in all; capacity of the staging buffer             */
    double   upload_ms;                  /* HIP events around the slice copies, on the context's stream     */
} lzani_prefilter_stream_info;
/* LZANI_ERR_STATE unless the context's current prefilter result came from lzani_prefilter_codes. */
int lzani_get_prefilter_stream_info(const lzani_ctx *ctx, lzani_prefilter_stream_info *info);

/* The cross form: a query set against a reference set.  The n genomes are one id space cut at n_ref: ids 0 .. n_ref - 1
 * are the references, ids n_ref .. n - 1 the queries (n_query = n - n_ref).  Everything defined above stays as it is --
 * window value, canonical k-mer, sampling, K(g), shared(a, b), the kept rule, bins, pass plan, key sweeps -- and the cross
 * form keeps exactly the pairs a < n_ref <= b that pass the kept rule: its result is the all-pairs result of the same set
 * restricted to those pairs, bit for bit.  kmers_of is that of all n genomes, shared that of every kept pair, ids ascend
 * inside a row, and the rows a >= n_ref are empty.  lzani_prefilter_fetch and the info calls above read a cross result
 * like any other: positions, distinct_kmers and postings are those of the all-pairs run (the key pipeline is the same),
 * entries is the number of kept cross pairs.
 *   matrix   n_ref rows of n_query counts, mat[(a - r0) * n_query + (b - n_ref)], worked in tiles of rows that cover
 *            0 .. n_ref only: min(n_ref, max(1, free / 2 / (4 * n_query))) rows, or LZANI_PREFILTER_TILE_ROWS clipped to
 *            n_ref.  A run of postings lists its references before its queries; only reference postings of the tile add,
 *            and only over the queries of their run, so no add is spent on a pair that is not a cross pair.
 * n_ref == 0 or n_ref >= n: LZANI_ERR_ARG.  Every other error, and what a failed call leaves behind, is that of the
 * all-pairs counterpart; lzani_prefilter_cross refuses an out-of-core set with LZANI_ERR_STATE, like lzani_prefilter. */
int lzani_prefilter_cross(lzani_ctx *ctx, int k, uint64_t sample_max, uint32_t min_shared, double min_ratio,
                          uint32_t n_ref, uint64_t *n_entries);                 /* resident set              */
int lzani_prefilter_codes_cross(lzani_ctx *ctx, uint32_t n, const uint8_t *const *codes, const uint32_t *len,
                                int k, uint64_t sample_max, uint32_t min_shared, double min_ratio,
                                uint64_t slice_bytes, uint32_t n_ref, uint64_t *n_entries);   /* streamed    */
typedef struct lzani_prefilter_cross_info {
    uint32_t n_ref, n_query;       /* n_query = n - n_ref                                        */
    uint32_t tile_rows, reserved_; /* height of the matrix tile as allocated; 0                  */
    uint64_t matrix_bytes;         /* tile_rows * n_query * 4, as allocated                      */
} lzani_prefilter_cross_info;
/* LZANI_ERR_STATE unless the context's current prefilter result came from a cross call. */
int lzani_get_prefilter_cross_info(const lzani_ctx *ctx, lzani_prefilter_cross_info *info);

/* Sparse counting: a second accumulator for the count stage of all four entry points.  The matrix holds n_rows * n_cols
 * counts whether or not a pair shares anything; the pair table holds the pairs that do, and its size follows them.  Results
 * are those of the dense form bit for bit: kmers_of, row_off, ids, shared, and positions, distinct_kmers, postings, entries.
 *   table     S slots, S a power of two, of a u64 key and a u32 count (12 B a slot).  key(a, b) = a << 32 | b with global
 *             genome ids (a < b; cross form a < n_ref <= b), all ones marks a free slot, the home slot is
 *             splitmix64(key) & (S - 1), collisions go to the next slot and wrap at S
 *   size      the largest power of two with 12 * S <= half of the device memory free where the matrix tile would be sized,
 *             at most the smallest power of two >= 2 * n_rows * n_cols, and at most 2^32 (the kept keys of a tile are
 *             sorted in one call).  LZANI_PREFILTER_TABLE_SLOTS=<S> forces it (a test and bench hook; a power of two >= 2,
 *             else LZANI_ERR_ARG)
 *   tiles     row ranges [r0, r1) as in the dense form, and one tile holds at most S / 2 distinct pairs over all its
 *             passes.  The first attempt takes all rows, h = n_rows.  An attempt that meets pair S / 2 + 1 is abandoned:
 *             the table is cleared, h = max(1, h / 2), and the same r0 starts again from its first pass.  A finished tile
 *             leaves h as it is (clipped to the rows left); h does not grow back.  One row above S / 2 pairs:
 *             LZANI_ERR_NOMEM, the message names the row and S; the dense form is the way out.  Whether a tile is
 *             finished depends on its number of distinct pairs only, not on the order the adds arrive in
 *   sweeps    one pass: the postings are built once and a new attempt only repeats the count, W = 3.  Several:
 *             W = 2 + 3 * pass_runs, pass_runs the (attempt, non-empty pass) pairs whose postings were built -- P' where
 *             nothing overflowed, against the dense form's T * P'.  |K(g)| of a pass is added once, whatever is repeated
 *   output    after a tile's last pass the keys of the slots that pass the kept rule are sorted, which puts them row after
 *             row with ascending ids; the table's own order is never visible
 *   mode      LZANI_PF_COUNTING_AUTO (the default) stays dense wherever the dense rule gives one tile or
 *             LZANI_PREFILTER_TILE_ROWS is set (a forced tile height is a statement about the matrix), and takes the table
 *             where the matrix would need more than one tile.  A choice, not a measurement: a set whose pairs nearly all
 *             share a k-mer is better off dense, and that is not detected.  _SPARSE ignores LZANI_PREFILTER_TILE_ROWS.
 * lzani_prefilter_info of a sparse result: tiles = finished tiles; count_ms = clearing the table and the inserts;
 * compact_ms = the scan of the slots, the sort and the look-up of the counts. */
#define LZANI_PF_COUNTING_AUTO   0
#define LZANI_PF_COUNTING_DENSE  1
#define LZANI_PF_COUNTING_SPARSE 2
/* Holds for the context's later prefilter calls; any other mode: LZANI_ERR_ARG.  An earlier result stays. */
int lzani_set_prefilter_counting(lzani_ctx *ctx, int mode);
typedef struct lzani_prefilter_sparse_info {
    uint32_t sparse;                /* 1: the current result was counted into the pair table      */
    uint32_t attempts, pass_runs;   /* tile attempts (abandoned ones included); (attempt, pass) pairs run */
    uint32_t reserved_;
    uint64_t slots, table_bytes;    /* as allocated                                                */
    uint64_t pairs_seen;            /* pairs with shared >= 1, summed over the finished tiles      */
    uint64_t max_fill;              /* most slots in use at the end of a finished tile             */
} lzani_prefilter_sparse_info;
/* LZANI_ERR_STATE without a prefilter result; all zero for a dense one, and for one that had nothing to count (a single
 * genome, no postings). */
int lzani_get_prefilter_sparse_info(const lzani_ctx *ctx, lzani_prefilter_sparse_info *info);
/* The tile rule as a pure host function (no GPU): row_pairs[r] = the distinct pairs of row r (shared >= 1, over all
 * passes), slots = S -> tile_r0[0 .. T] (may be NULL; up to n_rows + 1 entries, tile t holds the rows tile_r0[t] ..
 * tile_r0[t + 1]) and *attempts (may be NULL).  Returns T, LZANI_ERR_ARG (no rows, no row_pairs, slots not a power of
 * two >= 2), or LZANI_ERR_NOMEM for a row above slots / 2. */
int lzani_plan_sparse_tiles(uint32_t n_rows, const uint64_t *row_pairs, uint64_t slots, uint32_t *tile_r0, uint32_t *attempts);

/* Limit: every genome keeps its N best pairs (what Vclust's prefilter calls --max-seqs).  A post-stage over the context's
 * current prefilter result R, whichever entry point and whichever counting form made it: R is the kept pairs a < b with
 * shared(a, b), and kmers_of.  The stage bounds the pairs that go on to the alignment at limiting genomes * N, whatever
 * the sizes of the families are.
 *   score      q(a, b) = floor(shared(a, b) * (2^32 - 1) / min(|K(a)|, |K(b)|)) in unsigned 64-bit arithmetic (shared <=
 *              min < 2^32: the product fits; 1 <= q <= 2^32 - 1).  An integer score of this project's own, like Leiden's
 *              2^-20 units: no claim of equality with another program's ordering
 *   limiting   all-pairs result: every genome.  Cross result: the queries only (ids >= n_ref) -- a reference may be the
 *              best hit of any number of queries
 *   list       of genome g: all its partners h in R, whichever of the two has the smaller id, ordered by q descending,
 *              ties to the smaller h; rank_g(h) = h's position in it, from 0
 *   survival   pair (a, b) survives iff rank_a(b) < N for a limiting a, or rank_b(a) < N for a limiting b.  All-pairs: the
 *              union -- one endpoint that counts the other among its N best is enough.  Cross: the query's rank alone
 *   result     R restricted to the survivors: the same CSR form (row a, ids ascending), shared and kmers_of unchanged,
 *              lzani_prefilter_info.entries the new count and the other fields of that struct as they were.
 *              lzani_prefilter_fetch then reads the limited result, which lasts as long as any prefilter result does
 * What the definition gives:
 *   - N >= the largest degree changes nothing
 *   - applying the stage twice with the same N equals applying it once (a survivor's rank can only fall when entries ahead
 *     of it go)
 *   - every limiting genome of degree d keeps at least min(d, N) pairs (more where a partner's list keeps others)
 *   - the limited cross result is NOT the limited all-pairs result restricted to the cross pairs: the references do not
 *     limit, and a query ranks its references only
 * The device form: one key ~q << 32 | e per entry e in CSR order, sorted by its high half (stably: equal scores keep CSR
 * order, which for a fixed genome is ascending partner id); one directed key g << 32 | i per limiting endpoint g of sorted
 * position i, sorted stably by g, which leaves every genome's list in order; the first N of every list mark their entry;
 * the marked entries are compacted row by row.  Exact, independent of the schedule (the only atomics are integer adds),
 * O(entries) memory, no work quadratic in a degree.
 * LZANI_ERR_STATE without a prefilter result; LZANI_ERR_ARG for N == 0 and for a result of more than 2^31 - 9 entries
 * (twice as many keys must fit one sort call of 2^32 - 17).  The workspace is allocated whole before the result is
 * touched: LZANI_ERR_NOMEM or a device error leaves the unlimited result in place and readable. */
typedef struct lzani_prefilter_limit_info {
    uint32_t max_per_genome, limiting;   /* N; limiting genomes                               */
    uint64_t entries_in, entries_out;
    uint64_t genomes_cut;                /* limiting genomes whose list was longer than N     */
    uint64_t workspace_bytes;            /* as allocated                                      */
    double   limit_ms;                   /* HIP events on the context's stream                */
} lzani_prefilter_limit_info;
int lzani_prefilter_limit(lzani_ctx *ctx, uint32_t max_per_genome, uint64_t *n_entries);
/* LZANI_ERR_STATE without a prefilter result, or where the current one was never limited. */
int lzani_get_prefilter_limit_info(const lzani_ctx *ctx, lzani_prefilter_limit_info *info);
/* The rule as a pure host function (no GPU): keep[e] = 1 / 0 per CSR entry; n_ref 0 = all-pairs.  LZANI_ERR_ARG for
 * n == 0, N == 0, n_ref >= n, NULL arrays, offsets that do not start at 0 or descend, more than 2^31 - 9 entries, ids that
 * do not ascend strictly inside a row or are <= the row, an id >= n, shared == 0, shared > min(|K|), and in the cross form
 * an entry that is not a pair a < n_ref <= b. */
int lzani_prefilter_limit_host(uint32_t n, uint32_t n_ref, const uint32_t *kmers_of, const uint64_t *row_off,
                               const uint32_t *ids, const uint32_t *shared, uint32_t max_per_genome, uint8_t *keep);
/* Test hook, in the manner of lzani_debug_filter_results and lzani_debug_cluster_add_edges: installs a made-up prefilter
 * result (uploaded here) in place of the context's, so that the stage runs on chosen integers; n_ref 0 = all-pairs.  The
 * arrays are checked as lzani_prefilter_limit_host checks them (LZANI_ERR_ARG); an earlier result is dropped first. */
int lzani_debug_prefilter_set(lzani_ctx *ctx, uint32_t n, uint32_t n_ref, const uint32_t *kmers_of,
                              const uint64_t *row_off, const uint32_t *ids, const uint32_t *shared);

/* ---- Output filter on the device: only the pairs that pass come back -------------------------------------------
 * The reference's --out-filter drops a TSV line when one of its five ratios is below its minimum (lz_matcher.cpp:437-462).
 * A line needs the pair in both directions, which a finished run holds side by side in device memory; this stage reads
 * that buffer and keeps the unordered pairs of which at least one line survives, so that the host neither receives nor
 * stores the others.  It is a post-stage over a result buffer: the pair kernels and their dispatch know nothing of it.
 *   rows       a call's rows are the CSR of lzani_run_rows: ref_ids, row_off, and query_ids or NULL for dense rows
 *   leading    a directed entry (ref a, query b) with a < b; its mate is the entry (ref b, query a) of the same call; a
 *              leading entry without a mate is unpaired: dropped and counted.  Entries with b <= a are read as mates only
 *   lengths    report_len[n]: the lengths the ratios divide by (NULL: the genome set's own).  A host that prints lengths
 *              without contig separators passes those
 *   the rule   X = result of (ref a, query b), Y = result of (ref b, query a), la = report_len[a], lb = report_len[b];
 *              every division an IEEE double division of exact integers, the integer sums in 32-bit arithmetic:
 *                tani = (double)(X.m + Y.m) / (la + lb)                                  m: sym_in_matches, l: sym_in_literals
 *                line 0 (query b): gani = (double)X.m / lb;  ani = X.m + X.l != 0 ? (double)X.m / (X.m + X.l) : 0;
 *                                  qcov = (double)(X.m + X.l) / lb;  rcov = (double)(Y.m + Y.l) / la
 *                line 1 (query a): the same with X and Y, and la and lb, exchanged
 *              a line passes unless one of its five values is < its minimum (a NaN or inf value is below nothing); the
 *              pair is kept iff a line passes.  A NaN minimum: LZANI_ERR_ARG
 *   order      the kept records come in the order of the leading entries in the CSR: the call's rows, and ascending b
 *              inside a row.  Rows passed in ascending id order give the order of the reference's output file
 *   kept forms ref_ids must be distinct and, where query_ids is given, every row's ids ascend strictly: LZANI_ERR_ARG
 *              otherwise, checked on the host before anything runs (lzani_run_rows itself accepts what it accepted)
 * The result -- 36 B a kept pair -- stays in the context until the next kept call or lzani_set_genomes; its size is known
 * from a count pass before it is allocated, and LZANI_ERR_NOMEM leaves the context without a kept result and otherwise
 * unchanged. */
typedef struct lzani_out_filter { double min_tani, min_gani, min_ani, min_qcov, min_rcov; } lzani_out_filter;
typedef struct lzani_kept_pair {
    uint32_t a, b;            /* a < b */
    lzani_result x;           /* parse(query b, ref a) */
    lzani_result y;           /* parse(query a, ref b) */
    uint32_t lines;           /* bit 0: the line "b against a" passes; bit 1: "a against b" passes; never 0 */
} lzani_kept_pair;            /* 36 bytes, 32-bit fields only */
typedef struct lzani_kept_info {
    uint64_t entries, leading;        /* directed entries of the call; those with a < b                          */
    uint64_t unpaired;                /* leading entries without a mate                                          */
    uint64_t kept_pairs, kept_lines;  /* records; lines that pass, summed over them                              */
    uint64_t bytes_to_host;           /* copied out by the fetches so far                                        */
    double   filter_ms;               /* HIP events on the context's stream: count, scan, write                  */
} lzani_kept_info;
/* The rule as a pure host function (no GPU): the `lines` of one pair.  NULL pointers or a NaN minimum: 0xFFFFFFFF. */
uint32_t lzani_out_filter_lines(const lzani_out_filter *f, const lzani_result *x, const lzani_result *y, uint32_t len_a, uint32_t len_b);
/* lzani_run_rows into a device buffer, then the stage; the full result buffer never reaches the host.  Out-of-core sets too. */
int lzani_run_rows_kept(lzani_ctx *ctx, uint32_t n_rows, const uint32_t *ref_ids, const uint64_t *row_off, const uint32_t *query_ids,
                        const lzani_out_filter *f, const uint32_t *report_len, uint64_t *n_kept);
/* Records first .. first + count - 1 of the kept result.  A range past the end: LZANI_ERR_ARG; no result: LZANI_ERR_STATE. */
int lzani_kept_fetch(lzani_ctx *ctx, uint64_t first, uint64_t count, lzani_kept_pair *out);
/* The stage alone on a caller's device buffer (this context's GPU) of row_off[n_rows] lzani_result records of n genomes.
 * Needs no genome set; report_len must not be NULL. */
int lzani_filter_results_device(lzani_ctx *ctx, uint32_t n, const uint32_t *report_len, uint32_t n_rows, const uint32_t *ref_ids,
                                const uint64_t *row_off, const uint32_t *query_ids, const void *d_results,
                                const lzani_out_filter *f, uint64_t *n_kept);
/* Test hook: the same with the results in host memory (uploaded here): the stage on made-up integers.  LZANI_ERR_NOMEM at
 * the upload too leaves the context without a kept result. */
int lzani_debug_filter_results(lzani_ctx *ctx, uint32_t n, const uint32_t *report_len, uint32_t n_rows, const uint32_t *ref_ids,
                               const uint64_t *row_off, const uint32_t *query_ids, const lzani_result *results,
                               const lzani_out_filter *f, uint64_t *n_kept);
/* LZANI_ERR_STATE without a kept result. */
int lzani_get_kept_info(const lzani_ctx *ctx, lzani_kept_info *info);

/* ---- Alignment regions on the device: filtered, ordered, fetched in pieces --------------------------------------------
 * The reference's --out-alignment prints the regions of every directed pair (lz_matcher.cpp:102-169), pair by pair, and with
 * an --out-filter drops the pairs of which gani, ani or qcov over the region sums is below its minimum (115-138).  The pair
 * kernels leave the regions in a device buffer in no order; this stage sums each pair's regions, applies that rule, puts the
 * regions that stay into the file's order with the engine's radix sort and hands them back in pieces.  It is a post-stage
 * over a finished buffer, like the output filter: the pair kernels and their dispatch know nothing of it.
 *   rows       a call's rows are those of the kept forms: distinct ref_ids, strictly ascending lists, checked on the host
 *              before anything runs (LZANI_ERR_ARG).  Entry e of the CSR is the directed pair (ref a = its row's reference,
 *              query b); a region belongs to the entry its `pair` names
 *   sums       mat(e) = the sum of num_matches over the entry's regions, lit(e) = the sum of num_mismatches: 32-bit integer
 *              sums, as the reference makes them
 *   the rule   len = aln_len[b] (aln_len == NULL: the genome set's own lengths); every division an IEEE double division:
 *                gani = (double)mat / len;  ani = mat + lit != 0 ? (double)mat / (mat + lit) : 0;  qcov = (double)(mat + lit) / len
 *              with a filter f the entry is dropped iff gani < f.min_gani || ani < f.min_ani || qcov < f.min_qcov: a NaN or inf
 *              value is below nothing, a value equal to its minimum stays.  min_tani and min_rcov are not read (the reference
 *              reads only the three).  f == NULL: no entry is dropped (the reference with no --out-filter).  A NaN in one of
 *              the three minima: LZANI_ERR_ARG.  Entries without a region are neither kept nor dropped
 *   result     the regions of the entries that stay, with pair = e: entries in ascending e; inside an entry the longer
 *              seq_end - seq_start first, then the smaller seq_start; records equal in all three keep their input order
 *              (only made-up regions can be: a pair's regions are disjoint in the query).  Rows passed in ascending id order
 *              give the order of the reference's file
 *   limits     more than 2^32 - 17 regions (what one sort takes), or 2^32 or more entries in a call: LZANI_ERR_ARG
 *   capacity   the run writes its regions into a buffer whose size the library chooses: what lzani_set_region_capacity
 *              forced, else the smallest of (a) sum over the entries of floor((L_b + max_dist_in_ref) / max(min_region_len, 1))
 *              -- a region is at least min_region_len long in the query and a pair's regions are disjoint there --, (b) what
 *              one eighth of the free device memory holds at the call, (c) the sort's limit; and at least 1,024.  A run that
 *              finds more regions than the capacity is repeated once with the exact count: info.runs is 1 or 2
 * The result -- 32 B a region -- stays in the context until the next regions call or lzani_set_genomes.  LZANI_ERR_NOMEM from
 * lzani_run_rows_aligned or lzani_debug_order_regions leaves the context with neither a kept result nor a regions result and
 * otherwise unchanged (genome set, prefilter result and cluster state stay); the same call may be made again. */
typedef struct lzani_regions_info {
    uint64_t entries, found, kept;                  /* directed entries of the call; regions the run found; regions that stay */
    uint64_t entries_with_regions, entries_dropped; /* entries that own a region; those of them the rule drops               */
    uint64_t capacity, runs;                        /* regions the raw buffer held; runs made (1 or 2; 0: no run, made-up regions) */
    uint64_t sort_passes;                           /* radix passes of the three sorts, summed                                */
    uint64_t workspace_bytes;                       /* the stage's device memory beside the raw buffer and the result         */
    uint64_t bytes_to_host;                         /* copied out by the fetches so far                                       */
    double   sums_ms, sort_ms, write_ms;            /* HIP events on the context's stream: sums and rule; keys and sorts; gather */
} lzani_regions_info;
/* The first capacity of the later lzani_run_rows_aligned calls, in regions; 0 (the default): automatic. */
int lzani_set_region_capacity(lzani_ctx *ctx, uint64_t regions);
/* One run with the region sink in device memory, then the stages.  out (host, may be NULL): the results of lzani_run_rows.
 * kept_filter (may be NULL): the output filter's stage over the same result buffer; its records and info are exactly those
 * of lzani_run_rows_kept with report_len (NULL: the genome set's own lengths), read with lzani_kept_fetch; NULL: the call
 * leaves no kept result.  aln_filter (may be NULL), aln_len: the region stage as above.  *n_kept, *n_regions (may be NULL):
 * the kept pairs and the regions that stay.  Out-of-core sets too. */
int lzani_run_rows_aligned(lzani_ctx *ctx, uint32_t n_rows, const uint32_t *ref_ids, const uint64_t *row_off, const uint32_t *query_ids,
                           lzani_result *out, const lzani_out_filter *kept_filter, const uint32_t *report_len,
                           const lzani_out_filter *aln_filter, const uint32_t *aln_len, uint64_t *n_kept, uint64_t *n_regions);
/* Records first .. first + count - 1 of the regions result.  A range past the end: LZANI_ERR_ARG; no result: LZANI_ERR_STATE. */
int lzani_regions_fetch(lzani_ctx *ctx, uint64_t first, uint64_t count, lzani_region *out);
/* LZANI_ERR_STATE without a regions result. */
int lzani_get_regions_info(const lzani_ctx *ctx, lzani_regions_info *info);
/* Test hook: the stage alone on `count` made-up regions of n genomes in host memory (uploaded here).  Needs no genome set;
 * aln_len must not be NULL.  A region with pair at or beyond the entries, with seq_end <= seq_start or with a negative
 * field: LZANI_ERR_ARG, on the host.  A kept result there is stays, except where the call ends in LZANI_ERR_NOMEM. */
int lzani_debug_order_regions(lzani_ctx *ctx, uint32_t n, const uint32_t *aln_len, uint32_t n_rows, const uint32_t *ref_ids,
                              const uint64_t *row_off, const uint32_t *query_ids, const lzani_region *regions, uint64_t count,
                              const lzani_out_filter *f, uint64_t *n_regions);
/* The same statement as a pure host function (no GPU; a stable sort): the regions that stay to out (may be NULL: counted
 * only), their number to *n_out; info (may be NULL): entries, found, kept, entries_with_regions and entries_dropped, the
 * other fields 0.  The checks of lzani_debug_order_regions: LZANI_ERR_ARG. */
int lzani_regions_host(uint32_t n, const uint32_t *aln_len, uint32_t n_rows, const uint32_t *ref_ids, const uint64_t *row_off,
                       const uint32_t *query_ids, const lzani_region *regions, uint64_t count, const lzani_out_filter *f,
                       lzani_region *out, uint64_t *n_out, lzani_regions_info *info);

/* ---- Clustering the kept pairs on the device: single linkage, greedy, set cover and complete linkage ---------------
 * The kept records of the output filter are the edge list of the similarity graph; this stage clusters it where it lies.
 * It is a post-stage over finished kept results, like the output filter over a result buffer: the pair kernels and their
 * dispatch know nothing of it.  The five algorithms are defined by the statements below and by nothing else (no claim
 * of equality with another program's output is made); lzani_cluster_host is their sequential form.
 *   graph      the nodes are the n genomes, by the ids of lzani_set_genomes (the lz-ani binary reorders genomes: id 0 is
 *              the first line of its ids file).  The edge {a, b}, a < b, exists iff the pair is a kept pair of a kept call
 *              that was added: a pair of which at least one TSV line passes the output filter, which is therefore the
 *              edge threshold
 *   weight     with X, Y, la, lb and lines of the output filter above, every division an IEEE double division of exact
 *              integers (the integer sums in 32-bit arithmetic), one value per line -- line 0 has bit 0 of lines, line 1
 *              bit 1:
 *                LZANI_CLUSTER_TANI   (double)(X.m + Y.m) / (la + lb)                      for both lines
 *                LZANI_CLUSTER_GANI   line 0: (double)X.m / lb;   line 1: (double)Y.m / la
 *                LZANI_CLUSTER_ANI    line 0: X.m + X.l != 0 ? (double)X.m / (X.m + X.l) : 0;   line 1: the same with Y
 *              w is the largest value over the lines that `lines` names.  A NaN value reads as 0 (and so do the negative
 *              values and -0 that only made-up integers give); +inf stays.  So w >= 0, and weights order like their bit
 *              patterns read as 64-bit unsigned integers
 *   edge set   edges are added over one or several calls; adding an edge twice is the same as adding it once (it carries
 *              the same weight), and the order of additions never shows in a result
 *   rep_of     rep_of[v] is the representative of v's cluster; a representative has rep_of[r] == r
 *     LZANI_CLUSTER_SINGLE        the clusters are the connected components; rep_of[v] is the smallest id of v's component
 *     LZANI_CLUSTER_GREEDY_FIRST  greedy incremental, in the manner of CD-HIT: the genomes in ascending id order, v becomes
 *                                 a representative iff no earlier representative is its neighbour; otherwise rep_of[v] is
 *                                 the smallest id among its neighbouring representatives (always < v: one exists below v).
 *                                 The representatives are the lexicographically first maximal independent set
 *     LZANI_CLUSTER_GREEDY_BEST   nearest centroid, in the manner of UCLUST: the same representatives; for another v,
 *                                 rep_of[v] is the neighbouring representative r < v with the largest w, ties to the
 *                                 smallest r.  Representatives above v do not count: they did not exist when v was placed
 *     LZANI_CLUSTER_SET_COVER     greedy set cover, the default of MMseqs2-style clustering, on the graph with distinct
 *                                 edges (the same pair added twice, in either orientation or over several add calls, is
 *                                 one edge; weights and the measure play no part).  All nodes start unassigned.  While a
 *                                 node is unassigned: c(v) = the number of unassigned neighbours of the unassigned node
 *                                 v; the unassigned v with the largest c(v), ties to the smallest id, becomes a
 *                                 representative (rep_of[v] = v), every unassigned neighbour u of v gets rep_of[u] = v,
 *                                 and all of these are assigned.  An isolated or left-over node with c = 0 becomes its own
 *                                 representative.  Unlike the greedy forms, a representative may have a larger id than
 *                                 its members
 *     LZANI_CLUSTER_COMPLETE      complete linkage (farthest neighbour) at the output filter's cut, on the graph with
 *                                 distinct edges as for set cover; the weight of an edge is the smallest w over its
 *                                 records (kept records of one pair carry one weight; only made-up edges can differ, and
 *                                 the statement is one about the weakest link).  An edge of weight 0 is an edge.  Every
 *                                 node starts as a cluster of its own; id(C) is the smallest member id.  Two clusters A
 *                                 and B are linked iff every pair {a, b}, a in A, b in B, is an edge; the link's value
 *                                 s(A, B) is the smallest weight among those |A| * |B| edges.  A missing edge means no
 *                                 link, whatever the weights.  While a link exists: the link with the largest s, ties to
 *                                 the smallest lower id, then to the smallest other id, is taken and its two clusters
 *                                 merge.  rep_of[v] = id(final cluster of v).  Every final cluster is a clique of kept
 *                                 pairs, no two final clusters are linked, and the measure matters as for GREEDY_BEST
 *     LZANI_CLUSTER_LEIDEN        deterministic Leiden with the constant Potts model (CPM), on the graph with distinct
 *                                 edges as for set cover; the weight of an edge is the smallest w over its records.  No
 *                                 claim of equality with igraph or Clusty is made, as for the others.  Arithmetic: a weight
 *                                 is quantised once, q = min(floor(w * 2^20), 2^20) (the product with a power of two and
 *                                 the floor are exact in a double; +inf clamps to 2^20); the resolution gamma in [0, 1]
 *                                 (default 0.7) is read as g = llround(gamma * 2^20); everything below is signed 64-bit
 *                                 integer arithmetic.  n > 2^21: LZANI_ERR_ARG (g * n^2 stays inside 2^62; edge sums stay
 *                                 below 2^52 under the 2^32 - 17 record limit).
 *                                 A level is a graph of level nodes with sizes s (original genomes: 1) and distinct
 *                                 entries (a < b, q).  A community is a set of level nodes; its id is always its smallest
 *                                 member, recomputed after every round, so every rule is a function of the partition and
 *                                 not of label history.  S_C = the sum of the sizes in C; W(v, C) = the sum of q over the
 *                                 entries between v and the members of C other than v.
 *                                 val(v, C) = W(v, C) - g * s_v * (S_C - [v in C] * s_v).  The option "alone" has the
 *                                 value 0, exists only for a v that is not alone already, and its community is {v}.
 *                                 A moving round on a partition P: (1) from the snapshot at the round's start every v
 *                                 takes its best option among its own community, the communities of its neighbours and
 *                                 alone: the largest val, ties to staying first, then to the smallest community id, alone
 *                                 last; D(v) = val(best) - val(own); v is a candidate iff D(v) > 0.  (2) A candidate
 *                                 touches its own community and its target; alone touches only its own.  (3) v moves iff
 *                                 in each community it touches it has the largest key among all candidates that touch
 *                                 that community; the key is the largest D, ties to the smallest v.  (4) All moves are
 *                                 applied, then ids and sizes are recomputed (where the smallest member left, the
 *                                 remainder is renamed by the id rule).  (5) The phase ends with the first round that has
 *                                 no candidate.
 *                                 A refinement round inside P, from the partition R of singletons: v is eligible iff its
 *                                 R-community holds one level node (itself, never joined) and it is well connected,
 *                                 W(v, P(v)) >= g * s_v * (S_P(v) - s_v).  A target is an R-community C != {v} inside
 *                                 P(v) with W(v, C) > 0, that is itself well connected -- ext(C) >= g * S_C * (S_P - S_C),
 *                                 ext(C) the weight between C and the rest of its P-community -- and with
 *                                 D = W(v, C) - g * s_v * S_C >= 0.  The largest D wins, ties to the smallest id; the
 *                                 exclusivity rule of the moving round applies with the touched communities {v} and C;
 *                                 the phase ends with the first round without a mover.  This is Leiden's refinement with
 *                                 the random choice replaced by the greedy one (the limit theta -> 0 of the paper);
 *                                 R-communities are connected by construction.
 *                                 Aggregation: the new level nodes are the R-communities, numbered in ascending order of
 *                                 their smallest member; sizes are summed; entries are contracted through R with their q
 *                                 summed, those inside one R-community dropped (they enter no val); the new level starts
 *                                 from P.  An iteration, at each level: the moving phase; if every P-community is one
 *                                 level node, stop; the refinement; if this level neither moved nor merged anything,
 *                                 stop; aggregate.  `iterations` in 1..16 (default 2): each starts again from the original
 *                                 graph with the previous result as P; the run stops early after an iteration in which no
 *                                 moving round moved anything.  rep_of[v] = the smallest original id of v's final
 *                                 community.  The measure matters as for GREEDY_BEST.
 *                                 Why a round is well defined and the phases end: two movers of one round touch disjoint
 *                                 communities, so the communities a mover leaves and joins are those of the snapshot and
 *                                 its D is exactly its gain when applied.  The integer quality
 *                                 Q = sum_C (W_inside(C) - g * sum_{pairs u < v in C} s_u * s_v) rises by the sum of the
 *                                 applied D, strictly; the candidate with the globally largest key always moves; Q is
 *                                 bounded: the moving phase terminates, and the result of a round depends on the
 *                                 partition alone, not on any schedule.  In the refinement a node that moved is never
 *                                 eligible again, so at most n_level moves are made.  Safety stop: a phase that has run
 *                                 64 * n_level + 64 rounds ends the run in LZANI_ERR_DEVICE; this is a stop without a
 *                                 proof that valid inputs stay below it.  The host form applies the same cap, so a graph
 *                                 that reaches it is found on the CPU
 *   numbering  cluster_of[v] = the number of representatives with an id below rep_of[v]: clusters are numbered in
 *              ascending order of their representative; clusters = the number of representatives
 * The device stage: the union-find of SINGLE hooks the larger root under the smaller, so that parent[v] <= v at every
 * moment; the greedy representatives are the fixed point of rounds of an edge pass and a node pass whose stores are
 * idempotent and final, so the result is that of the statements whatever the schedule.  `rounds` is 1 for SINGLE and the
 * number of greedy rounds up to the first that left no node undecided (a path with ascending ids needs n / 2 to n).
 * SET_COVER on the device: the edge records are made distinct once per run in a workspace of the run (keys lo << 32 | hi,
 * sorted, unique; the edge buffer itself is only read).  key(v) = c(v) << 32 | (0xFFFFFFFF - v) for an unassigned v, 0 for
 * an assigned one: a strict total order, "largest c, then smallest id" on top, never 0 for an unassigned node as
 * v < n <= 2^32 - 1.  A round takes the unassigned nodes as they are at its start and selects every one whose key is the
 * largest among the unassigned nodes within two hops (itself, its unassigned neighbours, theirs); every selected node
 * covers its unassigned neighbours as of the round's start.  The rounds give exactly the sequential result: call a
 * selection valid when the node has the largest key within its two hops.  The sequential step is valid (the global maximum
 * is a local one).  Keys only fall, and the key of v changes only when a neighbour of v is assigned, which takes a
 * selection within two hops of v: so one valid selection leaves the key and the cover set of every other valid node as
 * they were, and that node valid.  The process ends, so every maximal schedule of valid selections ends in the same
 * representatives and members.  Two nodes selected in one round are more than two hops apart: their cover sets are
 * disjoint and neither covers the other.  (With a one-hop maximum the result is wrong: on the edges (0,1) (1,2) (2,3)
 * (3,4) (3,5) the statement gives rep_of = 0 0 3 3 3 3, and one hop selects 1 in the first round.)  `rounds` is the number
 * of the first round that left no node unassigned; the global maximum is selected in every round, so n rounds always do
 * (a path with ascending ids takes n / 3; disjoint near-cliques one or two).  More than 2^32 - 17 edge records:
 * LZANI_ERR_ARG; a workspace that does not fit: LZANI_ERR_NOMEM, and the cluster state is as before the run.
 * COMPLETE on the device: rounds of reciprocal best links.  From a cluster's own point of view its best link is the one
 * with the largest s, ties to the smallest neighbouring cluster id; in a round every pair of clusters that are each other's
 * best link merges.  The rounds give exactly the sequential result: (1) call a merge valid when the two clusters are each
 * other's best link.  (2) The sequential step is valid: a link that beats (A, B) from A's side or from B's side -- a larger
 * s, or the same s and a smaller neighbour id -- would precede (A, B) in the global order.  (3) For this linkage
 * s(X u Y, Z) = min(s(X, Z), s(Y, Z)), and there is no link where either is missing: a merge never raises a value and never
 * makes a link where there was none.  (4) If C and D are each other's best and X, Y merge elsewhere, the new link
 * (C, X u Y) can only tie with (C, D) when both (C, X) and (C, Y) tied with it; both then lost on id, so
 * min(id X, id Y) > id D still holds, and (C, D) stays C's best; the same from D's side.  (5) A valid merge therefore
 * leaves every other valid merge valid, merges of disjoint pairs commute, and the process ends (every merge takes a cluster
 * away): every maximal schedule of valid merges ends in the same partition.  Two pairs merged in one round are disjoint, by
 * reciprocity.  A round works on the entry list L of (ca, cb, count, wmin), ca < cb -- the links and link candidates of the
 * contracted graph, at first the edge records with count 1: the entries are relabelled and inserted into a table of
 * S >= 2 * |L| slots, S a power of two (key ca << 32 | cb, all ones a free slot, home splitmix64(key) & (S - 1), linear
 * probing; count added, weight bits taken to their minimum), which in the first round also makes the edges distinct; a slot
 * is a link iff count == |ca| * |cb| (in 64 bits); every cluster's best link is found in two passes (the largest weight
 * bits, then the smallest id among those); the links are compacted into the next L (a slot that is no link is dropped for
 * good: no superset of an incomplete pair is complete); the reciprocal pairs merge, the larger id under the smaller.
 * `rounds` is the number of the first round that merged nothing, 1 for an edgeless graph: a property of the graph, not of
 * the schedule (a path with ascending ids and equal weights takes n / 2 + 1).  The global best link merges in every round,
 * so n rounds always do.  More than 2^32 - 17 edge records: LZANI_ERR_ARG; a workspace that does not fit:
 * LZANI_ERR_NOMEM, and the cluster state is as before the run; a probe sequence that runs out: LZANI_ERR_DEVICE.
 * LEIDEN on the device: the edge records are made distinct once per run in a table keyed lo << 32 | hi with a 64-bit
 * atomicMin of q, compacted into the level-0 entry list (the edge buffer is only read).  A moving round sums W(v, C) in a
 * table keyed node << 32 | community of the other end (S a power of two >= 2 * the insertions, atomicCAS on the key, 64-bit
 * atomicAdd on the sum, probing bounded by S); per slot it takes val(own), then the largest D per node (atomicMax) and
 * the smallest community id among the slots that equal it (atomicMin); the same max-then-min pair runs per community over
 * the candidates; every node decides for itself, and the smallest members, ids and sizes are recomputed.  A refinement
 * round has the same skeleton, with an entry pass for ext and the member counts.  All of it are the statement's rounds word
 * for word: `levels`, the round counts, `moves`, `merges` and `quality` of lzani_cluster_leiden_info are properties of
 * the graph.  More than 2^32 - 17 edge records or n > 2^21: LZANI_ERR_ARG; a workspace that does not fit: LZANI_ERR_NOMEM,
 * and the cluster state is as before the run; a probe sequence that runs out or a phase at its cap: LZANI_ERR_DEVICE. */
#define LZANI_CLUSTER_SINGLE        0
#define LZANI_CLUSTER_GREEDY_FIRST  1
#define LZANI_CLUSTER_GREEDY_BEST   2
#define LZANI_CLUSTER_SET_COVER     4   /* 4, not 3: 3 stays an unknown algorithm (tests/test_cluster.py holds 3 and -1 to LZANI_ERR_ARG) */
#define LZANI_CLUSTER_COMPLETE      6   /* 6, not 5: 3 and 5 stay unknown algorithms (tests/test_cluster_cover.py holds 3, 5 and -1 to LZANI_ERR_ARG) */
#define LZANI_CLUSTER_LEIDEN        8   /* 8, not 7: 3, 5 and 7 stay unknown algorithms (tests/test_cluster_link.py holds them to LZANI_ERR_ARG) */
#define LZANI_CLUSTER_TANI          0
#define LZANI_CLUSTER_GANI          1
#define LZANI_CLUSTER_ANI           2
typedef struct lzani_cluster_edge { uint32_t a, b; double w; } lzani_cluster_edge;      /* 16 bytes */
typedef struct lzani_cluster_info {
    uint32_t n;                       /* genomes                                                                 */
    int32_t  algo, measure;           /* of the last run (-1 before one); of the begin                           */
    uint32_t rounds;                  /* of the last run                                                         */
    uint64_t edges;                   /* edge records added so far (an edge added twice counts twice)            */
    uint64_t clusters, singletons, largest;   /* of the last run: clusters, those of one genome, the largest's size */
    uint64_t edge_bytes;              /* device bytes of the edge buffer                                         */
    double   add_ms, run_ms;          /* HIP events on the context's stream: the add_kept calls summed; the last run */
} lzani_cluster_info;
typedef struct lzani_cluster_cover_info {      /* of a LZANI_CLUSTER_SET_COVER run */
    uint64_t distinct_edges;          /* edges of the graph: the edge records without their repetitions             */
    uint64_t duplicate_edges;         /* edge records beyond the first of their pair (edges - distinct_edges)       */
    uint64_t workspace_bytes;         /* device bytes of the run's workspace: keys, sort scratch, the per-node words */
    double   dedup_ms, rounds_ms;     /* HIP events on the context's stream: keys, sort and unique; the rounds      */
} lzani_cluster_cover_info;
typedef struct lzani_cluster_link_info {       /* of a LZANI_CLUSTER_COMPLETE run */
    uint64_t distinct_edges;          /* edges of the graph: the edge records without their repetitions             */
    uint64_t duplicate_edges;         /* edge records beyond the first of their pair (edges - distinct_edges)       */
    uint64_t merges;                  /* merges of two clusters over all rounds (n - clusters)                      */
    uint64_t table_slots;             /* S of the first round: the smallest power of two >= 2 * edge records        */
    uint64_t workspace_bytes;         /* device bytes of the run's workspace: table, entry list, the per-cluster words */
    double   dedup_ms, rounds_ms;     /* HIP events on the context's stream: the first round's insert; all rounds   */
} lzani_cluster_link_info;
typedef struct lzani_cluster_leiden_info {     /* of a LZANI_CLUSTER_LEIDEN run */
    uint64_t iterations;              /* iterations run (the run stops after one without a move)                    */
    uint64_t levels;                  /* moving phases, over all iterations                                         */
    uint64_t move_rounds, refine_rounds;   /* rounds of all phases, the last of each phase (no mover) included      */
    uint64_t moves, merges;           /* movers of the moving rounds; movers of the refinement rounds               */
    int64_t  quality;                 /* Q of the result on the original graph, in units of 2^-20                   */
    uint64_t resolution_q;            /* g = llround(resolution * 2^20)                                             */
    uint64_t distinct_edges;          /* edges of the graph: the edge records without their repetitions             */
    uint64_t duplicate_edges;         /* edge records beyond the first of their pair (edges - distinct_edges)       */
    uint64_t table_slots;             /* S of the largest table: the smallest power of two >= 4 * edge records      */
    uint64_t workspace_bytes;         /* device bytes of the run's workspace: table, entry lists, per-node words    */
    double   dedup_ms, rounds_ms;     /* HIP events on the context's stream: the distinct edges; all iterations     */
} lzani_cluster_leiden_info;
/* The weight as a pure host function (no GPU).  NULL pointers or an unknown measure: NaN. */
double lzani_cluster_weight(int measure, const lzani_result *x, const lzani_result *y, uint32_t lines, uint32_t len_a, uint32_t len_b);
/* The sequential statement as a pure host function (no GPU).  rep_of[n]; cluster_of[n] and n_clusters may be NULL.  An edge
 * with a == b, an id >= n, a NaN or negative w, or an unknown algo: LZANI_ERR_ARG.  (b, a) with b > a is the edge (a, b). */
int lzani_cluster_host(uint32_t n, const lzani_cluster_edge *edges, uint64_t count, int algo, uint32_t *rep_of, uint32_t *cluster_of,
                       uint32_t *n_clusters);
/* LZANI_CLUSTER_LEIDEN as a pure host function with its parameters (lzani_cluster_host runs it with the defaults 0.7 and 2):
 * a sequential form of exactly the rounds of the statement.  info (may be NULL) receives the counts, quality and
 * resolution_q; its device fields are 0.  resolution outside [0, 1] or NaN, iterations outside 1..16, n > 2^21, a bad edge:
 * LZANI_ERR_ARG; a phase at its cap of rounds: LZANI_ERR_DEVICE. */
int lzani_cluster_leiden_host(uint32_t n, const lzani_cluster_edge *edges, uint64_t count, double resolution, int iterations,
                              uint32_t *rep_of, uint32_t *cluster_of, lzani_cluster_leiden_info *info);
/* Test hook: the same with a phase's cap of rounds set to cap_mul * n_level + cap_add in place of 64 * n_level + 64. */
int lzani_debug_cluster_leiden_host_cap(uint32_t n, const lzani_cluster_edge *edges, uint64_t count, double resolution, int iterations,
                                        uint64_t cap_mul, uint64_t cap_add, uint32_t *rep_of, uint32_t *cluster_of,
                                        lzani_cluster_leiden_info *info);
/* The parameters of LZANI_CLUSTER_LEIDEN runs of this context, until it is destroyed; the defaults are 0.7 and 2.
 * resolution outside [0, 1] or NaN, iterations outside 1..16: LZANI_ERR_ARG, and the parameters stay. */
int lzani_set_cluster_leiden(lzani_ctx *ctx, double resolution, int iterations);
/* An empty edge set for n genomes, whose reported lengths (NULL: the genome set's own, n must be its size) stay on the device.
 * Drops the cluster state there was; lzani_set_genomes drops it too.  No genome set: LZANI_ERR_STATE.  The drop comes
 * first: LZANI_ERR_NOMEM leaves the context without a cluster state (the cluster calls: LZANI_ERR_STATE until a begin
 * succeeds). */
int lzani_cluster_begin(lzani_ctx *ctx, uint32_t n, const uint32_t *report_len, int measure);
/* Appends the edges of the context's current kept result, one per record, weighted on the device.  No begin or no kept
 * result: LZANI_ERR_STATE; a kept result of another n: LZANI_ERR_ARG; LZANI_ERR_NOMEM leaves the edges that were there. */
int lzani_cluster_add_kept(lzani_ctx *ctx, uint64_t *edges_total);
/* Test hook: appends made-up edges from host memory, checked like those of lzani_cluster_host before anything runs.
 * LZANI_ERR_NOMEM leaves the edges that were there, and the last run's result with them. */
int lzani_debug_cluster_add_edges(lzani_ctx *ctx, const lzani_cluster_edge *edges, uint64_t count);
/* May be called again with another algo on the same edges.  No begin: LZANI_ERR_STATE.  Every algorithm allocates all
 * its run needs -- the result buffers included -- before it drops the last run's result: LZANI_ERR_NOMEM leaves the
 * cluster state as before the run, lzani_cluster_fetch and the info calls answer as they did. */
int lzani_cluster_run(lzani_ctx *ctx, int algo, uint64_t *n_clusters);
/* rep_of[n], cluster_of[n] of the last run; either may be NULL.  No run since the begin or the last add: LZANI_ERR_STATE. */
int lzani_cluster_fetch(lzani_ctx *ctx, uint32_t *rep_of, uint32_t *cluster_of);
/* LZANI_ERR_STATE before a begin. */
int lzani_get_cluster_info(const lzani_ctx *ctx, lzani_cluster_info *info);
/* LZANI_ERR_STATE unless the last run was one of LZANI_CLUSTER_SET_COVER. */
int lzani_get_cluster_cover_info(const lzani_ctx *ctx, lzani_cluster_cover_info *info);
/* LZANI_ERR_STATE unless the last run was one of LZANI_CLUSTER_COMPLETE. */
int lzani_get_cluster_link_info(const lzani_ctx *ctx, lzani_cluster_link_info *info);
/* LZANI_ERR_STATE unless the last run was one of LZANI_CLUSTER_LEIDEN. */
int lzani_get_cluster_leiden_info(const lzani_ctx *ctx, lzani_cluster_leiden_info *info);

/* ---- Cluster levels: cuts at cluster time, several clusterings of one run ------------------------------------------
 * Above, the edge threshold of the graph is the output filter of the kept call.  A record store keeps the kept records of
 * one or more kept calls on the device (36 B each), and a LEVEL makes the edges of a clustering from the store under a CUT
 * of its own: the alignment runs once under a loose filter, and any number of levels (measure, cut, algorithm) follow.
 *
 * Cut.  Five minima as lzani_out_filter's, a minimum of len_ratio and a maximum of num_alns; all zero passes everything
 * that an output filter whose minima are not negative kept (a negative value, which only made-up integers give, is below
 * the minimum 0 there as here).
 * Rule, for one kept record (a < b, X, Y, lines) with the reported lengths la, lb (lzani_cluster_plan.h: cluster_cut_lines,
 * over out_pair_tani, out_line_ratios and out_filter_line of lzani_out_filter.h):
 *   - the five values of line 0 ("b against a") and of line 1 ("a against b") are the output filter's; a line passes the
 *     five minima as there: a value passes unless it is < its minimum, and NaN and inf are below nothing;
 *   - len_ratio of the pair is the emitter's: (double)min(la, lb) / (double)max(la, lb), one IEEE division, where both
 *     lengths are nonzero, else 0; both lines pass unless len_ratio < min_len_ratio;
 *   - num_alns of line 0 is X.no_components, of line 1 Y.no_components; a line passes iff max_num_alns == 0 or
 *     (int64)no_components <= (int64)max_num_alns;
 *   - cut_lines = lines & (pass0 | pass1 << 1): a cut only takes away lines that the output filter kept;
 *   - the record is an edge of the level iff cut_lines != 0, and its weight is lzani_cluster_weight(measure, X, Y,
 *     cut_lines, la, lb): the weight above over the lines that remain.
 * A NaN minimum or reserved_ != 0: LZANI_ERR_ARG.
 * What the definition gives:
 *   - an all-zero cut makes, record for record and bit for bit, the edges that lzani_cluster_add_kept makes (of records
 *     kept under minima that are not negative: every line they name passes 0 again);
 *   - if every minimum of F' is >= that of F, a kept call under F followed by a level whose five minima are F' gives the
 *     edges of a kept call under F' followed by lzani_cluster_add_kept (passing F' implies passing F, NaN included);
 *   - levels are independent clusterings: nothing nests a strict level's clusters inside a loose one's, except where the
 *     algorithm gives it (single linkage).
 * Record store.  A lifetime group of the context like the kept result and the cluster state, from
 * lzani_cluster_store_begin to the next one or lzani_set_genomes: n, the n reported lengths on the device, and a buffer of
 * 9-word records grown geometrically by allocate-and-copy, as the edge buffer grows.  A failed growth leaves the records
 * that were there.  The store is independent of the cluster state: a level reads it, and no cluster call changes it.
 * The device stage (k_cl_level): blocks of 256 threads over 4,096 records each, 16 a thread; a count pass (the rule; edges per block of 4,096 records, the
 * lines in and out summed), a scan, the edge buffer reserved at the exact total, a write pass that stores one 16-byte edge
 * per passing record, in record order.  Per record 36 B and two lengths read, per edge 16 B written. */
typedef struct lzani_cluster_cut {
    double   min_tani, min_gani, min_ani, min_qcov, min_rcov;  /* as lzani_out_filter's            */
    double   min_len_ratio;                                    /* 0: none                          */
    uint32_t max_num_alns;                                     /* 0: none                          */
    uint32_t reserved_;                                        /* must be 0                        */
} lzani_cluster_cut;                                           /* 56 bytes; all zero: see "Cut" above  */
typedef struct lzani_cluster_store_info {
    uint32_t n;                       /* genomes                                                                 */
    uint64_t records;                /* records added so far                                                    */
    uint64_t record_bytes;            /* device bytes of the record buffer                                       */
    double   add_ms;                  /* HIP events on the context's stream: the appends summed                  */
} lzani_cluster_store_info;
typedef struct lzani_cluster_level_info {
    uint64_t records_in, edges_out;   /* the store's records; those of which a line stays: the level's edges     */
    uint64_t lines_in, lines_out;     /* set bits of `lines` and of cut_lines, summed over the records           */
    double   level_ms;                /* HIP events on the context's stream: count pass to write pass, the total's read-back and the edge allocation between them included */
} lzani_cluster_level_info;
/* The rule as a pure host function (no GPU): cut_lines.  NULL pointers, a NaN minimum or reserved_ != 0: 0xFFFFFFFF. */
uint32_t lzani_cluster_cut_lines(const lzani_cluster_cut *cut, const lzani_result *x, const lzani_result *y, uint32_t lines,
                                 uint32_t len_a, uint32_t len_b);
/* An empty record store for n genomes; report_len, rules and errors as in lzani_cluster_begin.  The drop of the old store
 * comes first: LZANI_ERR_NOMEM leaves no store.  The cluster state is not touched. */
int lzani_cluster_store_begin(lzani_ctx *ctx, uint32_t n, const uint32_t *report_len);
/* Appends the records of the context's current kept result by a device copy.  No store or no kept result: LZANI_ERR_STATE;
 * a kept result of another n: LZANI_ERR_ARG; LZANI_ERR_NOMEM leaves the records that were there. */
int lzani_cluster_store_add_kept(lzani_ctx *ctx, uint64_t *records_total);
/* lzani_cluster_begin(n, the store's lengths, measure) followed by the level's edges: afterwards the context is in an
 * ordinary begun cluster state, and lzani_cluster_run, fetch, add_kept, debug_add_edges and every info call behave as after
 * a begin plus adds.  The store is only read: the call may be repeated with another cut or measure any number of times.  As
 * in lzani_cluster_begin the old cluster state is dropped first: LZANI_ERR_NOMEM leaves no cluster state, the store intact,
 * and the call may be made again.  No store: LZANI_ERR_STATE; a NaN minimum, reserved_ != 0 or an unknown measure:
 * LZANI_ERR_ARG, before anything is dropped; more records than one launch covers: LZANI_ERR_ARG. */
int lzani_cluster_level(lzani_ctx *ctx, int measure, const lzani_cluster_cut *cut, uint64_t *edges);
/* LZANI_ERR_STATE without a store. */
int lzani_get_cluster_store_info(const lzani_ctx *ctx, lzani_cluster_store_info *info);
/* LZANI_ERR_STATE unless the current cluster state came from lzani_cluster_level. */
int lzani_get_cluster_level_info(const lzani_ctx *ctx, lzani_cluster_level_info *info);
/* Test hook: appends made-up records from host memory, checked first (a < b < n, lines in 1..3): LZANI_ERR_ARG before
 * anything runs.  LZANI_ERR_NOMEM leaves the records that were there. */
int lzani_debug_cluster_store_add(lzani_ctx *ctx, const lzani_kept_pair *rec, uint64_t count);
/* Test hook: edges first .. first + count - 1 of the current cluster state, in the buffer's order.  No cluster state:
 * LZANI_ERR_STATE; a range past the end: LZANI_ERR_ARG. */
int lzani_debug_cluster_edges(lzani_ctx *ctx, uint64_t first, uint64_t count, lzani_cluster_edge *out);

/* ---- Sharding over GPUs ---------------------------------------------------------------
 * The unit that shards is the reference's own work unit, one reference ROW (lz_matcher.cpp:196-255: a worker
 * takes a reference, builds its index once and parses every query of the row).  Rows are independent; the
 * genome set is replicated on every GPU; the only exchange is one gather of the per-pair results.
 * The reference itself self-schedules rows over threads with an atomic counter (lz_matcher.cpp:200); over
 * GPUs the rows are dealt up front by the partition below. */

/* cost(row) = sum of the row's query lengths + LZANI_ROW_COST_REF_WEIGHT * reference length: a pair costs
 * time proportional to its query length, the per-row index build that of a few pairs. */
#define LZANI_ROW_COST_REF_WEIGHT 6
int lzani_row_costs(uint32_t n_rows, const uint32_t *ref_ids, const uint64_t *row_off, const uint32_t *query_ids,
                    uint32_t n, const uint32_t *len, uint64_t *cost);

/* part_of_row[k] in [0, n_parts): row_cost == NULL deals the rows cyclically (dense all2all rows in the
 * reordered, length-descending id order cost the same); otherwise greedy longest-processing-time
 * (heaviest row first onto the least loaded shard) for the ragged rows a kmer-db filter leaves
 * (filter.cpp:301-345, lz_matcher.cpp:234-250).  Pure host function: needs no GPU. */
int lzani_partition_rows(uint32_t n_rows, const uint64_t *row_cost, uint32_t n_parts, uint32_t *part_of_row);

/* One process per GPU (torchrun / MPI launchers): an RCCL communicator bound to the context's device and
 * stream.  Rank 0 obtains an id, the caller distributes the LZANI_UNIQUE_ID_BYTES bytes by any means (file,
 * torch.distributed, MPI_Bcast), every rank calls lzani_comm_init.  Buffers are device pointers.
 *   allgather: every rank contributes n_results records (padded equal shards), every rank receives
 *              n_ranks * n_results in rank order;
 *   gatherv:   rank p contributes counts[p] records, the root receives them concatenated in rank order
 *              (grouped ncclSend / ncclRecv; d_recv is ignored elsewhere). */
#define LZANI_UNIQUE_ID_BYTES 128
int lzani_comm_unique_id(uint8_t *id);
int lzani_comm_init(lzani_ctx *ctx, uint32_t n_ranks, uint32_t rank, const uint8_t *id);
int lzani_comm_allgather(lzani_ctx *ctx, const void *d_send, void *d_recv, uint64_t n_results);
int lzani_comm_gatherv(lzani_ctx *ctx, const void *d_send, void *d_recv, const uint64_t *counts, uint32_t root);

/* One process, several GPUs (what `lz-ani --gpus n` uses): a context per listed device, each driven by its
 * own host thread; lzani_group_run_rows has the contract of lzani_run_rows -- it partitions the rows as above,
 * runs every shard on its device, gathers the shards on the first device over RCCL (ncclCommInitAll + grouped
 * ncclSend/ncclRecv), restores the caller's CSR order there and copies the results out once.
 * Listing one device twice is allowed for rehearsals on a single GPU (shards then move by device copies).
 * LZANI_ERR_NOMEM of a group call: what the single-context call promises holds for every device context; the group's
 * own buffers (gathered results, shard buffers, scatter table, pinned staging) are kept or released whole, never with a
 * stale size, and the same call may be made again.  lzani_group_run_rows_kept then leaves the first device's context
 * without a kept result. */
typedef struct lzani_group lzani_group;
int lzani_group_create(const lzani_params *p, uint32_t n_devices, const int *device_ids, lzani_group **out);
void lzani_group_destroy(lzani_group *grp);
const char *lzani_group_last_error(const lzani_group *grp);   /* grp == NULL: why the calling thread's last lzani_group_create failed */
int lzani_group_set_genomes(lzani_group *grp, uint32_t n, const uint8_t *const *codes, const uint32_t *len);
int lzani_group_run_rows(lzani_group *grp, uint32_t n_rows, const uint32_t *ref_ids, const uint64_t *row_off,
                         const uint32_t *query_ids, lzani_result *out);
int lzani_group_get_timing(const lzani_group *grp, uint32_t device_index, lzani_timing *t, double *gather_ms);
/* lzani_set_genome_memory / lzani_get_residency for every device context of the group. */
int lzani_group_set_genome_memory(lzani_group *grp, uint64_t bytes);
int lzani_group_get_residency(const lzani_group *grp, uint32_t device_index, lzani_residency_info *info);
/* lzani_run_rows_kept for the group: the shards are gathered and put into the caller's CSR order on the first device as in
 * lzani_group_run_rows, the output filter's stage runs there on that buffer, and the copy of the full results to the host
 * is left out.  The kept result belongs to the first device's context; the fetch and the info read it. */
int lzani_group_run_rows_kept(lzani_group *grp, uint32_t n_rows, const uint32_t *ref_ids, const uint64_t *row_off,
                              const uint32_t *query_ids, const lzani_out_filter *f, const uint32_t *report_len, uint64_t *n_kept);
int lzani_group_kept_fetch(lzani_group *grp, uint64_t first, uint64_t count, lzani_kept_pair *out);
int lzani_group_get_kept_info(const lzani_group *grp, lzani_kept_info *info);
/* The cluster stage for the group: on the first device's context, where the group's kept results are. */
int lzani_group_cluster_begin(lzani_group *grp, uint32_t n, const uint32_t *report_len, int measure);
int lzani_group_cluster_add_kept(lzani_group *grp, uint64_t *edges_total);
int lzani_group_cluster_run(lzani_group *grp, int algo, uint64_t *n_clusters);
int lzani_group_cluster_fetch(lzani_group *grp, uint32_t *rep_of, uint32_t *cluster_of);
int lzani_group_get_cluster_info(const lzani_group *grp, lzani_cluster_info *info);
int lzani_group_get_cluster_cover_info(const lzani_group *grp, lzani_cluster_cover_info *info);
int lzani_group_get_cluster_link_info(const lzani_group *grp, lzani_cluster_link_info *info);
int lzani_group_set_cluster_leiden(lzani_group *grp, double resolution, int iterations);
int lzani_group_get_cluster_leiden_info(const lzani_group *grp, lzani_cluster_leiden_info *info);
/* Cluster levels for the group: the record store and the levels on the first device's context. */
int lzani_group_cluster_store_begin(lzani_group *grp, uint32_t n, const uint32_t *report_len);
int lzani_group_cluster_store_add_kept(lzani_group *grp, uint64_t *records_total);
int lzani_group_cluster_level(lzani_group *grp, int measure, const lzani_cluster_cut *cut, uint64_t *edges);
int lzani_group_get_cluster_store_info(const lzani_group *grp, lzani_cluster_store_info *info);
int lzani_group_get_cluster_level_info(const lzani_group *grp, lzani_cluster_level_info *info);

/* The shard bookkeeping of lzani_group_run_rows as a pure host function (no GPU): rows keep their order inside
 * their shard, the shards follow each other in the gathered buffer (shard d from result shard_base[d] on,
 * shard_base has n_parts + 1 entries); entry j of the scatter table -- j counts the rows shard by shard,
 * row_of_entry[j] (may be NULL) names the row -- says where the row's results sit in the gathered buffer (src[j]),
 * where they belong in the caller's CSR order (dst[j] = row_off[row]) and how many there are (cnt[j]). */
int lzani_plan_gather(uint32_t n_rows, const uint64_t *row_off, const uint32_t *part_of_row, uint32_t n_parts,
                      uint64_t *shard_base, uint64_t *src, uint64_t *dst, uint64_t *cnt, uint32_t *row_of_entry);

/* Test hook: an allocation fault.  Every device and pinned-host allocation of the library, of any context and any thread
 * of the process, is an attempt; the attempts are numbered from 1, starting again at every call of this function.  The
 * call arms the fault so that the first-th attempt from now fails, and the count - 1 attempts behind it (count = 2^63:
 * every one from there on); first == 0 disarms, first > 0 with count == 0 is LZANI_ERR_ARG.  An attempt that is hit
 * behaves as a refused allocation does -- the buffer is left empty, the caller sees the runtime's out-of-memory code --
 * but the runtime is not called: no memory is exhausted and no error of the runtime is left behind.  *seen (may be NULL)
 * receives the attempts counted since the previous call, refused ones included.  Needs no context and no GPU.  Not for
 * production use: the fault is process-wide. */
int lzani_debug_alloc_fault(uint64_t first, uint64_t count, uint64_t *seen);

/* Test hook: copies out the device-built packed reference text and anchor index of one genome
 * (any pointer may be NULL).  Sizes: nm = ((T+63)/64+2) u64, t2 = twice that, with
 * T = 2*len+3*mrd; dirz = 2^dirbits+1 u32; ent <= T u32.  geom = {kb, dirbits, posbits, tagmask}.
 * Entries ascend inside every bucket of up to 32 entries; larger buckets (long low-complexity runs) are in
 * fill order, which no reader of the index depends on. */
int lzani_debug_get_index(lzani_ctx *ctx, uint32_t id, uint64_t *t2, uint64_t *nm,
                          uint32_t *dirz, uint32_t *ent, uint32_t *n_ent, uint32_t *geom);

/* Test hook: the engine's own radix sort of 64-bit keys (csrc/lzani_sort.hip; it orders the k-mers of a long reference
 * into its anchor index in place of the hash-table fill of prepare_ht_long, parser.cpp:146-189) on host arrays: n_seg
 * segments of seg_len keys each, every segment sorted by itself, stably, by the key bits [begin_bit, end_bit). */
int lzani_debug_sort_segments(lzani_ctx *ctx, const uint64_t *keys, uint64_t *out, uint64_t seg_len, uint32_t n_seg,
                              int begin_bit, int end_bit);

/* Test hook: the anchor indexes of one batch -- rows reference ids, repeats allowed -- built by the run's own index build
 * into slots 0 .. rows-1 (the run's environment switches apply), with or without the presence filter and, where the build
 * is the sort form, the tag words (what a batch of a run decides: with_filter, with_tw).  info receives the geometry,
 * the strides in 32-bit words per slot (0: not built) and which build ran; every non-NULL buffer receives rows x its
 * stride words: dirz, ent (dirz[slot][2^dirbits] entries valid), bk (4 words a bucket), tw, fl (the presence filter:
 * bit v & filter_mask for every k-mer word v of the slot's text) and, for the LDS build, status (nonzero: the slot did not
 * fit the block's LDS and was built by the global-atomics kernels).  More rows than the context's slab budget: LZANI_ERR_ARG. */
#define LZANI_INDEX_BUILD_LDS      0      /* k_idx_build, one block per slot through LDS (overflowing slots: global atomics) */
#define LZANI_INDEX_BUILD_ATOMICS  1      /* count / scan / fill / sort / buckets with global atomics                          */
#define LZANI_INDEX_BUILD_SORT     2      /* keys, radix sort by slot segment, one streaming pass                             */
typedef struct lzani_slab_info {
    int32_t  key_bits, dir_bits, pos_bits;
    uint32_t tag_mask, filter_mask;
    int32_t  build;                       /* LZANI_INDEX_BUILD_*                                                               */
    uint64_t dir_stride, ent_stride, bk_stride, tw_stride, fl_stride;
} lzani_slab_info;
int lzani_debug_index_slab(lzani_ctx *ctx, uint32_t rows, const uint32_t *ref_ids, int with_filter, int with_tw,
                           lzani_slab_info *info, uint32_t *dirz, uint32_t *ent, uint32_t *bk, uint32_t *tw, uint32_t *fl,
                           uint32_t *status);

/* Test hook: lzani_run_rows, and after every batch's candidate stage (dense rows and qualifying query lists: candidate
 * bitmaps from a presence matrix) the first `words` 32-bit words of every pair's candidate bitmap into cbits[pair * words]
 * and, where the batch counted them, the pair's candidate count into pcount[pair] (0xFFFFFFFF elsewhere); either may be
 * NULL.  Bit p of a bitmap: query position p has an anchor candidate in the pair's reference.  plan receives the
 * candidate form of the run. */
typedef struct lzani_cand_plan {
    int32_t  pm;                          /* 1: candidate bitmaps from presence matrices                                     */
    int32_t  pm_bits, rshift;             /* matrix of 2^pm_bits rows; row of a mixed hash h = (h >> rshift) & (2^pm_bits-1)  */
    uint32_t pm_group;                    /* reference slots per matrix                                                       */
    uint64_t cb_words;                    /* 32-bit words of one pair's bitmap                                                */
    uint32_t batches, from_index_launches, cand_launches, counted_batches;   /* k_pm_from_index / k_pm_cand launches       */
} lzani_cand_plan;
int lzani_debug_run_candidates(lzani_ctx *ctx, uint32_t n_rows, const uint32_t *ref_ids, const uint64_t *row_off,
                               const uint32_t *query_ids, lzani_result *out, uint64_t words, uint32_t *cbits,
                               uint32_t *pcount, lzani_cand_plan *plan);

#ifdef __cplusplus
}
#endif
#endif
