// lzani_pair_dispatch.h -- which pair kernel a batch launches: the table of the pair-kernel instantiations (the launch
// record's rows) and the one function from the facts of a launch to its row.  No HIP types: it compiles with a plain C++
// compiler (tests/model/pair_dispatch_check.cpp runs it under the sanitizers over every consistent combination of the
// facts), and it is not among the sources a run-time compile embeds (lzani_rtc.h).  lzani_hip.hip keeps the kernels'
// host addresses beside the table, built from the same lists, and launches every pair kernel through its row.
#pragma once

namespace lzani {

// The instantiations, one list per kind and every row spelled once: its name, its fields and (lzani_hip.hip) its kernel
// come from the same tokens.  The names follow one grammar a test can build from the dispatch rules:
//   pairs fast=F nfree=N defp=D aln=A bk=B cand=C   k_pairs<F, N, D, A, B, C>
//   pairs_blk nfree=N defp=D                        k_pairs_blk<N, D>
//   split nfree=N defp=D mode=M                     k_split<N, D, M>   (mode 1 is the row behind mode 0)
//   rtc nfree=N cand=C                              the run-time compiled kernel (lzani_rtc.h), DEFP 9
// An instantiation added to the dispatch is one row here, one case of choose_pair_kernel and a cell in
// tests/test_gpu_instantiations.py.  The order is the order of the launch record (lzani_debug_kernel_name).
#define LZANI_PK_PAIRS_ROWS(X)                                                                                        \
    X(0, 0, 0, 1, 0, 0) X(1, 0, 0, 1, 1, 0) X(1, 0, 0, 1, 0, 0) X(0, 0, 0, 0, 0, 0)                                    \
    X(1, 0, 0, 0, 1, 2) X(1, 0, 1, 0, 1, 2) X(1, 0, 2, 0, 1, 2) X(1, 1, 0, 0, 1, 2) X(1, 1, 1, 0, 1, 2) X(1, 1, 2, 0, 1, 2) \
    X(1, 0, 0, 0, 1, 1) X(1, 0, 1, 0, 1, 1) X(1, 0, 2, 0, 1, 1) X(1, 1, 0, 0, 1, 1) X(1, 1, 1, 0, 1, 1) X(1, 1, 2, 0, 1, 1) \
    X(1, 0, 0, 0, 1, 0) X(1, 0, 1, 0, 1, 0) X(1, 1, 0, 0, 1, 0) X(1, 1, 1, 0, 1, 0)                                    \
    X(1, 0, 0, 0, 0, 0) X(1, 0, 1, 0, 0, 0) X(1, 1, 0, 0, 0, 0) X(1, 1, 1, 0, 0, 0)
#define LZANI_PK_BLK_ROWS(X) X(0, 0) X(0, 1) X(1, 0) X(1, 1)
#define LZANI_PK_SPLIT_ROWS(X)                                                                                        \
    X(0, 0, 0) X(0, 0, 1) X(0, 1, 0) X(0, 1, 1) X(0, 2, 0) X(0, 2, 1) X(1, 0, 0) X(1, 0, 1) X(1, 1, 0) X(1, 1, 1) X(1, 2, 0) X(1, 2, 1)
#define LZANI_PK_RTC_ROWS(X) X(0, 0) X(0, 1) X(0, 2) X(1, 0) X(1, 1) X(1, 2)

enum PairKernelKind { PK_PAIRS, PK_BLK, PK_SPLIT, PK_RTC };
struct PairKernelDesc { const char* name; int kind, fast, nfree, defp, aln, bk, cand, mode; };
#define LZANI_PK_PAIRS_DESC(F, N, D, A, B, C) {"pairs fast=" #F " nfree=" #N " defp=" #D " aln=" #A " bk=" #B " cand=" #C, PK_PAIRS, F, N, D, A, B, C, 0},
#define LZANI_PK_BLK_DESC(N, D) {"pairs_blk nfree=" #N " defp=" #D, PK_BLK, 1, N, D, 0, 1, 0, 0},
#define LZANI_PK_SPLIT_DESC(N, D, M) {"split nfree=" #N " defp=" #D " mode=" #M, PK_SPLIT, 1, N, D, 0, 1, 2, M},
#define LZANI_PK_RTC_DESC(N, C) {"rtc nfree=" #N " cand=" #C, PK_RTC, 1, N, 9, 0, 1, C, 0},
constexpr PairKernelDesc PAIR_KERNELS[] = {
    LZANI_PK_PAIRS_ROWS(LZANI_PK_PAIRS_DESC) LZANI_PK_BLK_ROWS(LZANI_PK_BLK_DESC) LZANI_PK_SPLIT_ROWS(LZANI_PK_SPLIT_DESC)
    LZANI_PK_RTC_ROWS(LZANI_PK_RTC_DESC)
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

// What a pair launch goes by.
struct PairFacts {
    bool regions = false;         // alignment output (lzani_run_rows_regions)
    bool fast = false;            // the genome set has k-mer words (mal, msl <= 15)
    bool tw = false;              // the index has tag words: the anchor queue
    bool pm = false;              // candidates from bitmaps made ahead (dense rows)
    bool split = false;           // ... few, long pairs: several waves a pair
    bool join = false;            // candidates by the join of sorted k-mer lists (long genomes)
    bool blk = false;             // rows for the block kernel, and its LDS filter fits
    bool nfree = false;           // no genome holds an N
    int dsel = 0;                 // the tuple folded ahead of time: 1 the defaults, 2 the long-genome parameters, 0 neither
    bool rtc = false;             // the tuple's run-time compiled kernel is in hand
};
// row: the ahead-of-time instantiation (a split: its mode 0, mode 1 is the next row); rtc_row: the run-time compiled
// kernel to try first, -1 = none.
struct PairChoice { int row, rtc_row; };

// CAND of the form a run's pair launches take -- 2 candidate bitmaps, 1 join, 0 probe with the anchor queue -- or -1:
// a form without a run-time compiled kernel.  (Before the batches: which kernel to ask lzani_rtc::get for.)
constexpr int pair_cand(bool pm, bool join, bool tw) { return pm ? 2 : (join && tw) ? 1 : tw ? 0 : -1; }

// The block kernel's row: the probe forms and the block kernel have no instance for the long-genome tuple, which runs
// their DEFP 0.  (Before the facts are complete: whether its LDS filter fits is asked of this kernel.)
constexpr int pair_blk_row(bool nfree, int dsel) { return pk_id(PK_BLK, 1, nfree, dsel == 1, 0, 1, 0, 0); }

// The pair kernel of a launch.
constexpr PairChoice choose_pair_kernel(const PairFacts& f)
{
    const int n = f.nfree, d2 = f.dsel == 1;
    // alignment output: one generic instantiation per index form
    if (f.regions) return {pk_id(PK_PAIRS, f.fast, 0, 0, 1, f.fast && f.tw, 0, 0), -1};
    if (!f.fast) return {pk_id(PK_PAIRS, 0, 0, 0, 0, 0, 0, 0), -1};
    if (f.pm && f.split) return {pk_id(PK_SPLIT, 1, n, f.dsel, 0, 1, 2, 0), -1};
    const int rtc_row = f.rtc ? pk_id(PK_RTC, 1, n, 9, 0, 1, pair_cand(f.pm, f.join, f.tw), 0) : -1;
    if (f.pm) return {pk_id(PK_PAIRS, 1, n, f.dsel, 0, 1, 2, 0), rtc_row};
    if (f.tw && f.join) return {pk_id(PK_PAIRS, 1, n, f.dsel, 0, 1, 1, 0), rtc_row};
    if (f.blk) return {pair_blk_row(f.nfree, f.dsel), -1};
    if (f.tw) return {pk_id(PK_PAIRS, 1, n, d2, 0, 1, 0, 0), rtc_row};
    return {pk_id(PK_PAIRS, 1, n, d2, 0, 0, 0, 0), -1};
}

}  // namespace lzani
