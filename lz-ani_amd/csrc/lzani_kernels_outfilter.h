// lzani_kernels_outfilter.h -- device kernels of the output filter (lzani_kept.h): from a finished buffer of directed
// results, the unordered pairs of which at least one TSV line passes the minima (lzani_out_filter.h states the rule).
// Included by lzani_hip.hip only, behind lzani_kernels_prefilter.h, whose compaction (pf_compact: count, then write, with
// the block sum and the block rank of lzani_block.h) and scan (k_pf_scan) it uses.
//   k_of_kept<WRITE>   one thread per directed entry e of the call's CSR.  kept(e, v): the row of e by a binary search in
//                      row_off; b <= a is left out; the mate -- the entry (ref b, query a) -- through row_of[b] (the row of
//                      genome b, 0xFFFFFFFF: none of this call): position a of a dense row, a binary search for a in a list
//                      row; the rule; v = mate << 2 | lines.  put(at, v): the record, 32-bit fields by vector stores.  The
//                      count pass also sums, per block and with one atomic each, the leading entries without a mate and the
//                      lines that pass.
// The mate is an uncoalesced 12-byte gather; nothing here is tiled or tuned.  No kernel waits for another block; entry
// indexes are 64-bit throughout.
#pragma once
#include "lzani_out_filter.h"

namespace lzani {

constexpr u32 OF_NO_ROW = 0xFFFFFFFFu;
enum { OF_UNPAIRED = 0, OF_LINES = 1, OF_COUNTERS = 2 };

// The call as the kernels see it.  res: 3 ints per directed entry, CSR-aligned.  query_ids null: dense rows of n - 1 entries.
struct OfCall {
    const int* __restrict__ res;
    const u64* __restrict__ row_off;              // n_rows + 1
    const u32* __restrict__ ref_ids;              // n_rows
    const u32* __restrict__ query_ids;
    const u32* __restrict__ row_of;               // n: the row whose reference a genome is, or OF_NO_ROW
    const u32* __restrict__ len;                  // n: the reported lengths
    u32 n_rows, n;
    lzani_out_filter f;
};

__device__ __forceinline__ lzani_result of_result(const int* __restrict__ res, u64 e)
{
    return lzani_result{res[3 * e], res[3 * e + 1], res[3 * e + 2]};
}
// the row k with row_off[k] <= e < row_off[k + 1] (e below row_off[n_rows]; empty rows are stepped over)
__device__ __forceinline__ u32 of_row_of_entry(const u64* __restrict__ row_off, u32 n_rows, u64 e)
{
    u32 lo = 0, hi = n_rows;                      // the first k in [0, n_rows] with row_off[k] > e, minus one
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (row_off[mid] <= e) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}
// the query of entry e of row k, whose reference is r
__device__ __forceinline__ u32 of_query(const OfCall& c, u32 k, u32 r, u64 e)
{
    if (c.query_ids) return c.query_ids[e];
    const u32 j = (u32)(e - c.row_off[k]);
    return j + (j >= r ? 1u : 0u);
}
// the entry (ref of row k, query q), q != the row's reference r; false: the row does not list q
__device__ __forceinline__ bool of_find(const OfCall& c, u32 k, u32 r, u32 q, u64& e)
{
    const u64 b0 = c.row_off[k], b1 = c.row_off[k + 1];
    if (!c.query_ids) { e = b0 + (q < r ? q : q - 1); return e < b1; }
    u64 lo = b0, hi = b1;
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (c.query_ids[mid] < q) lo = mid + 1; else hi = mid;
    }
    e = lo;
    return lo < b1 && c.query_ids[lo] == q;
}

struct OfItem {
    OfCall c;
    u32* __restrict__ out;                        // WRITE: 9 words a record
    u32* unpaired_;                               // the thread's counts (the count pass)
    u32* lines_;
    __device__ __forceinline__ bool kept(u64 e, u64& v)
    {
        const u32 k = of_row_of_entry(c.row_off, c.n_rows, e);
        const u32 a = c.ref_ids[k], b = of_query(c, k, a, e);
        if (b <= a) return false;
        const u32 kb = c.row_of[b];
        u64 mate = 0;
        if (kb == OF_NO_ROW || !of_find(c, kb, b, a, mate)) { *unpaired_ += 1; return false; }
        const u32 lines = out_filter_lines(c.f, of_result(c.res, e), of_result(c.res, mate), c.len[a], c.len[b]);
        *lines_ += (lines & 1u) + (lines >> 1);
        v = (mate << 2) | lines;
        return lines != 0;
    }
    // v names the mate, the entry (ref b, query a); the leading entry (ref a, query b) is found from it the same way
    __device__ __forceinline__ void put(u64 at, u64 v) const
    {
        const u64 mate = v >> 2;
        const u32 kb = of_row_of_entry(c.row_off, c.n_rows, mate);
        const u32 b = c.ref_ids[kb], a = of_query(c, kb, b, mate);
        u64 e = 0;
        (void)of_find(c, c.row_of[a], a, b, e);   // (it is there: it led to the mate)
        const lzani_result X = of_result(c.res, e), Y = of_result(c.res, mate);
        u32* __restrict__ o = out + 9 * at;
        o[0] = a; o[1] = b;
        o[2] = (u32)X.sym_in_matches; o[3] = (u32)X.sym_in_literals; o[4] = (u32)X.no_components;
        o[5] = (u32)Y.sym_in_matches; o[6] = (u32)Y.sym_in_literals; o[7] = (u32)Y.no_components;
        o[8] = (u32)(v & 3u);
    }
};

// Block b: the PF_CHUNK entries from b * PF_CHUNK on of n_entries.  Count pass: blkcnt[b] = the kept pairs among them,
// counters[OF_UNPAIRED] += the leading entries without a mate, counters[OF_LINES] += the lines that pass.  Write pass: the
// records from blkoff[b] on, in entry order.
template <bool WRITE>
__global__ void __launch_bounds__(PF_THREADS) k_of_kept(OfCall c, u64 n_entries, u32* __restrict__ blkcnt, const u64* __restrict__ blkoff,
                                                        u32* __restrict__ out, unsigned long long* __restrict__ counters)
{
    __shared__ u32 s_extra[OF_COUNTERS];
    u32 unpaired = 0, lines = 0;
    if (!WRITE && threadIdx.x < OF_COUNTERS) s_extra[threadIdx.x] = 0;       // (pf_compact's count pass begins with a barrier)
    pf_compact<WRITE>(n_entries, blkcnt, blkoff, OfItem{c, out, &unpaired, &lines});
    if (!WRITE) {
        block_sum(unpaired, &s_extra[OF_UNPAIRED]);
        block_sum(lines, &s_extra[OF_LINES]);
        if (threadIdx.x < OF_COUNTERS && s_extra[threadIdx.x]) atomicAdd(&counters[threadIdx.x], (unsigned long long)s_extra[threadIdx.x]);
    }
}

}  // namespace lzani
