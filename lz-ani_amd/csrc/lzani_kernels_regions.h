// lzani_kernels_regions.h -- device kernels of the alignment-region stage (lzani_regions.h): from a finished buffer of raw
// region records, in no order, the regions of the entries that pass the alignment's rule (lzani_aln_rule.h), in file order.
// Included by lzani_hip.hip only, behind lzani_kernels_outfilter.h, whose row search (of_row_of_entry) it uses, and
// lzani_kernels_prefilter.h, whose compaction (pf_compact) and scan (k_pf_scan) it uses.
//   k_rg_sums       one thread per raw region: its two counts added to its entry's sums (32-bit integer atomics: exact, so
//                   the order never shows) and the entry's bit set in the `has` bitmap.  An entry that owns thousands of
//                   regions is a hot address; the adds of one wave to one address are serialised by the L2 atomic unit and
//                   nothing waits for their result
//   k_rg_pass       one thread per entry: the rule on the sums of the entries that have a region; a wave's 64 verdicts are
//                   one ballot, written as one word of the `keep` bitmap by a plain vector store (entries are numbered from a
//                   multiple of 64 per wave).  Per block and with one atomic each: the entries with regions, those dropped
//   k_rg_keys<W>    pf_compact over the raw regions: those whose entry stays, as  seq_start << 32 | raw index, in raw order.
//                   The count pass also takes the largest seq_start and the largest length among them (the bits the sorts
//                   have to cover)
//   k_rg_rekey<F>   between two sorts: the key's field rebuilt from regions[index]: F = 1  maxlen - length, F = 2  the entry
//   k_rg_gather     the 32-byte records in the sorted order, two 16-byte loads and stores each
// The sorts between them are lzani_sort_keys (lzani_sort.hip): stable, least significant field first.  No kernel waits for
// another block; everything a later pass reads crosses a kernel boundary; indexes are 64-bit throughout.
#pragma once
#include "lzani_aln_rule.h"

namespace lzani {

enum { RG_WITH = 0, RG_DROPPED = 1, RG_MAX_START = 2, RG_MAX_LEN = 3, RG_COUNTERS = 4 };

// The call as k_rg_pass sees it.  query_ids null: dense rows.  filtered 0: no entry is dropped (a NULL filter).
struct RgCall {
    const u64* __restrict__ row_off;              // n_rows + 1
    const u32* __restrict__ ref_ids;              // n_rows
    const u32* __restrict__ query_ids;
    const u32* __restrict__ len;                  // n: the lengths the rule divides by
    u32 n_rows;
    int filtered;
    u64 entries;
    lzani_out_filter f;
};

__device__ __forceinline__ bool rg_bit(const unsigned long long* __restrict__ bits, u64 e) { return (bits[e >> 6] >> (e & 63)) & 1ull; }

__global__ void __launch_bounds__(PF_THREADS) k_rg_sums(const lzani_region* __restrict__ r, u64 n, u64 entries, int* __restrict__ sums,
                                                        unsigned long long* __restrict__ has)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= n) return;
    const u64 e = r[i].pair;
    if (e >= entries) return;                     // (no pair kernel writes one, and the host refuses one: nothing is written out of bounds)
    atomicAdd(&sums[2 * e], r[i].num_matches);
    atomicAdd(&sums[2 * e + 1], r[i].num_mismatches);
    atomicOr(&has[e >> 6], 1ull << (e & 63));
}

__global__ void __launch_bounds__(PF_THREADS) k_rg_pass(RgCall c, const int* __restrict__ sums, const unsigned long long* __restrict__ has,
                                                        unsigned long long* __restrict__ keep, unsigned long long* __restrict__ counters)
{
    __shared__ u32 s_cnt[2];
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const u64 e = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    bool with = false, stay = false;
    if (e < c.entries) {
        with = rg_bit(has, e);
        stay = with;
        if (with && c.filtered) {
            u32 b;
            if (c.query_ids) b = c.query_ids[e];
            else {
                const u32 k = of_row_of_entry(c.row_off, c.n_rows, e);
                const u32 a = c.ref_ids[k], j = (u32)(e - c.row_off[k]);
                b = j + (j >= a ? 1u : 0u);
            }
            stay = !aln_entry_dropped(c.f, sums[2 * e], sums[2 * e + 1], c.len[b]);
        }
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(stay);
    if ((threadIdx.x & 63) == 0 && e < c.entries) keep[e >> 6] = m;
    block_sum(with ? 1u : 0u, &s_cnt[RG_WITH]);
    block_sum(with && !stay ? 1u : 0u, &s_cnt[RG_DROPPED]);
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&counters[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

struct RgKeyItem {
    const lzani_region* __restrict__ r;
    const unsigned long long* __restrict__ keep;
    u64 entries;
    unsigned long long* __restrict__ out;         // WRITE
    u32* max_start_;                              // the thread's maxima (the count pass)
    u32* max_len_;
    __device__ __forceinline__ bool kept(u64 i, u64& v) const
    {
        const u64 e = r[i].pair;
        if (e >= entries || !rg_bit(keep, e)) return false;
        const u32 s = (u32)r[i].seq_start, l = (u32)(r[i].seq_end - r[i].seq_start);
        if (s > *max_start_) *max_start_ = s;
        if (l > *max_len_) *max_len_ = l;
        v = ((u64)s << 32) | (u32)i;
        return true;
    }
    __device__ __forceinline__ void put(u64 at, u64 v) const { out[at] = v; }
};

// Block b: the PF_CHUNK raw regions from b * PF_CHUNK on of n.  Count pass: blkcnt[b] = those that stay, and the two maxima
// into counters.  Write pass: their keys from blkoff[b] on, in raw order.
template <bool WRITE>
__global__ void __launch_bounds__(PF_THREADS) k_rg_keys(const lzani_region* __restrict__ r, u64 n, const unsigned long long* __restrict__ keep, u64 entries,
                                                        u32* __restrict__ blkcnt, const u64* __restrict__ blkoff, unsigned long long* __restrict__ out,
                                                        unsigned long long* __restrict__ counters)
{
    __shared__ u32 s_max[2];
    u32 ms = 0, ml = 0;
    if (!WRITE && threadIdx.x < 2) s_max[threadIdx.x] = 0;                    // (pf_compact's count pass begins with a barrier)
    pf_compact<WRITE>(n, blkcnt, blkoff, RgKeyItem{r, keep, entries, out, &ms, &ml});
    if (!WRITE) {
        for (int d = 32; d >= 1; d >>= 1) {
            const u32 os = __shfl_xor(ms, d), ol = __shfl_xor(ml, d);
            ms = os > ms ? os : ms;
            ml = ol > ml ? ol : ml;
        }
        if ((threadIdx.x & 63) == 0) { if (ms) atomicMax(&s_max[0], ms); if (ml) atomicMax(&s_max[1], ml); }
        __syncthreads();
        if (threadIdx.x < 2 && s_max[threadIdx.x]) atomicMax(&counters[RG_MAX_START + threadIdx.x], (unsigned long long)s_max[threadIdx.x]);
    }
}

template <int FIELD>
__global__ void __launch_bounds__(PF_THREADS) k_rg_rekey(const lzani_region* __restrict__ r, unsigned long long* __restrict__ keys, u64 n, u32 maxlen)
{
    const u64 j = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (j >= n) return;
    const u32 i = (u32)keys[j];
    const u32 v = FIELD == 1 ? maxlen - (u32)(r[i].seq_end - r[i].seq_start) : (u32)r[i].pair;
    keys[j] = ((u64)v << 32) | i;
}

__global__ void __launch_bounds__(PF_THREADS) k_rg_gather(const lzani_region* __restrict__ r, const unsigned long long* __restrict__ keys, u64 n,
                                                          lzani_region* __restrict__ out)
{
    const u64 j = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (j >= n) return;
    const uint4* src = reinterpret_cast<const uint4*>(r + (u32)keys[j]);
    uint4* dst = reinterpret_cast<uint4*>(out + j);
    const uint4 lo = src[0], hi = src[1];
    dst[0] = lo;
    dst[1] = hi;
}

}  // namespace lzani
