// lzani_aln_rule.h -- the rule of the alignment output, stated once (include/lzani.h, "alignment regions on the device"):
// which directed pairs keep their regions in the file of --out-alignment.  The reference sums a pair's regions and drops the
// pair when one of three ratios of the sums is below its minimum (lz_matcher.cpp:115-138); it reads min_gani, min_ani and
// min_qcov only.  The device stage (lzani_kernels_regions.h), the pure host statement lzani_regions_host (lzani_regions.h)
// and the host binary (host/match.h) all call it.  Free of HIP types, and so is the host statement of the whole stage below it
// (aln_host_order); compiled with -ffp-contract=off like the rest: every
// ratio is one IEEE double division of exact integers, so host and device give the same bits.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#include "lzani_out_filter.h"

namespace lzani {

// The three values of one directed entry: mat, lit the 32-bit sums over its regions, len the query's length.
struct aln_ratios { double gani, ani, qcov; };

LZANI_HD inline aln_ratios aln_entry_ratios(int32_t mat, int32_t lit, uint32_t len)
{
    const int32_t aligned = (int32_t)((uint32_t)mat + (uint32_t)lit);
    return aln_ratios{(double)mat / len, aligned != 0 ? (double)mat / aligned : 0, (double)aligned / len};
}

// the entry is dropped iff one of its values is below its minimum (NaN and inf are below nothing; equal stays)
LZANI_HD inline bool aln_entry_dropped(const lzani_out_filter& f, int32_t mat, int32_t lit, uint32_t len)
{
    const aln_ratios v = aln_entry_ratios(mat, lit, len);
    return v.gani < f.min_gani || v.ani < f.min_ani || v.qcov < f.min_qcov;
}

// a minimum of the three that is not a number: refused by every entry point
LZANI_HD inline bool aln_filter_has_nan(const lzani_out_filter& f)
{
    return f.min_gani != f.min_gani || f.min_ani != f.min_ani || f.min_qcov != f.min_qcov;
}

// The order inside an entry: the longer seq_end - seq_start first, then the smaller seq_start.
LZANI_HD inline bool aln_region_before(const lzani_region& x, const lzani_region& y)
{
    const int32_t lx = x.seq_end - x.seq_start, ly = y.seq_end - y.seq_start;
    if (x.pair != y.pair) return x.pair < y.pair;
    if (lx != ly) return lx > ly;
    return x.seq_start < y.seq_start;
}

// The statement of the stage on the host, the one copy of it: lzani_regions_host is this behind its checks, and a host binary
// whose library lacks that symbol calls it as it stands.  The call's rows passed the checks of the kept forms, every region's
// pair is one of its entries; f null: no entry is dropped.  order = the raw indexes of the regions that stay, in the
// result's order (a stable sort: ties keep their input order); the 32-bit sums are made as the reference makes them.
struct aln_host_counts { uint64_t entries_with_regions = 0, entries_dropped = 0; };

inline void aln_host_order(uint32_t n_rows, const uint32_t* ref_ids, const uint64_t* row_off, const uint32_t* query_ids, const uint32_t* aln_len,
                           const lzani_region* r, uint64_t count, const lzani_out_filter* f, std::vector<uint64_t>& order, aln_host_counts& cnt)
{
    std::vector<uint64_t> idx(count);
    for (uint64_t i = 0; i < count; ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](uint64_t x, uint64_t y) { return aln_region_before(r[x], r[y]); });
    order.clear();
    for (uint64_t k = 0; k < count;) {
        uint64_t k1 = k;
        uint32_t mat = 0, lit = 0;
        const uint64_t e = r[idx[k]].pair;
        for (; k1 < count && r[idx[k1]].pair == e; ++k1) { mat += (uint32_t)r[idx[k1]].num_matches; lit += (uint32_t)r[idx[k1]].num_mismatches; }
        cnt.entries_with_regions += 1;
        bool stay = true;
        if (f) {
            const uint32_t row = (uint32_t)(std::upper_bound(row_off, row_off + n_rows + 1, e) - row_off - 1);
            const uint32_t a = ref_ids[row], j = (uint32_t)(e - row_off[row]);
            const uint32_t b = query_ids ? query_ids[e] : j + (j >= a ? 1u : 0u);
            stay = !aln_entry_dropped(*f, (int32_t)mat, (int32_t)lit, aln_len[b]);
        }
        if (stay) order.insert(order.end(), idx.begin() + (ptrdiff_t)k, idx.begin() + (ptrdiff_t)k1);
        else cnt.entries_dropped += 1;
        k = k1;
    }
}

}  // namespace lzani
