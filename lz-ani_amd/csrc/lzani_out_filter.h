// lzani_out_filter.h -- the rule of the output filter, stated once (include/lzani.h, "output filter on the device"): which
// of the two TSV lines of an unordered pair pass the five minima.  The device stage (lzani_kernels_outfilter.h) and the pure
// host function lzani_out_filter_lines (lzani_kept.h) both call it.  Free of HIP types; compiled without fast-math and with
// -ffp-contract=off, like the rest of the library: every ratio is one IEEE double division of exact integers, as in the
// reference (lz_matcher.cpp:442-447), so host and device give the same bits.
#pragma once
#include <stdint.h>

#include "../../include/lzani.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LZANI_HD __host__ __device__
#else
#define LZANI_HD
#endif

namespace lzani {

// One line: the query's own result `own`, the other direction's `rev`, the query's and the reference's length.
LZANI_HD inline bool out_filter_line(const lzani_out_filter& f, double tani, const lzani_result& own, const lzani_result& rev, uint32_t qlen, uint32_t rlen)
{
    const int32_t aligned = (int32_t)((uint32_t)own.sym_in_matches + (uint32_t)own.sym_in_literals);
    const int32_t aligned_rev = (int32_t)((uint32_t)rev.sym_in_matches + (uint32_t)rev.sym_in_literals);
    const double gani = (double)own.sym_in_matches / qlen;
    const double ani = aligned != 0 ? (double)own.sym_in_matches / aligned : 0;
    const double qcov = (double)aligned / qlen;
    const double rcov = (double)aligned_rev / rlen;
    return !(tani < f.min_tani) && !(gani < f.min_gani) && !(ani < f.min_ani) && !(qcov < f.min_qcov) && !(rcov < f.min_rcov);
}

// lines of the pair a < b: X = result of (ref a, query b), Y = result of (ref b, query a), la / lb the reported lengths.
// Bit 0: the line "b against a" passes, bit 1: "a against b".
LZANI_HD inline uint32_t out_filter_lines(const lzani_out_filter& f, const lzani_result& X, const lzani_result& Y, uint32_t la, uint32_t lb)
{
    const int32_t mm = (int32_t)((uint32_t)X.sym_in_matches + (uint32_t)Y.sym_in_matches);
    const double tani = (double)mm / (uint32_t)(la + lb);
    return (out_filter_line(f, tani, X, Y, lb, la) ? 1u : 0u) | (out_filter_line(f, tani, Y, X, la, lb) ? 2u : 0u);
}

// a minimum that is not a number: refused by every entry point
LZANI_HD inline bool out_filter_has_nan(const lzani_out_filter& f)
{
    return f.min_tani != f.min_tani || f.min_gani != f.min_gani || f.min_ani != f.min_ani || f.min_qcov != f.min_qcov || f.min_rcov != f.min_rcov;
}

}  // namespace lzani
