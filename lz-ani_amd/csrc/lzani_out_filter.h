// lzani_out_filter.h -- the rule of the output filter, stated once (include/lzani.h, "output filter on the device"): the
// five values of a TSV line, and which of the two lines of an unordered pair pass the five minima.  The device stage
// (lzani_kernels_outfilter.h), the pure host function lzani_out_filter_lines (lzani_kept.h) and the host binary's emitter
// (host/emit.h, which prints the values it filters by) all call it.  Free of HIP types; compiled without fast-math and with
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

// The five values of one TSV line, as the emitter prints them and the filter compares them.
struct out_ratios { double tani, gani, ani, qcov, rcov; };

// tani of the pair a < b, shared by its two lines: the sums are unsigned 32-bit, the matches' cast back.
LZANI_HD inline double out_pair_tani(const lzani_result& X, const lzani_result& Y, uint32_t la, uint32_t lb)
{
    const int32_t mm = (int32_t)((uint32_t)X.sym_in_matches + (uint32_t)Y.sym_in_matches);
    return (double)mm / (uint32_t)(la + lb);
}

// One line: the query's own result `own`, the other direction's `rev`, the query's and the reference's length.
LZANI_HD inline out_ratios out_line_ratios(double tani, const lzani_result& own, const lzani_result& rev, uint32_t qlen, uint32_t rlen)
{
    const int32_t aligned = (int32_t)((uint32_t)own.sym_in_matches + (uint32_t)own.sym_in_literals);
    const int32_t aligned_rev = (int32_t)((uint32_t)rev.sym_in_matches + (uint32_t)rev.sym_in_literals);
    return out_ratios{tani, (double)own.sym_in_matches / qlen, aligned != 0 ? (double)own.sym_in_matches / aligned : 0, (double)aligned / qlen,
                      (double)aligned_rev / rlen};
}

// a line passes unless one of its values is below its minimum (NaN is below nothing, and nothing is below a NaN)
LZANI_HD inline bool out_filter_line(const lzani_out_filter& f, const out_ratios& v)
{
    return !(v.tani < f.min_tani) && !(v.gani < f.min_gani) && !(v.ani < f.min_ani) && !(v.qcov < f.min_qcov) && !(v.rcov < f.min_rcov);
}

// lines of the pair a < b: X = result of (ref a, query b), Y = result of (ref b, query a), la / lb the reported lengths.
// Bit 0: the line "b against a" passes, bit 1: "a against b".
LZANI_HD inline uint32_t out_filter_lines(const lzani_out_filter& f, const lzani_result& X, const lzani_result& Y, uint32_t la, uint32_t lb)
{
    const double tani = out_pair_tani(X, Y, la, lb);
    return (out_filter_line(f, out_line_ratios(tani, X, Y, lb, la)) ? 1u : 0u) | (out_filter_line(f, out_line_ratios(tani, Y, X, la, lb)) ? 2u : 0u);
}

// a minimum that is not a number: refused by every entry point
LZANI_HD inline bool out_filter_has_nan(const lzani_out_filter& f)
{
    return f.min_tani != f.min_tani || f.min_gani != f.min_gani || f.min_ani != f.min_ani || f.min_qcov != f.min_qcov || f.min_rcov != f.min_rcov;
}

}  // namespace lzani
