// lzani_sparse_plan.h -- the row tiles of the k-mer prefilter's count stage as one small host struct, and the tile plan
// of sparse counting (include/lzani.h: "Sparse counting") as a host function over it.  No HIP types: it compiles with a
// plain C++ compiler (tests/model/sparse_plan_check.cpp runs it under the sanitizers), and it is not among the sources a
// run-time compile embeds (lzani_rtc.h).  The driver of lzani_prefilter.h walks its tiles with PfTiles, and
// lzani_plan_sparse_tiles exports plan_sparse_tiles_impl.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "lzani.h"

namespace lzani {

// The row tiles of the count stage, one after the other: [r0, r1()) is the tile at work, of height h at most.  Dense: h is
// the matrix tile's height and every attempt finishes.  Sparse counting: h starts at n_rows; an attempt that overflowed
// the pair table halves it (halve(): false where one row alone was too much) and the same r0 is tried again; a finished
// tile leaves h as it is -- it does not grow back.
struct PfTiles {
    uint32_t n_rows, h, r0 = 0, attempts = 0, tiles = 0;
    PfTiles(uint32_t n_rows_, uint64_t h_) : n_rows(n_rows_), h((uint32_t)std::min<uint64_t>(std::max<uint64_t>(h_, 1), std::max<uint32_t>(n_rows_, 1))) {}
    bool more() const { return r0 < n_rows; }
    uint32_t r1() const { return (uint32_t)std::min<uint64_t>(n_rows, (uint64_t)r0 + h); }
    void attempt() { ++attempts; }
    bool halve() { if (h == 1) return false; h /= 2; return true; }
    void finished() { r0 = r1(); ++tiles; }
};
inline bool pf_slots_ok(uint64_t slots) { return slots >= 2 && (slots & (slots - 1)) == 0; }

// The tiles of sparse counting from the distinct pairs of every row (lzani_plan_sparse_tiles): an attempt overflows iff
// its rows hold more than slots / 2 pairs.  first[t] .. first[t + 1] are tile t's rows.  Returns the number of tiles,
// LZANI_ERR_ARG, or LZANI_ERR_NOMEM (a row above slots / 2).
inline int plan_sparse_tiles_impl(uint32_t n_rows, const uint64_t* row_pairs, uint64_t slots, std::vector<uint32_t>& first, uint32_t& attempts)
{
    if (!n_rows || !row_pairs || !pf_slots_ok(slots)) return LZANI_ERR_ARG;
    PfTiles t(n_rows, n_rows);
    first.assign(1, 0);
    while (t.more()) {
        t.attempt();
        uint64_t pairs = 0;
        for (uint32_t r = t.r0; r < t.r1() && pairs <= slots / 2; ++r) pairs += std::min<uint64_t>(row_pairs[r], slots);     // (no overflow of the sum)
        if (pairs > slots / 2) {
            if (!t.halve()) return LZANI_ERR_NOMEM;
            continue;
        }
        t.finished();
        first.push_back(t.r0);
    }
    attempts = t.attempts;
    return (int)t.tiles;
}

}  // namespace lzani
