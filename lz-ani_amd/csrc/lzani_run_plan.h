// lzani_run_plan.h -- the pure host decisions of a run (lzani_hip.hip, lzani_dense.h): the batches of its rows, the
// per-XCD work queues of every batch, the split / longest-pair-first rule of a dense batch, the bytes of one index slab
// slot.  No HIP types: it compiles with a plain C++ compiler (tests/model/run_plan_check.cpp runs it under the
// sanitizers), and it is not among the sources a run-time compile embeds (lzani_rtc.h).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <optional>
#include <vector>

namespace lzani {

// Batches of consecutive rows: at most rows_cap rows and cap_pairs pairs each (a row above cap_pairs is a batch of its
// own).  bstart: batch b = rows [bstart[b], bstart[b + 1]).  Returns the most pairs of a batch.
inline uint64_t cut_batches(uint32_t n_rows, const uint64_t* row_off, uint32_t rows_cap, uint64_t cap_pairs, std::vector<uint32_t>& bstart)
{
    bstart.assign(1, 0);
    uint32_t rows = 0;
    uint64_t pairs = 0, most = 0;
    for (uint32_t k = 0; k < n_rows; ++k) {
        const uint64_t len = row_off[k + 1] - row_off[k];
        if (rows && (rows == rows_cap || pairs + len > cap_pairs)) { bstart.push_back(k); most = std::max(most, pairs); rows = 0; pairs = 0; }
        ++rows; pairs += len;
    }
    bstart.push_back(n_rows);
    return std::max(most, pairs);
}

// The work queues of every batch, n_queues each (the pair kernels' NQUEUES: one per XCD): a batch's rows, longest first
// onto the least loaded queue (equal rows: round robin).  qorder: the batch's rows queue after queue, qcum: their running
// pair count (one entry more per batch), qb: where each queue begins in qorder (n_queues + 1 entries per batch).
struct QueuePlan { std::vector<uint32_t> qorder; std::vector<uint64_t> qcum; std::vector<uint32_t> qb; };

inline QueuePlan plan_queues(uint32_t n_rows, const uint64_t* row_off, const std::vector<uint32_t>& bstart, uint32_t n_queues)
{
    const uint32_t n_batches = (uint32_t)bstart.size() - 1;
    QueuePlan qp{std::vector<uint32_t>(n_rows), std::vector<uint64_t>((size_t)n_rows + n_batches), std::vector<uint32_t>((size_t)n_batches * (n_queues + 1))};
    std::vector<uint32_t> by_size;
    std::vector<std::vector<uint32_t>> queue(n_queues);
    std::vector<uint64_t> load(n_queues);
    for (uint32_t b = 0; b < n_batches; ++b) {
        const uint32_t k0 = bstart[b], rows = bstart[b + 1] - k0;
        auto rlen = [&](uint32_t k) { return row_off[k0 + k + 1] - row_off[k0 + k]; };
        by_size.resize(rows);
        for (uint32_t k = 0; k < rows; ++k) by_size[k] = k;
        std::stable_sort(by_size.begin(), by_size.end(), [&](uint32_t x, uint32_t y) { return rlen(x) > rlen(y); });
        std::fill(load.begin(), load.end(), 0);
        for (auto& q : queue) q.clear();
        for (uint32_t k : by_size) {
            uint32_t best = 0;
            for (uint32_t x = 1; x < n_queues; ++x) if (load[x] < load[best]) best = x;
            queue[best].push_back(k);
            load[best] += rlen(k);
        }
        uint32_t at = 0;
        uint64_t cum = 0;
        uint32_t* qo = qp.qorder.data() + k0;
        uint64_t* qc = qp.qcum.data() + k0 + b;
        qc[0] = 0;
        for (uint32_t x = 0; x < n_queues; ++x) {
            qp.qb[(size_t)b * (n_queues + 1) + x] = at;
            for (uint32_t k : queue[x]) { qo[at] = k; cum += rlen(k); qc[++at] = cum; }
        }
        qp.qb[(size_t)b * (n_queues + 1) + n_queues] = at;
    }
    return qp;
}

// The split / longest-pair-first rule of a dense batch whose candidates come from bitmaps.
//   pairs > 0: the batch's pairs;  slots: the device's wave slots;  cb_words: 32-bit words of one pair's candidate bitmap;
//   dmax: the longest genome + mrd, what a pair's scan covers.
// The switches as the run read them (empty: the rule decides): split, lpt; split_s segments a pair at most, split_seglen > 0
// the segment length instead.  (Which pairs of a split batch are cut -- split_all, split_thr -- is decided later, from the
// candidate counts: it does not bear on S, the segment length or lpt.)
struct SplitKnobs { std::optional<bool> split, lpt; uint64_t split_s = 64; int split_seglen = 0; };
// split_S >= 2: every pair by several waves, in segments of split_seglen positions; lpt: the candidate counts are wanted
// (ticket order, longest pair first -- or the split's choice of pairs)
struct SplitChoice { uint32_t split_S = 0; int split_seglen = 0; bool lpt = false; };

inline SplitChoice choose_split(uint64_t pairs, uint64_t slots, uint64_t cb_words, int dmax, const SplitKnobs& k)
{
    SplitChoice ch;
    const uint64_t bp = pairs;
    // Few, long pairs (the batch leaves a wave slot only a few of them): the launch is over when its slowest pair is.
    // (measured at the end of round 4, 5 Mbp: 56 pairs 6 ms a launch instead of 148, 240 pairs 8 instead of 147, 992 pairs 47
    // instead of 148: from 8 wave slots per pair on)
    // (... measured at 5 Mbp; for shorter queries -- from 256 kbp on -- from 16 wave slots per pair, as the suite has run it)
    const bool split = k.split.value_or(cb_words >= 8192 && (bp * 16 <= slots || (cb_words >= 65536 && bp * 8 <= slots)));
    if (split && bp * 2 <= 0xFFFFFFFFull / 64) {              // (segment numbers pair * S + segment are 32 bits)
        uint32_t S = (uint32_t)std::min<uint64_t>(k.split_s, std::max<uint64_t>(2, slots / bp));      // (8 x 5 Mbp: 67 / 58 / 42 ms a launch with 16 / 32 / 64 a pair)
        int seglen = (dmax + (int)S - 1) / (int)S;
        if (k.split_seglen > 0) { seglen = k.split_seglen; S = (uint32_t)std::min<int>(64, std::max(2, (dmax + seglen - 1) / seglen)); }
        seglen = std::max(seglen, 512);
        if ((dmax + seglen - 1) / seglen >= 2) { ch.split_S = std::min<uint32_t>(S, (uint32_t)((dmax + seglen - 1) / seglen)); ch.split_seglen = seglen; }
    }
    // (queries from ~256 kbp on; the split wants the candidate counts: which pairs to cut, which first)
    ch.lpt = (bp >= 2 && bp <= slots * 32 && k.lpt.value_or(cb_words >= 8192)) || ch.split_S >= 2;
    return ch;
}

// The bytes of one index slab slot, from the strides of the set's index form (32-bit words per slot): the tables
// (directory, entries, bucket table, tag words, presence filter) and, where the index is built by sorting, the build's keys
// (unsorted and sorted: 16 B per text position, count and start).  lzani_get_layout reports the tables.
struct SlabBytes { uint64_t tables, sort_keys; uint64_t total() const { return tables + sort_keys; } };

inline SlabBytes slab_bytes_per_slot(uint64_t dir_stride, uint64_t ent_stride, uint64_t bk_stride, uint64_t tw_stride, uint64_t fl_stride,
                                     bool sort_build, uint64_t Tmax)
{
    return SlabBytes{4 * (dir_stride + ent_stride + bk_stride + tw_stride + fl_stride), sort_build ? 16 * Tmax + 16 : 0};
}

}  // namespace lzani
