// lzani_shard_plan.h -- the shard bookkeeping of the one-process multi-GPU group (lzani_multi.h) as one host function.
// No HIP types: it compiles with a plain C++ compiler, and it is not among the sources a run-time compile embeds
// (lzani_rtc.h).  lzani_group_run_rows feeds the devices from it, and lzani_plan_gather exports the same result.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace lzani {

// What one device gets: its rows (the caller's row numbers, in the caller's order), their reference ids and query ids
// (each empty where the caller gave none), the row offsets counted from the shard's first result, and where that first
// result sits in the gathered buffer -- shards follow each other there in shard order.
struct Shard {
    std::vector<uint32_t> rows, ref, q;
    std::vector<uint64_t> off{0};
    uint64_t base = 0;
    uint64_t pairs() const { return off.back(); }
};

// tab = src[n_rows] | dst[n_rows] | cnt[n_rows]: entry j (j counts the rows shard by shard) says where the row's results
// sit in the gathered buffer, where they belong in the caller's CSR order, and how many there are.
struct ShardPlan {
    std::vector<Shard> shard;
    std::vector<uint64_t> tab;
};

// false for a shard number outside n_parts or a row table that runs backwards (the plan is then unusable)
inline bool plan_shards(uint32_t n_rows, const uint32_t* ref_ids, const uint64_t* row_off, const uint32_t* query_ids,
                        const uint32_t* part_of_row, uint32_t n_parts, ShardPlan& p)
{
    p.shard.assign(n_parts, Shard{});
    for (uint32_t k = 0; k < n_rows; ++k) {
        if (part_of_row[k] >= n_parts || row_off[k + 1] < row_off[k]) return false;
        Shard& s = p.shard[part_of_row[k]];
        s.rows.push_back(k);
        if (ref_ids) s.ref.push_back(ref_ids[k]);
        if (query_ids) s.q.insert(s.q.end(), query_ids + row_off[k], query_ids + row_off[k + 1]);
        s.off.push_back(s.pairs() + (row_off[k + 1] - row_off[k]));
    }
    for (uint32_t d = 1; d < n_parts; ++d) p.shard[d].base = p.shard[d - 1].base + p.shard[d - 1].pairs();
    p.tab.resize(3 * (size_t)n_rows);
    uint64_t *src = p.tab.data(), *dst = src + n_rows, *cnt = dst + n_rows;
    size_t j = 0;
    for (const Shard& s : p.shard)
        for (size_t i = 0; i < s.rows.size(); ++i, ++j) {
            src[j] = s.base + s.off[i];
            dst[j] = row_off[s.rows[i]];
            cnt[j] = s.off[i + 1] - s.off[i];
        }
    return true;
}

}  // namespace lzani
