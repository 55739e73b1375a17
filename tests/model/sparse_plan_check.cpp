// sparse_plan_check.cpp -- TEST INFRASTRUCTURE ONLY (a stand-alone host program, tests/test_prefilter_sparse_plan.py builds
// it with -fsanitize=address,undefined and runs it).
//
// The tile rule of sparse counting (lz-ani_amd/csrc/lzani_sparse_plan.h: PfTiles, plan_sparse_tiles_impl) on random rows,
// against what the rule promises: the tiles cover the rows in order, every tile holds at most slots / 2 pairs, the heights
// never grow, every abandoned attempt did overflow (checked by walking PfTiles a second time by hand), and
// LZANI_ERR_NOMEM comes exactly where the walk reaches, at height 1, a row that alone is above slots / 2.  Rows and slots
// go up to 2^64 - 1 and 2^63: the sums must not wrap.
// Exit status 0 = all as promised; it prints the number of plans made and of those refused.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -Iinclude tests/model/sparse_plan_check.cpp
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "../../lz-ani_amd/csrc/lzani_sparse_plan.h"

using namespace lzani;

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

int fail(const char* what, uint32_t n, uint64_t slots)
{
    fprintf(stderr, "sparse_plan_check: %s (n_rows %u, slots %llu)\n", what, n, (unsigned long long)slots);
    return 1;
}

}  // namespace

int main()
{
    unsigned long long plans = 0, refused = 0;
    std::vector<uint32_t> first;
    uint32_t attempts = 0;
    const uint64_t one = 1;
    if (plan_sparse_tiles_impl(0, &one, 16, first, attempts) != LZANI_ERR_ARG || plan_sparse_tiles_impl(1, nullptr, 16, first, attempts) != LZANI_ERR_ARG)
        return fail("empty input accepted", 0, 16);
    for (uint64_t bad : {0ull, 1ull, 3ull, 24ull, ~0ull})
        if (plan_sparse_tiles_impl(1, &one, bad, first, attempts) != LZANI_ERR_ARG) return fail("bad slots accepted", 1, bad);
    for (int round = 0; round < 20000; ++round) {
        const uint32_t n = 1 + (uint32_t)(rnd() % 97);
        const uint64_t slots = (uint64_t)1 << (1 + rnd() % (round % 50 == 0 ? 63 : 12));
        const uint64_t tops[5] = {1, slots / 8 + 1, slots / 2 + 1, slots, ~0ull};
        const uint64_t top = tops[rnd() % (round % 7 == 0 ? 5 : 4)];
        std::vector<uint64_t> pairs(n);
        for (auto& p : pairs) p = top == ~0ull ? rnd() : rnd() % (top + 1);
        const int T = plan_sparse_tiles_impl(n, pairs.data(), slots, first, attempts);
        // the same walk by hand
        PfTiles t(n, n);
        std::vector<uint32_t> want(1, 0);
        bool nomem = false;
        while (t.more() && !nomem) {
            t.attempt();
            unsigned __int128 sum = 0;
            for (uint32_t r = t.r0; r < t.r1(); ++r) sum += pairs[r];
            if (sum > slots / 2) { if (!t.halve()) nomem = true; continue; }
            t.finished();
            want.push_back(t.r0);
        }
        if (nomem) {
            ++refused;
            if (T != LZANI_ERR_NOMEM) return fail("a row above half the table was not refused", n, slots);
            if (pairs[t.r0] <= slots / 2) return fail("refused without a row above half the table", n, slots);
            continue;
        }
        ++plans;
        if (T != (int)t.tiles || first != want || attempts != t.attempts) return fail("the plan differs from the walk by hand", n, slots);
        if (first.size() != (size_t)T + 1 || first.front() != 0 || first.back() != n || attempts < (uint32_t)T) return fail("the tiles do not cover the rows", n, slots);
        uint32_t last_h = n;
        for (int i = 0; i < T; ++i) {
            if (first[i + 1] <= first[i]) return fail("an empty tile", n, slots);
            const uint32_t h = first[i + 1] - first[i];
            if (h > last_h) return fail("the height grew back", n, slots);
            last_h = h;
            unsigned __int128 sum = 0;
            for (uint32_t r = first[i]; r < first[i + 1]; ++r) sum += pairs[r];
            if (sum > slots / 2) return fail("a tile above half the table", n, slots);
        }
    }
    printf("%llu %llu\n", plans, refused);
    return plans > 1000 && refused > 1000 ? 0 : 1;
}
