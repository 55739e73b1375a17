// run_plan_check.cpp -- TEST INFRASTRUCTURE ONLY (a stand-alone host program, tests/test_run_plan.py builds it with
// -fsanitize=address,undefined and runs it).
//
// The pure decisions of a run (lz-ani_amd/csrc/lzani_run_plan.h) on seeded random rows at the smallest sizes where the
// rules can go wrong -- 1 to 40 rows of 0 to 50 pairs, empty rows and a row above cap_pairs among them, rows_cap 1 to 8 --
// against what each rule promises:
//   cut_batches   the batches partition the rows in order; none holds more than rows_cap rows, none more than cap_pairs
//                 pairs unless it is a single row; the cut is greedy (the next row would have broken one of the two limits);
//                 the return value is the largest batch's pairs
//   plan_queues   per batch: qorder is a permutation of its rows; qb starts at 0, does not decrease and ends at the row
//                 count; qcum is the running pair count from 0 to the batch's pairs; rows inside a queue do not get longer;
//                 the heaviest and the lightest queue differ by no more than the longest row
//   choose_split  split_S is 0 or within 2 .. 64 (split_s within its own 2 .. 64); a split has split_seglen >= 512 and
//                 split_S <= ceil(dmax / split_seglen); lpt holds whenever split_S >= 2
//   slab_bytes_per_slot   the two parts against the sum written out
// Then it prints the split decision for a fixed grid, one line each
//   grid <pairs> <cb_words> <dmax> <split knob: -1 unset, 0, 1> <split_s> <split_seglen> <split_S> <seglen> <lpt>
// which tests/test_run_plan.py compares with the rule as tests/util.py states it, and a last line with the cases run.
// Exit status 0 = all as promised.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan tests/model/run_plan_check.cpp
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../lz-ani_amd/csrc/lzani_run_plan.h"

using namespace lzani;

namespace {

uint64_t rng_state = 0x2545F4914F6CDD1DULL;
uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

int fail(const char* what, long long a = 0, long long b = 0)
{
    fprintf(stderr, "run_plan_check: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

// 0, or the line of the first promise a plan of these rows breaks
int check_rows(uint32_t n_rows, const std::vector<uint64_t>& off, uint32_t rows_cap, uint64_t cap_pairs, uint32_t nq)
{
    std::vector<uint32_t> bs;
    const uint64_t most = cut_batches(n_rows, off.data(), rows_cap, cap_pairs, bs);
    if (bs.size() < 2 || bs.front() != 0 || bs.back() != n_rows) return __LINE__;
    uint64_t seen_most = 0;
    for (size_t b = 0; b + 1 < bs.size(); ++b) {
        if (bs[b + 1] <= bs[b]) return __LINE__;                                       // in order, none empty
        const uint32_t rows = bs[b + 1] - bs[b];
        const uint64_t pairs = off[bs[b + 1]] - off[bs[b]];
        if (rows > rows_cap) return __LINE__;
        if (pairs > cap_pairs && rows != 1) return __LINE__;
        if (bs[b + 1] < n_rows && rows != rows_cap && pairs + (off[bs[b + 1] + 1] - off[bs[b + 1]]) <= cap_pairs) return __LINE__;     // greedy
        seen_most = std::max(seen_most, pairs);
    }
    if (most != seen_most) return __LINE__;

    const QueuePlan qp = plan_queues(n_rows, off.data(), bs, nq);
    if (qp.qorder.size() != n_rows || qp.qcum.size() != (size_t)n_rows + bs.size() - 1 || qp.qb.size() != (bs.size() - 1) * (nq + 1)) return __LINE__;
    for (size_t b = 0; b + 1 < bs.size(); ++b) {
        const uint32_t k0 = bs[b], rows = bs[b + 1] - k0;
        const uint32_t* qo = qp.qorder.data() + k0;
        const uint64_t* qc = qp.qcum.data() + k0 + b;
        const uint32_t* qb = qp.qb.data() + b * (nq + 1);
        auto rlen = [&](uint32_t k) { return off[k0 + k + 1] - off[k0 + k]; };
        std::vector<int> hit(rows, 0);
        for (uint32_t i = 0; i < rows; ++i) { if (qo[i] >= rows || hit[qo[i]]++) return __LINE__; }      // a permutation
        if (qb[0] != 0 || qb[nq] != rows) return __LINE__;
        for (uint32_t x = 0; x < nq; ++x) if (qb[x + 1] < qb[x]) return __LINE__;
        if (qc[0] != 0) return __LINE__;
        for (uint32_t i = 0; i < rows; ++i) if (qc[i + 1] != qc[i] + rlen(qo[i])) return __LINE__;
        if (qc[rows] != off[bs[b + 1]] - off[k0]) return __LINE__;
        uint64_t longest = 0, heavy = 0, light = ~0ull;
        for (uint32_t k = 0; k < rows; ++k) longest = std::max(longest, rlen(k));
        for (uint32_t x = 0; x < nq; ++x) {
            for (uint32_t i = qb[x]; i + 1 < qb[x + 1]; ++i) if (rlen(qo[i + 1]) > rlen(qo[i])) return __LINE__;
            const uint64_t load = qc[qb[x + 1]] - qc[qb[x]];
            heavy = std::max(heavy, load); light = std::min(light, load);
        }
        if (heavy - light > longest) return __LINE__;
    }
    return 0;
}

int check_split(uint64_t pairs, uint64_t slots, uint64_t cb_words, int dmax, const SplitKnobs& k)
{
    const SplitChoice ch = choose_split(pairs, slots, cb_words, dmax, k);
    if (ch.split_S == 1 || ch.split_S > 64) return __LINE__;
    if (ch.split_S == 0 && ch.split_seglen != 0) return __LINE__;
    if (ch.split_S >= 2) {
        if (ch.split_seglen < 512) return __LINE__;
        if ((int64_t)ch.split_S > ((int64_t)dmax + ch.split_seglen - 1) / ch.split_seglen) return __LINE__;
        if (!ch.lpt) return __LINE__;
        if (k.split && !*k.split) return __LINE__;                                     // switched off, yet split
        if (pairs * 2 > 0xFFFFFFFFull / 64) return __LINE__;                           // segment numbers beyond 32 bits
    }
    return 0;
}

}  // namespace

int main()
{
    unsigned long long row_cases = 0, split_cases = 0, above_cap = 0, empty_rows = 0, splits = 0;
    for (int round = 0; round < 6000; ++round) {
        const uint32_t n_rows = 1 + (uint32_t)(rnd() % 40);
        const uint32_t rows_cap = 1 + (uint32_t)(rnd() % 8);
        const uint64_t cap_pairs = round % 9 == 0 ? ~0ull : 1 + rnd() % 120;
        const uint32_t nq = round % 5 == 0 ? 1 + (uint32_t)(rnd() % 8) : 8;
        const int shape = (int)(rnd() % 4);                    // any length; mostly empty; all equal; one row above cap_pairs
        std::vector<uint64_t> off((size_t)n_rows + 1, 0);
        const uint64_t same = rnd() % 51;
        const uint32_t big = (uint32_t)(rnd() % n_rows);
        for (uint32_t r = 0; r < n_rows; ++r) {
            uint64_t len = shape == 2 ? same : rnd() % 51;
            if (shape == 1 && rnd() % 3) len = 0;
            if (shape == 3 && r == big && cap_pairs != ~0ull) { len = cap_pairs + 1 + rnd() % 20; ++above_cap; }
            empty_rows += len == 0;
            off[r + 1] = off[r] + len;
        }
        if (const int line = check_rows(n_rows, off, rows_cap, cap_pairs, nq)) return fail("a promise of cut_batches / plan_queues broken, line", line, round);
        ++row_cases;
    }
    const uint64_t cbw[4] = {32, 4096, 8192, 65536};
    for (int round = 0; round < 6000; ++round) {
        const uint64_t pairs = round % 11 == 0 ? ((uint64_t)1 << (20 + rnd() % 12)) + rnd() % 7 : 1 + rnd() % 6000;
        const uint64_t slots = round % 4 == 0 ? 4 * (1 + rnd() % 4096) : 8192;
        const uint64_t cb_words = cbw[rnd() % 4];
        const int dmax = round % 6 == 0 ? 1 + (int)(rnd() % 2000) : 1 + (int)(rnd() % 6000000);
        SplitKnobs k;
        if (rnd() % 3) k.split = (rnd() & 1) != 0;
        if (rnd() % 3 == 0) k.lpt = (rnd() & 1) != 0;
        k.split_s = 2 + rnd() % 63;
        k.split_seglen = rnd() % 3 ? 0 : 1 + (int)(rnd() % 4000);
        if (const int line = check_split(pairs, slots, cb_words, dmax, k)) return fail("a promise of choose_split broken, line", line, round);
        splits += choose_split(pairs, slots, cb_words, dmax, k).split_S >= 2;
        ++split_cases;
    }
    for (int round = 0; round < 200; ++round) {
        const uint64_t s[5] = {rnd() % (1u << 27), rnd() % (1u << 30), rnd() % (1u << 28), rnd() % (1u << 26), rnd() % (1u << 13)}, T = rnd() % (1u << 30);
        const SlabBytes on = slab_bytes_per_slot(s[0], s[1], s[2], s[3], s[4], true, T), no = slab_bytes_per_slot(s[0], s[1], s[2], s[3], s[4], false, T);
        const uint64_t tables = 4 * (s[0] + s[1] + s[2] + s[3] + s[4]);
        if (on.tables != tables || no.tables != tables || no.sort_keys != 0 || on.sort_keys != 16 * T + 16 || on.total() != tables + 16 * T + 16 || no.total() != tables)
            return fail("slab_bytes_per_slot", round);
    }
    // the fixed grid: the thresholds of the rule (pairs x 16 / x 8 against 8,192 wave slots; bitmaps of 8,192 / 65,536 words)
    // and the switches the suite forces; dmax is the longest scan a bitmap of cb_words words covers, or a short one
    struct G { int split; uint64_t split_s; int seglen; };
    const G knobs[6] = {{-1, 64, 0}, {0, 64, 0}, {1, 64, 0}, {1, 64, 1500}, {1, 64, 400}, {1, 2, 0}};
    const uint64_t gp[6] = {1, 2, 56, 240, 992, 5000}, gcb[3] = {4096, 8192, 65536};
    for (uint64_t pairs : gp)
        for (uint64_t cb_words : gcb)
            for (int dmax : {(int)(cb_words * 32 - 320), 900, 500})
                for (const G& g : knobs) {
                    SplitKnobs k;
                    if (g.split >= 0) k.split = g.split == 1;
                    k.split_s = g.split_s; k.split_seglen = g.seglen;
                    const SplitChoice ch = choose_split(pairs, 8192, cb_words, dmax, k);
                    printf("grid %llu %llu %d %d %llu %d %u %d %d\n", (unsigned long long)pairs, (unsigned long long)cb_words, dmax, g.split,
                           (unsigned long long)g.split_s, g.seglen, ch.split_S, ch.split_seglen, (int)ch.lpt);
                }
    printf("%llu %llu %llu %llu %llu\n", row_cases, split_cases, above_cap, empty_rows, splits);
    return row_cases >= 3000 && split_cases >= 3000 && above_cap > 100 && empty_rows > 1000 && splits > 100 ? 0 : 1;
}
