// set_plan_check.cpp -- TEST INFRASTRUCTURE ONLY (a stand-alone host program, tests/test_set_plan.py builds it with
// -fsanitize=address,undefined and runs it).
//
// The pure layout decisions of a genome set (lz-ani_amd/csrc/lzani_set_plan.h) against what each rule promises:
//   set_layout_of   over longest genomes {0, 1, 100, 40,000, 131,000, 132,000, 300,000, 5,000,000, 2^28} x six parameter
//                   tuples x n {1, 3, 4, 7, 8, 65,535, 70,000}: join => tag words => bucket table => k-mer words; a filter
//                   stride => tag words, no join and fmask + 1 == 32 * fl_stride; no filter => fmask == 31; sort build =>
//                   max_slots <= 2^min(16, 64 - kb - posbits) - 1; 1 <= max_slots <= 65535; join => ceil_log2(n + 1) + kb +
//                   posbits <= 64.  Every switch of SetKnobs, set alone, flips the decision it names on a case of the sweep
//                   where it was the other way, and never changes a decision that does not follow from the one it names
//   slab_slot_count within [1, min(want, max_slots)] unless the slabs hold more already, then what they hold; never below
//                   what is held; monotone in the free bytes
//   plan_blocks_impl  blocks contiguous, covering the set, each at most limit / 2 and greedy (the next genome would not
//                   have fitted); limit 0 is one block; a limit below twice the largest footprint is refused; the block
//                   bytes sum to the set's
//   auto_genome_limit  in-core exactly when tables + codes and tables + one slab slot both fit the free bytes, else free / 2
// Then it prints, for tests/test_set_plan.py to compare with the Python statements (tests/util.py, tests/ooc_model.py):
//   grid <Lmax> <n> <mal msl mrd mqd reg aw am ar> <key dir pos bits> <bk tw fl strides> <fmask> <join> <sort> <max_slots> <footprint of the longest genome>
//   blocks <mal msl mrd mqd reg aw am ar> <limit> <n> <len ...> : <block_of ... | refused>
// and a last line with the cases run.  `set_plan_check knobs` prints the SetKnobs the environment gives, and nothing else.
// Exit status 0 = all as promised.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan tests/model/set_plan_check.cpp
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../lz-ani_amd/csrc/lzani_set_plan.h"

using namespace lzani;

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

int fail(const char* what, long long a = 0, long long b = 0)
{
    fprintf(stderr, "set_plan_check: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

const Params TUPLES[6] = {
    {11, 7, 40, 40, 35, 15, 7, 3},            // the defaults
    {15, 9, 40, 40, 60, 15, 7, 3},            // the long-genome tuple
    {16, 16, 40, 40, 35, 15, 7, 3},           // no k-mer words
    {5, 5, 40, 40, 35, 15, 7, 3},             // a key space smaller than the directory
    {11, 7, 0, 40, 35, 15, 7, 3},             // mrd 0
    {11, 7, 1000, 64, 35, 15, 7, 3},          // a seed window beyond 128: no join
};
const int LONGEST[9] = {0, 1, 100, 40000, 131000, 132000, 300000, 5000000, 1 << 28};
const u32 COUNTS[7] = {1, 3, 4, 7, 8, 65535, 70000};

struct Case { Params P; int Lmax, Tmax; u32 n; IndexGeom geo; };

std::vector<Case> sweep()
{
    std::vector<Case> v;
    for (const Params& P : TUPLES)
        for (int L : LONGEST)
            for (u32 n : COUNTS) {
                const int T = ref_text_len(L, P.mrd);
                v.push_back(Case{P, L, T, n, index_geometry(T, P.mal)});
            }
    return v;
}

SetLayout layout(const Case& c, const SetKnobs& k) { return set_layout_of(c.P, c.geo, c.Tmax, c.n, k); }

// 0, or the line of the first promise this layout breaks
int check_layout(const Case& c, const SetLayout& f)
{
    if (f.join_mode && !f.tw_stride) return __LINE__;
    if (f.tw_stride && !f.bk_stride) return __LINE__;
    if (f.bk_stride && !kmer_words_of(c.P)) return __LINE__;
    if (f.bk_stride && f.bk_stride != (u64)4 << c.geo.dirbits) return __LINE__;
    if (f.tw_stride && f.tw_stride != (u64)1 << c.geo.dirbits) return __LINE__;
    if (f.fl_stride && (!f.tw_stride || f.join_mode || (u64)f.fmask + 1 != 32 * f.fl_stride)) return __LINE__;
    if (!f.fl_stride && f.fmask != 31) return __LINE__;
    if (f.sort_build && (u64)f.max_slots > (1ull << std::min(16, 64 - c.geo.kb - c.geo.posbits)) - 1) return __LINE__;
    if (f.max_slots < 1 || f.max_slots > 65535) return __LINE__;
    if (f.join_mode && ceil_log2((u64)c.n + 1) + c.geo.kb + c.geo.posbits > 64) return __LINE__;
    return 0;
}

// The decisions of a layout; a switch names one and may move those that follow from it.
enum { D_BK = 1, D_TW = 2, D_JOIN = 4, D_FILTER = 8, D_SORT = 16, D_SLOTS = 32 };
int differing(const SetLayout& a, const SetLayout& b)
{
    return (a.bk_stride != b.bk_stride ? D_BK : 0) | (a.tw_stride != b.tw_stride ? D_TW : 0) | (a.join_mode != b.join_mode ? D_JOIN : 0) |
           ((a.fl_stride != b.fl_stride || a.fmask != b.fmask) ? D_FILTER : 0) | (a.sort_build != b.sort_build ? D_SORT : 0) |
           (a.max_slots != b.max_slots ? D_SLOTS : 0);
}

struct Switch { const char* name; void (*set)(SetKnobs&); int names, follows; };
const Switch SWITCHES[] = {
    {"LZANI_BK_MAX_DIRBITS", [](SetKnobs& k) { k.bk_max_dirbits = 10; }, D_BK, D_TW | D_JOIN | D_FILTER},
    {"LZANI_NO_BUCKETS", [](SetKnobs& k) { k.buckets = false; }, D_BK, D_TW | D_JOIN | D_FILTER},
    {"LZANI_NO_TAGWORDS", [](SetKnobs& k) { k.tagwords = false; }, D_TW, D_JOIN | D_FILTER},
    {"LZANI_JOIN_MIN_BYTES", [](SetKnobs& k) { k.join_min_bytes = 0; }, D_JOIN, D_FILTER},
    {"LZANI_NO_JOIN", [](SetKnobs& k) { k.join = false; }, D_JOIN, D_FILTER},
    {"LZANI_SORT_INDEX_MIN_DIRBITS", [](SetKnobs& k) { k.sort_min_dirbits = 0; }, D_SORT, D_SLOTS},
    {"LZANI_NO_SORT_INDEX", [](SetKnobs& k) { k.sort_index = false; }, D_SORT, D_SLOTS},
    {"LZANI_FILTER_MAX_BITS", [](SetKnobs& k) { k.filter_max_bits = 12; }, D_FILTER, 0},
    {"LZANI_NO_FILTER", [](SetKnobs& k) { k.filter = false; }, D_FILTER, 0},
    {"LZANI_MAX_SLOTS", [](SetKnobs& k) { k.max_slots = 3; }, D_SLOTS, 0},
};

void print_knobs(const SetKnobs& k)
{
    printf("knobs %d %d %d %llu %d %d %d %d %d %d %lld\n", k.bk_max_dirbits, (int)k.buckets, (int)k.tagwords, (unsigned long long)k.join_min_bytes,
           (int)k.join, k.sort_min_dirbits, (int)k.sort_index, k.filter_max_bits, (int)k.filter, k.max_slots, k.free_bytes ? (long long)*k.free_bytes : -1LL);
}

void print_params(const Params& P) { printf("%d %d %d %d %d %d %d %d", P.mal, P.msl, P.mrd, P.mqd, P.reg, P.aw, P.am, P.ar); }

// 0, or the line of the first promise the block plan of these genomes breaks
int check_blocks(const std::vector<u32>& len, const Params& P, u64 limit, const SetKnobs& k)
{
    const u32 n = (u32)len.size();
    std::vector<u32> first, one;
    std::vector<u64> bytes, all;
    std::string msg;
    if (plan_blocks_impl(n, len.data(), P, 0, k, one, all, msg) != 1 || one.size() != 2 || one[0] != 0 || one[1] != n || all.size() != 1) return __LINE__;
    int Lmax = 0;
    for (u32 L : len) Lmax = std::max(Lmax, (int)L);
    const int Tmax = ref_text_len(Lmax, P.mrd);
    const bool join = set_layout_of(P, index_geometry(Tmax, P.mal), Tmax, n, k).join_mode;
    std::vector<u64> fp(n);
    u64 fmax = 0, total = 0;
    for (u32 g = 0; g < n; ++g) { fp[g] = ooc_genome_bytes((int)len[g], P, kmer_words_of(P), join); fmax = std::max(fmax, fp[g]); total += fp[g]; }
    if (all[0] != total) return __LINE__;
    const int nb = plan_blocks_impl(n, len.data(), P, limit, k, first, bytes, msg);
    if (limit == 0) return nb == 1 ? 0 : __LINE__;
    if (fmax > limit / 2) return nb == LZANI_ERR_ARG && !msg.empty() ? 0 : __LINE__;           // refused
    if (nb < 1 || first.size() != (size_t)nb + 1 || bytes.size() != (size_t)nb || first.front() != 0 || first.back() != n) return __LINE__;
    u64 sum = 0;
    for (int b = 0; b < nb; ++b) {
        if (first[b + 1] <= first[b]) return __LINE__;                                  // in order, none empty
        u64 s = 0;
        for (u32 g = first[b]; g < first[b + 1]; ++g) s += fp[g];
        if (s != bytes[b] || s > limit / 2) return __LINE__;
        if (b + 1 < nb && s + fp[first[b + 1]] <= limit / 2) return __LINE__;          // greedy
        sum += s;
    }
    return sum == total ? 0 : __LINE__;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "knobs")) { print_knobs(SetKnobs{}); return 0; }
    const SetKnobs k0{};                                   // (the test runs this program without any LZANI_* switch)
    const std::vector<Case> cases = sweep();
    unsigned long long layout_cases = 0, joins = 0, filters = 0, sorts = 0, slot_cases = 0, block_cases = 0, refused = 0, several = 0, res_cases = 0, in_core = 0;
    for (const Case& c : cases) {
        const SetLayout f = layout(c, k0);
        if (const int line = check_layout(c, f)) return fail("a promise of set_layout_of broken, line", line, c.Lmax);
        joins += f.join_mode; filters += f.fl_stride != 0; sorts += f.sort_build;
        ++layout_cases;
    }
    for (const Switch& s : SWITCHES) {
        SetKnobs k = k0;
        s.set(k);
        bool flipped = false;
        for (const Case& c : cases) {
            const SetLayout a = layout(c, k0), b = layout(c, k);
            if (const int line = check_layout(c, b)) return fail(s.name, line, c.Lmax);
            const int d = differing(a, b);
            if (d & ~(s.names | s.follows)) return fail(s.name, d, c.Lmax);             // a decision that does not follow from it
            if ((d & s.follows) && !(d & s.names)) return fail(s.name, d, -c.Lmax);      // ... or follows without the named one
            flipped |= (d & s.names) != 0;
        }
        if (!flipped) return fail(s.name, -1);
    }
    // the slot count of the slabs
    for (int round = 0; round < 20000; ++round) {
        const u64 per_slot = 1 + rnd() % (round % 3 ? (1u << 20) : (1ull << 34));
        const u32 held = round % 4 == 0 ? 0 : (u32)(rnd() % 70);
        const u32 want = 1 + (u32)(rnd() % (round % 5 ? 100 : 80000)), max_slots = 1 + (u32)(rnd() % 65535);
        const u64 free_b = rnd() % (round % 2 ? (1ull << 38) : 64 * per_slot + 1), more = free_b + rnd() % (1ull << 30);
        const u32 s = slab_slot_count(free_b, held, per_slot, want, max_slots), s2 = slab_slot_count(more, held, per_slot, want, max_slots);
        const u32 cap = std::min(want, max_slots);
        if (s < 1 || s < held) return fail("slab_slot_count below 1 or below what is held", round, s);
        if (held <= cap ? s > cap : s != held) return fail("slab_slot_count above min(want, max_slots)", round, s);
        if (s2 < s) return fail("slab_slot_count not monotone in the free bytes", round, s);
        ++slot_cases;
    }
    // the block plan
    for (int round = 0; round < 4000; ++round) {
        const Params& P = TUPLES[rnd() % 6];
        std::vector<u32> len(1 + rnd() % 40);
        for (u32& L : len) L = round % 7 == 0 ? (u32)(rnd() % 3) : (u32)(rnd() % 200000);
        u64 fmax = 0, total = 0;
        for (u32 L : len) { const u64 b = ooc_genome_bytes((int)L, P, kmer_words_of(P), false); fmax = std::max(fmax, b); total += b; }
        const int shape = round % 5;           // one block; refused; the minimum; a few blocks; everything fits
        const u64 limit = shape == 0 ? 0 : shape == 1 ? 2 * fmax - 1 - rnd() % fmax : shape == 2 ? 2 * fmax : shape == 3 ? 2 * fmax + rnd() % (2 * total) : 2 * total + rnd() % 100;
        if (const int line = check_blocks(len, P, limit, k0)) return fail("a promise of plan_blocks_impl broken, line", line, round);
        std::vector<u32> first;
        std::vector<u64> bytes;
        std::string msg;
        const int nb = plan_blocks_impl((u32)len.size(), len.data(), P, limit, k0, first, bytes, msg);
        refused += nb < 0; several += nb > 1;
        ++block_cases;
    }
    // the residency decision
    for (int round = 0; round < 4000; ++round) {
        const u64 tables = rnd() % (1ull << 36), codes = rnd() % (1ull << 34), per_slot = rnd() % (1ull << 33);
        const u64 free_b = round % 3 == 0 ? tables + std::max(codes, per_slot) - 1 + rnd() % 3 : rnd() % (1ull << 37);
        const u64 limit = auto_genome_limit(tables, codes, per_slot, free_b);
        const bool fits = tables + codes <= free_b && tables + per_slot <= free_b;
        if (fits ? limit != 0 : limit != free_b / 2) return fail("auto_genome_limit", round);
        in_core += fits;
        ++res_cases;
    }
    // the grid: every case of the sweep with n 1, 4 and 70,000
    for (const Case& c : cases) {
        if (c.n != 1 && c.n != 4 && c.n != 70000) continue;
        const SetLayout f = layout(c, k0);
        printf("grid %d %u ", c.Lmax, c.n);
        print_params(c.P);
        printf(" %d %d %d %llu %llu %llu %u %d %d %u %llu\n", c.geo.kb, c.geo.dirbits, c.geo.posbits, (unsigned long long)f.bk_stride, (unsigned long long)f.tw_stride,
               (unsigned long long)f.fl_stride, f.fmask, (int)f.join_mode, (int)f.sort_build, f.max_slots,
               (unsigned long long)ooc_genome_bytes(c.Lmax, c.P, kmer_words_of(c.P), f.join_mode));
    }
    // block plans: viral sizes and long genomes (with join lists at the long-genome tuple), at limits from refused to one block
    const std::vector<std::vector<u32>> sets = {{40000, 35000, 0, 52000, 41000, 100, 38000, 47000}, {5000000, 4800000, 5100000, 300, 4000000}, {7}};
    for (int t = 0; t < 2; ++t)
        for (const std::vector<u32>& len : sets) {
            u64 fmax = 0, total = 0;
            for (u32 L : len) { const u64 b = ooc_genome_bytes((int)L, TUPLES[t], true, false); fmax = std::max(fmax, b); total += b; }
            for (u64 limit : {(u64)0, fmax, 2 * fmax + 64 * len[0], 3 * fmax, 5 * fmax, total, 4 * total}) {
                std::vector<u32> first;
                std::vector<u64> bytes;
                std::string msg;
                const int nb = plan_blocks_impl((u32)len.size(), len.data(), TUPLES[t], limit, k0, first, bytes, msg);
                printf("blocks ");
                print_params(TUPLES[t]);
                printf(" %llu %zu", (unsigned long long)limit, len.size());
                for (u32 L : len) printf(" %u", L);
                printf(" :");
                if (nb < 0) printf(" refused");
                for (int b = 0; b < nb; ++b) for (u32 g = first[b]; g < first[b + 1]; ++g) printf(" %d", b);
                printf("\n");
            }
        }
    printf("%llu %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", layout_cases, joins, filters, sorts, slot_cases, block_cases, refused, several, res_cases, in_core);
    return layout_cases == 6 * 9 * 7 && joins > 0 && filters > 0 && sorts > 0 && slot_cases >= 20000 && block_cases >= 4000 && refused > 100 && several > 100 &&
                   res_cases >= 4000 && in_core > 100 && in_core < res_cases - 100 ? 0 : 1;
}
