// split_stitch_check.cpp -- TEST INFRASTRUCTURE ONLY.
//
// split_stitch (lz-ani_amd/csrc/lzani_core.h) on hand-made chains of segment records, in a program of its own so that it
// runs under the address and undefined-behaviour sanitizers (tests/test_split_repair.py builds and runs it).  The arrays are
// heap blocks of exactly n records: a read outside them is the sanitizer's to report.
//   broken chains -- a stop at or before the segment, a stop at or beyond n, two segments that hand over to each other,
//   segment 0 with a dropped first region, n = 1 -- must come back false with void_at = -1 (nothing to retry), cause 5
//   unless the stitch names another; a segment without a checkpoint in the chain is void itself (cause 0) and can be
//   retried; causes 1 to 4 by their definitions in the comment above split_stitch; and the chains next to each of them
//   that get through, with the counts the comment above SplitOut promises.
// Prints "ok <checks>" and returns 0, or the failed checks and 1.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../lz-ani_amd/csrc/lzani_core.h"

using namespace lzani;

namespace {

int g_checks = 0, g_bad = 0;

struct Chain {
    int n;
    SplitStart* st;
    SplitOut* so;
    explicit Chain(int n_) : n(n_)
    {
        st = (SplitStart*)malloc(sizeof(SplitStart) * n);
        so = (SplitOut*)malloc(sizeof(SplitOut) * n);
        for (int j = 0; j < n; ++j) {
            st[j] = SplitStart{j ? 512 * j : -1, 0, -1, 0, 0, 0};
            memset(&so[j], 0, sizeof(SplitOut));
            so[j].first = j ? 0 : 3; so[j].stop = -1; so[j].open_rs = -1; so[j].synced = 1;
        }
    }
    ~Chain() { free(st); free(so); }
    Chain(const Chain&) = delete;
};

// the stitch of c: ok, and where it is void at / from / why; where it gets through, the counts
void expect(const char* what, const Chain& c, int reg, bool ok, int at, int from, int why, int tm = 0, int tl = 0, int tc = 0)
{
    int res[3] = {-7, -7, -7}, g_at = 99, g_from = 99, g_why = 99;
    const bool got = split_stitch(c.st, c.so, c.n, reg, res, &g_at, &g_from, &g_why);
    ++g_checks;
    bool good = got == ok;
    if (ok) good = good && res[0] == tm && res[1] == tl && res[2] == tc;
    else good = good && g_at == at && g_from == from && g_why == why;
    if (!good) {
        ++g_bad;
        printf("FAILED %s: got %d (at %d from %d why %d; %d %d %d), expected %d (at %d from %d why %d; %d %d %d)\n", what, (int)got, g_at, g_from,
               g_why, res[0], res[1], res[2], (int)ok, at, from, why, tm, tl, tc);
    }
    // (the optional arguments left out: the same answer, nothing written)
    int res2[3] = {0, 0, 0};
    ++g_checks;
    if (split_stitch(c.st, c.so, c.n, reg, res2) != got || (got && memcmp(res, res2, sizeof res) != 0)) { ++g_bad; printf("FAILED %s: without the optional arguments\n", what); }
}

// two segments: segment 0 closed (tm, tl, tc) = (10, 2, 1), stands in an open region of 30 matches and 3 literals that began
// at query position 100, its floor 90 and true, and hands over to cut 1, whose checkpoint saw 5 matches and 1 literal
// of that region
void two(Chain& c)
{
    c.so[0].tm = 10; c.so[0].tl = 2; c.so[0].tc = 1;
    c.so[0].stop = 1; c.so[0].open_cl = 30; c.so[0].open_clit = 3; c.so[0].open_rs = 100; c.so[0].synced = 1; c.so[0].floor = 90;
    c.st[1].cl = 5; c.st[1].clit = 1;
    c.so[1].tm = 7; c.so[1].tl = 1; c.so[1].tc = 1; c.so[1].stop = -1;
}

}  // namespace

int main()
{
    const int reg = 35;
    // ---- chains that cannot be followed
    for (int n : {1, 2, 3, 5}) {
        for (int stop : {0, n, n + 1, INT_MAX, -2, INT_MIN}) {                 // at or before segment 0, at or beyond n
            Chain c(n);
            c.so[0].stop = stop;
            if (stop < 0) { expect("a negative stop is the end of the query", c, reg, true, 0, 0, 0, 0, 0, 0); continue; }
            expect("segment 0: stop out of range", c, reg, false, -1, -1, 5);
        }
    }
    {
        Chain c(1);                                                          // n = 1: segment 0 alone is the whole scan
        c.so[0].tm = 123; c.so[0].tl = 45; c.so[0].tc = 6;
        expect("n = 1", c, reg, true, 0, 0, 0, 123, 45, 6);
    }
    for (int n : {2, 4}) {
        Chain c(n);                                                          // 0 -> last -> 0: a cycle
        c.so[0].stop = n - 1; c.so[n - 1].stop = 0;
        expect("a cycle", c, reg, false, -1, 0, 5);
        c.so[n - 1].stop = n - 1;                                            // ... a segment that hands over to itself
        expect("a self-loop", c, reg, false, -1, 0, 5);
        c.so[n - 1].stop = n;                                                // ... a later segment's stop beyond n
        expect("a later stop at n", c, reg, false, -1, 0, 5);
    }
    {
        Chain c(3);                                                          // segment 0 cannot have dropped a first region apart
        c.so[0].first = 2; c.so[0].stop = 1;
        expect("first = 2 on segment 0", c, reg, false, -1, -1, 0);
    }
    {
        Chain c(3);                                                          // a cut without a checkpoint in the chain: its segment is void, retry from 0
        c.so[0].stop = 1;
        c.st[1].i = -1; c.so[1].first = 2; c.so[1].stop = -1;
        expect("a segment without a checkpoint in the chain", c, reg, false, 1, 0, 0);
        c.so[0].stop = 2; c.so[2].stop = -1;                                 // ... passed over: not in the chain
        expect("a segment without a checkpoint beside the chain", c, reg, true, 0, 0, 0, 0, 0, 0);
    }
    // ---- the first region of segment 1 closed inside it (first = 1), ending at first_re: dropped by the true scan iff first_re - 100 < reg
    {
        Chain c(2);
        two(c);
        c.so[1].first = 1; c.so[1].first_cl = 20; c.so[1].first_clit = 4; c.so[1].first_re = 200; c.so[1].assumed = 1;
        // kept by both: 30 - 5 + 20 = 45 matches, 3 - 1 + 4 = 6 literals, a region of its own
        expect("assumed kept, kept", c, reg, true, 0, 0, 0, 10 + 45 + 7, 2 + 6 + 1, 3);
        c.so[1].first_re = 100 + reg;                                        // the span is exactly reg: kept
        expect("assumed kept, span = reg", c, reg, true, 0, 0, 0, 62, 9, 3);
        c.so[1].first_re = 100 + reg - 1;                                    // cause 1: kept by the segment, dropped by the true scan
        expect("cause 1", c, reg, false, 1, 0, 1);
        c.so[1].assumed = 2; c.so[1].first_floor = 90;                       // dropped by both, the true floor (90) no higher than the look-backs hold for
        expect("assumed dropped, dropped", c, reg, true, 0, 0, 0, 10 + 7, 2 + 1, 2);
        c.so[1].first_floor = 89;                                            // cause 3: the true floor above it
        expect("cause 3", c, reg, false, 1, 0, 3);
        c.so[0].synced = 0;                                                  // (segment 0's floor not the true one: the stitch's own, 0, stands)
        expect("assumed dropped, floor of an unsynced segment ignored", c, reg, true, 0, 0, 0, 17, 3, 2);
        c.so[0].synced = 1; c.so[1].first_floor = 90; c.so[1].first_re = 200;   // cause 2: dropped by the segment, kept by the true scan
        expect("cause 2", c, reg, false, 1, 0, 2);
        c.so[1].assumed = 3; c.so[1].first_floor = 1;                        // kept on a guess, kept: the cut-short look-back does not matter
        expect("assumed kept on a guess, kept", c, reg, true, 0, 0, 0, 62, 9, 3);
        c.so[1].first_re = 120;                                              // cause 4: ... dropped by the true scan, and a look-back was cut short
        expect("cause 4", c, reg, false, 1, 0, 4);
        c.so[1].first_floor = 0;                                             // ... none was: the guess did no harm
        expect("assumed kept on a guess, dropped, no look-back cut short", c, reg, true, 0, 0, 0, 17, 3, 2);
        c.so[1].assumed = 1; c.so[1].first_re = 200; c.so[1].first_cl = 0; c.so[1].first_clit = 0;
        c.so[0].open_cl = 5; c.so[0].open_clit = 1;                          // kept, but nothing in it (cl = 0): no region counted
        expect("kept, empty", c, reg, true, 0, 0, 0, 17, 3, 2);
        c.so[1].first_cl = 10; c.so[1].first_clit = 24;                      // cl + clit = 34 < reg: not counted;  35: counted
        expect("kept, cl + clit below reg", c, reg, true, 0, 0, 0, 17, 3, 2);
        c.so[1].first_clit = 25;
        expect("kept, cl + clit = reg", c, reg, true, 0, 0, 0, 17 + 10, 3 + 25, 3);
    }
    {
        Chain c(2);                                                          // the first region still open at the end of the query (first = 0)
        two(c);
        c.so[1].first = 0; c.so[1].open_cl = 8; c.so[1].open_clit = 2;
        expect("open at the end, long enough", c, reg, true, 0, 0, 0, 10 + 33 + 7, 2 + 4 + 1, 3);      // 30 - 5 + 8, 3 - 1 + 2: 37 >= reg
        c.so[1].open_cl = 5;
        expect("open at the end, too short", c, reg, true, 0, 0, 0, 17, 3, 2);                            // 30 + 4 = 34 < reg
    }
    {
        // three segments: the region open at cut 1 stays open through segment 1 (first = 0) and closes in segment 2, whose
        // keep test takes the TRUE start, segment 0's 100; the void segment is 2 and the one to resume is 1
        Chain c(4);
        two(c);
        c.so[1].first = 0; c.so[1].stop = 3; c.so[1].open_cl = 9; c.so[1].open_clit = 2; c.so[1].open_rs = 600; c.so[1].synced = 0;
        c.st[3].cl = 4; c.st[3].clit = 1;
        c.so[3].first = 1; c.so[3].first_cl = 6; c.so[3].first_clit = 2; c.so[3].first_re = 100 + reg - 1; c.so[3].assumed = 1;
        c.so[3].tm = 1; c.so[3].tl = 1; c.so[3].tc = 1; c.so[3].stop = -1;
        expect("cause 1 two hand-overs on", c, reg, false, 3, 1, 1);
        c.so[3].first_re = 100 + reg;                                        // 30 - 5 + 9 = 34, - 4 + 6 = 36 matches; 3 - 1 + 2 = 4, - 1 + 2 = 5 literals
        expect("kept two hand-overs on", c, reg, true, 0, 0, 0, 10 + 7 + 36 + 1, 2 + 1 + 5 + 1, 4);
    }
    if (g_bad) { printf("%d of %d checks failed\n", g_bad, g_checks); return 1; }
    printf("ok %d\n", g_checks);
    return 0;
}
