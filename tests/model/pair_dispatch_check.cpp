// pair_dispatch_check.cpp -- TEST INFRASTRUCTURE ONLY (a stand-alone host program, tests/test_pair_dispatch.py builds it
// with -fsanitize=address,undefined and runs it).
//
// The table of the pair-kernel instantiations and the choice of a launch's kernel (lz-ani_amd/csrc/lzani_pair_dispatch.h):
//   every row    its fields are what its name says under the grammar of the launch record (tests/util.py:
//                KERNEL_NAME_RE), the fields a kind's name leaves out hold the kind's fixed values, and pk_id of the
//                fields returns the row
//   the choice   over every consistent combination of the facts of a launch -- blk only with fast, tw and none of join, pm,
//                regions; split only with pm; join only without regions; rtc only with dsel 0, fast and no regions -- the
//                rows are inside the table, the run-time compiled row is one; every ahead-of-time row is chosen by some
//                combination (a split's mode 1 with its mode 0: the row behind it, the same nfree and defp) and every
//                run-time compiled row is offered by one
// It prints one line per combination, tab-separated: the ten facts (regions fast tw pm split join blk nfree dsel rtc),
// the ahead-of-time name, the run-time compiled name or "-"; tests/test_pair_dispatch.py compares every line with the
// rule as tests/util.py states it.  Exit status 0 = all as promised.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan tests/model/pair_dispatch_check.cpp
#include <cstdio>
#include <cstring>

#include "../../lz-ani_amd/csrc/lzani_pair_dispatch.h"

using namespace lzani;

namespace {

int fail(const char* what, long long a = 0, long long b = 0)
{
    fprintf(stderr, "pair_dispatch_check: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

bool in01(int v) { return v == 0 || v == 1; }
bool in012(int v) { return v >= 0 && v <= 2; }

// 0, or the line of the first promise row i breaks
int check_row(int i)
{
    const PairKernelDesc& d = PAIR_KERNELS[i];
    char again[96];
    int f = -1, n = -1, dp = -1, a = -1, b = -1, c = -1, m = -1;
    if (sscanf(d.name, "pairs fast=%d nfree=%d defp=%d aln=%d bk=%d cand=%d", &f, &n, &dp, &a, &b, &c) == 6) {
        snprintf(again, sizeof again, "pairs fast=%d nfree=%d defp=%d aln=%d bk=%d cand=%d", f, n, dp, a, b, c);
        if (!in01(f) || !in01(n) || !in012(dp) || !in01(a) || !in01(b) || !in012(c)) return __LINE__;
        if (d.kind != PK_PAIRS || d.fast != f || d.nfree != n || d.defp != dp || d.aln != a || d.bk != b || d.cand != c || d.mode != 0) return __LINE__;
    } else if (sscanf(d.name, "pairs_blk nfree=%d defp=%d", &n, &dp) == 2) {
        snprintf(again, sizeof again, "pairs_blk nfree=%d defp=%d", n, dp);
        if (!in01(n) || !in01(dp)) return __LINE__;
        if (d.kind != PK_BLK || d.fast != 1 || d.nfree != n || d.defp != dp || d.aln != 0 || d.bk != 1 || d.cand != 0 || d.mode != 0) return __LINE__;
    } else if (sscanf(d.name, "split nfree=%d defp=%d mode=%d", &n, &dp, &m) == 3) {
        snprintf(again, sizeof again, "split nfree=%d defp=%d mode=%d", n, dp, m);
        if (!in01(n) || !in012(dp) || !in01(m)) return __LINE__;
        if (d.kind != PK_SPLIT || d.fast != 1 || d.nfree != n || d.defp != dp || d.aln != 0 || d.bk != 1 || d.cand != 2 || d.mode != m) return __LINE__;
    } else if (sscanf(d.name, "rtc nfree=%d cand=%d", &n, &c) == 2) {
        snprintf(again, sizeof again, "rtc nfree=%d cand=%d", n, c);
        if (!in01(n) || !in012(c)) return __LINE__;
        if (d.kind != PK_RTC || d.fast != 1 || d.nfree != n || d.defp != 9 || d.aln != 0 || d.bk != 1 || d.cand != c || d.mode != 0) return __LINE__;
    } else return __LINE__;
    if (strcmp(again, d.name) != 0) return __LINE__;                                   // nothing before, between or behind the fields
    if (pk_id(d.kind, d.fast, d.nfree, d.defp, d.aln, d.bk, d.cand, d.mode) != i) return __LINE__;
    return 0;
}

}  // namespace

int main()
{
    for (int i = 0; i < PK_COUNT; ++i)
        if (const int line = check_row(i)) return fail("a row of PAIR_KERNELS against its name, line", line, i);
    if (pk_id(PK_PAIRS, 1, 0, 2, 0, 1, 0, 0) != -1 || pk_id(PK_BLK, 1, 0, 2, 0, 1, 0, 0) != -1) return fail("pk_id finds a row that is not there");

    int chosen[PK_COUNT] = {0}, offered[PK_COUNT] = {0};
    unsigned long long lines = 0;
    for (int bits = 0; bits < 512; ++bits)
        for (int dsel = 0; dsel < 3; ++dsel) {
            PairFacts f;
            f.regions = bits & 1; f.fast = bits & 2; f.tw = bits & 4; f.pm = bits & 8; f.split = bits & 16; f.join = bits & 32;
            f.blk = bits & 64; f.nfree = bits & 128; f.rtc = bits & 256; f.dsel = dsel;
            if (f.blk && !(f.fast && f.tw && !f.join && !f.pm && !f.regions)) continue;
            if (f.split && !f.pm) continue;
            if (f.join && f.regions) continue;
            if (f.rtc && !(dsel == 0 && f.fast && !f.regions)) continue;
            const PairChoice ch = choose_pair_kernel(f);
            if (ch.row < 0 || ch.row >= PK_COUNT || PAIR_KERNELS[ch.row].kind == PK_RTC) return fail("the chosen row", ch.row, bits * 3 + dsel);
            if (ch.rtc_row < -1 || ch.rtc_row >= PK_COUNT || (ch.rtc_row >= 0 && PAIR_KERNELS[ch.rtc_row].kind != PK_RTC)) return fail("the run-time compiled row", ch.rtc_row, bits * 3 + dsel);
            if (ch.rtc_row >= 0 && !f.rtc) return fail("a run-time compiled row without a kernel in hand", ch.rtc_row, bits * 3 + dsel);
            chosen[ch.row] += 1;
            if (PAIR_KERNELS[ch.row].kind == PK_SPLIT) {
                const PairKernelDesc &m0 = PAIR_KERNELS[ch.row], &m1 = PAIR_KERNELS[ch.row + 1 < PK_COUNT ? ch.row + 1 : ch.row];
                if (m0.mode != 0 || m1.kind != PK_SPLIT || m1.mode != 1 || m1.nfree != m0.nfree || m1.defp != m0.defp) return fail("a split's mode 1 is not the row behind its mode 0", ch.row);
                chosen[ch.row + 1] += 1;
            }
            if (ch.rtc_row >= 0) offered[ch.rtc_row] += 1;
            printf("%d %d %d %d %d %d %d %d %d %d\t%s\t%s\n", (int)f.regions, (int)f.fast, (int)f.tw, (int)f.pm, (int)f.split, (int)f.join, (int)f.blk,
                   (int)f.nfree, f.dsel, (int)f.rtc, PAIR_KERNELS[ch.row].name, ch.rtc_row >= 0 ? PAIR_KERNELS[ch.rtc_row].name : "-");
            ++lines;
        }
    for (int i = 0; i < PK_COUNT; ++i) {
        const bool rtc = PAIR_KERNELS[i].kind == PK_RTC;
        if (rtc ? (!offered[i] || chosen[i]) : (!chosen[i] || offered[i])) return fail("a row no combination of the facts reaches", i);
    }
    return lines > 0 ? 0 : 1;
}
