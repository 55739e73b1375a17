// seed_word_check.cpp -- TEST INFRASTRUCTURE ONLY (a stand-alone host program, tests/test_seed_word.py builds and runs it).
//
// At msl <= 7 the seed word kmS[p] of a text position is redundant data: the low 2 * msl bits of the packed text from p
// on (lzani_core.h: kms_from_syms over a funnel shift of two 32-bit text words), and "the position holds an msl-mer"
// follows from the N flags (kmer_valid_n) or, in the head of a genome without N, from the run structure of the text
// (kms_valid_nfree_head).  This program checks both against k_kmers' statement
//     kmS[p] = kmer_at(R, p, msl, key) ? key : KM_INVALID
// at EVERY position of random reference texts (with and without N runs, mrd 0 included: no pad between the strands;
// every length mod 16, lengths below 64), for msl 5, 6 and 7.  Exit status 0 = all equal; it prints the number of
// positions compared.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/model/seed_word_check.cpp   (memory check of the same run)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../lz-ani_amd/csrc/lzani_core.h"
#include "../../lz-ani_amd/csrc/lzani_layout.h"

using namespace lzani;

namespace {

u64 rng_state = 0xD1B54A32D192ED03ULL;
u32 rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (u32)(rng_state >> 32);
}

struct Text {
    int L, T, mrd;
    bool nfree;
    std::vector<u64> t2, nm;
};

// fwd | N^2mrd | RC | N^mrd, spare symbols flagged N (k_pack; tests/model/lzani_model.cpp: pack_genome)
Text pack(const std::vector<uint8_t>& codes, int mrd)
{
    Text g;
    g.L = (int)codes.size(); g.T = ref_text_len(g.L, mrd); g.mrd = mrd; g.nfree = true;
    for (uint8_t c : codes) if (c >= 4) g.nfree = false;
    g.t2.assign(text_words2(g.T), 0);
    g.nm.assign(text_wordsN(g.T), ~0ULL);
    auto put = [&](int p, int c) {
        if (c < 4) { g.t2[p >> 5] |= (u64)c << ((p & 31) * 2); g.nm[p >> 6] &= ~(1ULL << (p & 63)); }
    };
    for (int j = 0; j < g.L; ++j) put(j, codes[j]);
    const int rc0 = g.L + 2 * mrd;
    for (int j = 0; j < g.L; ++j) { const int c = codes[g.L - 1 - j]; put(rc0 + j, c < 4 ? 3 - c : 4); }
    return g;
}

// v_alignbit_b32: the low 32 bits of (hi:lo) >> s, s < 32
u32 funnel(u32 hi, u32 lo, u32 s) { return (u32)(((((u64)hi) << 32) | lo) >> s); }

long check(const Text& g, int msl, long& bad)
{
    const TextView R = ref_view(g.t2.data(), g.nm.data(), g.L, g.mrd, g.nfree);
    const u32* const w = reinterpret_cast<const u32*>(g.t2.data());
    long n = 0;
    for (int p = 0; p < g.T; ++p, ++n) {
        u64 key = 0;
        const bool want_ok = kmer_at(R, p, msl, key);
        const u32 want = want_ok ? (u32)key : 0xFFFFFFFFu;
        const u32* const pq = w + ((u32)p >> 4);
        const u32 syms = funnel(pq[1], pq[0], ((u32)p & 15u) * 2u);
        const bool ok_n = kmer_valid_n(R, p, msl, winN(R.nm, p));
        const u32 got = ok_n ? kms_from_syms(syms, msl) : 0xFFFFFFFFu;
        bool fail = got != want || ok_n != want_ok;
        const bool head = g.nfree && p < g.L + g.mrd;               // a position of a query view of a genome without N
        u32 got_head = 0;
        if (head) {
            got_head = kms_valid_nfree_head(g.L, g.mrd, p, msl) ? kms_from_syms(syms, msl) : 0xFFFFFFFFu;
            if (got_head != want) fail = true;
        }
        if (fail && bad++ < 10)
            fprintf(stderr, "msl %d L %d mrd %d nfree %d p %d: want %08x (%d), from the text %08x (%d), by the head rule %08x (%d)\n", msl, g.L,
                    g.mrd, (int)g.nfree, p, want, (int)want_ok, got, (int)ok_n, got_head, (int)head);
    }
    return n;
}

}  // namespace

int main()
{
    static_assert(kms_is_text(5) && kms_is_text(7) && !kms_is_text(8) && !kms_is_text(9), "the word carries hash bits from msl 8 on");
    long n = 0, bad = 0;
    std::vector<int> lens = {0, 1, 4, 6, 7, 8, 31, 33, 63, 64, 65, 200};
    for (int r = 0; r < 16; ++r) { lens.push_back(40 + r); lens.push_back(1000 + r); }      // every L mod 16, below 64 and above
    const int mrds[] = {0, 1, 7, 40};
    for (int msl : {5, 6, 7})
        for (int mrd : mrds)
            for (int L : lens)
                for (int with_n = 0; with_n < 3; ++with_n) {
                    std::vector<uint8_t> codes((size_t)L);
                    for (auto& c : codes) c = (uint8_t)(rnd() & 3u);
                    // N runs of 1 .. 20 symbols; with_n 2: one of them at either end
                    for (int k = 0; with_n && L > 0 && k < 1 + L / 150; ++k) {
                        const int a = (int)(rnd() % (u32)L), len = 1 + (int)(rnd() % 20u);
                        for (int j = a; j < L && j < a + len; ++j) codes[(size_t)j] = 5;
                    }
                    if (with_n == 2 && L > 0) { codes[0] = 5; codes[(size_t)L - 1] = 5; }
                    n += check(pack(codes, mrd), msl, bad);
                }
    printf("%ld positions compared, %ld differ\n", n, bad);
    return bad ? 1 : 0;
}
