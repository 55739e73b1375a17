// refill_hash_check.cpp -- TEST INFRASTRUCTURE ONLY (a stand-alone host program, tests/test_refill_hash.py builds and runs it).
//
// The pair kernel's refill (DevWave::refill, bitmap form) no longer reads the query's mal-mer word kmL[qp]: it makes the
// word from the packed text words it loads anyway (lzani_core.h: kml_from_syms over a funnel shift of two 32-bit text
// words) and decides "the position holds a mal-mer" from the N flags (kmer_valid_n) or, for genomes without N, from the
// run structure of the text (kmer_valid_nfree_head).  This program checks both against k_kmers' statement
//     kmL[p] = kmer_at(R, p, mal, key) ? mix_key(key, 2 * mal) : KM_INVALID
// at EVERY position of random reference texts (with and without N runs, mrd 0 included: no pad between the strands),
// for mal 9, 11 and 15.  Exit status 0 = all equal; it prints the number of positions compared.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/model/refill_hash_check.cpp   (memory check of the same run)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../lz-ani_amd/csrc/lzani_core.h"
#include "../../lz-ani_amd/csrc/lzani_layout.h"

using namespace lzani;

namespace {

u64 rng_state = 0x9E3779B97F4A7C15ULL;
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

long check(const Text& g, int mal, long& bad)
{
    const TextView R = ref_view(g.t2.data(), g.nm.data(), g.L, g.mrd, g.nfree);
    const u32* const w = reinterpret_cast<const u32*>(g.t2.data());
    long n = 0;
    for (int p = 0; p < g.T; ++p, ++n) {
        u64 key = 0;
        const bool want_ok = kmer_at(R, p, mal, key);
        const u32 want = want_ok ? (u32)mix_key(key, 2 * mal) : 0xFFFFFFFFu;
        const u32* const pq = w + ((u32)p >> 4);
        const u32 syms = funnel(pq[1], pq[0], ((u32)p & 15u) * 2u);
        const bool ok_n = kmer_valid_n(R, p, mal, winN(R.nm, p));
        const u32 got = ok_n ? kml_from_syms(syms, mal) : 0xFFFFFFFFu;
        bool fail = got != want || ok_n != want_ok;
        const bool head = g.nfree && p < g.L + g.mrd;               // a position of a query view of a genome without N
        if (head && kmer_valid_nfree_head(g.L, g.mrd, p, mal) != want_ok) fail = true;
        if (fail && bad++ < 10)
            fprintf(stderr, "mal %d L %d mrd %d nfree %d p %d: want %08x (%d), from the text %08x (%d / %d)\n", mal, g.L, g.mrd,
                    (int)g.nfree, p, want, (int)want_ok, got, (int)ok_n, head ? (int)kmer_valid_nfree_head(g.L, g.mrd, p, mal) : -1);
    }
    return n;
}

}  // namespace

int main()
{
    long n = 0, bad = 0;
    const int lens[] = {0, 1, 8, 14, 15, 16, 17, 31, 33, 63, 64, 65, 200, 1000, 4097};
    const int mrds[] = {0, 1, 7, 40};
    for (int mal : {9, 11, 15})
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
                    n += check(pack(codes, mrd), mal, bad);
                }
    printf("%ld positions compared, %ld differ\n", n, bad);
    return bad ? 1 : 0;
}
