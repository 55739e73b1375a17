// refill_resolve_check.cpp -- TEST INFRASTRUCTURE ONLY (a stand-alone host program, tests/test_refill_resolve.py builds and runs it).
//
// The pair kernel's refill (DevWave::refill) resolves a queued candidate from ONE fetch of each text: the dwords
// (p >> 4) - 1 .. (p >> 4) + 3 around the query position qp and the reference position pos (lzani_core.h: text_words5),
// reduced to four XOR words aligned to the candidate (resolve_diff).  The 32-symbol compare (diff_same32) and the
// candidate's null-extension record (null_ext_record_diff, which builds validity masks only where a window leaves its
// strand) come out of those.  This program checks them against the statements they replace:
//     same  = the first differing symbol of win2f(R, pos) ^ win2f(Q, qp);  al = imin(same, bound of both runs)
//     record = null_ext_record(P, R, Q, qp, pos, al), in its 16-symbol AND its 32-symbol form (the latter shares no mask
//              code with the new function)
// What is independent here are the windows (which symbols are looked at) and the validity masks.  The ENCODING of a record
// from its two mismatch masks is not: null_ext_record and null_ext_record_diff both call ext_record_bwd / ext_record_fwd,
// so an error there would show on both sides.  The encoding is pinned elsewhere -- by the host model against the oracle
// (tests/test_model.py) and by every GPU test that compares pairs with the oracle.
// on random N-free texts -- the reference with its reverse-complement half (mrd 0, 5, 40), the query without one --
// for every (qp & 15, pos & 15), planted matches of every length 0..40 with mismatching flanks, starts at 0..33 in
// either text, matches ending 0..48 symbols in front of L, rc0, rc0 + L, len of the reference and L, D of the query,
// and (aw, am, ar) = (2, 0, 1), (8, 3, 2), (15, 7, 3).  Exit status 0 = all equal; it prints the number of cases.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/model/refill_resolve_check.cpp   (memory check of the same run)
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
    std::vector<u64> t2, nm;
};

// fwd | N^2mrd | RC | N^mrd, spare symbols flagged N (k_pack; tests/model/lzani_model.cpp: pack_genome).  The vectors
// hold exactly text_words2 / text_wordsN words: a read behind what the layout guarantees is a sanitizer error.
Text pack(const std::vector<uint8_t>& codes, int mrd)
{
    Text g;
    g.L = (int)codes.size(); g.T = ref_text_len(g.L, mrd); g.mrd = mrd;
    g.t2.assign(text_words2(g.T), 0);
    g.nm.assign(text_wordsN(g.T), ~0ULL);
    auto put = [&](int p, int c) { g.t2[p >> 5] |= (u64)c << ((p & 31) * 2); g.nm[p >> 6] &= ~(1ULL << (p & 63)); };
    for (int j = 0; j < g.L; ++j) put(j, codes[j]);
    const int rc0 = g.L + 2 * mrd;
    for (int j = 0; j < g.L; ++j) put(rc0 + j, 3 - codes[g.L - 1 - j]);
    return g;
}

// symbol x of the reference text, -1 = a pad
int ref_sym(const std::vector<uint8_t>& rc, int mrd, int x)
{
    const int L = (int)rc.size(), rc0 = L + 2 * mrd;
    if (x >= 0 && x < L) return rc[(size_t)x];
    if (x >= rc0 && x < rc0 + L) return 3 - rc[(size_t)(L - 1 - (x - rc0))];
    return -1;
}

long n_cases = 0, n_bad = 0, n_rec = 0, n_masked = 0;
long seen_al[41], seen_off[256];

const Params PS[3] = {{11, 7, 40, 40, 35, 2, 0, 1}, {11, 7, 40, 40, 35, 8, 3, 2}, {11, 7, 40, 40, 35, 15, 7, 3}};

// one candidate: the query is the reference's neighbourhood of pos, mutated, laid around qp, with exactly m matching
// symbols from qp on where the texts allow it and mismatching symbols on both sides of them
void run_case(const std::vector<uint8_t>& rcodes, const Text& RT, int mrd, int Lq, int qp, int pos, int m, int m_sel)
{
    if (qp < 0 || pos < 0 || qp >= Lq + mrd || pos >= RT.T || Lq < 1) return;
    std::vector<uint8_t> qc((size_t)Lq);
    for (auto& c : qc) c = (uint8_t)(rnd() & 3u);
    const u32 rate = (rnd() % 3u == 0) ? 3u : (rnd() % 2u ? 12u : 40u);    // mismatches per 64 symbols of the flanks
    for (int j = -40; j < m + 40; ++j) {
        const int x = qp + j, s = ref_sym(rcodes, mrd, pos + j);
        if (x < 0 || x >= Lq || s < 0) continue;
        const bool match = (j >= 0 && j < m) || (j != -1 && j != m && rnd() % 64u >= rate);
        qc[(size_t)x] = (uint8_t)(match ? s : (s + 1 + (int)(rnd() % 3u)) & 3);
    }
    const Text QT = pack(qc, mrd);
    const TextView R = ref_view(RT.t2.data(), RT.nm.data(), RT.L, mrd, true);
    const TextView Q = qry_view(QT.t2.data(), QT.nm.data(), QT.L, mrd, true);

    const u64 x = win2f(R.t2, pos) ^ win2f(Q.t2, qp);
    const u64 mm = (x | (x >> 1)) & 0x5555555555555555ULL;
    const int want_same = mm ? (int)__builtin_ctzll(mm) >> 1 : 32;
    const int bound = imin(run_end(R, pos) - pos, run_end(Q, qp) - qp);
    const int al = imin(want_same, bound);

    const ResolveDiff D = resolve_diff(text_words5(R.t2, pos), pos, text_words5(Q.t2, qp), qp);
    const int got_same = diff_same32(D);
    bool fail = got_same != want_same;
    const bool lng = want_same == 32 && bound > 32;                       // (such a candidate carries no record)
    seen_al[lng ? 33 : al] += 1;
    seen_off[(qp & 15) * 16 + (pos & 15)] += 1;
    u32 want = 0, wide = 0, got = 0;
    if (!lng) {
        const Params& P = PS[m_sel];
        want = null_ext_record(P, R, Q, qp, pos, al, true);
        wide = null_ext_record(P, R, Q, qp, pos, al, false);
        got = null_ext_record_diff(P, R, Q, D, qp, pos, al);
        fail |= got != want || got != wide;
        n_rec += 1;
        n_masked += !(span_in_strand(R, pos, al + 16) & span_in_strand(Q, qp, al + 16));
    }
    n_cases += 1;
    if (fail && n_bad++ < 10)
        fprintf(stderr, "Lr %d Lq %d mrd %d qp %d pos %d m %d aw %d: same %d want %d, bound %d, record %08x want %08x (wide %08x)\n",
                RT.L, Lq, mrd, qp, pos, m, PS[m_sel].aw, got_same, want_same, bound, got, want, wide);
}

}  // namespace

int main()
{
    for (long& v : seen_al) v = 0;
    for (long& v : seen_off) v = 0;
    const int mrds[] = {0, 5, 40};
    for (int mrd : mrds) {
        const int Lr = 150 + (int)(rnd() % 60u), Lq = 140 + (int)(rnd() % 60u);
        std::vector<uint8_t> rc((size_t)Lr);
        for (auto& c : rc) c = (uint8_t)(rnd() & 3u);
        const Text RT = pack(rc, mrd);
        const int rc0 = Lr + 2 * mrd, D = Lq + mrd;
        for (int ps = 0; ps < 3; ++ps) {
            // every (qp & 15, pos & 15) x every length, in the forward and in the reverse-complement half
            for (int a = 0; a < 16; ++a)
                for (int b = 0; b < 16; ++b)
                    for (int m = 0; m <= 40; ++m) {
                        run_case(rc, RT, mrd, Lq, 48 + a, 64 + b, m, ps);
                        run_case(rc, RT, mrd, Lq, 32 + a, rc0 + 48 + b, m, ps);
                    }
            // starts at 0..33 in either text
            for (int a = 0; a <= 33; ++a)
                for (int b = 0; b <= 33; ++b)
                    for (int m = 0; m <= 40; m += (a + b) % 3 + 1) {
                        run_case(rc, RT, mrd, Lq, a, b, m, ps);
                        run_case(rc, RT, mrd, Lq, a, 50 + b, m, ps);
                        run_case(rc, RT, mrd, Lq, 50 + a, b, m, ps);
                        run_case(rc, RT, mrd, Lq, a, rc0 + b, m, ps);
                    }
            // matches ending e symbols in front of every end of the reference, and of the query
            const int rends[4] = {Lr, rc0, rc0 + Lr, RT.T}, qends[2] = {Lq, D};
            for (int e = 0; e <= 48; ++e)
                for (int m = 0; m <= 40; ++m) {
                    for (int k = 0; k < 4; ++k) run_case(rc, RT, mrd, Lq, 40 + (e * 7 + m) % 16, rends[k] - e - m, m, ps);
                    for (int k = 0; k < 2; ++k) run_case(rc, RT, mrd, Lq, qends[k] - e - m, 40 + (e * 5 + m) % 16, m, ps);
                    for (int k = 0; k < 2; ++k) run_case(rc, RT, mrd, Lq, qends[k] - e - m, rends[2 * k] - e - m, m, ps);   // both at once
                }
        }
    }
    int missing = 0;
    for (int k = 0; k <= 33; ++k) missing += seen_al[k] == 0;                // al 0..32, and candidates longer than the compare
    for (int k = 0; k < 256; ++k) missing += seen_off[k] == 0;
    printf("%ld cases compared, %ld differ; %ld records, %ld of them with validity masks; %d lengths or offsets never seen\n", n_cases, n_bad, n_rec,
           n_masked, missing);
    return (n_bad || missing || n_masked < 1000) ? 1 : 0;
}
