// tile_plan_check.cpp -- TEST INFRASTRUCTURE ONLY (a stand-alone host program, tests/test_tile_plan.py builds it with
// -fsanitize=address,undefined and runs it).
//
// The decisions of an out-of-core run (lz-ani_amd/csrc/lzani_tile_plan.h) on seeded random block plans and rows, against
// what they promise:
//   the steps can be carried out from the given state of the halves and end in the state the plan returns; their tiles
//   are exactly the tiles that have pairs;
//   every CSR position of the caller is in exactly one tile's pos, once; every pair's reference lies in block i and its
//   query in block j, lref and lq are their local ids (A's genomes, then B's; A's own when j == i); the local offsets start
//   at 0, never fall, end at the tile's pair count, and the tile's rows are the caller's rows with pairs in it, in order;
//   the local genome table of every tile and the host tables of every upload equal their formulas.
// A violation exits non-zero with a message.  Every case's inputs and step list are printed for the test to compare with
// tests/ooc_model.py; the last line holds the totals: cases, A keeps / trades / uploads, B already holds the block, tiles
// with j == i, reference blocks skipped, dense rows whose own block has one genome.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan tests/model/tile_plan_check.cpp
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "../../lz-ani_amd/csrc/lzani_tile_plan.h"

using namespace lzani;

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}
uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

unsigned long long case_no = 0;
[[noreturn]] void fail(const char* what)
{
    fprintf(stderr, "tile_plan_check: %s (case %llu)\n", what, case_no);
    exit(1);
}
void need(bool ok, const char* what) { if (!ok) fail(what); }

// `m` of the genomes in [lo, hi) other than r, in random order
std::vector<uint32_t> pick(uint32_t lo, uint32_t hi, uint32_t r, uint32_t m)
{
    std::vector<uint32_t> all;
    for (uint32_t x = lo; x < hi; ++x) if (x != r) all.push_back(x);
    for (size_t k = all.size(); k > 1; --k) std::swap(all[k - 1], all[below((uint32_t)k)]);
    all.resize(std::min<size_t>(m, all.size()));
    return all;
}

struct Rows { std::vector<uint32_t> ref, q; std::vector<uint64_t> off{0}; bool dense; };

// The four row forms: dense rows of every genome, of a subset; ragged query lists (0 to 12 queries, references repeated
// and out of order, empty rows); lists that stay inside their reference's block.
Rows make_rows(int form, uint32_t n, const std::vector<uint32_t>& blk_first, const std::vector<uint32_t>& bof)
{
    Rows r;
    r.dense = form < 2;
    if (form == 0) { r.ref.resize(n); std::iota(r.ref.begin(), r.ref.end(), 0u); }
    else if (form == 1) r.ref = pick(0, n, n, 1 + below(n));
    else for (uint32_t k = 0, rows = below(41); k < rows; ++k) r.ref.push_back(below(n));
    for (size_t k = 0; k < r.ref.size(); ++k) {
        const uint32_t g = r.ref[k], b = bof[g];
        if (form == 2 && k % 7 != 3) { const auto q = pick(0, n, g, 1 + below(12)); r.q.insert(r.q.end(), q.begin(), q.end()); }
        if (form == 3) { const auto q = pick(blk_first[b], blk_first[b + 1], g, below(13)); r.q.insert(r.q.end(), q.begin(), q.end()); }
        r.off.push_back(r.dense ? r.off.back() + (n - 1) : r.q.size());
    }
    return r;
}

unsigned long long tot[8] = {0};      // the last line

void run_case(const std::vector<uint32_t>& blk_first, const std::vector<uint32_t>& bof, const TileSet& set, const Rows& rw, Halves& h)
{
    ++case_no;
    const uint32_t n = blk_first.back(), nb = (uint32_t)blk_first.size() - 1;
    const TileRows rows{(uint32_t)rw.ref.size(), rw.ref.data(), rw.off.data(), rw.dense ? nullptr : rw.q.data()};
    const uint64_t n_pairs = rw.off.back();
    printf("case %u %u", n, nb);
    for (uint32_t x : blk_first) printf(" %u", x);
    printf(" %d %d %d %u\nref", h.block[h.a], h.block[h.a ^ 1], (int)rw.dense, rows.n_rows);
    for (uint32_t x : rw.ref) printf(" %u", x);
    printf("\noff");
    for (uint64_t x : rw.off) printf(" %llu", (unsigned long long)x);
    printf("\nq");
    if (!rw.dense) for (uint32_t x : rw.q) printf(" %u", x);
    printf("\n");

    Halves sim = h;                                   // the driver's part, by hand
    const std::vector<TileStep> steps = plan_tile_steps(blk_first, bof, rows, h);
    std::vector<unsigned char> seen(n_pairs, 0), has_rows(nb, 0);
    std::vector<TileTable> tiles;
    uint64_t covered = 0;
    uint32_t last_i = 0;
    for (uint32_t k = 0; k < rows.n_rows; ++k) {
        if (rw.off[k + 1] > rw.off[k]) has_rows[bof[rw.ref[k]]] = 1;
        const uint32_t b = bof[rw.ref[k]];
        if (rw.dense && blk_first[b + 1] - blk_first[b] == 1) ++tot[7];
    }
    for (const TileStep& s : steps) {
        const uint32_t i = s.i, a0 = blk_first[i], nA = blk_first[i + 1] - a0;
        need(i < nb && has_rows[i] && (&s == &steps[0] || i > last_i), "reference blocks not ascending, or one without rows");
        last_i = i;
        has_rows[i] = 2;
        std::vector<uint32_t> want_rows;
        for (uint32_t k = 0; k < rows.n_rows; ++k) if (bof[rw.ref[k]] == i && rw.off[k + 1] > rw.off[k]) want_rows.push_back(k);
        need(s.rows == want_rows, "the step's rows are not the block's rows with pairs, in order");
        if (s.a == TILE_A_KEEPS) need(sim.block[sim.a] == (int)i, "A keeps a block it does not hold");
        else if (s.a == TILE_A_TRADES) { need(sim.block[sim.a] != (int)i && sim.block[sim.a ^ 1] == (int)i, "the halves trade places without cause"); sim.a ^= 1; }
        else { need(sim.block[0] != (int)i && sim.block[1] != (int)i, "A uploads a block that is resident"); sim.block[sim.a] = (int)i; }
        need(s.half_a == sim.a, "half_a is not the half that holds block i");
        tot[1 + s.a] += 1;
        printf("step %u %d", i, (int)s.a);
        plan_tile_tables(blk_first, bof, rows, s, tiles);
        need(tiles.size() == nb && !s.q.empty(), "a reference block without tiles");
        std::vector<unsigned char> in_step(nb, 0);
        for (const TileStep::Query& sq : s.q) {
            const uint32_t j = sq.j;
            printf(" %u %d", j, (int)sq.b_upload);
            need(j < nb && !in_step[j], "a query block twice");
            in_step[j] = 1;
            const int hB = sim.a ^ 1;
            if (sq.b_upload) { need(j != i && sim.block[hB] != (int)j, "B uploads a block that is resident"); sim.block[hB] = (int)j; }
            else need(j == i || sim.block[hB] == (int)j, "a tile whose query block is not resident");
            tot[4] += j != i && !sq.b_upload;
            tot[5] += j == i;
            // the row tables
            const TileTable& t = tiles[j];
            const uint32_t b0 = blk_first[j];
            const uint64_t tp = t.pairs();
            need(tp > 0 && sq.pairs == tp && t.lq.size() == tp && t.lref.size() == t.rows.size() && t.off.size() == t.rows.size() + 1, "table sizes");
            need(t.off[0] == 0 && t.off.back() == tp, "local offsets do not span the tile");
            for (size_t k = 0; k < t.rows.size(); ++k) {
                const uint32_t row = t.rows[k];
                need(row < rows.n_rows && (k == 0 || row > t.rows[k - 1]), "rows out of the caller's order");
                need(t.off[k + 1] > t.off[k], "a row without a pair in the tile, or falling offsets");
                need(bof[rw.ref[row]] == i && t.lref[k] == rw.ref[row] - a0, "local reference id");
                for (uint64_t e = t.off[k]; e < t.off[k + 1]; ++e) {
                    const uint64_t p = t.pos[e];
                    need(p >= rw.off[row] && p < rw.off[row + 1] && (e == t.off[k] || p > t.pos[e - 1]), "pos outside its row, or out of order");
                    need(!seen[p], "a CSR position twice");
                    seen[p] = 1;
                    const uint64_t x = p - rw.off[row];
                    const uint32_t q = rw.dense ? (uint32_t)(x < rw.ref[row] ? x : x + 1) : rw.q[p];
                    need(bof[q] == j, "query outside block j");
                    need(t.lq[e] == (j == i ? q - a0 : nA + (q - b0)), "local query id");
                }
            }
            covered += tp;
            // the genome table
            const TileGenomes g = plan_tile_genomes(set, i, j, s.half_a);
            const uint32_t nB = j == i ? 0 : blk_first[j + 1] - b0;
            need(g.L.size() == nA + nB && g.hasN.size() == nA + nB && g.nmoff.size() == nA + nB, "local genome table: size");
            for (uint32_t x = 0; x < nA + nB; ++x) {
                const uint32_t first = x < nA ? a0 : b0, gg = x < nA ? a0 + x : b0 + (x - nA);
                const uint64_t half = x < nA ? s.half_a : s.half_a ^ 1;
                need(g.L[x] == set.L[gg] && g.hasN[x] == set.hasN[gg], "local genome table: length or N flag");
                need(g.nmoff[x] == half * set.half_words + (set.nmoff[gg] - set.nmoff[first]), "local genome table: word offset");
            }
        }
        for (uint32_t j = 0; j < nb; ++j) need(in_step[j] || tiles[j].pairs() == 0, "a tile with pairs is not among the steps");
        printf("\n");
        // the uploads of this reference block
        for (size_t u = 0; u <= s.q.size(); ++u) {
            if (u == 0 ? s.a != TILE_A_UPLOADS : !s.q[u - 1].b_upload) continue;
            const uint32_t b = u == 0 ? i : s.q[u - 1].j, g0 = blk_first[b], cnt = blk_first[b + 1] - g0, hg = set.half_genomes;
            const uint64_t half = u == 0 ? s.half_a : s.half_a ^ 1;
            const TileUpload up = plan_tile_upload(set, b, (int)half);
            need(up.tab.size() == 2 * (size_t)hg && up.Ls.size() == 2 * (size_t)hg, "upload tables: size");
            need(up.code0 == set.codeoff[g0] && up.bases == set.codeoff[g0 + cnt] - set.codeoff[g0], "upload tables: codes");
            int Lmax = 0;
            for (uint32_t x = 0; x < hg; ++x) {
                const bool in = x < cnt;
                need(up.tab[x] == (in ? set.codeoff[g0 + x] - set.codeoff[g0] : 0), "upload tables: code offset");
                need(up.tab[hg + x] == (in ? half * set.half_words + (set.nmoff[g0 + x] - set.nmoff[g0]) : 0), "upload tables: word offset");
                need(up.Ls[x] == (in ? set.L[g0 + x] : 0) && up.Ls[hg + x] == 0, "upload tables: lengths");
                if (in) Lmax = std::max(Lmax, set.L[g0 + x]);
            }
            need(up.Lmax == Lmax, "upload tables: longest genome");
        }
    }
    need(covered == n_pairs && std::find(seen.begin(), seen.end(), 0) == seen.end(), "a CSR position in no tile");
    need(sim.a == h.a && sim.block[0] == h.block[0] && sim.block[1] == h.block[1], "the state after the run");
    for (uint32_t b = 0; b < nb; ++b) { need(has_rows[b] != 1, "a reference block with rows was skipped"); tot[6] += has_rows[b] == 0; }
    uint64_t n_tiles = 0, n_up = 0;
    for (const TileStep& s : steps) { n_tiles += s.q.size(); n_up += s.a == TILE_A_UPLOADS; for (const auto& sq : s.q) n_up += sq.b_upload; }
    printf("after %d %d %llu %llu\n", h.block[h.a], h.block[h.a ^ 1], (unsigned long long)n_tiles, (unsigned long long)n_up);
    ++tot[0];
}

}  // namespace

int main()
{
    for (int plan = 0; plan < 1500; ++plan) {
        const uint32_t n = 2 + below(23), nb = 2 + below(std::min<uint32_t>(6, n - 1));
        std::vector<uint32_t> blk_first = pick(1, n, n, nb - 1);      // nb - 1 cuts between the genomes
        blk_first.push_back(0); blk_first.push_back(n);
        std::sort(blk_first.begin(), blk_first.end());
        const std::vector<uint32_t> bof = block_of_genomes(blk_first);
        need(bof.size() == n, "block_of_genomes: size");
        for (uint32_t g = 0; g < n; ++g) need(blk_first[bof[g]] <= g && g < blk_first[bof[g] + 1], "block_of_genomes");
        // a genome set: lengths (empty genomes among them), word offsets, N flags, code offsets; the halves' sizes
        std::vector<int> L(n), hasN(n);
        std::vector<uint64_t> nmoff(n), codeoff(n + 1, 0);
        uint64_t words = 0, half_words = 0;
        uint32_t half_genomes = 0;
        for (uint32_t g = 0; g < n; ++g) {
            L[g] = below(5) ? (int)below(5000) : 0; hasN[g] = (int)below(2);
            nmoff[g] = words; words += (uint64_t)(2 * L[g] + 120 + 63) / 64 + 2;
            codeoff[g + 1] = codeoff[g] + (uint64_t)L[g];
        }
        for (uint32_t b = 0; b < nb; ++b) {
            half_words = std::max(half_words, (blk_first[b + 1] < n ? nmoff[blk_first[b + 1]] : words) - nmoff[blk_first[b]]);
            half_genomes = std::max(half_genomes, blk_first[b + 1] - blk_first[b]);
        }
        const TileSet set{blk_first, L, nmoff, hasN, codeoff, half_words, half_genomes};
        Halves h;                                     // empty halves, then what the run before left
        for (int run = 0; run < 3; ++run) run_case(blk_first, bof, set, make_rows((plan + run) % 4, n, blk_first, bof), h);
    }
    printf("%llu %llu %llu %llu %llu %llu %llu %llu\n", tot[0], tot[1], tot[2], tot[3], tot[4], tot[5], tot[6], tot[7]);
    return 0;
}
