// lzani_tile_plan.h -- the decisions of an out-of-core run (lzani_ooc.h) as host functions: the order of its tiles and what
// the two halves do before each, the local row tables of a reference block's tiles, the local genome table of a tile and
// the host tables of a block upload.  No HIP types: it compiles with a plain C++ compiler, and it is not among the sources
// a run-time compile embeds (lzani_rtc.h).  run_rows_tiled and ooc_upload copy and launch what these functions hand them.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace lzani {

// The caller's rows: CSR over (reference, queries); query_ids null for dense rows, whose row of reference r holds every
// other genome in id order.
struct TileRows {
    uint32_t n_rows;
    const uint32_t* ref_ids;
    const uint64_t* row_off;
    const uint32_t* query_ids;
};

// block b = genomes [blk_first[b], blk_first[b + 1]) -> the block of every genome
inline std::vector<uint32_t> block_of_genomes(const std::vector<uint32_t>& blk_first)
{
    std::vector<uint32_t> bof(blk_first.back());
    for (uint32_t b = 0; b + 1 < blk_first.size(); ++b) std::fill(bof.begin() + blk_first[b], bof.begin() + blk_first[b + 1], b);
    return bof;
}

// ---- the step list of a run

// The block each half of the resident region holds (-1: none), and which half is A, the reference block's.
struct Halves {
    int block[2] = {-1, -1};
    int a = 0;
};

enum TileA { TILE_A_KEEPS = 0, TILE_A_TRADES = 1, TILE_A_UPLOADS = 2 };

// Reference block i goes to A -- it is there, or the halves trade places, or it is uploaded -- which is half half_a from
// here on; then the tiles (i, q[..].j) in this order, each behind an upload of block j into B where b_upload says so;
// `pairs` is what the tile holds.  rows: the caller's rows whose reference is in block i and that have pairs, in order.
struct TileStep {
    struct Query { uint32_t j; bool b_upload; uint64_t pairs; };
    uint32_t i;
    TileA a;
    int half_a;
    std::vector<Query> q;
    std::vector<uint32_t> rows;
};

// The order of a run (the rule lzani_ooc.h documents): reference blocks ascending, those that have rows with pairs;
// the query blocks of block i that have pairs of its rows: i itself first (its queries are in A), then the block B
// holds, then the others ascending.  `h` is the state of the halves before the run and after it.
inline std::vector<TileStep> plan_tile_steps(const std::vector<uint32_t>& blk_first, const std::vector<uint32_t>& bof, const TileRows& r, Halves& h)
{
    const uint32_t nb = (uint32_t)blk_first.size() - 1;
    std::vector<uint64_t> pairs((size_t)nb * nb, 0);                   // of tile (i, j)
    std::vector<std::vector<uint32_t>> rows_of(nb);
    for (uint32_t k = 0; k < r.n_rows; ++k) {
        if (r.row_off[k + 1] == r.row_off[k]) continue;
        const uint32_t i = bof[r.ref_ids[k]];
        rows_of[i].push_back(k);
        uint64_t* row = pairs.data() + (size_t)i * nb;
        if (r.query_ids) for (uint64_t e = r.row_off[k]; e < r.row_off[k + 1]; ++e) ++row[bof[r.query_ids[e]]];
        else for (uint32_t j = 0; j < nb; ++j) row[j] += blk_first[j + 1] - blk_first[j] - (j == i ? 1 : 0);
    }
    std::vector<TileStep> steps;
    for (uint32_t i = 0; i < nb; ++i) {
        const uint64_t* row = pairs.data() + (size_t)i * nb;
        if (rows_of[i].empty()) continue;
        TileStep s{i, TILE_A_KEEPS, h.a, {}, std::move(rows_of[i])};
        if (h.block[h.a] != (int)i) {
            if (h.block[h.a ^ 1] == (int)i) { s.a = TILE_A_TRADES; h.a ^= 1; }
            else { s.a = TILE_A_UPLOADS; h.block[h.a] = (int)i; }
        }
        s.half_a = h.a;
        int& held = h.block[h.a ^ 1];
        std::vector<uint32_t> order;
        if (row[i]) order.push_back(i);
        if (held >= 0 && held != (int)i && row[held]) order.push_back((uint32_t)held);
        for (uint32_t j = 0; j < nb; ++j) if (j != i && (int)j != held && row[j]) order.push_back(j);
        for (uint32_t j : order) {
            const bool up = j != i && held != (int)j;
            if (up) held = (int)j;
            s.q.push_back({j, up, row[j]});
        }
        steps.push_back(std::move(s));
    }
    return steps;
}

// ---- the local row tables of one reference block's tiles

// Tile (i, j) as a run of its own on the local genome table (A's genomes 0 .. nA-1, then B's; A's own when j == i):
// the caller's rows that have pairs in it, in the caller's order; their local reference ids; the local CSR (closed:
// off.back() is the tile's pair count) and query ids; pos[e], the caller's CSR position of the tile's pair e.
struct TileTable {
    std::vector<uint32_t> rows, lref, lq;
    std::vector<uint64_t> off, pos;
    uint64_t pairs() const { return pos.size(); }
};

// The tables of step s's tiles into t[j] (whose vectors keep their memory from block to block), sized once by the step's
// pair counts.
inline void plan_tile_tables(const std::vector<uint32_t>& blk_first, const std::vector<uint32_t>& bof, const TileRows& r, const TileStep& s, std::vector<TileTable>& t)
{
    const uint32_t nb = (uint32_t)blk_first.size() - 1, i = s.i, a0 = blk_first[i], nA = blk_first[i + 1] - a0;
    t.resize(nb);
    for (TileTable& x : t) { x.rows.clear(); x.lref.clear(); x.lq.clear(); x.off.clear(); x.pos.clear(); }
    for (const TileStep::Query& sq : s.q) { t[sq.j].lq.reserve(sq.pairs); t[sq.j].pos.reserve(sq.pairs); }
    for (uint32_t k : s.rows) {
        const uint32_t ref = r.ref_ids[k];
        const uint64_t e0 = r.row_off[k], e1 = r.row_off[k + 1];
        for (uint64_t e = e0; e < e1; ++e) {
            const uint32_t q = r.query_ids ? r.query_ids[e] : (uint32_t)(e - e0 < ref ? e - e0 : e - e0 + 1);
            TileTable& x = t[bof[q]];
            if (x.rows.empty() || x.rows.back() != k) { x.rows.push_back(k); x.lref.push_back(ref - a0); x.off.push_back(x.pairs()); }
            x.lq.push_back(q);
            x.pos.push_back(e);
        }
    }
    for (uint32_t j = 0; j < nb; ++j) {
        TileTable& x = t[j];
        x.off.push_back(x.pairs());
        const uint32_t b0 = blk_first[j];
        for (uint32_t& q : x.lq) q = j == i ? q - a0 : nA + (q - b0);          // the set's id -> the tile's
    }
}

// ---- the local genome table of a tile, the host tables of an upload

// What of an out-of-core genome set they are made from (GenomeSet): the block plan, per genome its length, the word
// offset of its packed text in the set, whether it holds an N and the offset of its codes in the host copy; the packed
// words of one half and the genomes of the largest block.
struct TileSet {
    const std::vector<uint32_t>& blk_first;
    const std::vector<int>& L;
    const std::vector<uint64_t>& nmoff;
    const std::vector<int>& hasN;
    const std::vector<uint64_t>& codeoff;
    uint64_t half_words;
    uint32_t half_genomes;
    // where genome g of block b sits in half h, in packed words
    uint64_t word_off(uint32_t b, uint32_t g, int h) const { return (uint64_t)h * half_words + (nmoff[g] - nmoff[blk_first[b]]); }
};

// The genome table of tile (i, j) with A in half half_a: block i's genomes, then block j's unless j == i.
struct TileGenomes {
    std::vector<int> L, hasN;
    std::vector<uint64_t> nmoff;
};
inline TileGenomes plan_tile_genomes(const TileSet& s, uint32_t i, uint32_t j, int half_a)
{
    TileGenomes t;
    const size_t n = (s.blk_first[i + 1] - s.blk_first[i]) + (j != i ? s.blk_first[j + 1] - s.blk_first[j] : 0);
    t.L.reserve(n); t.hasN.reserve(n); t.nmoff.reserve(n);
    const auto add = [&](uint32_t b, int h) {
        for (uint32_t g = s.blk_first[b]; g < s.blk_first[b + 1]; ++g) {
            t.L.push_back(s.L[g]);
            t.hasN.push_back(s.hasN[g]);
            t.nmoff.push_back(s.word_off(b, g, h));
        }
    };
    add(i, half_a);
    if (j != i) add(j, half_a ^ 1);
    return t;
}

// The upload of block b into half h: `bases` codes from code0 of the host copy; tab = per genome of the block the offset
// of its codes in them, then (from half_genomes on) its word offset in the region; Ls = the lengths, then (from
// half_genomes on) room for the N flags, cleared; the longest of the lengths.
struct TileUpload {
    uint64_t code0, bases;
    std::vector<uint64_t> tab;
    std::vector<int> Ls;
    int Lmax;
};
inline TileUpload plan_tile_upload(const TileSet& s, uint32_t b, int h)
{
    const uint32_t g0 = s.blk_first[b], g1 = s.blk_first[b + 1], hg = s.half_genomes;
    TileUpload u{s.codeoff[g0], s.codeoff[g1] - s.codeoff[g0], std::vector<uint64_t>((size_t)2 * hg, 0), std::vector<int>((size_t)2 * hg, 0), 0};
    for (uint32_t g = g0; g < g1; ++g) {
        u.tab[g - g0] = s.codeoff[g] - s.codeoff[g0];
        u.tab[hg + g - g0] = s.word_off(b, g, h);
        u.Ls[g - g0] = s.L[g];
        u.Lmax = std::max(u.Lmax, s.L[g]);
    }
    return u;
}

}  // namespace lzani
