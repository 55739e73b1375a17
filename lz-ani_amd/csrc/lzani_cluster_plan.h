// lzani_cluster_plan.h -- the rule and the sequential statement of the cluster stage (include/lzani.h, "clustering the kept
// pairs"): the weight of an edge, and the five algorithms on a host edge array -- union-find with the smaller root as
// parent, the greedy sweep over adjacency lists, greedy set cover by a lazy max-heap, and complete linkage by a map from
// link to (count, smallest weight) with a lazy max-heap of the links.  The device stage (lzani_kernels_cluster.h, lzani_cluster.h) calls the
// weight; the pure host functions lzani_cluster_weight and lzani_cluster_host (lzani_cluster.h) and the host binary, which
// includes this header directly, call both.  Free of HIP but for the guard macro; compiled without fast-math and with
// -ffp-contract=off: every ratio is one IEEE double division of exact integers, so host and device give the same bits.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <queue>
#include <tuple>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/lzani.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LZANI_CL_HD __host__ __device__
#else
#define LZANI_CL_HD
#endif

namespace lzani {

LZANI_CL_HD inline bool cluster_measure_known(int measure) { return measure >= LZANI_CLUSTER_TANI && measure <= LZANI_CLUSTER_ANI; }
LZANI_CL_HD inline bool cluster_algo_known(int algo)
{
    return (algo >= LZANI_CLUSTER_SINGLE && algo <= LZANI_CLUSTER_GREEDY_BEST) || algo == LZANI_CLUSTER_SET_COVER || algo == LZANI_CLUSTER_COMPLETE;
}

// a value that is not above 0 -- NaN, and the negative values and -0 that only made-up integers give -- reads as +0
LZANI_CL_HD inline double cluster_value(double v) { return v > 0 ? v : 0.0; }

// The weight of the pair a < b: X = result of (ref a, query b), Y = result of (ref b, query a), la / lb the reported lengths,
// lines as the output filter gives them.  The largest value of the measure over the lines that `lines` names; 0 for none.
LZANI_CL_HD inline double cluster_weight(int measure, const lzani_result& X, const lzani_result& Y, uint32_t lines, uint32_t la, uint32_t lb)
{
    double v0, v1;
    if (measure == LZANI_CLUSTER_TANI) {
        const int32_t mm = (int32_t)((uint32_t)X.sym_in_matches + (uint32_t)Y.sym_in_matches);
        v0 = v1 = (double)mm / (uint32_t)(la + lb);
    } else if (measure == LZANI_CLUSTER_GANI) {
        v0 = (double)X.sym_in_matches / lb;
        v1 = (double)Y.sym_in_matches / la;
    } else {
        const int32_t ax = (int32_t)((uint32_t)X.sym_in_matches + (uint32_t)X.sym_in_literals);
        const int32_t ay = (int32_t)((uint32_t)Y.sym_in_matches + (uint32_t)Y.sym_in_literals);
        v0 = ax != 0 ? (double)X.sym_in_matches / ax : 0;
        v1 = ay != 0 ? (double)Y.sym_in_matches / ay : 0;
    }
    v0 = (lines & 1u) ? cluster_value(v0) : 0.0;
    v1 = (lines & 2u) ? cluster_value(v1) : 0.0;
    return v0 > v1 ? v0 : v1;
}

// w >= 0 (or +inf): weights order like these
inline uint64_t cluster_weight_bits(double w)
{
    uint64_t b;
    memcpy(&b, &w, 8);
    return b;
}

// What every entry point checks of an edge passed in by hand.
inline bool cluster_edge_ok(uint32_t n, const lzani_cluster_edge& e) { return e.a != e.b && e.a < n && e.b < n && e.w >= 0; }

// rep_of -> cluster_of and the number of clusters: clusters numbered in ascending order of their representative.
inline uint32_t cluster_number(uint32_t n, const uint32_t* rep_of, uint32_t* cluster_of)
{
    std::vector<uint32_t> below((size_t)n + 1, 0);
    for (uint32_t v = 0; v < n; ++v) below[v + 1] = below[v] + (rep_of[v] == v ? 1u : 0u);
    if (cluster_of)
        for (uint32_t v = 0; v < n; ++v) cluster_of[v] = below[rep_of[v]];
    return below[n];
}

// The key of set cover: the unassigned node with the largest key is the next representative -- the largest count c of
// unassigned neighbours, ties to the smallest id.  v < n <= 2^32 - 1, so a key is never 0 (what an assigned node has on the
// device).
LZANI_CL_HD inline uint64_t cluster_cover_key(uint32_t c, uint32_t v) { return ((uint64_t)c << 32) | (0xFFFFFFFFu - v); }
LZANI_CL_HD inline uint32_t cluster_cover_node(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }

// LZANI_CLUSTER_SET_COVER on the edges as they come: the distinct pairs (normalised, sorted, unique), adjacency lists of
// both directions, and a max-heap of keys that is never repaired -- a popped key that is no longer its node's key is
// dropped, a count that falls pushes the new key.  Every edge lowers a count at most twice: O(E log E).
inline void cluster_cover_host(uint32_t n, const lzani_cluster_edge* edges, uint64_t count, uint32_t* rep_of)
{
    std::vector<uint64_t> pairs(count);
    for (uint64_t i = 0; i < count; ++i) {
        const uint32_t lo = edges[i].a < edges[i].b ? edges[i].a : edges[i].b, hi = edges[i].a < edges[i].b ? edges[i].b : edges[i].a;
        pairs[i] = ((uint64_t)lo << 32) | hi;
    }
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    std::vector<uint64_t> off((size_t)n + 1, 0);
    for (uint64_t p : pairs) { off[(p >> 32) + 1]++; off[(uint32_t)p + 1]++; }
    for (uint32_t v = 0; v < n; ++v) off[v + 1] += off[v];
    std::vector<uint32_t> nb(2 * pairs.size());
    std::vector<uint64_t> at(off.begin(), off.end() - 1);
    for (uint64_t p : pairs) { nb[at[p >> 32]++] = (uint32_t)p; nb[at[(uint32_t)p]++] = (uint32_t)(p >> 32); }
    std::vector<uint32_t> c(n);
    std::vector<char> assigned(n, 0);
    std::priority_queue<uint64_t> heap;
    for (uint32_t v = 0; v < n; ++v) { c[v] = (uint32_t)(off[v + 1] - off[v]); heap.push(cluster_cover_key(c[v], v)); }
    std::vector<uint32_t> taken;
    while (!heap.empty()) {
        const uint64_t key = heap.top();
        heap.pop();
        const uint32_t v = cluster_cover_node(key);
        if (assigned[v] || key != cluster_cover_key(c[v], v)) continue;          // (a key of before a count fell)
        taken.assign(1, v);
        for (uint64_t e = off[v]; e < off[v + 1]; ++e)
            if (!assigned[nb[e]]) taken.push_back(nb[e]);
        for (uint32_t u : taken) { rep_of[u] = v; assigned[u] = 1; }
        for (uint32_t u : taken)
            for (uint64_t e = off[u]; e < off[u + 1]; ++e) {
                const uint32_t y = nb[e];
                if (!assigned[y]) heap.push(cluster_cover_key(--c[y], y));
            }
    }
}

// LZANI_CLUSTER_COMPLETE on the edges as they come.  The distinct pairs with their smallest weight (sorted by pair, then by
// weight bits: the first record of a pair).  A cluster is known by a handle, the id it had when it was a node; id[h] is
// its smallest member.  pair[key(h, z)] = (count, wmin) of the edges between two live clusters, kept only while the pair can
// still be a link: when x and y merge, the neighbours of the union are those z of the shorter adjacency list that both
// have an entry with and whose summed count is |x u y| * |z| -- every other entry is incomplete for good (no superset of
// an incomplete pair is complete), so a count kept here is never above the true one and equals it where it matters.  The
// heap holds (s, ~lower id, ~other id, handles) of every link there is, pushed when it comes to be; it is never repaired:
// a popped entry counts only if both handles live, carry those ids, and their pair is a link of that value now.  A merge
// costs the shorter of two adjacency lists and the lists only shrink: O(E log E) on sparse graphs.
inline void cluster_link_host(uint32_t n, const lzani_cluster_edge* edges, uint64_t count, uint32_t* rep_of)
{
    typedef std::pair<uint64_t, uint64_t> Rec;                                    // (lo << 32 | hi, weight bits); later (count, wmin)
    std::vector<Rec> recs(count);
    for (uint64_t i = 0; i < count; ++i) {
        const uint32_t lo = edges[i].a < edges[i].b ? edges[i].a : edges[i].b, hi = edges[i].a < edges[i].b ? edges[i].b : edges[i].a;
        recs[i] = Rec(((uint64_t)lo << 32) | hi, cluster_weight_bits(cluster_value(edges[i].w)));
    }
    std::sort(recs.begin(), recs.end());
    recs.erase(std::unique(recs.begin(), recs.end(), [](const Rec& x, const Rec& y) { return x.first == y.first; }), recs.end());
    auto key = [](uint32_t x, uint32_t y) { return x < y ? ((uint64_t)x << 32) | y : ((uint64_t)y << 32) | x; };
    typedef std::tuple<uint64_t, uint32_t, uint32_t, uint32_t, uint32_t> Link;    // s, ~lower id, ~other id, the two handles
    std::priority_queue<Link> heap;
    std::unordered_map<uint64_t, Rec> pair;
    pair.reserve(recs.size());
    std::vector<std::vector<uint32_t>> adj(n);
    std::vector<uint32_t> id(n), size(n, 1), into(n);
    std::vector<char> live(n, 1);
    for (uint32_t v = 0; v < n; ++v) id[v] = into[v] = v;
    for (const Rec& r : recs) {
        const uint32_t lo = (uint32_t)(r.first >> 32), hi = (uint32_t)r.first;
        pair[r.first] = Rec(1, r.second);
        adj[lo].push_back(hi); adj[hi].push_back(lo);
        heap.push(Link(r.second, ~lo, ~hi, lo, hi));
    }
    std::vector<uint32_t> next;
    while (!heap.empty()) {
        const Link top = heap.top();
        heap.pop();
        uint32_t x = std::get<3>(top), y = std::get<4>(top);
        if (!live[x] || !live[y]) continue;
        if ((id[x] < id[y] ? id[x] : id[y]) != ~std::get<1>(top) || (id[x] < id[y] ? id[y] : id[x]) != ~std::get<2>(top)) continue;
        const auto it = pair.find(key(x, y));
        if (it == pair.end() || it->second.first != (uint64_t)size[x] * size[y] || it->second.second != std::get<0>(top)) continue;
        pair.erase(it);
        if (adj[x].size() > adj[y].size()) std::swap(x, y);                       // x has the shorter list and goes into y
        const uint32_t merged = size[x] + size[y], mid = id[x] < id[y] ? id[x] : id[y];
        next.clear();
        for (uint32_t z : adj[x]) {
            if (z == y || !live[z]) continue;
            const auto xz = pair.find(key(x, z));
            if (xz == pair.end()) continue;                                       // (listed twice, or dropped before)
            const Rec ex = xz->second;
            pair.erase(xz);
            const auto yz = pair.find(key(y, z));
            if (yz == pair.end()) continue;
            const Rec both(ex.first + yz->second.first, ex.second < yz->second.second ? ex.second : yz->second.second);
            if (both.first != (uint64_t)merged * size[z]) { pair.erase(yz); continue; }
            yz->second = both;
            next.push_back(z);
            heap.push(Link(both.second, ~(mid < id[z] ? mid : id[z]), ~(mid < id[z] ? id[z] : mid), y, z));
        }
        live[x] = 0; into[x] = y;
        size[y] = merged; id[y] = mid;
        adj[y].swap(next);
        std::vector<uint32_t>().swap(adj[x]);
    }
    for (uint32_t v = 0; v < n; ++v) {
        uint32_t h = v;
        while (into[h] != h) { into[h] = into[into[h]]; h = into[h]; }
        rep_of[v] = id[h];
    }
}

// The sequential statement.  rep_of[n] is written; cluster_of and n_clusters may be null.  LZANI_ERR_ARG for an edge that
// cluster_edge_ok refuses or an unknown algo; (b, a) with b > a is the edge (a, b).
inline int cluster_host(uint32_t n, const lzani_cluster_edge* edges, uint64_t count, int algo, uint32_t* rep_of, uint32_t* cluster_of, uint32_t* n_clusters)
{
    if (!rep_of || (count && !edges) || !cluster_algo_known(algo)) return LZANI_ERR_ARG;
    for (uint64_t i = 0; i < count; ++i)
        if (!cluster_edge_ok(n, edges[i])) return LZANI_ERR_ARG;
    if (algo == LZANI_CLUSTER_SINGLE) {
        std::vector<uint32_t> parent(n);
        for (uint32_t v = 0; v < n; ++v) parent[v] = v;
        auto root = [&](uint32_t v) {
            while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; }
            return v;
        };
        for (uint64_t i = 0; i < count; ++i) {
            const uint32_t ra = root(edges[i].a), rb = root(edges[i].b);
            if (ra != rb) parent[ra > rb ? ra : rb] = ra > rb ? rb : ra;         // the smaller root is the parent
        }
        for (uint32_t v = 0; v < n; ++v) rep_of[v] = root(v);                     // ... so a root is its tree's smallest id
    } else if (algo == LZANI_CLUSTER_SET_COVER) {
        cluster_cover_host(n, edges, count, rep_of);
    } else if (algo == LZANI_CLUSTER_COMPLETE) {
        cluster_link_host(n, edges, count, rep_of);
    } else {
        // adjacency lists of the neighbours below each node
        std::vector<uint64_t> off((size_t)n + 1, 0);
        for (uint64_t i = 0; i < count; ++i) off[(edges[i].a > edges[i].b ? edges[i].a : edges[i].b) + 1]++;
        for (uint32_t v = 0; v < n; ++v) off[v + 1] += off[v];
        std::vector<uint32_t> nb(count);
        std::vector<double> nw(count);
        std::vector<uint64_t> at(off.begin(), off.end() - 1);
        for (uint64_t i = 0; i < count; ++i) {
            const uint32_t lo = edges[i].a < edges[i].b ? edges[i].a : edges[i].b, hi = edges[i].a < edges[i].b ? edges[i].b : edges[i].a;
            nb[at[hi]] = lo; nw[at[hi]] = edges[i].w; at[hi]++;
        }
        for (uint32_t v = 0; v < n; ++v) {              // the sweep: every node below v is placed
            uint32_t best = v;
            double best_w = 0;
            for (uint64_t e = off[v]; e < off[v + 1]; ++e) {
                const uint32_t r = nb[e];
                if (rep_of[r] != r) continue;
                const bool better = best == v || (algo == LZANI_CLUSTER_GREEDY_FIRST ? r < best : (nw[e] > best_w || (nw[e] == best_w && r < best)));
                if (better) { best = r; best_w = nw[e]; }
            }
            rep_of[v] = best;
        }
    }
    const uint32_t k = cluster_number(n, rep_of, cluster_of);
    if (n_clusters) *n_clusters = k;
    return LZANI_OK;
}

}  // namespace lzani
