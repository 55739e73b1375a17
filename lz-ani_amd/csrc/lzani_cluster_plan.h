// lzani_cluster_plan.h -- the rule and the sequential statement of the cluster stage (include/lzani.h, "clustering the kept
// pairs"): the weight of an edge, the cut of a cluster level (cluster_cut_lines, over lzani_out_filter.h), and the six algorithms on a host edge array -- union-find with the smaller root as
// parent, the greedy sweep over adjacency lists, greedy set cover by a lazy max-heap, complete linkage by a map from
// link to (count, smallest weight) with a lazy max-heap of the links, and Leiden (CPM) by the rounds of its statement over
// adjacency lists per level.  The device stage (lzani_kernels_cluster.h, lzani_cluster.h) calls the
// weight (and Leiden's quantisation); the pure host functions lzani_cluster_weight, lzani_cluster_host and lzani_cluster_leiden_host (lzani_cluster.h) and the host binary, which
// includes this header directly, call both.  Free of HIP but for the guard macro; compiled without fast-math and with
// -ffp-contract=off: every ratio is one IEEE double division of exact integers, so host and device give the same bits.
#pragma once
#include <stdint.h>
#include <string.h>

#include <math.h>

#include <algorithm>
#include <map>
#include <queue>
#include <tuple>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/lzani.h"
#include "lzani_out_filter.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LZANI_CL_HD __host__ __device__
#else
#define LZANI_CL_HD
#endif

namespace lzani {

LZANI_CL_HD inline bool cluster_measure_known(int measure) { return measure >= LZANI_CLUSTER_TANI && measure <= LZANI_CLUSTER_ANI; }
LZANI_CL_HD inline bool cluster_algo_known(int algo)
{
    return (algo >= LZANI_CLUSTER_SINGLE && algo <= LZANI_CLUSTER_GREEDY_BEST) || algo == LZANI_CLUSTER_SET_COVER || algo == LZANI_CLUSTER_COMPLETE ||
           algo == LZANI_CLUSTER_LEIDEN;
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

// ---- the cut of a cluster level (include/lzani.h, "cluster levels") ---------------------------------------------------
// a cut that every entry point takes: no minimum that is not a number, the reserved word 0
LZANI_CL_HD inline bool cluster_cut_ok(const lzani_cluster_cut& c)
{
    const lzani_out_filter f{c.min_tani, c.min_gani, c.min_ani, c.min_qcov, c.min_rcov};
    return !out_filter_has_nan(f) && c.min_len_ratio == c.min_len_ratio && c.reserved_ == 0;
}

// len_ratio of a pair as the emitter prints it (host/emit.h): the shorter length over the longer, 0 where either is 0
LZANI_CL_HD inline double cluster_len_ratio(uint32_t la, uint32_t lb)
{
    if (!la || !lb) return 0.0;
    return la < lb ? (double)la / (double)lb : (double)lb / (double)la;
}

// a line's num_alns against the cut's maximum (0: none)
LZANI_CL_HD inline bool cluster_cut_alns(const lzani_cluster_cut& c, const lzani_result& own)
{
    return c.max_num_alns == 0 || (int64_t)own.no_components <= (int64_t)c.max_num_alns;
}

// The lines of the kept record (a < b, X, Y, lines) that stay under the cut: the five minima as the output filter applies
// them to each line, len_ratio for both, num_alns for each; never a line that `lines` does not name.  The record is an edge
// of the level iff the result is not 0, with the weight cluster_weight(measure, X, Y, result, la, lb).
LZANI_CL_HD inline uint32_t cluster_cut_lines(const lzani_cluster_cut& c, const lzani_result& X, const lzani_result& Y, uint32_t lines, uint32_t la, uint32_t lb)
{
    const lzani_out_filter f{c.min_tani, c.min_gani, c.min_ani, c.min_qcov, c.min_rcov};
    const double tani = out_pair_tani(X, Y, la, lb);
    const bool both = !(cluster_len_ratio(la, lb) < c.min_len_ratio);
    const bool pass0 = both && cluster_cut_alns(c, X) && out_filter_line(f, out_line_ratios(tani, X, Y, lb, la));
    const bool pass1 = both && cluster_cut_alns(c, Y) && out_filter_line(f, out_line_ratios(tani, Y, X, la, lb));
    return lines & ((pass0 ? 1u : 0u) | (pass1 ? 2u : 0u));
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

// ---- LZANI_CLUSTER_LEIDEN ---------------------------------------------------------------------------------------------
// The arithmetic of the statement: weights and the resolution in units of 2^-20, everything else in signed 64 bits.
constexpr int64_t CL_LEIDEN_ONE = (int64_t)1 << 20;
constexpr uint32_t CL_LEIDEN_MAX_N = 1u << 21;          // g * n^2 stays inside 2^62
constexpr double CL_LEIDEN_RESOLUTION = 0.7;
constexpr int CL_LEIDEN_ITERATIONS = 2, CL_LEIDEN_MAX_ITERATIONS = 16;
constexpr uint64_t CL_LEIDEN_CAP_MUL = 64, CL_LEIDEN_CAP_ADD = 64;   // a phase of cap_mul * n_level + cap_add rounds is stopped
// w >= 0 or +inf: min(floor(w * 2^20), 2^20).  The product is exact, the conversion truncates what is not negative.
LZANI_CL_HD inline int64_t cluster_leiden_q(double w) { return w >= 1.0 ? CL_LEIDEN_ONE : (int64_t)(w * 1048576.0); }
inline bool cluster_leiden_params_ok(double resolution, int iterations)
{
    return resolution >= 0 && resolution <= 1 && iterations >= 1 && iterations <= CL_LEIDEN_MAX_ITERATIONS;   // (NaN fails the first)
}
inline int64_t cluster_leiden_g(double resolution) { return (int64_t)llround(resolution * 1048576.0); }

// A level of the sequential form: sizes, the distinct entries a < b with their q, the partition P (a community's id is its
// smallest member) and the adjacency map of every node.
struct LeidenLevel {
    uint32_t m = 0;
    std::vector<int64_t> s;
    std::vector<uint64_t> key;
    std::vector<int64_t> q;
    std::vector<uint32_t> P;
    std::vector<std::vector<std::pair<uint32_t, int64_t>>> adj;
    void link()
    {
        adj.assign(m, std::vector<std::pair<uint32_t, int64_t>>());
        for (size_t i = 0; i < key.size(); ++i) {
            const uint32_t a = (uint32_t)(key[i] >> 32), b = (uint32_t)key[i];
            adj[a].push_back(std::make_pair(b, q[i]));
            adj[b].push_back(std::make_pair(a, q[i]));
        }
    }
};

// labels (any values below `span`) -> the smallest member of every label's set
inline void leiden_smallest_member(std::vector<uint32_t>& part, const std::vector<uint32_t>& labels, size_t span)
{
    std::vector<uint32_t> low(span, 0xFFFFFFFFu);
    for (uint32_t v = 0; v < labels.size(); ++v)
        if (v < low[labels[v]]) low[labels[v]] = v;
    for (uint32_t v = 0; v < labels.size(); ++v) part[v] = low[labels[v]];
}

// The largest key of a community over the candidates that touch it: the largest D, ties to the smallest node.
struct LeidenTouch {
    std::vector<int64_t> D;
    std::vector<uint32_t> v;
    explicit LeidenTouch(uint32_t m) : D(m, -1), v(m, 0xFFFFFFFFu) {}
    void touch(uint32_t c, int64_t d, uint32_t node)
    {
        if (d > D[c] || (d == D[c] && node < v[c])) { D[c] = d; v[c] = node; }
    }
};

// One moving round; returns the movers.
inline uint64_t leiden_move_round(LeidenLevel& L, int64_t g)
{
    const uint32_t m = L.m, ALONE = m;
    std::vector<int64_t> S(m, 0), D(m, 0);
    std::vector<uint32_t> T(m, 0);
    for (uint32_t v = 0; v < m; ++v) S[L.P[v]] += L.s[v];
    std::map<uint32_t, int64_t> W;
    for (uint32_t v = 0; v < m; ++v) {
        W.clear();
        for (const auto& e : L.adj[v]) W[L.P[e.first]] += e.second;
        const uint32_t own = L.P[v];
        const auto at = W.find(own);
        const int64_t val_own = (at == W.end() ? 0 : at->second) - g * L.s[v] * (S[own] - L.s[v]);
        int64_t best = val_own;                                                   // staying first
        uint32_t target = own;
        for (const auto& c : W) {                                                 // then the smallest community id
            if (c.first == own) continue;
            const int64_t val = c.second - g * L.s[v] * S[c.first];
            if (val > best) { best = val; target = c.first; }
        }
        if (S[own] != L.s[v] && 0 > best) { best = 0; target = ALONE; }          // alone last
        D[v] = best - val_own; T[v] = target;
    }
    LeidenTouch t(m);
    for (uint32_t v = 0; v < m; ++v) {
        if (D[v] <= 0) continue;
        t.touch(L.P[v], D[v], v);
        if (T[v] != ALONE) t.touch(T[v], D[v], v);
    }
    std::vector<uint32_t> labels(L.P);
    uint64_t movers = 0;
    for (uint32_t v = 0; v < m; ++v)
        if (D[v] > 0 && t.v[L.P[v]] == v && (T[v] == ALONE || t.v[T[v]] == v)) { labels[v] = T[v] == ALONE ? m + v : T[v]; ++movers; }
    leiden_smallest_member(L.P, labels, 2 * (size_t)m);
    return movers;
}

// One refinement round on R inside L.P; returns the movers.
inline uint64_t leiden_refine_round(const LeidenLevel& L, int64_t g, std::vector<uint32_t>& R, const std::vector<char>& well, const std::vector<int64_t>& SP)
{
    const uint32_t m = L.m, NONE = 0xFFFFFFFFu;
    std::vector<int64_t> SR(m, 0), ext(m, 0), D(m, -1);
    std::vector<uint32_t> members(m, 0), T(m, NONE);
    for (uint32_t v = 0; v < m; ++v) { SR[R[v]] += L.s[v]; members[R[v]]++; }
    for (size_t i = 0; i < L.key.size(); ++i) {
        const uint32_t a = (uint32_t)(L.key[i] >> 32), b = (uint32_t)L.key[i];
        if (L.P[a] == L.P[b] && R[a] != R[b]) { ext[R[a]] += L.q[i]; ext[R[b]] += L.q[i]; }
    }
    std::map<uint32_t, int64_t> W;
    for (uint32_t v = 0; v < m; ++v) {
        if (members[R[v]] != 1 || !well[v]) continue;
        W.clear();
        for (const auto& e : L.adj[v])
            if (L.P[e.first] == L.P[v] && R[e.first] != R[v]) W[R[e.first]] += e.second;
        for (const auto& c : W) {
            if (c.second <= 0 || ext[c.first] < g * SR[c.first] * (SP[L.P[v]] - SR[c.first])) continue;
            const int64_t d = c.second - g * L.s[v] * SR[c.first];
            if (d >= 0 && d > D[v]) { D[v] = d; T[v] = c.first; }
        }
    }
    LeidenTouch t(m);
    for (uint32_t v = 0; v < m; ++v)
        if (T[v] != NONE) { t.touch(R[v], D[v], v); t.touch(T[v], D[v], v); }
    std::vector<uint32_t> labels(R);
    uint64_t movers = 0;
    for (uint32_t v = 0; v < m; ++v)
        if (T[v] != NONE && t.v[R[v]] == v && t.v[T[v]] == v) { labels[v] = T[v]; ++movers; }
    leiden_smallest_member(R, labels, m);
    return movers;
}

// LZANI_CLUSTER_LEIDEN on the edges as they come: a sequential form of exactly the rounds of the statement.  rep_of[n] is
// written; info's counts, quality and resolution_q too (its device fields stay 0).  LZANI_ERR_DEVICE where a phase reaches
// its cap of rounds.
inline int cluster_leiden_host(uint32_t n, const lzani_cluster_edge* edges, uint64_t count, double resolution, int iterations, uint32_t* rep_of,
                               lzani_cluster_leiden_info* info, uint64_t cap_mul = CL_LEIDEN_CAP_MUL, uint64_t cap_add = CL_LEIDEN_CAP_ADD)
{
    if (!cluster_leiden_params_ok(resolution, iterations) || n > CL_LEIDEN_MAX_N) return LZANI_ERR_ARG;
    const int64_t g = cluster_leiden_g(resolution);
    typedef std::pair<uint64_t, int64_t> Rec;
    std::vector<Rec> recs(count);
    for (uint64_t i = 0; i < count; ++i) {
        const uint32_t lo = edges[i].a < edges[i].b ? edges[i].a : edges[i].b, hi = edges[i].a < edges[i].b ? edges[i].b : edges[i].a;
        recs[i] = Rec(((uint64_t)lo << 32) | hi, cluster_leiden_q(cluster_value(edges[i].w)));
    }
    std::sort(recs.begin(), recs.end());                                          // by pair, then by q: the first record has the smallest
    recs.erase(std::unique(recs.begin(), recs.end(), [](const Rec& x, const Rec& y) { return x.first == y.first; }), recs.end());
    lzani_cluster_leiden_info st{};
    st.resolution_q = (uint64_t)g; st.distinct_edges = recs.size(); st.duplicate_edges = count - recs.size();
    for (uint32_t v = 0; v < n; ++v) rep_of[v] = v;
    for (int it = 0; it < iterations; ++it) {
        st.iterations++;
        LeidenLevel L;
        L.m = n; L.s.assign(n, 1); L.P.assign(rep_of, rep_of + n);
        L.key.resize(recs.size()); L.q.resize(recs.size());
        for (size_t i = 0; i < recs.size(); ++i) { L.key[i] = recs[i].first; L.q[i] = recs[i].second; }
        L.link();
        std::vector<uint32_t> node_of(n);
        for (uint32_t v = 0; v < n; ++v) node_of[v] = v;
        uint64_t moved_in_iteration = 0;
        for (;;) {
            st.levels++;
            const uint32_t m = L.m;
            const uint64_t cap = cap_mul * m + cap_add;
            uint64_t moved = 0, merged = 0;
            for (uint64_t rounds = 0;; ) {
                if (rounds >= cap) return LZANI_ERR_DEVICE;
                ++rounds; st.move_rounds++;
                const uint64_t k = leiden_move_round(L, g);
                moved += k;
                if (!k) break;
            }
            st.moves += moved; moved_in_iteration += moved;
            bool single = true;
            for (uint32_t v = 0; v < m && single; ++v) single = L.P[v] == v;
            if (single) break;
            std::vector<int64_t> SP(m, 0);
            for (uint32_t v = 0; v < m; ++v) SP[L.P[v]] += L.s[v];
            std::vector<char> well(m);
            for (uint32_t v = 0; v < m; ++v) {
                int64_t w = 0;
                for (const auto& e : L.adj[v])
                    if (L.P[e.first] == L.P[v]) w += e.second;
                well[v] = w >= g * L.s[v] * (SP[L.P[v]] - L.s[v]);
            }
            std::vector<uint32_t> R(m);
            for (uint32_t v = 0; v < m; ++v) R[v] = v;
            for (uint64_t rounds = 0;; ) {
                if (rounds >= cap) return LZANI_ERR_DEVICE;
                ++rounds; st.refine_rounds++;
                const uint64_t k = leiden_refine_round(L, g, R, well, SP);
                merged += k;
                if (!k) break;
            }
            st.merges += merged;
            if (!moved && !merged) break;
            // aggregation: the R-communities in ascending order of their smallest member
            std::vector<uint32_t> index(m, 0);
            uint32_t m2 = 0;
            for (uint32_t v = 0; v < m; ++v)
                if (R[v] == v) index[v] = m2++;
            LeidenLevel N;
            N.m = m2; N.s.assign(m2, 0); N.P.resize(m2);
            for (uint32_t v = 0; v < m; ++v) N.s[index[R[v]]] += L.s[v];
            for (uint32_t v = 0; v < m; ++v)
                if (R[v] == v) N.P[index[v]] = index[L.P[v]];                      // (P's smallest member is the smallest of its R-community)
            std::map<uint64_t, int64_t> sum;
            for (size_t i = 0; i < L.key.size(); ++i) {
                const uint32_t x = index[R[(uint32_t)(L.key[i] >> 32)]], y = index[R[(uint32_t)L.key[i]]];
                if (x != y) sum[x < y ? ((uint64_t)x << 32) | y : ((uint64_t)y << 32) | x] += L.q[i];
            }
            for (const auto& e : sum) { N.key.push_back(e.first); N.q.push_back(e.second); }
            N.link();
            for (uint32_t v = 0; v < n; ++v) node_of[v] = index[R[node_of[v]]];
            L = std::move(N);
        }
        std::vector<uint32_t> labels(n);
        for (uint32_t v = 0; v < n; ++v) labels[v] = L.P[node_of[v]];
        std::vector<uint32_t> part(n);
        leiden_smallest_member(part, labels, n);
        for (uint32_t v = 0; v < n; ++v) rep_of[v] = part[v];
        if (!moved_in_iteration) break;
    }
    std::vector<int64_t> size(n, 0);
    for (uint32_t v = 0; v < n; ++v) size[rep_of[v]]++;
    int64_t quality = 0;
    for (const Rec& r : recs)
        if (rep_of[(uint32_t)(r.first >> 32)] == rep_of[(uint32_t)r.first]) quality += r.second;
    for (uint32_t v = 0; v < n; ++v) quality -= g * (size[v] * (size[v] - 1) / 2);
    st.quality = quality;
    if (info) *info = st;
    return LZANI_OK;
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
    } else if (algo == LZANI_CLUSTER_LEIDEN) {
        if (int rc = cluster_leiden_host(n, edges, count, CL_LEIDEN_RESOLUTION, CL_LEIDEN_ITERATIONS, rep_of, nullptr)) return rc;
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
