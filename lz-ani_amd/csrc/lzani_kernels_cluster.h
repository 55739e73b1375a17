// lzani_kernels_cluster.h -- device kernels of the cluster stage (lzani_cluster.h; include/lzani.h states the definitions,
// lzani_cluster_plan.h the weight).  Included by lzani_hip.hip only, behind lzani_kernels_outfilter.h; of
// lzani_kernels_prefilter.h it uses PF_THREADS (256-thread blocks), the scan k_pf_scan and the compaction pf_compact, of
// lzani_prefilter_defs.h pf_splitmix64, of lzani_block.h block_sum.
//   k_cl_add_kept    one thread per kept record: the weight, one 16-byte edge by one 16-byte vector store
//   k_cl_level       <false>, k_pf_scan, <true>: the edges of a cluster level -- the records of the store of which a line stays
//                    under the cut (cluster_cut_lines), in record order, by pf_compact; the count pass sums the lines in
//                    and out as well
//   k_cl_init        per node: parent = v, state = UNDECIDED, blocked = 0, best = 0, size = 0
//   k_cl_hook        SINGLE, one thread per edge: the two roots by following parent, the larger hooked under the smaller
//                    with atomicCAS(&parent[hi], hi, lo); on a lost CAS, look again.  parent[v] <= v at every moment: no
//                    cycle, and every retry follows a hook that some thread made
//   k_cl_roots       SINGLE, per node, behind the kernel boundary: rep_of[v] = root(v)
//   k_cl_greedy_edges / k_cl_greedy_nodes   one round of the greedy representatives (below)
//   k_cl_assign_init, k_cl_assign_best, k_cl_assign_min   rep_of of the nodes that are no representatives
//   k_cl_flags, k_cl_number   the numbering: flags rep_of[v] == v and cluster sizes; behind the scan cluster_of and the
//                    counts of singletons and of the largest cluster
//   k_cl_cover_*     greedy set cover: the keys of the distinct edges, and the passes of a round (behind the numbering)
//   k_cl_link_*      complete linkage: the cluster-pair table and the passes of a round
//   k_ld_*           Leiden (CPM): the node-community table and the passes of the rounds (at the end of this file)
// Words that other blocks write inside a launch (parent, state, blocked) are read and written with relaxed agent-scope
// atomics only: the L2 of an XCD is not coherent with the others for plain accesses inside a kernel.  No thread ever waits
// for a value that another block has yet to write; edge indexes are 64-bit throughout.
#pragma once
#include "lzani_cluster_plan.h"

namespace lzani {

enum : u32 { CL_UNDECIDED = 0, CL_REP = 1, CL_NONREP = 2 };
enum { CL_SINGLETONS = 0, CL_LARGEST = 1, CL_COUNTERS = 2 };
constexpr u32 CL_NONE = 0xFFFFFFFFu;

__device__ __forceinline__ u32 cl_load(const u32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cl_store(u32* p, u32 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// an edge as the passes read it: one 16-byte load; lo < hi
struct ClEdge { u32 lo, hi; u64 wbits; };
__device__ __forceinline__ ClEdge cl_edge(const lzani_cluster_edge* __restrict__ edges, u64 i)
{
    const uint4 v = reinterpret_cast<const uint4*>(edges)[i];
    return ClEdge{v.x, v.y, ((u64)v.w << 32) | v.z};
}

// rec: 9 words a kept pair (lzani_kept_pair); the edges from `base` on
__global__ void __launch_bounds__(PF_THREADS) k_cl_add_kept(const u32* __restrict__ rec, u64 count, const u32* __restrict__ len, int measure,
                                                            lzani_cluster_edge* __restrict__ edges, u64 base)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= count) return;
    const u32* __restrict__ r = rec + 9 * i;
    const u32 a = r[0], b = r[1];
    const lzani_result X{(int)r[2], (int)r[3], (int)r[4]}, Y{(int)r[5], (int)r[6], (int)r[7]};
    const double w = cluster_weight(measure, X, Y, r[8], len[a], len[b]);
    const u64 bits = (u64)__double_as_longlong(w);
    reinterpret_cast<uint4*>(edges)[base + i] = make_uint4(a, b, (u32)bits, (u32)(bits >> 32));
}

// A cluster level's edges, by pf_compact: a block of 256 threads takes 4,096 records, 16 a thread.  Per record 36 B and two lengths read (by either pass), per edge 16 B written by one vector store.
// The count pass counts the block's edges (blkcnt) and adds the set bits of `lines` and of cut_lines to counters[CL_LV_LINES_IN]
// and [CL_LV_LINES_OUT]: a block sum each and one atomic add per block.  No block waits for another.
enum { CL_LV_LINES_IN = 0, CL_LV_LINES_OUT = 1, CL_LV_COUNTERS = 2 };
template <bool WRITE>
struct ClLevelItem {
    const u32* __restrict__ rec;
    const u32* __restrict__ len;
    lzani_cluster_cut cut;
    int measure;
    lzani_cluster_edge* __restrict__ edges;
    u32* lines_in;                                               // this thread's sums (the count pass)
    u32* lines_out;
    uint4* edge;                                                 // this thread's edge between kept and put (the write pass)
    __device__ __forceinline__ bool kept(u64 i, u64&) const
    {
        const u32* __restrict__ r = rec + 9 * i;
        const u32 a = r[0], b = r[1], lines = r[8];
        const lzani_result X{(int)r[2], (int)r[3], (int)r[4]}, Y{(int)r[5], (int)r[6], (int)r[7]};
        const u32 la = len[a], lb = len[b];
        const u32 stay = cluster_cut_lines(cut, X, Y, lines, la, lb);
        if (!WRITE) { *lines_in += (u32)__popc(lines); *lines_out += (u32)__popc(stay); }
        else if (stay) {
            const u64 bits = (u64)__double_as_longlong(cluster_weight(measure, X, Y, stay, la, lb));
            *edge = make_uint4(a, b, (u32)bits, (u32)(bits >> 32));
        }
        return stay != 0;
    }
    __device__ __forceinline__ void put(u64 at, u64) const { reinterpret_cast<uint4*>(edges)[at] = *edge; }
};
template <bool WRITE>
__global__ void __launch_bounds__(PF_THREADS) k_cl_level(const u32* __restrict__ rec, u64 count, const u32* __restrict__ len, lzani_cluster_cut cut, int measure,
                                                         u32* __restrict__ blkcnt, const u64* __restrict__ blkoff, lzani_cluster_edge* __restrict__ edges,
                                                         unsigned long long* __restrict__ counters)
{
    __shared__ u32 s_in, s_out;
    if (!WRITE && threadIdx.x == 0) { s_in = 0; s_out = 0; }     // (the count pass of pf_compact begins with a barrier)
    u32 lines_in = 0, lines_out = 0;
    uint4 edge = make_uint4(0, 0, 0, 0);
    pf_compact<WRITE>(count, blkcnt, blkoff, ClLevelItem<WRITE>{rec, len, cut, measure, edges, &lines_in, &lines_out, &edge});
    if (!WRITE) {
        block_sum(lines_in, &s_in);
        block_sum(lines_out, &s_out);
        if (threadIdx.x == 0) {
            if (s_in) atomicAdd(&counters[CL_LV_LINES_IN], (unsigned long long)s_in);
            if (s_out) atomicAdd(&counters[CL_LV_LINES_OUT], (unsigned long long)s_out);
        }
    }
}

__global__ void __launch_bounds__(PF_THREADS) k_cl_init(u32 n, u32* __restrict__ parent, u32* __restrict__ state, u32* __restrict__ blocked,
                                                        unsigned long long* __restrict__ best, u32* __restrict__ size)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v >= n) return;
    parent[v] = v; state[v] = CL_UNDECIDED; blocked[v] = 0; best[v] = 0; size[v] = 0;
}

// The root of v's tree, halving the path on the way: parent[x] is replaced by an ancestor of x only, with an atomic store
// (a node that has a parent below it is never a root again, so the store cannot undo a hook).
__device__ __forceinline__ u32 cl_root(u32* parent, u32 v)
{
    for (;;) {
        const u32 p = cl_load(&parent[v]);
        if (p == v) return v;
        const u32 g = cl_load(&parent[p]);
        if (g == p) return p;
        cl_store(&parent[v], g);
        v = g;
    }
}

__global__ void __launch_bounds__(PF_THREADS) k_cl_hook(const lzani_cluster_edge* __restrict__ edges, u64 count, u32* parent)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= count) return;
    const ClEdge e = cl_edge(edges, i);
    u32 a = cl_root(parent, e.lo), b = cl_root(parent, e.hi);
    while (a != b) {
        const u32 lo = a < b ? a : b, hi = a < b ? b : a;
        const u32 old = atomicCAS(&parent[hi], hi, lo);          // (device scope)
        if (old == hi) break;
        a = cl_root(parent, old);                                // hi has a parent now: look again from there
        b = cl_root(parent, lo);
    }
}

__global__ void __launch_bounds__(PF_THREADS) k_cl_roots(u32 n, const u32* __restrict__ parent, u32* __restrict__ rep_of)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v >= n) return;
    u32 x = v;
    for (u32 p = parent[x]; p != x; p = parent[x]) x = p;
    rep_of[v] = x;
}

// One round of the greedy representatives.  Edge pass, a < b: state[a] == REP stores state[b] = NONREP; state[a] ==
// UNDECIDED stores blocked[b] = 1.  Node pass: an UNDECIDED node with blocked == 0 becomes REP; blocked is cleared; the
// nodes still undecided are counted.  Both stored values are idempotent, REP and NONREP are final, and a stale UNDECIDED
// read inside a round only delays a decision: the fixed point is the set of the definition whatever the schedule, and the
// lowest undecided node is decided in every round.
__global__ void __launch_bounds__(PF_THREADS) k_cl_greedy_edges(const lzani_cluster_edge* __restrict__ edges, u64 count, u32* state, u32* blocked)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= count) return;
    const ClEdge e = cl_edge(edges, i);
    if (cl_load(&state[e.hi]) != CL_UNDECIDED) return;           // (final: nothing left to say about it)
    const u32 s = cl_load(&state[e.lo]);
    if (s == CL_REP) cl_store(&state[e.hi], CL_NONREP);
    else if (s == CL_UNDECIDED) cl_store(&blocked[e.hi], 1u);
}

__global__ void __launch_bounds__(PF_THREADS) k_cl_greedy_nodes(u32 n, u32* __restrict__ state, u32* __restrict__ blocked, u32* __restrict__ undecided)
{
    __shared__ u32 s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    u32 mine = 0;
    if (v < n && state[v] == CL_UNDECIDED) {
        if (blocked[v]) { blocked[v] = 0; mine = 1; }
        else state[v] = CL_REP;
    }
    block_sum(mine, &s_cnt);
    if (threadIdx.x == 0 && s_cnt) atomicAdd(undecided, s_cnt);
}

__global__ void __launch_bounds__(PF_THREADS) k_cl_assign_init(u32 n, const u32* __restrict__ state, u32* __restrict__ rep_of)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v < n) rep_of[v] = state[v] == CL_REP ? v : CL_NONE;
}
// BEST, first pass: the largest weight's bits over the representative neighbours below a node
__global__ void __launch_bounds__(PF_THREADS) k_cl_assign_best(const lzani_cluster_edge* __restrict__ edges, u64 count, const u32* __restrict__ state,
                                                               unsigned long long* __restrict__ best)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= count) return;
    const ClEdge e = cl_edge(edges, i);
    if (state[e.lo] == CL_REP && state[e.hi] == CL_NONREP) atomicMax(&best[e.hi], (unsigned long long)e.wbits);
}
// FIRST (best null): the smallest representative neighbour; BEST, second pass: among the edges of the largest weight
__global__ void __launch_bounds__(PF_THREADS) k_cl_assign_min(const lzani_cluster_edge* __restrict__ edges, u64 count, const u32* __restrict__ state,
                                                              const unsigned long long* __restrict__ best, u32* __restrict__ rep_of)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= count) return;
    const ClEdge e = cl_edge(edges, i);
    if (state[e.lo] != CL_REP || state[e.hi] != CL_NONREP) return;
    if (best && best[e.hi] != e.wbits) return;
    atomicMin(&rep_of[e.hi], e.lo);
}

__global__ void __launch_bounds__(PF_THREADS) k_cl_flags(u32 n, const u32* __restrict__ rep_of, u32* __restrict__ flag, u32* __restrict__ size)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v >= n) return;
    const u32 r = rep_of[v];
    flag[v] = r == v ? 1u : 0u;
    if (r < n) atomicAdd(&size[r], 1u);                          // (every node has a representative; a defect must not write astray)
}
// below[v] = the representatives with an id below v (the scan of the flags)
__global__ void __launch_bounds__(PF_THREADS) k_cl_number(u32 n, const u32* __restrict__ rep_of, const u64* __restrict__ below, const u32* __restrict__ size,
                                                          u32* __restrict__ cluster_of, u32* __restrict__ counters)
{
    __shared__ u32 s_one, s_max;
    if (threadIdx.x == 0) { s_one = 0; s_max = 0; }
    __syncthreads();
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    u32 one = 0, sz = 0;
    if (v < n) {
        const u32 r = rep_of[v];
        cluster_of[v] = r < n ? (u32)below[r] : CL_NONE;
        sz = size[v];
        one = sz == 1 ? 1u : 0u;
    }
    block_sum(one, &s_one);
    for (int d = 32; d >= 1; d >>= 1) { const u32 o = __shfl_xor(sz, d); sz = sz > o ? sz : o; }
    if ((threadIdx.x & 63) == 0 && sz) atomicMax(&s_max, sz);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_one) atomicAdd(&counters[CL_SINGLETONS], s_one);
        if (s_max) atomicMax(&counters[CL_LARGEST], s_max);
    }
}

// ---- LZANI_CLUSTER_SET_COVER ----------------------------------------------------------------------------------------
// The passes run over the distinct edges: keys lo << 32 | hi (k_cl_cover_keys), sorted and made unique on the host side's
// order (lzani_sort_keys, k_pf_uniq).  A node is unassigned while rep_of[v] == CL_NONE; rep_of is written by the decide
// pass only, so between two decide passes it is the round's snapshot.  A round, with key(v) = cluster_cover_key(c(v), v)
// for an unassigned node and 0 for an assigned one:
//   k_cl_cover_count   per edge of two unassigned ends: cnt += 1 at both (atomicAdd)
//   k_cl_cover_key     per node: key = m1 = its key from cnt, m2 = 0, cnt = 0 for the next round
//   k_cl_cover_max     key -> m1, per edge of two unassigned ends: the larger key into m1 of the other end (one atomicMax;
//                      the end with the larger key has it in its own m1 already).  Behind it m1[v] = the largest key of v
//                      and its unassigned neighbours
//   k_cl_cover_max     m1 -> m2, per such edge: the larger m1 into m2 of the other end, nothing where they are equal.
//                      Behind it max(m1[w], m2[w]) = the largest key within two hops of w
//   k_cl_cover_decide  per unassigned node v, with w = the node of the key m1[v] (v itself or a neighbour): w is selected
//                      iff its two-hop maximum is its own key, and v is assigned in this round iff w is selected, with
//                      rep_of[v] = w.  For: a selected v has w == v; a v with a selected neighbour u has all of its
//                      neighbourhood within two hops of u, so m1[v] is u's key; and a selected w is v or a neighbour of
//                      v.  So the selected node and the nodes it covers take their representative in one node pass, one
//                      plain store each, and the nodes left unassigned are summed into the round's counter
// Every pass reads only words that no thread writes in the same launch, or goes through the atomics named; everything else
// crosses a kernel boundary.  A round behind the one that left no node unassigned finds every key 0 and changes nothing.
__global__ void __launch_bounds__(PF_THREADS) k_cl_cover_keys(const lzani_cluster_edge* __restrict__ edges, u64 count, unsigned long long* __restrict__ keys)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= count) return;
    const ClEdge e = cl_edge(edges, i);
    keys[i] = ((u64)e.lo << 32) | e.hi;
}

__global__ void __launch_bounds__(PF_THREADS) k_cl_cover_init(u32 n, u32* __restrict__ rep_of, u32* __restrict__ cnt, u32* __restrict__ size)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v >= n) return;
    rep_of[v] = CL_NONE; cnt[v] = 0; size[v] = 0;
}

__global__ void __launch_bounds__(PF_THREADS) k_cl_cover_count(const unsigned long long* __restrict__ pairs, u64 count, u32 n, const u32* __restrict__ rep_of,
                                                               u32* __restrict__ cnt)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= count) return;
    const u64 p = pairs[i];
    const u32 lo = (u32)(p >> 32), hi = (u32)p;
    if (lo >= n || hi >= n) return;                              // (ids are checked where edges come in; a defect must not write astray)
    if (rep_of[lo] != CL_NONE || rep_of[hi] != CL_NONE) return;
    atomicAdd(&cnt[lo], 1u);
    atomicAdd(&cnt[hi], 1u);
}

__global__ void __launch_bounds__(PF_THREADS) k_cl_cover_key(u32 n, const u32* __restrict__ rep_of, u32* __restrict__ cnt, unsigned long long* __restrict__ key,
                                                             unsigned long long* __restrict__ m1, unsigned long long* __restrict__ m2)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v >= n) return;
    const u64 k = rep_of[v] == CL_NONE ? cluster_cover_key(cnt[v], v) : 0;
    key[v] = k; m1[v] = k; m2[v] = 0; cnt[v] = 0;
}

// from[]: key for the first hop (into = m1), m1 for the second (into = m2); 0 marks an assigned node in both
__global__ void __launch_bounds__(PF_THREADS) k_cl_cover_max(const unsigned long long* __restrict__ pairs, u64 count, u32 n,
                                                             const unsigned long long* __restrict__ from, unsigned long long* __restrict__ into)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= count) return;
    const u64 p = pairs[i];
    const u32 lo = (u32)(p >> 32), hi = (u32)p;
    if (lo >= n || hi >= n) return;
    const u64 a = from[lo], b = from[hi];
    if (!a || !b || a == b) return;
    if (a > b) atomicMax(&into[hi], (unsigned long long)a);
    else atomicMax(&into[lo], (unsigned long long)b);
}

__global__ void __launch_bounds__(PF_THREADS) k_cl_cover_decide(u32 n, const unsigned long long* __restrict__ m1, const unsigned long long* __restrict__ m2,
                                                                u32* __restrict__ rep_of, u32* __restrict__ unassigned)
{
    __shared__ u32 s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    u32 mine = 0;
    const u64 m = v < n ? m1[v] : 0;
    if (m) {                                                     // v is unassigned
        const u32 w = cluster_cover_node(m);
        const u64 a = w < n ? m1[w] : 0, b = w < n ? m2[w] : 0;
        if (w < n && (a > b ? a : b) == m) rep_of[v] = w;
        else mine = 1;
    }
    block_sum(mine, &s_cnt);
    if (threadIdx.x == 0 && s_cnt) atomicAdd(unassigned, s_cnt);
}

// ---- LZANI_CLUSTER_COMPLETE -----------------------------------------------------------------------------------------
// Rounds of reciprocal best links (include/lzani.h has the statement and the argument).  A cluster is known by its id, its
// smallest member; label[c] == c while c lives, else the cluster that took it in the round it went; csize[c] is a live
// cluster's size.  The entry list L (lkey, lcnt, lw: ca << 32 | cb with ca < cb, count, smallest weight bits) holds the
// links of the last round's table; the first round reads the edge records in its place, count 1 each.  The table: S slots,
// a power of two >= 2 * entries, of tkey (CL_LINK_FREE, all ones, marks a free slot: no key, as ca < cb <= 2^32 - 2), tcnt
// and tw.  A round:
//   (memsets)          tkey = tw = all ones, tcnt = 0 over the round's S; ctl = 0
//   k_cl_link_insert   per entry: both ends through label[], entries inside one cluster skipped; the slot of the key from
//                      its home pf_splitmix64(key) & (S - 1), the next slot on a collision, wrapping at S: atomicCAS on
//                      the key, atomicAdd on the count (of the edge records, which make the edges distinct here, only the
//                      one that claims the slot adds), 64-bit atomicMin on the weight bits.  At most S probe steps: a
//                      sequence that runs out, or an id >= n, raises ctl[CL_LINK_ERR] and the run ends in
//                      LZANI_ERR_DEVICE.  No step waits for another thread
//   k_cl_link_clear    per cluster: bestw = 0, bestid = CL_NONE
//   k_cl_link_bestw    per slot that is a link -- count == (u64)csize[ca] * csize[cb] --: atomicMax of the weight bits into
//                      bestw of both ends
//   k_cl_link_bestid   per link whose weight is an end's bestw: atomicMin of the other id into bestid of that end.  (A
//                      cluster without a link keeps CL_NONE; one whose best weight is 0 has links of weight 0 to show it)
//   k_cl_link_compact  <false>, k_pf_scan, <true>: the links into L, in the table's order, by pf_compact; before the merge,
//                      as the sizes say what a link is
//   k_cl_link_merge    per cluster a with b = bestid[a]: bestid[b] == a and a < b: label[b] = a, csize[a] += csize[b], one
//                      merge counted.  a's words are written by a's thread alone, b's label too, and csize[b] is read
//                      by it alone: b's own thread merges nothing, as its partner a lies below it
//   k_cl_link_relabel  per node: rep_of[v] = label[rep_of[v]]: one hop, as only pairs merge in a round
// Within a launch the table's words and bestw / bestid are touched through the atomics named and through nothing else;
// label, csize, rep_of and L are read, or written by one thread a word, and cross a kernel boundary before another thread
// reads them.  Slot and entry indexes are 64-bit.
constexpr u64 CL_LINK_FREE = ~0ULL;
enum { CL_LINK_ERR = 0, CL_LINK_MERGES = 1, CL_LINK_CTL = 2 };

struct ClLinkTable { unsigned long long* __restrict__ key; unsigned long long* __restrict__ cnt; unsigned long long* __restrict__ w; u64 S; };

__global__ void __launch_bounds__(PF_THREADS) k_cl_link_init(u32 n, u32* __restrict__ label, u32* __restrict__ csize, u32* __restrict__ rep_of, u32* __restrict__ size)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v >= n) return;
    label[v] = v; csize[v] = 1; rep_of[v] = v; size[v] = 0;
}

// edges != null: the first round, entry i is edge record i; else entry i of L
__global__ void __launch_bounds__(PF_THREADS) k_cl_link_insert(const lzani_cluster_edge* __restrict__ edges, const unsigned long long* __restrict__ lkey,
                                                               const unsigned long long* __restrict__ lcnt, const unsigned long long* __restrict__ lw, u64 count,
                                                               u32 n, const u32* __restrict__ label, ClLinkTable t, u32* __restrict__ ctl)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= count) return;
    u32 a, b;
    u64 c, w;
    if (edges) { const ClEdge e = cl_edge(edges, i); a = e.lo; b = e.hi; c = 1; w = e.wbits; }
    else { const u64 k = lkey[i]; a = (u32)(k >> 32); b = (u32)k; c = lcnt[i]; w = lw[i]; }
    if (a >= n || b >= n) { atomicOr(&ctl[CL_LINK_ERR], 1u); return; }   // (ids are checked where edges come in; a defect must not read astray)
    a = label[a]; b = label[b];
    if (a == b) return;
    if (a >= n || b >= n) { atomicOr(&ctl[CL_LINK_ERR], 1u); return; }
    const u64 key = a < b ? ((u64)a << 32) | b : ((u64)b << 32) | a, mask = t.S - 1;
    u64 slot = pf_splitmix64(key) & mask;
    bool mine = false;
    for (u64 step = 0; step < t.S; ++step, slot = (slot + 1) & mask) {
        u64 cur = __hip_atomic_load(&t.key[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == CL_LINK_FREE) {
            cur = atomicCAS(&t.key[slot], (unsigned long long)CL_LINK_FREE, (unsigned long long)key);
            if (cur == CL_LINK_FREE) { cur = key; mine = true; }          // the slot is this thread's
        }
        if (cur == key) {
            if (!edges || mine) atomicAdd(&t.cnt[slot], (unsigned long long)c);  // (an edge record given again is the same edge)
            atomicMin(&t.w[slot], (unsigned long long)w);
            return;
        }
    }
    atomicOr(&ctl[CL_LINK_ERR], 1u);
}

__global__ void __launch_bounds__(PF_THREADS) k_cl_link_clear(u32 n, unsigned long long* __restrict__ bestw, u32* __restrict__ bestid)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v >= n) return;
    bestw[v] = 0; bestid[v] = CL_NONE;
}

// Whether slot i holds a link, and then its ends and weight bits.  Read behind the insert's kernel boundary.
__device__ __forceinline__ bool cl_link_at(const ClLinkTable& t, u64 i, u32 n, const u32* __restrict__ csize, u32& a, u32& b, u64& w)
{
    const u64 key = t.key[i];
    if (key == CL_LINK_FREE) return false;
    a = (u32)(key >> 32); b = (u32)key;
    if (a >= n || b >= n) return false;
    w = t.w[i];
    return t.cnt[i] == (u64)csize[a] * (u64)csize[b];
}

__global__ void __launch_bounds__(PF_THREADS) k_cl_link_bestw(ClLinkTable t, u32 n, const u32* __restrict__ csize, unsigned long long* __restrict__ bestw)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    u32 a, b;
    u64 w;
    if (i >= t.S || !cl_link_at(t, i, n, csize, a, b, w)) return;
    atomicMax(&bestw[a], (unsigned long long)w);
    atomicMax(&bestw[b], (unsigned long long)w);
}

__global__ void __launch_bounds__(PF_THREADS) k_cl_link_bestid(ClLinkTable t, u32 n, const u32* __restrict__ csize, const unsigned long long* __restrict__ bestw,
                                                               u32* __restrict__ bestid)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    u32 a, b;
    u64 w;
    if (i >= t.S || !cl_link_at(t, i, n, csize, a, b, w)) return;
    if (bestw[a] == w) atomicMin(&bestid[a], b);
    if (bestw[b] == w) atomicMin(&bestid[b], a);
}

// The links of the table, counted or written by pf_compact: slot i goes to entry `at` of L.
struct ClLinkItem {
    ClLinkTable t;
    u32 n;
    const u32* __restrict__ csize;
    unsigned long long* __restrict__ lkey;
    unsigned long long* __restrict__ lcnt;
    unsigned long long* __restrict__ lw;
    __device__ __forceinline__ bool kept(u64 i, u64& slot) const
    {
        u32 a, b;
        u64 w;
        slot = i;
        return cl_link_at(t, i, n, csize, a, b, w);
    }
    __device__ __forceinline__ void put(u64 at, u64 slot) const { lkey[at] = t.key[slot]; lcnt[at] = t.cnt[slot]; lw[at] = t.w[slot]; }
};
template <bool WRITE>
__global__ void __launch_bounds__(PF_THREADS) k_cl_link_compact(ClLinkTable t, u32 n, const u32* __restrict__ csize, u32* __restrict__ blkcnt,
                                                                const u64* __restrict__ blkoff, unsigned long long* __restrict__ lkey,
                                                                unsigned long long* __restrict__ lcnt, unsigned long long* __restrict__ lw)
{
    pf_compact<WRITE>(t.S, blkcnt, blkoff, ClLinkItem{t, n, csize, lkey, lcnt, lw});
}

__global__ void __launch_bounds__(PF_THREADS) k_cl_link_merge(u32 n, const u32* __restrict__ bestid, u32* label, u32* csize, u32* __restrict__ ctl)
{
    __shared__ u32 s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const u32 a = blockIdx.x * PF_THREADS + threadIdx.x;
    u32 mine = 0;
    if (a < n) {
        const u32 b = bestid[a];
        if (b < n && a < b && bestid[b] == a) { label[b] = a; csize[a] += csize[b]; mine = 1; }
    }
    block_sum(mine, &s_cnt);
    if (threadIdx.x == 0 && s_cnt) atomicAdd(&ctl[CL_LINK_MERGES], s_cnt);
}

__global__ void __launch_bounds__(PF_THREADS) k_cl_link_relabel(u32 n, const u32* __restrict__ label, u32* __restrict__ rep_of)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v >= n) return;
    const u32 r = rep_of[v];
    if (r < n) rep_of[v] = label[r];
}

// ---- LZANI_CLUSTER_LEIDEN -------------------------------------------------------------------------------------------
// Rounds of the statement in include/lzani.h, in signed 64-bit integers (q and g in units of 2^-20).  A level: m nodes with
// sizes s, the entry list (lkey = a << 32 | b with a < b, lq), the partition P with SP[c] = the size of community c (a
// community's id is its smallest member).  The table: S slots, a power of two >= 2 * the insertions, of tkey (CL_LD_FREE,
// all ones, marks a free slot: no key, as every id is below 2^21) and tval; home pf_splitmix64(key) & (S - 1), the next
// slot on a collision, wrapping at S, at most S probe steps: a sequence that runs out, or an id out of range, raises
// ctl[CL_LD_ERR] and the run ends in LZANI_ERR_DEVICE.  No step waits for another thread.
//   k_ld_dedup         once per run, per edge record: key lo << 32 | hi, 64-bit atomicMin of q into tval (all ones before)
//   k_ld_compact       <false>, k_pf_scan, <true>: the occupied slots into an entry list, in the table's order (pf_compact)
// A moving round (memsets: tkey all ones, tval 0 over the round's S; ownw 0):
//   k_ld_move_insert   per entry, for both ends: tval += q at the key node << 32 | community of the other end (atomicCAS on
//                      the key, 64-bit atomicAdd on the sum)
//   k_ld_move_stay     per slot of a node's own community: ownw[v] = W(v, own), one plain store by the one such slot
//   k_ld_move_node     per node: valown = val(v, own); bestd = the D of alone where that is an option and above 0, else 0;
//                      bestid = none; and, v read as a community, cd = 0, cv = none
//   k_ld_move_bestd    per slot of another community with D = val - valown > 0: atomicMax of D into bestd[v]
//   k_ld_move_bestid   per such slot with D == bestd[v]: atomicMin of the community into bestid[v].  (bestd > 0 and bestid
//                      none: alone won; a community that ties with alone wins, as alone comes last)
//   k_ld_cand_max      per candidate (bestd > 0): atomicMax of D into cd of its own community and of its target
//   k_ld_cand_min      per candidate: atomicMin of v into cv of those of the two where cd == D
//   k_ld_decide        per node, plain stores by its own thread: v moves iff cv names it in every community it touches;
//                      newlab[v] = the target (m + v for alone: no community has that label), else its own; the labels'
//                      smallest members cleared; the movers summed into the round's counter
//   k_ld_minm, k_ld_newid, k_ld_sizes   relabel: atomicMin of the smallest member per label; part[v] = that member, the
//                      sizes cleared; the sizes (and member counts) summed, the communities counted
// A refinement round inside P on R (SR, cntr: sizes and member counts of the R-communities; well: the phase's
// well-connected nodes, from k_ld_wp and k_ld_well) has the same skeleton: k_ld_refine_insert (entries inside one
// P-community between two R-communities; also ext[R] += q at both ends), k_ld_refine_node, k_ld_refine_bestd / _bestid (D + 1,
// so that D = 0 counts), then k_ld_cand_max .. k_ld_sizes on R.  Aggregation: k_ld_agg_flags, k_pf_scan, k_ld_agg_nodes,
// k_ld_agg_nodeof, k_ld_agg_insert (the contracted key, q summed), k_ld_compact.
// Within a launch the table's words, bestd / bestid, cd / cv, ext, the smallest members, sizes and counts are touched through
// the atomics named and through nothing else; every other word is read, or written by one thread, and crosses a kernel
// boundary before another thread reads it.  Slot and entry indexes are 64-bit.
typedef long long i64;
constexpr u64 CL_LD_FREE = ~0ULL;
enum { CL_LD_BATCH = 4 };                                // rounds launched between two reads of the control words
enum { CL_LD_ERR = 0, CL_LD_MOVERS = 1, CL_LD_COMMS = 1 + CL_LD_BATCH, CL_LD_CTL = 1 + 2 * CL_LD_BATCH };

struct ClLdTable { unsigned long long* key; unsigned long long* val; u64 S; };

// The slot of `key`, claimed where it is new; t.S where the probe sequence runs out.
__device__ __forceinline__ u64 cl_ld_slot(const ClLdTable& t, u64 key)
{
    const u64 mask = t.S - 1;
    u64 slot = pf_splitmix64(key) & mask;
    for (u64 step = 0; step < t.S; ++step, slot = (slot + 1) & mask) {
        u64 cur = __hip_atomic_load(&t.key[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == CL_LD_FREE) {
            cur = atomicCAS(&t.key[slot], (unsigned long long)CL_LD_FREE, (unsigned long long)key);
            if (cur == CL_LD_FREE) cur = key;
        }
        if (cur == key) return slot;
    }
    return t.S;
}
__device__ __forceinline__ void cl_ld_add(const ClLdTable& t, u64 key, i64 q, u32* __restrict__ ctl)
{
    const u64 slot = cl_ld_slot(t, key);
    if (slot >= t.S) { atomicOr(&ctl[CL_LD_ERR], 1u); return; }
    atomicAdd(&t.val[slot], (unsigned long long)q);
}
// the sum of x over the wave, in every lane
__device__ __forceinline__ i64 cl_ld_wave_sum(i64 x)
{
    for (int d = 32; d >= 1; d >>= 1) {
        const u32 lo = __shfl_xor((u32)(u64)x, d), hi = __shfl_xor((u32)((u64)x >> 32), d);
        x += (i64)(((u64)hi << 32) | lo);
    }
    return x;
}

__global__ void __launch_bounds__(PF_THREADS) k_ld_init(u32 n, u32* __restrict__ rep_of, u32* __restrict__ size)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v >= n) return;
    rep_of[v] = v; size[v] = 0;
}

__global__ void __launch_bounds__(PF_THREADS) k_ld_dedup(const lzani_cluster_edge* __restrict__ edges, u64 count, u32 n, ClLdTable t, u32* __restrict__ ctl)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= count) return;
    const ClEdge e = cl_edge(edges, i);
    if (e.lo >= e.hi || e.hi >= n) { atomicOr(&ctl[CL_LD_ERR], 1u); return; }   // (ids are checked where edges come in; a defect must not write astray)
    const u64 slot = cl_ld_slot(t, ((u64)e.lo << 32) | e.hi);
    if (slot >= t.S) { atomicOr(&ctl[CL_LD_ERR], 1u); return; }
    atomicMin(&t.val[slot], (unsigned long long)cluster_leiden_q(__longlong_as_double((long long)e.wbits)));
}

struct ClLdItem {
    ClLdTable t;
    unsigned long long* __restrict__ lkey;
    i64* __restrict__ lq;
    __device__ __forceinline__ bool kept(u64 i, u64& slot) const { slot = i; return t.key[i] != CL_LD_FREE; }
    __device__ __forceinline__ void put(u64 at, u64 slot) const { lkey[at] = t.key[slot]; lq[at] = (i64)t.val[slot]; }
};
template <bool WRITE>
__global__ void __launch_bounds__(PF_THREADS) k_ld_compact(ClLdTable t, u32* __restrict__ blkcnt, const u64* __restrict__ blkoff,
                                                           unsigned long long* __restrict__ lkey, i64* __restrict__ lq)
{
    pf_compact<WRITE>(t.S, blkcnt, blkoff, ClLdItem{t, lkey, lq});
}

// The start of an iteration: the original graph with the last result as P.
__global__ void __launch_bounds__(PF_THREADS) k_ld_level0(u32 n, const u32* __restrict__ rep_of, u32* __restrict__ s, u32* __restrict__ P, u32* __restrict__ node_of)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v >= n) return;
    s[v] = 1; P[v] = rep_of[v]; node_of[v] = v;
}

// S[part[v]] += s[v] (s null: 1), cnt[part[v]] += 1 (cnt may be null); the communities (part[v] == v) into *comms (may be null)
__global__ void __launch_bounds__(PF_THREADS) k_ld_sizes(u32 m, const u32* __restrict__ s, const u32* __restrict__ part, u32* __restrict__ S, u32* __restrict__ cnt,
                                                         u32* __restrict__ comms)
{
    __shared__ u32 s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    u32 mine = 0;
    if (v < m) {
        const u32 c = part[v];
        if (c < m) {
            atomicAdd(&S[c], s ? s[v] : 1u);
            if (cnt) atomicAdd(&cnt[c], 1u);
        }
        mine = c == v ? 1u : 0u;
    }
    block_sum(mine, &s_cnt);
    if (comms && threadIdx.x == 0 && s_cnt) atomicAdd(comms, s_cnt);
}

__global__ void __launch_bounds__(PF_THREADS) k_ld_move_insert(const unsigned long long* __restrict__ lkey, const i64* __restrict__ lq, u64 count, u32 m,
                                                               const u32* __restrict__ P, ClLdTable t, u32* __restrict__ ctl)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= count) return;
    const u64 k = lkey[i];
    const u32 a = (u32)(k >> 32), b = (u32)k;
    if (a >= m || b >= m) { atomicOr(&ctl[CL_LD_ERR], 1u); return; }
    const i64 q = lq[i];
    cl_ld_add(t, ((u64)a << 32) | P[b], q, ctl);
    cl_ld_add(t, ((u64)b << 32) | P[a], q, ctl);
}

__global__ void __launch_bounds__(PF_THREADS) k_ld_move_stay(ClLdTable t, u32 m, const u32* __restrict__ P, i64* __restrict__ ownw)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= t.S) return;
    const u64 key = t.key[i];
    if (key == CL_LD_FREE) return;
    const u32 v = (u32)(key >> 32);
    if (v < m && P[v] == (u32)key) ownw[v] = (i64)t.val[i];
}

__global__ void __launch_bounds__(PF_THREADS) k_ld_move_node(u32 m, i64 g, const u32* __restrict__ s, const u32* __restrict__ P, const u32* __restrict__ SP,
                                                             const i64* __restrict__ ownw, i64* __restrict__ valown, unsigned long long* __restrict__ bestd,
                                                             u32* __restrict__ bestid, unsigned long long* __restrict__ cd, u32* __restrict__ cv)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v >= m) return;
    const u32 own = P[v];
    const i64 sv = s[v], So = own < m ? SP[own] : sv;
    const i64 vo = ownw[v] - g * sv * (So - sv);
    valown[v] = vo;
    bestd[v] = (So != sv && vo < 0) ? (unsigned long long)(-vo) : 0ULL;       // alone: val 0, only for a node that is not alone
    bestid[v] = CL_NONE;
    cd[v] = 0; cv[v] = CL_NONE;
}

// Whether slot i is an option of its node in another community, and then the node, the community and D.
__device__ __forceinline__ bool cl_ld_move_at(const ClLdTable& t, u64 i, u32 m, i64 g, const u32* __restrict__ s, const u32* __restrict__ P,
                                              const u32* __restrict__ SP, const i64* __restrict__ valown, u32& v, u32& c, i64& D)
{
    const u64 key = t.key[i];
    if (key == CL_LD_FREE) return false;
    v = (u32)(key >> 32); c = (u32)key;
    if (v >= m || c >= m || P[v] == c) return false;
    D = (i64)t.val[i] - g * (i64)s[v] * (i64)SP[c] - valown[v];
    return D > 0;
}

__global__ void __launch_bounds__(PF_THREADS) k_ld_move_bestd(ClLdTable t, u32 m, i64 g, const u32* __restrict__ s, const u32* __restrict__ P,
                                                              const u32* __restrict__ SP, const i64* __restrict__ valown, unsigned long long* __restrict__ bestd)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    u32 v, c;
    i64 D;
    if (i >= t.S || !cl_ld_move_at(t, i, m, g, s, P, SP, valown, v, c, D)) return;
    atomicMax(&bestd[v], (unsigned long long)D);
}

__global__ void __launch_bounds__(PF_THREADS) k_ld_move_bestid(ClLdTable t, u32 m, i64 g, const u32* __restrict__ s, const u32* __restrict__ P,
                                                               const u32* __restrict__ SP, const i64* __restrict__ valown,
                                                               const unsigned long long* __restrict__ bestd, u32* __restrict__ bestid)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    u32 v, c;
    i64 D;
    if (i >= t.S || !cl_ld_move_at(t, i, m, g, s, P, SP, valown, v, c, D)) return;
    if (bestd[v] == (unsigned long long)D) atomicMin(&bestid[v], c);
}

// part: P of a moving round, R of a refinement round.  A candidate has bestd > 0; its target is bestid (none: alone).
__global__ void __launch_bounds__(PF_THREADS) k_ld_cand_max(u32 m, const u32* __restrict__ part, const unsigned long long* __restrict__ bestd,
                                                            const u32* __restrict__ bestid, unsigned long long* __restrict__ cd)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v >= m) return;
    const u64 D = bestd[v];
    if (!D) return;
    const u32 own = part[v], to = bestid[v];
    if (own < m) atomicMax(&cd[own], (unsigned long long)D);
    if (to < m) atomicMax(&cd[to], (unsigned long long)D);
}

__global__ void __launch_bounds__(PF_THREADS) k_ld_cand_min(u32 m, const u32* __restrict__ part, const unsigned long long* __restrict__ bestd,
                                                            const u32* __restrict__ bestid, const unsigned long long* __restrict__ cd, u32* __restrict__ cv)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v >= m) return;
    const u64 D = bestd[v];
    if (!D) return;
    const u32 own = part[v], to = bestid[v];
    if (own < m && cd[own] == D) atomicMin(&cv[own], v);
    if (to < m && cd[to] == D) atomicMin(&cv[to], v);
}

// minm has 2 * m words: the labels of the communities, and m + v for a node that goes alone
__global__ void __launch_bounds__(PF_THREADS) k_ld_decide(u32 m, const u32* __restrict__ part, const unsigned long long* __restrict__ bestd,
                                                          const u32* __restrict__ bestid, const u32* __restrict__ cv, u32* __restrict__ newlab,
                                                          u32* __restrict__ minm, u32* __restrict__ movers)
{
    __shared__ u32 s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    u32 mine = 0;
    if (v < m) {
        const u32 own = part[v], to = bestid[v];
        u32 lab = own;
        if (bestd[v] && own < m && cv[own] == v && (to == CL_NONE || (to < m && cv[to] == v))) { lab = to == CL_NONE ? m + v : to; mine = 1; }
        newlab[v] = lab;
        minm[v] = CL_NONE; minm[m + v] = CL_NONE;
    }
    block_sum(mine, &s_cnt);
    if (threadIdx.x == 0 && s_cnt) atomicAdd(movers, s_cnt);
}

__global__ void __launch_bounds__(PF_THREADS) k_ld_minm(u32 m, const u32* __restrict__ newlab, u32* __restrict__ minm)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v >= m) return;
    const u32 lab = newlab[v];
    if (lab < 2 * m) atomicMin(&minm[lab], v);
}

// part[v] = the smallest member of v's label; S[v] and cnt[v] (may be null) cleared for k_ld_sizes
__global__ void __launch_bounds__(PF_THREADS) k_ld_newid(u32 m, const u32* __restrict__ newlab, const u32* __restrict__ minm, u32* __restrict__ part,
                                                         u32* __restrict__ S, u32* __restrict__ cnt)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v >= m) return;
    const u32 lab = newlab[v];
    part[v] = lab < 2 * m ? minm[lab] : CL_NONE;
    S[v] = 0;
    if (cnt) cnt[v] = 0;
}

// The start of a refinement: R = singletons, their sizes and counts; wp cleared for k_ld_wp.
__global__ void __launch_bounds__(PF_THREADS) k_ld_refine_init(u32 m, const u32* __restrict__ s, u32* __restrict__ R, u32* __restrict__ SR, u32* __restrict__ cntr,
                                                               i64* __restrict__ wp)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v >= m) return;
    R[v] = v; SR[v] = s[v]; cntr[v] = 1; wp[v] = 0;
}
// wp[v] = W(v, P(v))
__global__ void __launch_bounds__(PF_THREADS) k_ld_wp(const unsigned long long* __restrict__ lkey, const i64* __restrict__ lq, u64 count, u32 m,
                                                      const u32* __restrict__ P, i64* __restrict__ wp)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= count) return;
    const u64 k = lkey[i];
    const u32 a = (u32)(k >> 32), b = (u32)k;
    if (a >= m || b >= m || P[a] != P[b]) return;
    atomicAdd(reinterpret_cast<unsigned long long*>(&wp[a]), (unsigned long long)lq[i]);
    atomicAdd(reinterpret_cast<unsigned long long*>(&wp[b]), (unsigned long long)lq[i]);
}
__global__ void __launch_bounds__(PF_THREADS) k_ld_well(u32 m, i64 g, const u32* __restrict__ s, const u32* __restrict__ P, const u32* __restrict__ SP,
                                                        const i64* __restrict__ wp, u32* __restrict__ well)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v >= m) return;
    const u32 own = P[v];
    const i64 sv = s[v], So = own < m ? SP[own] : sv;
    well[v] = wp[v] >= g * sv * (So - sv) ? 1u : 0u;
}

__global__ void __launch_bounds__(PF_THREADS) k_ld_refine_insert(const unsigned long long* __restrict__ lkey, const i64* __restrict__ lq, u64 count, u32 m,
                                                                 const u32* __restrict__ P, const u32* __restrict__ R, ClLdTable t, i64* __restrict__ ext,
                                                                 u32* __restrict__ ctl)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= count) return;
    const u64 k = lkey[i];
    const u32 a = (u32)(k >> 32), b = (u32)k;
    if (a >= m || b >= m) { atomicOr(&ctl[CL_LD_ERR], 1u); return; }
    if (P[a] != P[b]) return;
    const u32 ra = R[a], rb = R[b];
    if (ra == rb) return;
    if (ra >= m || rb >= m) { atomicOr(&ctl[CL_LD_ERR], 1u); return; }
    const i64 q = lq[i];
    cl_ld_add(t, ((u64)a << 32) | rb, q, ctl);
    cl_ld_add(t, ((u64)b << 32) | ra, q, ctl);
    atomicAdd(reinterpret_cast<unsigned long long*>(&ext[ra]), (unsigned long long)q);
    atomicAdd(reinterpret_cast<unsigned long long*>(&ext[rb]), (unsigned long long)q);
}

__global__ void __launch_bounds__(PF_THREADS) k_ld_refine_node(u32 m, unsigned long long* __restrict__ bestd, u32* __restrict__ bestid,
                                                               unsigned long long* __restrict__ cd, u32* __restrict__ cv)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v >= m) return;
    bestd[v] = 0; bestid[v] = CL_NONE; cd[v] = 0; cv[v] = CL_NONE;
}

struct ClLdRefine {
    i64 g;
    const u32* __restrict__ s;
    const u32* __restrict__ P;
    const u32* __restrict__ R;
    const u32* __restrict__ SP;
    const u32* __restrict__ SR;
    const u32* __restrict__ cntr;
    const u32* __restrict__ well;
    const i64* __restrict__ ext;
};
// Whether slot i is a target of its node, and then the node, the R-community and D + 1.
__device__ __forceinline__ bool cl_ld_refine_at(const ClLdTable& t, u64 i, u32 m, const ClLdRefine& r, u32& v, u32& c, u64& D1)
{
    const u64 key = t.key[i];
    if (key == CL_LD_FREE) return false;
    v = (u32)(key >> 32); c = (u32)key;
    if (v >= m || c >= m) return false;
    const u32 rv = r.R[v], pv = r.P[v];
    if (rv >= m || pv >= m || r.cntr[rv] != 1 || !r.well[v]) return false;
    const i64 W = (i64)t.val[i], Sc = r.SR[c];
    if (W <= 0 || r.ext[c] < r.g * Sc * ((i64)r.SP[pv] - Sc)) return false;
    const i64 D = W - r.g * (i64)r.s[v] * Sc;
    D1 = (u64)(D + 1);
    return D >= 0;
}

__global__ void __launch_bounds__(PF_THREADS) k_ld_refine_bestd(ClLdTable t, u32 m, ClLdRefine r, unsigned long long* __restrict__ bestd)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    u32 v, c;
    u64 D1;
    if (i >= t.S || !cl_ld_refine_at(t, i, m, r, v, c, D1)) return;
    atomicMax(&bestd[v], (unsigned long long)D1);
}

__global__ void __launch_bounds__(PF_THREADS) k_ld_refine_bestid(ClLdTable t, u32 m, ClLdRefine r, const unsigned long long* __restrict__ bestd, u32* __restrict__ bestid)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    u32 v, c;
    u64 D1;
    if (i >= t.S || !cl_ld_refine_at(t, i, m, r, v, c, D1)) return;
    if (bestd[v] == D1) atomicMin(&bestid[v], c);
}

__global__ void __launch_bounds__(PF_THREADS) k_ld_agg_flags(u32 m, const u32* __restrict__ R, u32* __restrict__ flag)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v < m) flag[v] = R[v] == v ? 1u : 0u;
}
// below[v] = the R-communities with a smallest member below v: the new node of the R-community v
__global__ void __launch_bounds__(PF_THREADS) k_ld_agg_nodes(u32 m, const u32* __restrict__ R, const u32* __restrict__ P, const u32* __restrict__ SR,
                                                             const u64* __restrict__ below, u32* __restrict__ s2, u32* __restrict__ P2)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    if (v >= m || R[v] != v) return;
    const u32 i = (u32)below[v], p = P[v];
    if (i >= m) return;
    s2[i] = SR[v];
    P2[i] = p < m ? (u32)below[p] : CL_NONE;                     // (P's smallest member is the smallest of its R-community)
}
__global__ void __launch_bounds__(PF_THREADS) k_ld_agg_nodeof(u32 n, u32 m, const u32* __restrict__ R, const u64* __restrict__ below, u32* __restrict__ node_of)
{
    const u32 x = blockIdx.x * PF_THREADS + threadIdx.x;
    if (x >= n) return;
    const u32 v = node_of[x];
    const u32 r = v < m ? R[v] : CL_NONE;
    node_of[x] = r < m ? (u32)below[r] : CL_NONE;
}
__global__ void __launch_bounds__(PF_THREADS) k_ld_agg_insert(const unsigned long long* __restrict__ lkey, const i64* __restrict__ lq, u64 count, u32 m,
                                                              const u32* __restrict__ R, const u64* __restrict__ below, ClLdTable t, u32* __restrict__ ctl)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= count) return;
    const u64 k = lkey[i];
    const u32 a = (u32)(k >> 32), b = (u32)k;
    if (a >= m || b >= m) { atomicOr(&ctl[CL_LD_ERR], 1u); return; }
    const u32 ra = R[a], rb = R[b];
    if (ra == rb) return;
    if (ra >= m || rb >= m) { atomicOr(&ctl[CL_LD_ERR], 1u); return; }
    const u32 x = (u32)below[ra], y = (u32)below[rb];
    cl_ld_add(t, x < y ? ((u64)x << 32) | y : ((u64)y << 32) | x, lq[i], ctl);
}

// The end of an iteration: the label of an original genome is the community of its level node.
__global__ void __launch_bounds__(PF_THREADS) k_ld_final(u32 n, u32 m, const u32* __restrict__ node_of, const u32* __restrict__ P, u32* __restrict__ newlab,
                                                         u32* __restrict__ minm)
{
    const u32 x = blockIdx.x * PF_THREADS + threadIdx.x;
    if (x >= n) return;
    const u32 v = node_of[x];
    newlab[x] = v < m ? P[v] : CL_NONE;
    minm[x] = CL_NONE; minm[n + x] = CL_NONE;
}

// quality += the q of the level-0 entries inside one cluster; -= g * size * (size - 1) / 2 per cluster (cnt: k_ld_sizes)
__global__ void __launch_bounds__(PF_THREADS) k_ld_quality_edges(const unsigned long long* __restrict__ lkey, const i64* __restrict__ lq, u64 count, u32 n,
                                                                 const u32* __restrict__ rep_of, unsigned long long* __restrict__ quality)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    i64 mine = 0;
    if (i < count) {
        const u64 k = lkey[i];
        const u32 a = (u32)(k >> 32), b = (u32)k;
        if (a < n && b < n && rep_of[a] == rep_of[b]) mine = lq[i];
    }
    mine = cl_ld_wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(quality, (unsigned long long)mine);
}
__global__ void __launch_bounds__(PF_THREADS) k_ld_quality_nodes(u32 n, i64 g, const u32* __restrict__ cnt, unsigned long long* __restrict__ quality)
{
    const u32 v = blockIdx.x * PF_THREADS + threadIdx.x;
    i64 mine = 0;
    if (v < n) { const i64 z = cnt[v]; mine = g * (z * (z - 1) / 2); }
    mine = cl_ld_wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(quality, (unsigned long long)(-mine));
}

}  // namespace lzani
