// lzani_cluster.h -- host side of the cluster stage (include/lzani.h states the definitions): the edge buffer and its growth,
// the run -- union-find for single linkage, rounds of the greedy representatives, assignment, the distinct edges and
// the rounds of set cover, the contraction rounds of complete linkage, or the levels and rounds of Leiden; numbering --
// and the entry points
// (lzani_cluster_begin, lzani_cluster_add_kept, lzani_debug_cluster_add_edges, lzani_cluster_run, lzani_cluster_fetch,
// lzani_get_cluster_info, lzani_get_cluster_cover_info, lzani_get_cluster_link_info, lzani_set_cluster_leiden,
// lzani_get_cluster_leiden_info and the pure lzani_cluster_weight, lzani_cluster_host and lzani_cluster_leiden_host).  Included by lzani_hip.hip only,
// behind lzani_kept.h; of that file it uses lzani_ctx (which holds the Cluster and the Kept), fail, HIPCHK and sort_keys, of
// lzani_prefilter.h pf_blocks and pf_chunks, of lzani_devmem.h DevMem and StreamSpan.  The kernels are lzani_kernels_cluster.h; the group's form is in
// lzani_multi.h.
//
// What the stage reads and writes.  add_kept, per record: 36 B and two lengths read, 16 B written.  SINGLE: per edge 16 B
// and the two paths to the roots, one CAS per hook that is won; per node one path.  A greedy round: per edge 16 B and one or
// two state words read, at most one word stored; per node two words.  The assignment: per edge 16 B and two state words,
// one atomic per edge of a node that is no representative (BEST: two passes).  The numbering: per node three words, one
// atomic, and the scan of n flags.  Set cover, once per run: per edge record 16 B read and 8 B written, two sorts of as
// many bits as an id has, and the compaction (8 B read twice, 8 B written per distinct edge).  A set-cover round, per
// distinct edge: 8 B three times; two rep_of words and two atomic adds (count); two keys and one atomic max (first hop);
// two m1 words and at most one atomic max (second hop: none inside a clique, where every m1 is the same); per node six
// words read and five written.  Worst case of the rounds: the path with ascending ids, n / 3.  Complete linkage, a round
// over an entry list of |L| (the first: the E edge records, 16 B each; later 24 B an entry) and its table of S slots, the
// smallest power of two >= 2 |L|: 24 B a slot set; per entry its read, two labels, and at a load of at most 1 / 2 a few
// probes, one CAS where the slot is new, one atomic add and one atomic min; per slot 8 B four times (best weight, best id,
// the compaction's count and write), and per link two sizes, 16 B more, two atomic max, up to two atomic min, and 24 B
// written to the next list; per cluster 12 B cleared, one or two best ids read and, where it merges, four words; per node
// two words.  The merges and |L| are read back once a round (two words and one: no batching as in the greedy rounds, since
// the next round's grid is |L|'s).  Worst case of the rounds: the path with ascending ids and equal weights, n / 2 + 1.
// Leiden, a moving round over the level's |L| entries, m nodes and a table of S slots, the smallest power of two >= 4 |L|:
// 16 B a slot and 8 B a node set; per entry 16 B, two community words, two probe sequences, a CAS where the slot is new and
// two 64-bit atomic adds; per slot key and sum three times, one atomic max and at most one atomic min; per node some 60 B,
// two atomic max and up to two atomic min on the community words, one atomic min on its label's smallest member and one
// atomic add on its community's size.  A refinement round: the same, and two atomic adds an entry more.  The control words
// are read back once in CL_LD_BATCH rounds, the aggregation's two counts once a level.  Worst case: one clique of n, n
// moving rounds.
#pragma once

namespace {

enum { CL_BATCH = 8 };                                  // greedy rounds launched between two reads of the undecided counts

int cluster_state(lzani_ctx* c, const std::string& fn)
{
    if (!c->cl.begun) return fail(c, LZANI_ERR_STATE, fn + ": no cluster state (call lzani_cluster_begin first)");
    return LZANI_OK;
}

// Room for `need` edges: kept if there is, else a buffer of at least twice the size, the edges copied on the device.  A
// failure leaves the buffer and its edges as they were.
int cluster_reserve(lzani_ctx* c, u64 need)
{
    Cluster& k = c->cl;
    if ((need + PF_THREADS - 1) / PF_THREADS > 0x7FFFFFFFull) return fail(c, LZANI_ERR_ARG, "cluster stage: more edges than one launch covers");
    if (need <= k.edges.capacity()) return LZANI_OK;
    DevMem<lzani_cluster_edge> bigger;
    const u64 twice = std::max<u64>(need, 2 * (u64)k.edges.capacity());
    if (!got(bigger.alloc((size_t)twice))) HIPCHK(c, bigger.alloc((size_t)need));
    if (k.info.edges) {
        HIPCHK(c, hipMemcpyAsync(bigger.get(), k.edges.get(), (size_t)k.info.edges * sizeof(lzani_cluster_edge), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    k.edges = std::move(bigger);
    k.info.edge_bytes = k.edges.bytes();
    return LZANI_OK;
}

// The workspace of a set-cover run, allocated whole before the run touches the cluster state: the keys of the edge records
// and of the distinct edges (two buffers of E, the sort's in and out in turn), the sort's scratch, the compaction's block
// counts and offsets, and per node the counter and the three 64-bit words of a round.
constexpr u64 CL_COVER_MAX_EDGES = 0xFFFFFFEFull;       // 2^32 - 17: lzani_sort_keys' limit
struct CoverWork {
    DevMem<unsigned long long> ka, kb, key, m1, m2;
    DevMem<unsigned char> scratch;
    DevMem<u32> ucnt, cnt;
    DevMem<u64> uoff;
    int bits = 1;                                       // of an id below n
    u64 bytes() const { return ka.bytes() + kb.bytes() + key.bytes() + m1.bytes() + m2.bytes() + scratch.bytes() + ucnt.bytes() + cnt.bytes() + uoff.bytes(); }
};

int cluster_cover_alloc(lzani_ctx* c, CoverWork& w)
{
    const u32 n = c->cl.info.n;
    const u64 E = c->cl.info.edges;
    if (E > CL_COVER_MAX_EDGES) return fail(c, LZANI_ERR_ARG, "lzani_cluster_run: set cover sorts at most 2^32 - 17 edge records");
    while (w.bits < 32 && ((u64)1 << w.bits) < n) ++w.bits;
    size_t need = 0;                                    // (the same for the two sorts: as many bits, as many keys)
    if (int rc = sort_scratch_bytes(c, (size_t)E, 1, 0, w.bits, "lzani_cluster_run: sort", need)) return rc;
    HIPCHK(c, w.ka.alloc((size_t)E)); HIPCHK(c, w.kb.alloc((size_t)E)); HIPCHK(c, w.scratch.alloc(need));
    HIPCHK(c, w.ucnt.alloc((size_t)pf_chunks(E))); HIPCHK(c, w.uoff.alloc((size_t)pf_chunks(E) + 1));
    HIPCHK(c, w.cnt.alloc(n)); HIPCHK(c, w.key.alloc(n)); HIPCHK(c, w.m1.alloc(n)); HIPCHK(c, w.m2.alloc(n));
    return LZANI_OK;
}

// The distinct edges of the context's edge records, ascending, in w.kb: D of them.  The edge buffer is only read.
int cluster_cover_dedup(lzani_ctx* c, CoverWork& w, u64& D)
{
    const u64 E = c->cl.info.edges;
    D = 0;
    if (!E) return LZANI_OK;
    hipLaunchKernelGGL(k_cl_cover_keys, dim3(pf_blocks(E)), dim3(PF_THREADS), 0, c->stream, (const lzani_cluster_edge*)c->cl.edges.get(), E, w.ka.get());
    HIPCHK(c, hipGetLastError());
    // by hi, then (the sort is stable) by lo: only the bits an id below n has
    if (int rc = sort_keys(c, w.scratch, w.ka.get(), w.kb.get(), (size_t)E, 1, 0, w.bits, "lzani_cluster_run: sort", false)) return rc;
    if (int rc = sort_keys(c, w.scratch, w.kb.get(), w.ka.get(), (size_t)E, 1, 32, 32 + w.bits, "lzani_cluster_run: sort", false)) return rc;
    const u32 blocks = (u32)pf_chunks(E);
    hipLaunchKernelGGL(k_pf_uniq<false>, dim3(blocks), dim3(PF_THREADS), 0, c->stream, (const unsigned long long*)w.ka.get(), E, w.ucnt.get(),
                       (const u64*)w.uoff.get(), w.kb.get(), (u32*)nullptr, 0u);
    hipLaunchKernelGGL(k_pf_scan, dim3(1), dim3(1024), 0, c->stream, (const u32*)w.ucnt.get(), (u64)blocks, w.uoff.get());
    hipLaunchKernelGGL(k_pf_uniq<true>, dim3(blocks), dim3(PF_THREADS), 0, c->stream, (const unsigned long long*)w.ka.get(), E, w.ucnt.get(),
                       (const u64*)w.uoff.get(), w.kb.get(), (u32*)nullptr, 0u);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(&D, w.uoff.get() + blocks, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (D > E) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: more distinct edges than edge records");
    return LZANI_OK;
}

// The rounds of set cover over the D distinct edges of w.kb (lzani_kernels_cluster.h): rep_of, and the number of the first
// round that left no node unassigned.
int cluster_cover_rounds(lzani_ctx* c, CoverWork& w, u64 D, u32* rep_of, u32* undecided, u64& rounds)
{
    const u32 n = c->cl.info.n;
    const dim3 nodes(pf_blocks(n)), edge_blocks(pf_blocks(D)), threads(PF_THREADS);
    const unsigned long long* pairs = w.kb.get();
    rounds = 0;
    for (bool done = false; !done;) {
        // the unassigned node with the largest key is selected in every round: n rounds always do, and a defect ends here instead of spinning
        if (rounds >= (u64)n + 1) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: nodes still unassigned after n + 1 rounds");
        const u32 batch = (u32)std::min<u64>(CL_BATCH, (u64)n + 1 - rounds);
        HIPCHK(c, hipMemsetAsync(undecided, 0, CL_BATCH * sizeof(u32), c->stream));
        for (u32 r = 0; r < batch; ++r) {
            if (D) hipLaunchKernelGGL(k_cl_cover_count, edge_blocks, threads, 0, c->stream, pairs, D, n, (const u32*)rep_of, w.cnt.get());
            hipLaunchKernelGGL(k_cl_cover_key, nodes, threads, 0, c->stream, n, (const u32*)rep_of, w.cnt.get(), w.key.get(), w.m1.get(), w.m2.get());
            if (D) hipLaunchKernelGGL(k_cl_cover_max, edge_blocks, threads, 0, c->stream, pairs, D, n, (const unsigned long long*)w.key.get(), w.m1.get());
            if (D) hipLaunchKernelGGL(k_cl_cover_max, edge_blocks, threads, 0, c->stream, pairs, D, n, (const unsigned long long*)w.m1.get(), w.m2.get());
            hipLaunchKernelGGL(k_cl_cover_decide, nodes, threads, 0, c->stream, n, (const unsigned long long*)w.m1.get(), (const unsigned long long*)w.m2.get(),
                               rep_of, undecided + r);
        }
        HIPCHK(c, hipGetLastError());
        u32 left[CL_BATCH];
        HIPCHK(c, hipMemcpyAsync(left, undecided, sizeof left, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        u32 r = 0;
        while (r < batch && left[r]) ++r;
        done = r < batch;
        rounds += done ? r + 1 : batch;                 // (the rounds behind the first that left no node change nothing)
    }
    return LZANI_OK;
}

// The workspace of a complete-linkage run, allocated whole before the run touches the cluster state: the table of S slots
// (S for the first round, the largest), the entry list (at most one entry per distinct edge), the compaction's block counts
// and offsets, per cluster label, size, best weight and best id, and the round's two control words.
constexpr u64 CL_LINK_MAX_EDGES = 0xFFFFFFEFull;        // 2^32 - 17, as for set cover
struct LinkWork {
    DevMem<unsigned long long> tkey, tcnt, tw, lkey, lcnt, lw, bestw;
    DevMem<u32> label, csize, bestid, ucnt, ctl;
    DevMem<u64> uoff;
    u64 S = 1;                                          // of the first round
    u64 bytes() const
    {
        return tkey.bytes() + tcnt.bytes() + tw.bytes() + lkey.bytes() + lcnt.bytes() + lw.bytes() + bestw.bytes() + label.bytes() + csize.bytes() +
               bestid.bytes() + ucnt.bytes() + ctl.bytes() + uoff.bytes();
    }
};

// the smallest power of two >= 2 * entries (1 for none)
u64 cluster_link_slots(u64 entries)
{
    u64 S = 1;
    while (S < 2 * entries) S <<= 1;
    return S;
}

int cluster_link_alloc(lzani_ctx* c, LinkWork& w)
{
    const u32 n = c->cl.info.n;
    const u64 E = c->cl.info.edges;
    if (E > CL_LINK_MAX_EDGES) return fail(c, LZANI_ERR_ARG, "lzani_cluster_run: complete linkage takes at most 2^32 - 17 edge records");
    w.S = cluster_link_slots(E);
    HIPCHK(c, w.tkey.alloc((size_t)w.S)); HIPCHK(c, w.tcnt.alloc((size_t)w.S)); HIPCHK(c, w.tw.alloc((size_t)w.S));
    HIPCHK(c, w.lkey.alloc((size_t)E)); HIPCHK(c, w.lcnt.alloc((size_t)E)); HIPCHK(c, w.lw.alloc((size_t)E));
    HIPCHK(c, w.ucnt.alloc((size_t)pf_chunks(w.S))); HIPCHK(c, w.uoff.alloc((size_t)pf_chunks(w.S) + 1));
    HIPCHK(c, w.label.alloc(n)); HIPCHK(c, w.csize.alloc(n)); HIPCHK(c, w.bestw.alloc(n)); HIPCHK(c, w.bestid.alloc(n));
    HIPCHK(c, w.ctl.alloc(CL_LINK_CTL));
    return LZANI_OK;
}

// The rounds of complete linkage (lzani_kernels_cluster.h): rep_of, the number of the first round that merged nothing, the
// merges, the distinct edges (the first round's links: every distinct edge is one) and the time of the first insert.
int cluster_link_rounds(lzani_ctx* c, LinkWork& w, u32* rep_of, u64& rounds, u64& merges, u64& D, float& dedup_ms)
{
    const Cluster& k = c->cl;
    const u32 n = k.info.n;
    const dim3 nodes(pf_blocks(n)), threads(PF_THREADS);
    u64 L = k.info.edges;                               // entries of the round: edge records, then the last round's links
    rounds = 1; merges = 0; D = 0; dedup_ms = 0;
    StreamSpan first;
    for (; L; ++rounds) {                               // (no entry: no link, and the round merges nothing)
        // the link with the largest value merges in every round: n rounds always do, and a defect ends here instead of spinning
        if (rounds > (u64)n + 1) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: links still merging after n + 1 rounds");
        const ClLinkTable t{w.tkey.get(), w.tcnt.get(), w.tw.get(), cluster_link_slots(L)};
        if (t.S > w.S) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: more link entries than edge records");
        const dim3 slots(pf_blocks(t.S));
        const u32 chunks = (u32)pf_chunks(t.S);
        if (rounds == 1) HIPCHK(c, first.begin(c->stream));
        HIPCHK(c, hipMemsetAsync(t.key, 0xFF, (size_t)t.S * 8, c->stream));
        HIPCHK(c, hipMemsetAsync(t.w, 0xFF, (size_t)t.S * 8, c->stream));
        HIPCHK(c, hipMemsetAsync(t.cnt, 0, (size_t)t.S * 8, c->stream));
        HIPCHK(c, hipMemsetAsync(w.ctl, 0, CL_LINK_CTL * sizeof(u32), c->stream));
        hipLaunchKernelGGL(k_cl_link_insert, dim3(pf_blocks(L)), threads, 0, c->stream, rounds == 1 ? (const lzani_cluster_edge*)k.edges.get() : nullptr,
                           (const unsigned long long*)w.lkey.get(), (const unsigned long long*)w.lcnt.get(), (const unsigned long long*)w.lw.get(), L, n,
                           (const u32*)w.label.get(), t, w.ctl.get());
        if (rounds == 1) HIPCHK(c, first.end(c->stream));
        hipLaunchKernelGGL(k_cl_link_clear, nodes, threads, 0, c->stream, n, w.bestw.get(), w.bestid.get());
        hipLaunchKernelGGL(k_cl_link_bestw, slots, threads, 0, c->stream, t, n, (const u32*)w.csize.get(), w.bestw.get());
        hipLaunchKernelGGL(k_cl_link_bestid, slots, threads, 0, c->stream, t, n, (const u32*)w.csize.get(), (const unsigned long long*)w.bestw.get(), w.bestid.get());
        hipLaunchKernelGGL(k_cl_link_compact<false>, dim3(chunks), threads, 0, c->stream, t, n, (const u32*)w.csize.get(), w.ucnt.get(), (const u64*)w.uoff.get(),
                           w.lkey.get(), w.lcnt.get(), w.lw.get());
        hipLaunchKernelGGL(k_pf_scan, dim3(1), dim3(1024), 0, c->stream, (const u32*)w.ucnt.get(), (u64)chunks, w.uoff.get());
        hipLaunchKernelGGL(k_cl_link_compact<true>, dim3(chunks), threads, 0, c->stream, t, n, (const u32*)w.csize.get(), w.ucnt.get(), (const u64*)w.uoff.get(),
                           w.lkey.get(), w.lcnt.get(), w.lw.get());
        hipLaunchKernelGGL(k_cl_link_merge, nodes, threads, 0, c->stream, n, (const u32*)w.bestid.get(), w.label.get(), w.csize.get(), w.ctl.get());
        hipLaunchKernelGGL(k_cl_link_relabel, nodes, threads, 0, c->stream, n, (const u32*)w.label.get(), rep_of);
        HIPCHK(c, hipGetLastError());
        u32 ctl[CL_LINK_CTL] = {0, 0};
        u64 links = 0;
        HIPCHK(c, hipMemcpyAsync(ctl, w.ctl.get(), sizeof ctl, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&links, w.uoff.get() + chunks, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (ctl[CL_LINK_ERR]) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: the cluster-pair table's probe sequence ran out, or an id out of range");
        if (links > L) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: more links than entries");
        if (rounds == 1) { D = links; HIPCHK(c, first.elapsed(dedup_ms)); }
        if (!ctl[CL_LINK_MERGES]) break;
        merges += ctl[CL_LINK_MERGES];
        L = links;
    }
    return LZANI_OK;
}

// The workspace of a Leiden run, allocated whole before the run touches the cluster state: the table of S slots (S for the
// largest round there can be: 2 * E insertions), the level-0 entry list and the working list of the higher levels (at most
// one entry per distinct edge each), the compaction's block counts and offsets, the per-node and per-community words of
// the rounds (two sets of sizes and partitions: a level and the one aggregated from it), and the control words.
constexpr u64 CL_LEIDEN_MAX_EDGES = 0xFFFFFFEFull;      // 2^32 - 17, as for set cover
struct LeidenWork {
    DevMem<unsigned long long> tkey, tval, e0key, wkey, bestd, cd, quality;
    DevMem<i64> e0q, wq, ownw, valown, ext;             // ownw: W(v, own) of a moving round, W(v, P(v)) of a refinement
    DevMem<u32> s, s2, P, P2, R, SP, SR, cntr, well, bestid, cv, newlab, minm, node_of, flag, ucnt, ctl;
    DevMem<u64> uoff, below;
    u64 S = 1;
    u64 bytes() const
    {
        return tkey.bytes() + tval.bytes() + e0key.bytes() + wkey.bytes() + bestd.bytes() + cd.bytes() + quality.bytes() + e0q.bytes() + wq.bytes() +
               ownw.bytes() + valown.bytes() + ext.bytes() + s.bytes() + s2.bytes() + P.bytes() + P2.bytes() + R.bytes() + SP.bytes() + SR.bytes() +
               cntr.bytes() + well.bytes() + bestid.bytes() + cv.bytes() + newlab.bytes() + minm.bytes() + node_of.bytes() + flag.bytes() +
               ucnt.bytes() + ctl.bytes() + uoff.bytes() + below.bytes();
    }
};

int cluster_leiden_alloc(lzani_ctx* c, LeidenWork& w)
{
    const u32 n = c->cl.info.n;
    const u64 E = c->cl.info.edges;
    if (n > CL_LEIDEN_MAX_N) return fail(c, LZANI_ERR_ARG, "lzani_cluster_run: Leiden takes at most 2^21 genomes");
    if (E > CL_LEIDEN_MAX_EDGES) return fail(c, LZANI_ERR_ARG, "lzani_cluster_run: Leiden takes at most 2^32 - 17 edge records");
    w.S = cluster_link_slots(2 * E);
    HIPCHK(c, w.tkey.alloc((size_t)w.S)); HIPCHK(c, w.tval.alloc((size_t)w.S));
    HIPCHK(c, w.e0key.alloc((size_t)E)); HIPCHK(c, w.e0q.alloc((size_t)E)); HIPCHK(c, w.wkey.alloc((size_t)E)); HIPCHK(c, w.wq.alloc((size_t)E));
    HIPCHK(c, w.ucnt.alloc((size_t)pf_chunks(w.S))); HIPCHK(c, w.uoff.alloc((size_t)pf_chunks(w.S) + 1));
    HIPCHK(c, w.bestd.alloc(n)); HIPCHK(c, w.cd.alloc(n)); HIPCHK(c, w.ownw.alloc(n)); HIPCHK(c, w.valown.alloc(n)); HIPCHK(c, w.ext.alloc(n));
    HIPCHK(c, w.s.alloc(n)); HIPCHK(c, w.s2.alloc(n)); HIPCHK(c, w.P.alloc(n)); HIPCHK(c, w.P2.alloc(n)); HIPCHK(c, w.R.alloc(n));
    HIPCHK(c, w.SP.alloc(n)); HIPCHK(c, w.SR.alloc(n)); HIPCHK(c, w.cntr.alloc(n)); HIPCHK(c, w.well.alloc(n)); HIPCHK(c, w.bestid.alloc(n));
    HIPCHK(c, w.cv.alloc(n)); HIPCHK(c, w.newlab.alloc(n)); HIPCHK(c, w.minm.alloc(2 * (size_t)n)); HIPCHK(c, w.node_of.alloc(n));
    HIPCHK(c, w.flag.alloc(n)); HIPCHK(c, w.below.alloc((size_t)n + 1));
    HIPCHK(c, w.quality.alloc(1)); HIPCHK(c, w.ctl.alloc(CL_LD_CTL));
    return LZANI_OK;
}

// A phase on a level of m nodes: round(r) launches one round whose movers go to ctl[CL_LD_MOVERS + r] (and, where it counts
// them, the communities behind it to ctl[CL_LD_COMMS + r]); batches of CL_LD_BATCH rounds between two reads of the control
// words, as a round behind the one without a mover changes nothing.  rounds: up to the first without a mover, that one
// included; movers: their sum; comms: the communities behind the last round.
template <class Round>
int cluster_leiden_phase(lzani_ctx* c, LeidenWork& w, u32 m, const char* what, Round round, u64& rounds, u64& movers, u32& comms)
{
    const u64 cap = CL_LEIDEN_CAP_MUL * m + CL_LEIDEN_CAP_ADD;
    rounds = 0; movers = 0; comms = 0;
    for (bool done = false; !done;) {
        // a safety stop, not a bound that is proved: see include/lzani.h
        if (rounds >= cap) return fail(c, LZANI_ERR_DEVICE, std::string("lzani_cluster_run: Leiden's ") + what + " still moves nodes after 64 * n + 64 rounds");
        const u32 batch = (u32)std::min<u64>(CL_LD_BATCH, cap - rounds);
        HIPCHK(c, hipMemsetAsync(w.ctl, 0, CL_LD_CTL * sizeof(u32), c->stream));
        for (u32 r = 0; r < batch; ++r) HIPCHK(c, round(r));
        HIPCHK(c, hipGetLastError());
        u32 ctl[CL_LD_CTL];
        HIPCHK(c, hipMemcpyAsync(ctl, w.ctl, sizeof ctl, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (ctl[CL_LD_ERR]) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: the node-community table's probe sequence ran out, or an id out of range");
        u32 r = 0;
        while (r < batch && ctl[CL_LD_MOVERS + r]) movers += ctl[CL_LD_MOVERS + r++];
        done = r < batch;
        rounds += done ? r + 1 : batch;
        comms = ctl[CL_LD_COMMS + (done ? r : batch - 1)];
    }
    return LZANI_OK;
}

// The table of a round cleared: the keys all ones, the values `fill` bytes.
hipError_t cluster_leiden_clear(lzani_ctx* c, const ClLdTable& t, int fill)
{
    const hipError_t e = hipMemsetAsync(t.key, 0xFF, (size_t)t.S * 8, c->stream);
    return e != hipSuccess ? e : hipMemsetAsync(t.val, fill, (size_t)t.S * 8, c->stream);
}

// The table's occupied slots into the entry list (key, q); their number at w.uoff[pf_chunks(t.S)].
void cluster_leiden_compact(lzani_ctx* c, LeidenWork& w, const ClLdTable& t, unsigned long long* key, i64* q)
{
    const u32 chunks = (u32)pf_chunks(t.S);
    const dim3 threads(PF_THREADS);
    hipLaunchKernelGGL(k_ld_compact<false>, dim3(chunks), threads, 0, c->stream, t, w.ucnt.get(), (const u64*)w.uoff.get(), key, q);
    hipLaunchKernelGGL(k_pf_scan, dim3(1), dim3(1024), 0, c->stream, (const u32*)w.ucnt.get(), (u64)chunks, w.uoff.get());
    hipLaunchKernelGGL(k_ld_compact<true>, dim3(chunks), threads, 0, c->stream, t, w.ucnt.get(), (const u64*)w.uoff.get(), key, q);
}

// The iterations of Leiden (lzani_kernels_cluster.h): rep_of (v at the start) and what the run did.
int cluster_leiden_rounds(lzani_ctx* c, LeidenWork& w, u32* rep_of, lzani_cluster_leiden_info& out)
{
    const Cluster& k = c->cl;
    const u32 n = k.info.n;
    const u64 E = k.info.edges;
    const i64 g = cluster_leiden_g(c->leiden_resolution);
    const dim3 threads(PF_THREADS), all(pf_blocks(n));
    out = lzani_cluster_leiden_info{};
    out.resolution_q = (u64)g; out.table_slots = w.S; out.workspace_bytes = w.bytes();
    // the distinct edges with their smallest q: the level-0 entry list
    StreamSpan dedup, span;
    u64 D = 0;
    HIPCHK(c, dedup.begin(c->stream));
    if (E) {
        const ClLdTable t{w.tkey.get(), w.tval.get(), cluster_link_slots(E)};
        HIPCHK(c, cluster_leiden_clear(c, t, 0xFF));
        HIPCHK(c, hipMemsetAsync(w.ctl, 0, CL_LD_CTL * sizeof(u32), c->stream));
        hipLaunchKernelGGL(k_ld_dedup, dim3(pf_blocks(E)), threads, 0, c->stream, (const lzani_cluster_edge*)k.edges.get(), E, n, t, w.ctl.get());
        cluster_leiden_compact(c, w, t, w.e0key.get(), w.e0q.get());
        HIPCHK(c, hipGetLastError());
        u32 err = 0;
        HIPCHK(c, hipMemcpyAsync(&err, w.ctl.get() + CL_LD_ERR, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&D, w.uoff.get() + pf_chunks(t.S), 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (err) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: the edge table's probe sequence ran out, or an id out of range");
        if (D > E) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: more distinct edges than edge records");
    }
    HIPCHK(c, dedup.end(c->stream));
    out.distinct_edges = D; out.duplicate_edges = E - D;
    HIPCHK(c, span.begin(c->stream));
    for (int it = 0; it < c->leiden_iterations; ++it) {
        out.iterations++;
        u32 m = n;                                      // the level: its nodes, its entries and where they are
        u64 L = D;
        const unsigned long long* lkey = w.e0key.get();
        const i64* lq = w.e0q.get();
        hipLaunchKernelGGL(k_ld_level0, all, threads, 0, c->stream, n, (const u32*)rep_of, w.s.get(), w.P.get(), w.node_of.get());
        HIPCHK(c, hipMemsetAsync(w.SP, 0, (size_t)n * 4, c->stream));
        hipLaunchKernelGGL(k_ld_sizes, all, threads, 0, c->stream, n, (const u32*)w.s.get(), (const u32*)w.P.get(), w.SP.get(), (u32*)nullptr, (u32*)nullptr);
        u64 moved_in_iteration = 0;
        for (;;) {
            out.levels++;
            const dim3 nodes(pf_blocks(m)), entries(pf_blocks(L));
            const ClLdTable t{w.tkey.get(), w.tval.get(), cluster_link_slots(2 * L)};
            if (t.S > w.S) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: more entries than edge records");
            const dim3 slots(pf_blocks(t.S));
            u32 *s = w.s.get(), *P = w.P.get(), *R = w.R.get(), *SP = w.SP.get(), *SR = w.SR.get(), *cntr = w.cntr.get(), *ctl = w.ctl.get();
            u64 rounds = 0, moved = 0, merged = 0;
            u32 comms = 0;
            auto share = [&](u32* part, u32* S, u32* cnt, u32 r, bool count_comms) {         // the passes both kinds of round end in
                hipLaunchKernelGGL(k_ld_cand_max, nodes, threads, 0, c->stream, m, (const u32*)part, (const unsigned long long*)w.bestd.get(),
                                   (const u32*)w.bestid.get(), w.cd.get());
                hipLaunchKernelGGL(k_ld_cand_min, nodes, threads, 0, c->stream, m, (const u32*)part, (const unsigned long long*)w.bestd.get(),
                                   (const u32*)w.bestid.get(), (const unsigned long long*)w.cd.get(), w.cv.get());
                hipLaunchKernelGGL(k_ld_decide, nodes, threads, 0, c->stream, m, (const u32*)part, (const unsigned long long*)w.bestd.get(),
                                   (const u32*)w.bestid.get(), (const u32*)w.cv.get(), w.newlab.get(), w.minm.get(), ctl + CL_LD_MOVERS + r);
                hipLaunchKernelGGL(k_ld_minm, nodes, threads, 0, c->stream, m, (const u32*)w.newlab.get(), w.minm.get());
                hipLaunchKernelGGL(k_ld_newid, nodes, threads, 0, c->stream, m, (const u32*)w.newlab.get(), (const u32*)w.minm.get(), part, S, cnt);
                hipLaunchKernelGGL(k_ld_sizes, nodes, threads, 0, c->stream, m, (const u32*)s, (const u32*)part, S, cnt,
                                   count_comms ? ctl + CL_LD_COMMS + r : (u32*)nullptr);
            };
            auto move_round = [&](u32 r) -> hipError_t {
                if (hipError_t e = cluster_leiden_clear(c, t, 0)) return e;
                if (hipError_t e = hipMemsetAsync(w.ownw, 0, (size_t)m * 8, c->stream)) return e;
                if (L) hipLaunchKernelGGL(k_ld_move_insert, entries, threads, 0, c->stream, lkey, lq, L, m, (const u32*)P, t, ctl);
                hipLaunchKernelGGL(k_ld_move_stay, slots, threads, 0, c->stream, t, m, (const u32*)P, w.ownw.get());
                hipLaunchKernelGGL(k_ld_move_node, nodes, threads, 0, c->stream, m, g, (const u32*)s, (const u32*)P, (const u32*)SP, (const i64*)w.ownw.get(),
                                   w.valown.get(), w.bestd.get(), w.bestid.get(), w.cd.get(), w.cv.get());
                hipLaunchKernelGGL(k_ld_move_bestd, slots, threads, 0, c->stream, t, m, g, (const u32*)s, (const u32*)P, (const u32*)SP,
                                   (const i64*)w.valown.get(), w.bestd.get());
                hipLaunchKernelGGL(k_ld_move_bestid, slots, threads, 0, c->stream, t, m, g, (const u32*)s, (const u32*)P, (const u32*)SP,
                                   (const i64*)w.valown.get(), (const unsigned long long*)w.bestd.get(), w.bestid.get());
                share(P, SP, nullptr, r, true);
                return hipSuccess;
            };
            if (int rc = cluster_leiden_phase(c, w, m, "moving phase", move_round, rounds, moved, comms)) return rc;
            out.move_rounds += rounds; out.moves += moved; moved_in_iteration += moved;
            if (comms == m) break;                      // every community is one level node
            hipLaunchKernelGGL(k_ld_refine_init, nodes, threads, 0, c->stream, m, (const u32*)s, R, SR, cntr, w.ownw.get());
            if (L) hipLaunchKernelGGL(k_ld_wp, entries, threads, 0, c->stream, lkey, lq, L, m, (const u32*)P, w.ownw.get());
            hipLaunchKernelGGL(k_ld_well, nodes, threads, 0, c->stream, m, g, (const u32*)s, (const u32*)P, (const u32*)SP, (const i64*)w.ownw.get(), w.well.get());
            const ClLdRefine rf{g, s, P, R, SP, SR, cntr, w.well.get(), w.ext.get()};
            auto refine_round = [&](u32 r) -> hipError_t {
                if (hipError_t e = cluster_leiden_clear(c, t, 0)) return e;
                if (hipError_t e = hipMemsetAsync(w.ext, 0, (size_t)m * 8, c->stream)) return e;
                if (L) hipLaunchKernelGGL(k_ld_refine_insert, entries, threads, 0, c->stream, lkey, lq, L, m, (const u32*)P, (const u32*)R, t, w.ext.get(), ctl);
                hipLaunchKernelGGL(k_ld_refine_node, nodes, threads, 0, c->stream, m, w.bestd.get(), w.bestid.get(), w.cd.get(), w.cv.get());
                hipLaunchKernelGGL(k_ld_refine_bestd, slots, threads, 0, c->stream, t, m, rf, w.bestd.get());
                hipLaunchKernelGGL(k_ld_refine_bestid, slots, threads, 0, c->stream, t, m, rf, (const unsigned long long*)w.bestd.get(), w.bestid.get());
                share(R, SR, cntr, r, false);
                return hipSuccess;
            };
            if (int rc = cluster_leiden_phase(c, w, m, "refinement", refine_round, rounds, merged, comms)) return rc;
            out.refine_rounds += rounds; out.merges += merged;
            if (!moved && !merged) break;               // nothing can change any more
            // aggregation: the R-communities, numbered in ascending order of their smallest member, and the entries between them
            hipLaunchKernelGGL(k_ld_agg_flags, nodes, threads, 0, c->stream, m, (const u32*)R, w.flag.get());
            hipLaunchKernelGGL(k_pf_scan, dim3(1), dim3(1024), 0, c->stream, (const u32*)w.flag.get(), (u64)m, w.below.get());
            hipLaunchKernelGGL(k_ld_agg_nodes, nodes, threads, 0, c->stream, m, (const u32*)R, (const u32*)P, (const u32*)SR, (const u64*)w.below.get(),
                               w.s2.get(), w.P2.get());
            hipLaunchKernelGGL(k_ld_agg_nodeof, all, threads, 0, c->stream, n, m, (const u32*)R, (const u64*)w.below.get(), w.node_of.get());
            const ClLdTable ta{w.tkey.get(), w.tval.get(), cluster_link_slots(L)};
            HIPCHK(c, cluster_leiden_clear(c, ta, 0));
            HIPCHK(c, hipMemsetAsync(w.ctl, 0, CL_LD_CTL * sizeof(u32), c->stream));
            if (L) hipLaunchKernelGGL(k_ld_agg_insert, entries, threads, 0, c->stream, lkey, lq, L, m, (const u32*)R, (const u64*)w.below.get(), ta, ctl);
            cluster_leiden_compact(c, w, ta, w.wkey.get(), w.wq.get());
            HIPCHK(c, hipGetLastError());
            u64 m2 = 0, L2 = 0;
            u32 err = 0;
            HIPCHK(c, hipMemcpyAsync(&m2, w.below.get() + m, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(&L2, w.uoff.get() + pf_chunks(ta.S), 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(&err, w.ctl.get() + CL_LD_ERR, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (err) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: the contraction table's probe sequence ran out, or an id out of range");
            if (!m2 || m2 > m || L2 > L) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: an aggregated level larger than the level it comes from");
            std::swap(w.s, w.s2); std::swap(w.P, w.P2);
            m = (u32)m2; L = L2; lkey = w.wkey.get(); lq = w.wq.get();
            HIPCHK(c, hipMemsetAsync(w.SP, 0, (size_t)m * 4, c->stream));
            hipLaunchKernelGGL(k_ld_sizes, dim3(pf_blocks(m)), threads, 0, c->stream, m, (const u32*)w.s.get(), (const u32*)w.P.get(), w.SP.get(), (u32*)nullptr,
                               (u32*)nullptr);
        }
        // rep_of: the smallest original id of every final community
        hipLaunchKernelGGL(k_ld_final, all, threads, 0, c->stream, n, m, (const u32*)w.node_of.get(), (const u32*)w.P.get(), w.newlab.get(), w.minm.get());
        hipLaunchKernelGGL(k_ld_minm, all, threads, 0, c->stream, n, (const u32*)w.newlab.get(), w.minm.get());
        hipLaunchKernelGGL(k_ld_newid, all, threads, 0, c->stream, n, (const u32*)w.newlab.get(), (const u32*)w.minm.get(), rep_of, w.SP.get(), (u32*)nullptr);
        HIPCHK(c, hipGetLastError());
        if (!moved_in_iteration) break;
    }
    // Q of the result on the original graph (k_ld_newid left SP cleared)
    HIPCHK(c, hipMemsetAsync(w.quality, 0, 8, c->stream));
    hipLaunchKernelGGL(k_ld_sizes, all, threads, 0, c->stream, n, (const u32*)nullptr, (const u32*)rep_of, w.SP.get(), (u32*)nullptr, (u32*)nullptr);
    if (D) hipLaunchKernelGGL(k_ld_quality_edges, dim3(pf_blocks(D)), threads, 0, c->stream, (const unsigned long long*)w.e0key.get(), (const i64*)w.e0q.get(), D, n,
                              (const u32*)rep_of, w.quality.get());
    hipLaunchKernelGGL(k_ld_quality_nodes, all, threads, 0, c->stream, n, g, (const u32*)w.SP.get(), w.quality.get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, span.end(c->stream));
    unsigned long long quality = 0;
    HIPCHK(c, hipMemcpyAsync(&quality, w.quality.get(), 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float dedup_ms = 0, rounds_ms = 0;
    HIPCHK(c, dedup.elapsed(dedup_ms));
    HIPCHK(c, span.elapsed(rounds_ms));
    out.quality = (int64_t)quality; out.dedup_ms = dedup_ms; out.rounds_ms = rounds_ms;
    return LZANI_OK;
}

// What every algorithm's run works in, and what it leaves: allocated whole before the run touches the cluster state, like
// the workspaces of set cover, complete linkage and Leiden above.
struct StageWork {
    DevMem<u32> parent, state, blocked, flag, size, counters, undecided;     // parent, state, blocked, best: SINGLE and the greedy forms
    DevMem<unsigned long long> best;
    DevMem<u64> below;
    DevMem<u32> rep_of, cluster_of;                                          // the run's result
};
bool cluster_algo_plain(int algo) { return algo != LZANI_CLUSTER_SET_COVER && algo != LZANI_CLUSTER_COMPLETE && algo != LZANI_CLUSTER_LEIDEN; }
int cluster_stage_alloc(lzani_ctx* c, int algo, StageWork& s)
{
    const u32 n = c->cl.info.n;
    if (cluster_algo_plain(algo)) { HIPCHK(c, s.parent.alloc(n)); HIPCHK(c, s.state.alloc(n)); HIPCHK(c, s.blocked.alloc(n)); HIPCHK(c, s.best.alloc(n)); }
    HIPCHK(c, s.flag.alloc(n)); HIPCHK(c, s.size.alloc(n)); HIPCHK(c, s.below.alloc((size_t)n + 1));
    HIPCHK(c, s.counters.alloc(CL_COUNTERS)); HIPCHK(c, s.undecided.alloc(CL_BATCH));
    HIPCHK(c, s.rep_of.alloc(n)); HIPCHK(c, s.cluster_of.alloc(n));
    return LZANI_OK;
}

// The run on the context's edges: fills sw.rep_of, sw.cluster_of and the run's part of `info` (set cover: `cover`, from `work`;
// complete linkage: `link`, from `lwork`).  It allocates nothing.
int cluster_run_stage(lzani_ctx* c, int algo, StageWork& sw, lzani_cluster_info& info, CoverWork& work,
                      lzani_cluster_cover_info& cover, LinkWork& lwork, lzani_cluster_link_info& link, LeidenWork& ldwork,
                      lzani_cluster_leiden_info& leiden)
{
    const Cluster& k = c->cl;
    const u32 n = k.info.n;
    const u64 E = k.info.edges;
    const lzani_cluster_edge* edges = k.edges.get();
    const bool set_cover = algo == LZANI_CLUSTER_SET_COVER, complete = algo == LZANI_CLUSTER_COMPLETE, is_leiden = algo == LZANI_CLUSTER_LEIDEN;
    const bool plain = cluster_algo_plain(algo);
    DevMem<u32>&parent = sw.parent, &state = sw.state, &blocked = sw.blocked, &flag = sw.flag, &size = sw.size, &counters = sw.counters, &undecided = sw.undecided;
    DevMem<unsigned long long>& best = sw.best;
    DevMem<u64>& below = sw.below;
    DevMem<u32>&rep_of = sw.rep_of, &cluster_of = sw.cluster_of;
    const dim3 nodes(pf_blocks(n)), edge_blocks(pf_blocks(E)), threads(PF_THREADS);
    StreamSpan span;
    HIPCHK(c, span.begin(c->stream));
    HIPCHK(c, hipMemsetAsync(counters, 0, CL_COUNTERS * sizeof(u32), c->stream));
    if (plain) hipLaunchKernelGGL(k_cl_init, nodes, threads, 0, c->stream, n, parent.get(), state.get(), blocked.get(), best.get(), size.get());
    u64 rounds = 1;
    if (set_cover) {
        StreamSpan dedup, cover_rounds;
        u64 D = 0;
        HIPCHK(c, dedup.begin(c->stream));
        if (int rc = cluster_cover_dedup(c, work, D)) return rc;
        HIPCHK(c, dedup.end(c->stream));
        HIPCHK(c, cover_rounds.begin(c->stream));
        hipLaunchKernelGGL(k_cl_cover_init, nodes, threads, 0, c->stream, n, rep_of.get(), work.cnt.get(), size.get());
        if (int rc = cluster_cover_rounds(c, work, D, rep_of.get(), undecided.get(), rounds)) return rc;
        HIPCHK(c, cover_rounds.end(c->stream));
        float dedup_ms = 0, rounds_ms = 0;
        HIPCHK(c, dedup.elapsed(dedup_ms));
        HIPCHK(c, cover_rounds.elapsed(rounds_ms));
        cover = lzani_cluster_cover_info{D, E - D, work.bytes(), dedup_ms, rounds_ms};
    } else if (complete) {
        StreamSpan link_rounds;
        u64 merges = 0, D = 0;
        float dedup_ms = 0, rounds_ms = 0;
        HIPCHK(c, link_rounds.begin(c->stream));
        hipLaunchKernelGGL(k_cl_link_init, nodes, threads, 0, c->stream, n, lwork.label.get(), lwork.csize.get(), rep_of.get(), size.get());
        if (int rc = cluster_link_rounds(c, lwork, rep_of.get(), rounds, merges, D, dedup_ms)) return rc;
        HIPCHK(c, link_rounds.end(c->stream));
        HIPCHK(c, link_rounds.elapsed(rounds_ms));
        link = lzani_cluster_link_info{D, E - D, merges, lwork.S, lwork.bytes(), dedup_ms, rounds_ms};
    } else if (is_leiden) {
        hipLaunchKernelGGL(k_ld_init, nodes, threads, 0, c->stream, n, rep_of.get(), size.get());
        if (int rc = cluster_leiden_rounds(c, ldwork, rep_of.get(), leiden)) return rc;
        rounds = leiden.move_rounds + leiden.refine_rounds;
    } else if (algo == LZANI_CLUSTER_SINGLE) {
        if (E) hipLaunchKernelGGL(k_cl_hook, edge_blocks, threads, 0, c->stream, edges, E, parent.get());
        hipLaunchKernelGGL(k_cl_roots, nodes, threads, 0, c->stream, n, (const u32*)parent.get(), rep_of.get());
    } else {
        rounds = 0;
        for (bool done = false; !done;) {
            // the lowest undecided node is decided in every round: n rounds always do, and a defect ends here instead of spinning
            if (rounds >= (u64)n + 1) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: nodes still undecided after n + 1 rounds");
            const u32 batch = (u32)std::min<u64>(CL_BATCH, (u64)n + 1 - rounds);
            HIPCHK(c, hipMemsetAsync(undecided, 0, CL_BATCH * sizeof(u32), c->stream));
            for (u32 r = 0; r < batch; ++r) {
                if (E) hipLaunchKernelGGL(k_cl_greedy_edges, edge_blocks, threads, 0, c->stream, edges, E, state.get(), blocked.get());
                hipLaunchKernelGGL(k_cl_greedy_nodes, nodes, threads, 0, c->stream, n, state.get(), blocked.get(), undecided.get() + r);
            }
            HIPCHK(c, hipGetLastError());
            u32 left[CL_BATCH];
            HIPCHK(c, hipMemcpyAsync(left, undecided, sizeof left, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            u32 r = 0;
            while (r < batch && left[r]) ++r;
            done = r < batch;
            rounds += done ? r + 1 : batch;             // (the rounds behind the first that left no node change nothing)
        }
        hipLaunchKernelGGL(k_cl_assign_init, nodes, threads, 0, c->stream, n, (const u32*)state.get(), rep_of.get());
        if (E && algo == LZANI_CLUSTER_GREEDY_BEST)
            hipLaunchKernelGGL(k_cl_assign_best, edge_blocks, threads, 0, c->stream, edges, E, (const u32*)state.get(), best.get());
        if (E) hipLaunchKernelGGL(k_cl_assign_min, edge_blocks, threads, 0, c->stream, edges, E, (const u32*)state.get(),
                                  algo == LZANI_CLUSTER_GREEDY_BEST ? (const unsigned long long*)best.get() : nullptr, rep_of.get());
    }
    hipLaunchKernelGGL(k_cl_flags, nodes, threads, 0, c->stream, n, (const u32*)rep_of.get(), flag.get(), size.get());
    hipLaunchKernelGGL(k_pf_scan, dim3(1), dim3(1024), 0, c->stream, (const u32*)flag.get(), (u64)n, below.get());
    hipLaunchKernelGGL(k_cl_number, nodes, threads, 0, c->stream, n, (const u32*)rep_of.get(), (const u64*)below.get(), (const u32*)size.get(),
                       cluster_of.get(), counters.get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, span.end(c->stream));
    u32 h_counters[CL_COUNTERS] = {0, 0};
    u64 clusters = 0;
    HIPCHK(c, hipMemcpyAsync(h_counters, counters, sizeof h_counters, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&clusters, below.get() + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    HIPCHK(c, span.elapsed(ms));
    info.algo = algo; info.rounds = (u32)rounds; info.clusters = clusters; info.singletons = h_counters[CL_SINGLETONS];
    info.largest = h_counters[CL_LARGEST]; info.run_ms = ms;
    TRACE("cluster: algo=%d n=%u edges=%llu rounds=%llu clusters=%llu", algo, n, (unsigned long long)E, (unsigned long long)rounds, (unsigned long long)clusters);
    return LZANI_OK;
}

}  // namespace

extern "C" {

double lzani_cluster_weight(int measure, const lzani_result* x, const lzani_result* y, uint32_t lines, uint32_t len_a, uint32_t len_b)
{
    if (!x || !y || !cluster_measure_known(measure)) return __builtin_nan("");
    return cluster_weight(measure, *x, *y, lines, len_a, len_b);
}

int lzani_cluster_host(uint32_t n, const lzani_cluster_edge* edges, uint64_t count, int algo, uint32_t* rep_of, uint32_t* cluster_of, uint32_t* n_clusters)
{
    try { return cluster_host(n, edges, count, algo, rep_of, cluster_of, n_clusters); }
    catch (const std::bad_alloc&) { return LZANI_ERR_NOMEM; }
}

// the edges checked as cluster_host checks them, then Leiden with its parameters and the numbering
static int cluster_leiden_host_call(uint32_t n, const lzani_cluster_edge* edges, uint64_t count, double resolution, int iterations, uint64_t cap_mul,
                                    uint64_t cap_add, uint32_t* rep_of, uint32_t* cluster_of, lzani_cluster_leiden_info* info)
{
    if (!rep_of || (count && !edges)) return LZANI_ERR_ARG;
    for (uint64_t i = 0; i < count; ++i)
        if (!cluster_edge_ok(n, edges[i])) return LZANI_ERR_ARG;
    try {
        if (int rc = cluster_leiden_host(n, edges, count, resolution, iterations, rep_of, info, cap_mul, cap_add)) return rc;
        cluster_number(n, rep_of, cluster_of);
        return LZANI_OK;
    } catch (const std::bad_alloc&) { return LZANI_ERR_NOMEM; }
}

int lzani_cluster_leiden_host(uint32_t n, const lzani_cluster_edge* edges, uint64_t count, double resolution, int iterations, uint32_t* rep_of,
                              uint32_t* cluster_of, lzani_cluster_leiden_info* info)
{
    return cluster_leiden_host_call(n, edges, count, resolution, iterations, CL_LEIDEN_CAP_MUL, CL_LEIDEN_CAP_ADD, rep_of, cluster_of, info);
}

int lzani_debug_cluster_leiden_host_cap(uint32_t n, const lzani_cluster_edge* edges, uint64_t count, double resolution, int iterations, uint64_t cap_mul,
                                        uint64_t cap_add, uint32_t* rep_of, uint32_t* cluster_of, lzani_cluster_leiden_info* info)
{
    return cluster_leiden_host_call(n, edges, count, resolution, iterations, cap_mul, cap_add, rep_of, cluster_of, info);
}

int lzani_set_cluster_leiden(lzani_ctx* c, double resolution, int iterations)
{
    if (!c) return LZANI_ERR_ARG;
    if (!cluster_leiden_params_ok(resolution, iterations))
        return fail(c, LZANI_ERR_ARG, "lzani_set_cluster_leiden: the resolution lies in [0, 1], the iterations in 1..16");
    c->leiden_resolution = resolution; c->leiden_iterations = iterations;
    return LZANI_OK;
}

int lzani_cluster_begin(lzani_ctx* c, uint32_t n, const uint32_t* report_len, int measure)
{
    if (!c) return LZANI_ERR_ARG;
    const std::string fn = "lzani_cluster_begin";
    if (!c->gs.n) return fail(c, LZANI_ERR_STATE, fn + ": no genomes set");
    if (!n || !cluster_measure_known(measure)) return fail(c, LZANI_ERR_ARG, fn + ": no genomes or an unknown measure");
    if (!report_len && n != c->gs.n) return fail(c, LZANI_ERR_ARG, fn + ": the genome set's own lengths are those of its n genomes");
    std::vector<u32> own;
    if (!report_len) { own = kept_own_lengths(c); report_len = own.data(); }
    HIPCHK(c, hipSetDevice(c->dev));
    c->cl = Cluster{};                                         // the last state goes first
    Cluster k;
    HIPCHK(c, k.len.alloc(n));
    HIPCHK(c, hipMemcpyAsync(k.len.get(), report_len, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    k.info.n = n; k.info.measure = measure; k.info.algo = -1;
    k.begun = true;
    c->cl = std::move(k);
    return LZANI_OK;
}

int lzani_cluster_add_kept(lzani_ctx* c, uint64_t* edges_total)
{
    if (!c) return LZANI_ERR_ARG;
    const std::string fn = "lzani_cluster_add_kept";
    if (int rc = cluster_state(c, fn)) return rc;
    if (!c->kept.done) return fail(c, LZANI_ERR_STATE, fn + ": no kept result (call lzani_run_rows_kept first)");
    Cluster& k = c->cl;
    if (c->kept.n != k.info.n) return fail(c, LZANI_ERR_ARG, fn + ": the kept result is one of " + std::to_string(c->kept.n) + " genomes, the cluster state of " + std::to_string(k.info.n));
    const u64 K = c->kept.info.kept_pairs;                     // the buffer's need, known before the kernel runs
    HIPCHK(c, hipSetDevice(c->dev));
    if (int rc = cluster_reserve(c, k.info.edges + K)) return rc;
    if (K) {
        StreamSpan span;
        HIPCHK(c, span.begin(c->stream));
        hipLaunchKernelGGL(k_cl_add_kept, dim3(pf_blocks(K)), dim3(PF_THREADS), 0, c->stream, (const u32*)c->kept.rec.get(), K, (const u32*)k.len.get(),
                           (int)k.info.measure, k.edges.get(), k.info.edges);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, span.end(c->stream));
        float ms = 0;
        HIPCHK(c, span.elapsed(ms));
        k.info.add_ms += ms;
        k.info.edges += K;
        k.ran = false;
    }
    if (edges_total) *edges_total = k.info.edges;
    return LZANI_OK;
}

int lzani_debug_cluster_add_edges(lzani_ctx* c, const lzani_cluster_edge* edges, uint64_t count)
{
    if (!c) return LZANI_ERR_ARG;
    const std::string fn = "lzani_debug_cluster_add_edges";
    if (int rc = cluster_state(c, fn)) return rc;
    if (count && !edges) return fail(c, LZANI_ERR_ARG, fn + ": null edges");
    Cluster& k = c->cl;
    std::vector<lzani_cluster_edge> norm(edges, edges + count);
    for (lzani_cluster_edge& e : norm) {
        if (!cluster_edge_ok(k.info.n, e)) return fail(c, LZANI_ERR_ARG, fn + ": an edge with a == b, an id out of range, or a weight that is negative or not a number");
        if (e.a > e.b) std::swap(e.a, e.b);
        e.w = cluster_value(e.w);
    }
    if (!count) return LZANI_OK;
    HIPCHK(c, hipSetDevice(c->dev));
    if (int rc = cluster_reserve(c, k.info.edges + count)) return rc;
    HIPCHK(c, hipMemcpyAsync(k.edges.get() + k.info.edges, norm.data(), (size_t)count * sizeof(lzani_cluster_edge), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    k.info.edges += count;
    k.ran = false;
    return LZANI_OK;
}

int lzani_cluster_run(lzani_ctx* c, int algo, uint64_t* n_clusters)
{
    if (!c) return LZANI_ERR_ARG;
    const std::string fn = "lzani_cluster_run";
    if (int rc = cluster_state(c, fn)) return rc;
    if (!cluster_algo_known(algo)) return fail(c, LZANI_ERR_ARG, fn + ": unknown algorithm");
    HIPCHK(c, hipSetDevice(c->dev));
    Cluster& k = c->cl;
    CoverWork work;                                            // set cover: refused, or short of memory, with the state as it was
    if (algo == LZANI_CLUSTER_SET_COVER)
        if (int rc = cluster_cover_alloc(c, work)) return rc;
    LinkWork lwork;                                            // complete linkage: the same
    if (algo == LZANI_CLUSTER_COMPLETE)
        if (int rc = cluster_link_alloc(c, lwork)) return rc;
    LeidenWork ldwork;                                         // Leiden: the same
    if (algo == LZANI_CLUSTER_LEIDEN)
        if (int rc = cluster_leiden_alloc(c, ldwork)) return rc;
    StageWork sw;                                              // every algorithm: the same
    if (int rc = cluster_stage_alloc(c, algo, sw)) return rc;
    k.ran = false;
    k.rep_of.reset(); k.cluster_of.reset();                    // the last run's result goes before the run, not before its memory is had
    lzani_cluster_info info = k.info;
    lzani_cluster_cover_info cover{};
    lzani_cluster_link_info link{};
    lzani_cluster_leiden_info leiden{};
    const int rc = cluster_run_stage(c, algo, sw, info, work, cover, lwork, link, ldwork, leiden);
    if (rc != LZANI_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    k.info = info;
    k.cover = cover;
    k.link = link;
    k.leiden = leiden;
    k.rep_of = std::move(sw.rep_of); k.cluster_of = std::move(sw.cluster_of);
    k.ran = true;
    if (n_clusters) *n_clusters = info.clusters;
    return LZANI_OK;
}

int lzani_cluster_fetch(lzani_ctx* c, uint32_t* rep_of, uint32_t* cluster_of)
{
    if (!c) return LZANI_ERR_ARG;
    const std::string fn = "lzani_cluster_fetch";
    if (int rc = cluster_state(c, fn)) return rc;
    const Cluster& k = c->cl;
    if (!k.ran) return fail(c, LZANI_ERR_STATE, fn + ": no run since the begin or the last added edges (call lzani_cluster_run first)");
    HIPCHK(c, hipSetDevice(c->dev));
    if (rep_of) HIPCHK(c, hipMemcpy(rep_of, k.rep_of.get(), (size_t)k.info.n * 4, hipMemcpyDeviceToHost));
    if (cluster_of) HIPCHK(c, hipMemcpy(cluster_of, k.cluster_of.get(), (size_t)k.info.n * 4, hipMemcpyDeviceToHost));
    return LZANI_OK;
}

int lzani_get_cluster_info(const lzani_ctx* c, lzani_cluster_info* info)
{
    if (!c || !info) return LZANI_ERR_ARG;
    if (!c->cl.begun) return LZANI_ERR_STATE;
    *info = c->cl.info;
    return LZANI_OK;
}

int lzani_get_cluster_cover_info(const lzani_ctx* c, lzani_cluster_cover_info* info)
{
    if (!c || !info) return LZANI_ERR_ARG;
    if (!c->cl.begun || c->cl.info.algo != LZANI_CLUSTER_SET_COVER) return LZANI_ERR_STATE;
    *info = c->cl.cover;
    return LZANI_OK;
}

int lzani_get_cluster_link_info(const lzani_ctx* c, lzani_cluster_link_info* info)
{
    if (!c || !info) return LZANI_ERR_ARG;
    if (!c->cl.begun || c->cl.info.algo != LZANI_CLUSTER_COMPLETE) return LZANI_ERR_STATE;
    *info = c->cl.link;
    return LZANI_OK;
}

int lzani_get_cluster_leiden_info(const lzani_ctx* c, lzani_cluster_leiden_info* info)
{
    if (!c || !info) return LZANI_ERR_ARG;
    if (!c->cl.begun || c->cl.info.algo != LZANI_CLUSTER_LEIDEN) return LZANI_ERR_STATE;
    *info = c->cl.leiden;
    return LZANI_OK;
}

}  // extern "C"
