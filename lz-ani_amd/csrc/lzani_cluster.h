// lzani_cluster.h -- host side of the cluster stage (include/lzani.h states the definitions): the edge buffer and its growth
// (cluster_reserve); ClusterStage, what every run works in and leaves (flag, size, below, the counters, a batch's round
// words, rep_of, cluster_of, rounds); the helpers the units share -- cluster_rounds (rounds launched in batches between two
// reads of their words: the one place of that arithmetic), cluster_compact (count pass, k_pf_scan, write pass),
// cluster_table_slots, cluster_table_clear and CL_ALLOC (a workspace buffer, counted into the unit's bytes as it is had) --;
// one unit per family of algorithms -- PlainUnit (SINGLE and the greedy forms), CoverUnit, LinkUnit, LeidenUnit --, each with
// its device buffers, alloc(c) with its limits and refusals, run(c, stage), which fills stage.rep_of and stage.rounds, and
// `info`, its own info struct (PlainUnit: none); cluster_run_stage (span and counters, the unit's run, the numbering) and
// cluster_run_as<Unit> (the unit, then the stage, allocated whole before the cluster state is touched); and the entry points
// (lzani_cluster_begin, lzani_cluster_add_kept, lzani_debug_cluster_add_edges, lzani_cluster_run -- the one choice of a unit
// by `algo` --, lzani_cluster_fetch, lzani_get_cluster_info, lzani_get_cluster_cover_info, lzani_get_cluster_link_info,
// lzani_set_cluster_leiden, lzani_get_cluster_leiden_info and the pure lzani_cluster_weight, lzani_cluster_host and
// lzani_cluster_leiden_host); and the cluster levels -- the record store of the context (cluster_store_reserve,
// cluster_store_append: a device copy behind a growth step), the level's edges (cluster_level_run: count pass, scan, write
// pass of k_cl_level into a fresh cluster state) and their entry points (lzani_cluster_store_begin,
// lzani_cluster_store_add_kept, lzani_debug_cluster_store_add, lzani_cluster_level, lzani_debug_cluster_edges,
// lzani_get_cluster_store_info, lzani_get_cluster_level_info and the pure lzani_cluster_cut_lines).  A further algorithm is one more unit and one more case in lzani_cluster_run.
// Included by lzani_hip.hip only, behind lzani_kept.h; of that file it uses lzani_ctx (which holds the Cluster and the Kept),
// fail, HIPCHK and sort_keys, of lzani_prefilter.h pf_blocks and pf_chunks, of lzani_devmem.h DevMem and StreamSpan.  The
// kernels are lzani_kernels_cluster.h; the group's form is in lzani_multi.h.
//
// What the stage reads and writes.  add_kept, per record: 36 B and two lengths read, 16 B written.  A level, per record of
// the store: 36 B and two lengths read by either pass, and per edge 16 B written; the store's append: 36 B copied.  SINGLE: per edge 16 B
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

enum { CL_BATCH = 8 };                                  // greedy and set-cover rounds launched between two reads of their words
constexpr u64 CL_MAX_EDGES = 0xFFFFFFEFull;             // 2^32 - 17: lzani_sort_keys' limit, and that of the units with a workspace

int cluster_state(lzani_ctx* c, const std::string& fn)
{
    if (!c->cl.begun) return fail(c, LZANI_ERR_STATE, fn + ": no cluster state (call lzani_cluster_begin first)");
    return LZANI_OK;
}

// whether one launch of a thread per item covers `items` edges or records: the one statement of that limit
bool cluster_launch_covers(u64 items) { return (items + PF_THREADS - 1) / PF_THREADS <= 0x7FFFFFFFull; }

// Room for `need` edges: kept if there is, else a buffer of at least twice the size, the edges copied on the device.  A
// failure leaves the buffer and its edges as they were.
int cluster_reserve(lzani_ctx* c, u64 need)
{
    Cluster& k = c->cl;
    if (!cluster_launch_covers(need)) return fail(c, LZANI_ERR_ARG, "cluster stage: more edges than one launch covers");
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

// What every algorithm's run works in, and what it leaves.  Like the units' workspaces it is allocated whole before the run
// touches the cluster state.
struct ClusterStage {
    int algo = 0;
    u64 rounds = 1;                                     // the unit's run says
    DevMem<u32> flag, size, counters, undecided;        // undecided: a word per round of a batch (the greedy forms, set cover)
    DevMem<u64> below;
    DevMem<u32> rep_of, cluster_of;                     // the run's result
    int alloc(lzani_ctx* c)
    {
        const u32 n = c->cl.info.n;
        HIPCHK(c, flag.alloc(n)); HIPCHK(c, size.alloc(n)); HIPCHK(c, below.alloc((size_t)n + 1));
        HIPCHK(c, counters.alloc(CL_COUNTERS)); HIPCHK(c, undecided.alloc(CL_BATCH));
        HIPCHK(c, rep_of.alloc(n)); HIPCHK(c, cluster_of.alloc(n));
        return LZANI_OK;
    }
};

// One buffer of a unit's workspace: its own allocation and its own attempt, counted into the unit's `bytes` as it is had, so
// that `count` is the one statement of its size.
#define CL_ALLOC(buf, count) do { HIPCHK(c, buf.alloc(count)); bytes += buf.bytes(); } while (0)

// Rounds launched `batch` at a time between two reads of their words: round r of a batch leaves words[first + r] != 0 while
// there is more to do, and a round behind the first that left 0 changes nothing.  More than `cap` rounds: `still`.
struct ClRounds {
    u32 batch;
    u64 cap;
    const char* still;
    u32* words;                                        // `count` of them, cleared before every batch and read back whole
    u32 count, first;
};
// launch(r) launches round r of a batch; seen(words, r, last) is given every batch's words on the host, the number r of its
// rounds that had more to do and the index of the last that counts.  rounds: up to the first that left 0, that one included.
template <class Launch, class Seen = int (*)(const u32*, u32, u32)>
int cluster_rounds(lzani_ctx* c, const ClRounds& p, u64& rounds, Launch launch, Seen seen = [](const u32*, u32, u32) { return (int)LZANI_OK; })
{
    u32 words[CL_LD_CTL];
    static_assert(CL_LD_CTL >= CL_BATCH, "the host copy holds either family's words");
    rounds = 0;
    for (bool done = false; !done;) {
        if (rounds >= p.cap) return fail(c, LZANI_ERR_DEVICE, p.still);      // a defect ends here instead of spinning
        const u32 batch = (u32)std::min<u64>(p.batch, p.cap - rounds);
        HIPCHK(c, hipMemsetAsync(p.words, 0, p.count * sizeof(u32), c->stream));
        for (u32 r = 0; r < batch; ++r) HIPCHK(c, launch(r));
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(words, p.words, p.count * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        u32 r = 0;
        while (r < batch && words[p.first + r]) ++r;
        done = r < batch;
        rounds += done ? r + 1 : batch;
        if (int rc = seen(words, r, done ? r : batch - 1)) return rc;
    }
    return LZANI_OK;
}

// The kept ones of `items` into a list: pass(std::false_type, chunks) launches the count pass over `chunks` blocks,
// k_pf_scan makes the blocks' offsets, pass(std::true_type, chunks) writes.  Returns where the total is, on the device.
template <class Pass>
const u64* cluster_compact(lzani_ctx* c, u64 items, u32* ucnt, u64* uoff, Pass pass)
{
    const u32 chunks = (u32)pf_chunks(items);
    pass(std::false_type{}, chunks);
    hipLaunchKernelGGL(k_pf_scan, dim3(1), dim3(1024), 0, c->stream, ucnt, (u64)chunks, uoff);
    pass(std::true_type{}, chunks);
    return uoff + chunks;
}

// ---- the record store of the cluster levels, and a level's edges ----
int cluster_store_state(lzani_ctx* c, const std::string& fn)
{
    if (!c->cls.begun) return fail(c, LZANI_ERR_STATE, fn + ": no record store (call lzani_cluster_store_begin first)");
    return LZANI_OK;
}
// Room for `need` records: kept if there is, else a buffer of at least twice the size, the records copied on the device.  A
// failure leaves the buffer and its records as they were.
int cluster_store_reserve(lzani_ctx* c, u64 need)
{
    ClusterStore& s = c->cls;
    if (9 * need <= s.rec.capacity()) return LZANI_OK;
    DevMem<u32> bigger;
    const u64 twice = std::max<u64>(9 * need, 2 * (u64)s.rec.capacity());
    if (!got(bigger.alloc((size_t)twice))) HIPCHK(c, bigger.alloc((size_t)(9 * need)));
    if (s.info.records) {
        HIPCHK(c, hipMemcpyAsync(bigger.get(), s.rec.get(), (size_t)s.info.records * 36, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    s.rec = std::move(bigger);
    s.info.record_bytes = s.rec.bytes();
    return LZANI_OK;
}
// `count` records from `src` (device or host memory, by `kind`) behind the store's: the growth step, then the copy
int cluster_store_append(lzani_ctx* c, const u32* src, u64 count, hipMemcpyKind kind)
{
    ClusterStore& s = c->cls;
    if (int rc = cluster_store_reserve(c, s.info.records + count)) return rc;
    if (!count) return LZANI_OK;
    StreamSpan span;
    HIPCHK(c, span.begin(c->stream));
    HIPCHK(c, hipMemcpyAsync(s.rec.get() + 9 * s.info.records, src, (size_t)count * 36, kind, c->stream));
    HIPCHK(c, span.end(c->stream));
    float ms = 0;
    HIPCHK(c, span.elapsed(ms));
    s.info.add_ms += ms;
    s.info.records += count;
    return LZANI_OK;
}

// The level's edges of the store's records into the fresh cluster state `k`: count pass, k_pf_scan, the exact total read
// back, the edge buffer at that size, write pass -- cluster_compact's three launches with the read-back and the allocation
// between the second and the third, hence launched here one by one.  level_ms runs from the count pass to the write pass,
// that read-back and allocation included.  Everything it allocates is its own or k's.
int cluster_level_run(lzani_ctx* c, Cluster& k, int measure, const lzani_cluster_cut& cut)
{
    const ClusterStore& s = c->cls;
    const u32 n = s.info.n;
    const u64 R = s.info.records, chunks = pf_chunks(R);
    HIPCHK(c, k.len.alloc(n));
    HIPCHK(c, hipMemcpyAsync(k.len.get(), s.len.get(), (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream));
    k.info.n = n; k.info.measure = measure; k.info.algo = -1;
    k.from_level = true;
    k.level.records_in = R;
    DevMem<u32> ucnt;
    DevMem<u64> uoff;
    DevMem<unsigned long long> counters;
    HIPCHK(c, ucnt.alloc((size_t)chunks));
    HIPCHK(c, uoff.alloc((size_t)chunks + 1));
    HIPCHK(c, counters.alloc(CL_LV_COUNTERS));
    u64 total = 0;
    unsigned long long h_counters[CL_LV_COUNTERS] = {0, 0};
    StreamSpan span;
    HIPCHK(c, span.begin(c->stream));
    if (R) {
        HIPCHK(c, hipMemsetAsync(counters, 0, CL_LV_COUNTERS * sizeof(unsigned long long), c->stream));
        hipLaunchKernelGGL(k_cl_level<false>, dim3((u32)chunks), dim3(PF_THREADS), 0, c->stream, s.rec.get(), R, k.len.get(), cut, measure, ucnt.get(),
                           (const u64*)uoff.get(), (lzani_cluster_edge*)nullptr, counters.get());
        hipLaunchKernelGGL(k_pf_scan, dim3(1), dim3(1024), 0, c->stream, (const u32*)ucnt.get(), chunks, uoff.get());
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&total, uoff.get() + chunks, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(h_counters, counters, sizeof h_counters, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (total > R) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_level: more edges than records");
    }
    HIPCHK(c, k.edges.alloc((size_t)total));                   // the exact size, known before the buffer is made
    k.info.edge_bytes = k.edges.bytes();
    if (total) {
        hipLaunchKernelGGL(k_cl_level<true>, dim3((u32)chunks), dim3(PF_THREADS), 0, c->stream, s.rec.get(), R, k.len.get(), cut, measure, ucnt.get(),
                           (const u64*)uoff.get(), k.edges.get(), counters.get());
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, span.end(c->stream));
    float ms = 0;
    HIPCHK(c, span.elapsed(ms));
    k.info.edges = total;
    k.level.edges_out = total; k.level.lines_in = h_counters[CL_LV_LINES_IN]; k.level.lines_out = h_counters[CL_LV_LINES_OUT]; k.level.level_ms = ms;
    TRACE("cluster level: measure=%d records=%llu edges=%llu lines %llu -> %llu", measure, (unsigned long long)R, (unsigned long long)total,
          h_counters[CL_LV_LINES_IN], h_counters[CL_LV_LINES_OUT]);
    return LZANI_OK;
}

// the slots of a table of `insertions`: the smallest power of two >= 2 * insertions (1 for none)
u64 cluster_table_slots(u64 insertions)
{
    u64 S = 1;
    while (S < 2 * insertions) S <<= 1;
    return S;
}

struct ClFill { unsigned long long* words; int byte; };
// A round's table cleared: S keys all ones, and S words of every other array of `byte` bytes.
hipError_t cluster_table_clear(lzani_ctx* c, u64 S, unsigned long long* key, std::initializer_list<ClFill> others)
{
    hipError_t e = hipMemsetAsync(key, 0xFF, (size_t)S * 8, c->stream);
    for (const ClFill& f : others)
        if (e == hipSuccess) e = hipMemsetAsync(f.words, f.byte, (size_t)S * 8, c->stream);
    return e;
}

// SINGLE (union-find) and the greedy forms (rounds of representatives, then the assignment).
struct PlainUnit {
    DevMem<u32> parent, state, blocked;
    DevMem<unsigned long long> best;
    std::monostate info;
    int alloc(lzani_ctx* c)
    {
        const u32 n = c->cl.info.n;
        HIPCHK(c, parent.alloc(n)); HIPCHK(c, state.alloc(n)); HIPCHK(c, blocked.alloc(n)); HIPCHK(c, best.alloc(n));
        return LZANI_OK;
    }
    int run(lzani_ctx* c, ClusterStage& st)
    {
        const u32 n = c->cl.info.n;
        const u64 E = c->cl.info.edges;
        const lzani_cluster_edge* edges = c->cl.edges;
        const dim3 nodes(pf_blocks(n)), edge_blocks(pf_blocks(E)), threads(PF_THREADS);
        hipLaunchKernelGGL(k_cl_init, nodes, threads, 0, c->stream, n, parent, state, blocked, best, st.size);
        if (st.algo == LZANI_CLUSTER_SINGLE) {
            if (E) hipLaunchKernelGGL(k_cl_hook, edge_blocks, threads, 0, c->stream, edges, E, parent);
            hipLaunchKernelGGL(k_cl_roots, nodes, threads, 0, c->stream, n, parent, st.rep_of);
            return LZANI_OK;
        }
        // the lowest undecided node is decided in every round: n rounds always do
        const ClRounds p{CL_BATCH, (u64)n + 1, "lzani_cluster_run: nodes still undecided after n + 1 rounds", st.undecided, CL_BATCH, 0};
        auto round = [&](u32 r) {
            if (E) hipLaunchKernelGGL(k_cl_greedy_edges, edge_blocks, threads, 0, c->stream, edges, E, state, blocked);
            hipLaunchKernelGGL(k_cl_greedy_nodes, nodes, threads, 0, c->stream, n, state, blocked, st.undecided.get() + r);
            return hipSuccess;
        };
        if (int rc = cluster_rounds(c, p, st.rounds, round)) return rc;
        const bool by_weight = st.algo == LZANI_CLUSTER_GREEDY_BEST;
        hipLaunchKernelGGL(k_cl_assign_init, nodes, threads, 0, c->stream, n, state, st.rep_of);
        if (E && by_weight) hipLaunchKernelGGL(k_cl_assign_best, edge_blocks, threads, 0, c->stream, edges, E, state, best);
        if (E) hipLaunchKernelGGL(k_cl_assign_min, edge_blocks, threads, 0, c->stream, edges, E, state, by_weight ? best.get() : nullptr, st.rep_of);
        return LZANI_OK;
    }
};

// Set cover.  The workspace: the keys of the edge records and of the distinct edges (two buffers of E, the sort's in and out
// in turn), the sort's scratch, the compaction's block counts and offsets, and per node the counter and the three 64-bit
// words of a round.
struct CoverUnit {
    DevMem<unsigned long long> ka, kb, key, m1, m2;
    DevMem<unsigned char> scratch;
    DevMem<u32> ucnt, cnt;
    DevMem<u64> uoff;
    int bits = 1;                                       // of an id below n
    u64 bytes = 0;
    lzani_cluster_cover_info info{};
    int alloc(lzani_ctx* c)
    {
        const u32 n = c->cl.info.n;
        const u64 E = c->cl.info.edges;
        if (E > CL_MAX_EDGES) return fail(c, LZANI_ERR_ARG, "lzani_cluster_run: set cover sorts at most 2^32 - 17 edge records");
        while (bits < 32 && ((u64)1 << bits) < n) ++bits;
        size_t need = 0;                                // (the same for the two sorts: as many bits, as many keys)
        if (int rc = sort_scratch_bytes(c, (size_t)E, 1, 0, bits, "lzani_cluster_run: sort", need)) return rc;
        CL_ALLOC(ka, (size_t)E); CL_ALLOC(kb, (size_t)E); CL_ALLOC(scratch, need);
        CL_ALLOC(ucnt, (size_t)pf_chunks(E)); CL_ALLOC(uoff, (size_t)pf_chunks(E) + 1);
        CL_ALLOC(cnt, n); CL_ALLOC(key, n); CL_ALLOC(m1, n); CL_ALLOC(m2, n);
        return LZANI_OK;
    }
    // The distinct edges of the context's edge records, ascending, in kb: D of them.  The edge buffer is only read.
    int dedup(lzani_ctx* c, u64& D)
    {
        const u64 E = c->cl.info.edges;
        D = 0;
        if (!E) return LZANI_OK;
        hipLaunchKernelGGL(k_cl_cover_keys, dim3(pf_blocks(E)), dim3(PF_THREADS), 0, c->stream, c->cl.edges, E, ka);
        HIPCHK(c, hipGetLastError());
        // by hi, then (the sort is stable) by lo: only the bits an id below n has
        if (int rc = sort_keys(c, scratch, ka, kb, (size_t)E, 1, 0, bits, "lzani_cluster_run: sort", false)) return rc;
        if (int rc = sort_keys(c, scratch, kb, ka, (size_t)E, 1, 32, 32 + bits, "lzani_cluster_run: sort", false)) return rc;
        const u64* total = cluster_compact(c, E, ucnt, uoff, [&](auto write, u32 chunks) {
            hipLaunchKernelGGL(k_pf_uniq<decltype(write)::value>, dim3(chunks), dim3(PF_THREADS), 0, c->stream, ka, E, ucnt, uoff, kb, (u32*)nullptr, 0u);
        });
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&D, total, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (D > E) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: more distinct edges than edge records");
        return LZANI_OK;
    }
    // The dedup, then the rounds over the D distinct edges of kb (lzani_kernels_cluster.h): rounds is the number of the first
    // that left no node unassigned.
    int run(lzani_ctx* c, ClusterStage& st)
    {
        const u32 n = c->cl.info.n;
        const dim3 nodes(pf_blocks(n)), threads(PF_THREADS);
        StreamSpan dedup_span, rounds_span;
        u64 D = 0;
        HIPCHK(c, dedup_span.begin(c->stream));
        if (int rc = dedup(c, D)) return rc;
        HIPCHK(c, dedup_span.end(c->stream));
        HIPCHK(c, rounds_span.begin(c->stream));
        hipLaunchKernelGGL(k_cl_cover_init, nodes, threads, 0, c->stream, n, st.rep_of, cnt, st.size);
        const dim3 edge_blocks(pf_blocks(D));
        // the unassigned node with the largest key is selected in every round: n rounds always do
        const ClRounds p{CL_BATCH, (u64)n + 1, "lzani_cluster_run: nodes still unassigned after n + 1 rounds", st.undecided, CL_BATCH, 0};
        auto round = [&](u32 r) {
            if (D) hipLaunchKernelGGL(k_cl_cover_count, edge_blocks, threads, 0, c->stream, kb, D, n, st.rep_of, cnt);
            hipLaunchKernelGGL(k_cl_cover_key, nodes, threads, 0, c->stream, n, st.rep_of, cnt, key, m1, m2);
            if (D) hipLaunchKernelGGL(k_cl_cover_max, edge_blocks, threads, 0, c->stream, kb, D, n, key, m1);
            if (D) hipLaunchKernelGGL(k_cl_cover_max, edge_blocks, threads, 0, c->stream, kb, D, n, m1, m2);
            hipLaunchKernelGGL(k_cl_cover_decide, nodes, threads, 0, c->stream, n, m1, m2, st.rep_of, st.undecided.get() + r);
            return hipSuccess;
        };
        if (int rc = cluster_rounds(c, p, st.rounds, round)) return rc;
        HIPCHK(c, rounds_span.end(c->stream));
        float dedup_ms = 0, rounds_ms = 0;
        HIPCHK(c, dedup_span.elapsed(dedup_ms));
        HIPCHK(c, rounds_span.elapsed(rounds_ms));
        info = lzani_cluster_cover_info{D, c->cl.info.edges - D, bytes, dedup_ms, rounds_ms};
        return LZANI_OK;
    }
};

// Complete linkage.  The workspace: the table of S slots (S for the first round, the largest), the entry list (at most one
// entry per distinct edge), the compaction's block counts and offsets, per cluster label, size, best weight and best id,
// and the round's two control words.
struct LinkUnit {
    DevMem<unsigned long long> tkey, tcnt, tw, lkey, lcnt, lw, bestw;
    DevMem<u32> label, csize, bestid, ucnt, ctl;
    DevMem<u64> uoff;
    u64 S = 1;                                          // of the first round
    u64 bytes = 0;
    lzani_cluster_link_info info{};
    int alloc(lzani_ctx* c)
    {
        const u32 n = c->cl.info.n;
        const u64 E = c->cl.info.edges;
        if (E > CL_MAX_EDGES) return fail(c, LZANI_ERR_ARG, "lzani_cluster_run: complete linkage takes at most 2^32 - 17 edge records");
        S = cluster_table_slots(E);
        CL_ALLOC(tkey, (size_t)S); CL_ALLOC(tcnt, (size_t)S); CL_ALLOC(tw, (size_t)S);
        CL_ALLOC(lkey, (size_t)E); CL_ALLOC(lcnt, (size_t)E); CL_ALLOC(lw, (size_t)E);
        CL_ALLOC(ucnt, (size_t)pf_chunks(S)); CL_ALLOC(uoff, (size_t)pf_chunks(S) + 1);
        CL_ALLOC(label, n); CL_ALLOC(csize, n); CL_ALLOC(bestw, n); CL_ALLOC(bestid, n);
        CL_ALLOC(ctl, CL_LINK_CTL);
        return LZANI_OK;
    }
    // The rounds (lzani_kernels_cluster.h): rounds is the number of the first that merged nothing; the info holds the merges,
    // the distinct edges (the first round's links: every distinct edge is one) and the time of the first insert.
    int run(lzani_ctx* c, ClusterStage& st)
    {
        const u32 n = c->cl.info.n;
        const u64 E = c->cl.info.edges;
        const dim3 nodes(pf_blocks(n)), threads(PF_THREADS);
        u64 L = E;                                      // entries of the round: edge records, then the last round's links
        u64 rounds = 1, merges = 0, D = 0;
        float dedup_ms = 0, rounds_ms = 0;
        StreamSpan span, first;
        HIPCHK(c, span.begin(c->stream));
        hipLaunchKernelGGL(k_cl_link_init, nodes, threads, 0, c->stream, n, label, csize, st.rep_of, st.size);
        for (; L; ++rounds) {                           // (no entry: no link, and the round merges nothing)
            // the link with the largest value merges in every round: n rounds always do, and a defect ends here instead of spinning
            if (rounds > (u64)n + 1) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: links still merging after n + 1 rounds");
            const ClLinkTable t{tkey, tcnt, tw, cluster_table_slots(L)};
            if (t.S > S) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: more link entries than edge records");
            const dim3 slots(pf_blocks(t.S));
            if (rounds == 1) HIPCHK(c, first.begin(c->stream));
            HIPCHK(c, cluster_table_clear(c, t.S, t.key, {{t.w, 0xFF}, {t.cnt, 0}}));
            HIPCHK(c, hipMemsetAsync(ctl, 0, CL_LINK_CTL * sizeof(u32), c->stream));
            hipLaunchKernelGGL(k_cl_link_insert, dim3(pf_blocks(L)), threads, 0, c->stream, rounds == 1 ? c->cl.edges.get() : nullptr, lkey, lcnt, lw, L, n,
                               label, t, ctl);
            if (rounds == 1) HIPCHK(c, first.end(c->stream));
            hipLaunchKernelGGL(k_cl_link_clear, nodes, threads, 0, c->stream, n, bestw, bestid);
            hipLaunchKernelGGL(k_cl_link_bestw, slots, threads, 0, c->stream, t, n, csize, bestw);
            hipLaunchKernelGGL(k_cl_link_bestid, slots, threads, 0, c->stream, t, n, csize, bestw, bestid);
            const u64* total = cluster_compact(c, t.S, ucnt, uoff, [&](auto write, u32 chunks) {
                hipLaunchKernelGGL(k_cl_link_compact<decltype(write)::value>, dim3(chunks), threads, 0, c->stream, t, n, csize, ucnt, uoff, lkey, lcnt, lw);
            });
            hipLaunchKernelGGL(k_cl_link_merge, nodes, threads, 0, c->stream, n, bestid, label, csize, ctl);
            hipLaunchKernelGGL(k_cl_link_relabel, nodes, threads, 0, c->stream, n, label, st.rep_of);
            HIPCHK(c, hipGetLastError());
            u32 h_ctl[CL_LINK_CTL] = {0, 0};
            u64 links = 0;
            HIPCHK(c, hipMemcpyAsync(h_ctl, ctl, sizeof h_ctl, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(&links, total, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (h_ctl[CL_LINK_ERR]) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: the cluster-pair table's probe sequence ran out, or an id out of range");
            if (links > L) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: more links than entries");
            if (rounds == 1) { D = links; HIPCHK(c, first.elapsed(dedup_ms)); }
            if (!h_ctl[CL_LINK_MERGES]) break;
            merges += h_ctl[CL_LINK_MERGES];
            L = links;
        }
        HIPCHK(c, span.end(c->stream));
        HIPCHK(c, span.elapsed(rounds_ms));
        st.rounds = rounds;
        info = lzani_cluster_link_info{D, E - D, merges, S, bytes, dedup_ms, rounds_ms};
        return LZANI_OK;
    }
};

// Leiden.  The workspace: the table of S slots (S for the largest round there can be: 2 * E insertions), the level-0 entry
// list and the working list of the higher levels (at most one entry per distinct edge each), the compaction's block counts
// and offsets, the per-node and per-community words of the rounds (two sets of sizes and partitions: a level and the one
// aggregated from it), and the control words.
struct LeidenUnit {
    DevMem<unsigned long long> tkey, tval, e0key, wkey, bestd, cd, quality;
    DevMem<i64> e0q, wq, ownw, valown, ext;             // ownw: W(v, own) of a moving round, W(v, P(v)) of a refinement
    DevMem<u32> s, s2, P, P2, R, SP, SR, cntr, well, bestid, cv, newlab, minm, node_of, flag, ucnt, ctl;
    DevMem<u64> uoff, below;
    u64 S = 1;
    u64 bytes = 0;
    lzani_cluster_leiden_info info{};
    int alloc(lzani_ctx* c)
    {
        const u32 n = c->cl.info.n;
        const u64 E = c->cl.info.edges;
        if (n > CL_LEIDEN_MAX_N) return fail(c, LZANI_ERR_ARG, "lzani_cluster_run: Leiden takes at most 2^21 genomes");
        if (E > CL_MAX_EDGES) return fail(c, LZANI_ERR_ARG, "lzani_cluster_run: Leiden takes at most 2^32 - 17 edge records");
        S = cluster_table_slots(2 * E);
        CL_ALLOC(tkey, (size_t)S); CL_ALLOC(tval, (size_t)S);
        CL_ALLOC(e0key, (size_t)E); CL_ALLOC(e0q, (size_t)E); CL_ALLOC(wkey, (size_t)E); CL_ALLOC(wq, (size_t)E);
        CL_ALLOC(ucnt, (size_t)pf_chunks(S)); CL_ALLOC(uoff, (size_t)pf_chunks(S) + 1);
        CL_ALLOC(bestd, n); CL_ALLOC(cd, n); CL_ALLOC(ownw, n); CL_ALLOC(valown, n); CL_ALLOC(ext, n);
        CL_ALLOC(s, n); CL_ALLOC(s2, n); CL_ALLOC(P, n); CL_ALLOC(P2, n); CL_ALLOC(R, n);
        CL_ALLOC(SP, n); CL_ALLOC(SR, n); CL_ALLOC(cntr, n); CL_ALLOC(well, n); CL_ALLOC(bestid, n);
        CL_ALLOC(cv, n); CL_ALLOC(newlab, n); CL_ALLOC(minm, 2 * (size_t)n); CL_ALLOC(node_of, n);
        CL_ALLOC(flag, n); CL_ALLOC(below, (size_t)n + 1);
        CL_ALLOC(quality, 1); CL_ALLOC(ctl, CL_LD_CTL);
        return LZANI_OK;
    }
    // A phase on a level of m nodes: round(r) launches one round whose movers go to ctl[CL_LD_MOVERS + r] (and, where it
    // counts them, the communities behind it to ctl[CL_LD_COMMS + r]).  rounds: up to the first without a mover, that one
    // included; movers: their sum; comms: the communities behind the last round.
    template <class Round>
    int phase(lzani_ctx* c, u32 m, const char* still, Round round, u64& rounds, u64& movers, u32& comms)
    {
        // the cap is a safety stop, not a bound that is proved: see include/lzani.h
        const ClRounds p{CL_LD_BATCH, CL_LEIDEN_CAP_MUL * m + CL_LEIDEN_CAP_ADD, still, ctl, CL_LD_CTL, CL_LD_MOVERS};
        movers = 0; comms = 0;
        return cluster_rounds(c, p, rounds, round, [&](const u32* h, u32 moving, u32 last) {
            if (h[CL_LD_ERR]) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: the node-community table's probe sequence ran out, or an id out of range");
            for (u32 r = 0; r < moving; ++r) movers += h[CL_LD_MOVERS + r];
            comms = h[CL_LD_COMMS + last];
            return (int)LZANI_OK;
        });
    }
    // The table's occupied slots into the entry list (key, q); returns where their number is.
    const u64* compact(lzani_ctx* c, const ClLdTable& t, unsigned long long* key, i64* q)
    {
        return cluster_compact(c, t.S, ucnt, uoff, [&](auto write, u32 chunks) {
            hipLaunchKernelGGL(k_ld_compact<decltype(write)::value>, dim3(chunks), dim3(PF_THREADS), 0, c->stream, t, ucnt, uoff, key, q);
        });
    }
    // The iterations (lzani_kernels_cluster.h): rep_of (v at the start), rounds, and what the run did.
    int run(lzani_ctx* c, ClusterStage& st)
    {
        const u32 n = c->cl.info.n;
        const u64 E = c->cl.info.edges;
        const i64 g = cluster_leiden_g(c->leiden_resolution);
        const dim3 threads(PF_THREADS), all(pf_blocks(n));
        u32* rep_of = st.rep_of;
        hipLaunchKernelGGL(k_ld_init, all, threads, 0, c->stream, n, rep_of, st.size);
        lzani_cluster_leiden_info& out = info;
        out = lzani_cluster_leiden_info{};
        out.resolution_q = (u64)g; out.table_slots = S; out.workspace_bytes = bytes;
        // the distinct edges with their smallest q: the level-0 entry list
        StreamSpan dedup, span;
        u64 D = 0;
        HIPCHK(c, dedup.begin(c->stream));
        if (E) {
            const ClLdTable t{tkey, tval, cluster_table_slots(E)};
            HIPCHK(c, cluster_table_clear(c, t.S, t.key, {{t.val, 0xFF}}));
            HIPCHK(c, hipMemsetAsync(ctl, 0, CL_LD_CTL * sizeof(u32), c->stream));
            hipLaunchKernelGGL(k_ld_dedup, dim3(pf_blocks(E)), threads, 0, c->stream, c->cl.edges, E, n, t, ctl);
            const u64* total = compact(c, t, e0key, e0q);
            HIPCHK(c, hipGetLastError());
            u32 err = 0;
            HIPCHK(c, hipMemcpyAsync(&err, ctl.get() + CL_LD_ERR, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(&D, total, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (err) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: the edge table's probe sequence ran out, or an id out of range");
            if (D > E) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: more distinct edges than edge records");
        }
        HIPCHK(c, dedup.end(c->stream));
        out.distinct_edges = D; out.duplicate_edges = E - D;
        HIPCHK(c, span.begin(c->stream));
        for (int it = 0; it < c->leiden_iterations; ++it) {
            out.iterations++;
            u32 m = n;                                  // the level: its nodes, its entries and where they are
            u64 L = D;
            const unsigned long long* lkey = e0key;
            const i64* lq = e0q;
            hipLaunchKernelGGL(k_ld_level0, all, threads, 0, c->stream, n, rep_of, s, P, node_of);
            HIPCHK(c, hipMemsetAsync(SP, 0, (size_t)n * 4, c->stream));
            hipLaunchKernelGGL(k_ld_sizes, all, threads, 0, c->stream, n, s, P, SP, (u32*)nullptr, (u32*)nullptr);
            u64 moved_in_iteration = 0;
            for (;;) {
                out.levels++;
                const dim3 nodes(pf_blocks(m)), entries(pf_blocks(L));
                const ClLdTable t{tkey, tval, cluster_table_slots(2 * L)};
                if (t.S > S) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: more entries than edge records");
                const dim3 slots(pf_blocks(t.S));
                u64 rounds = 0, moved = 0, merged = 0;
                u32 comms = 0;
                auto share = [&](u32* part, u32* sizes, u32* cnt, u32 r, bool count_comms) {      // the passes both kinds of round end in
                    hipLaunchKernelGGL(k_ld_cand_max, nodes, threads, 0, c->stream, m, part, bestd, bestid, cd);
                    hipLaunchKernelGGL(k_ld_cand_min, nodes, threads, 0, c->stream, m, part, bestd, bestid, cd, cv);
                    hipLaunchKernelGGL(k_ld_decide, nodes, threads, 0, c->stream, m, part, bestd, bestid, cv, newlab, minm, ctl.get() + CL_LD_MOVERS + r);
                    hipLaunchKernelGGL(k_ld_minm, nodes, threads, 0, c->stream, m, newlab, minm);
                    hipLaunchKernelGGL(k_ld_newid, nodes, threads, 0, c->stream, m, newlab, minm, part, sizes, cnt);
                    hipLaunchKernelGGL(k_ld_sizes, nodes, threads, 0, c->stream, m, s, part, sizes, cnt, count_comms ? ctl.get() + CL_LD_COMMS + r : (u32*)nullptr);
                };
                auto move_round = [&](u32 r) -> hipError_t {
                    if (hipError_t e = cluster_table_clear(c, t.S, t.key, {{t.val, 0}})) return e;
                    if (hipError_t e = hipMemsetAsync(ownw, 0, (size_t)m * 8, c->stream)) return e;
                    if (L) hipLaunchKernelGGL(k_ld_move_insert, entries, threads, 0, c->stream, lkey, lq, L, m, P, t, ctl);
                    hipLaunchKernelGGL(k_ld_move_stay, slots, threads, 0, c->stream, t, m, P, ownw);
                    hipLaunchKernelGGL(k_ld_move_node, nodes, threads, 0, c->stream, m, g, s, P, SP, ownw, valown, bestd, bestid, cd, cv);
                    hipLaunchKernelGGL(k_ld_move_bestd, slots, threads, 0, c->stream, t, m, g, s, P, SP, valown, bestd);
                    hipLaunchKernelGGL(k_ld_move_bestid, slots, threads, 0, c->stream, t, m, g, s, P, SP, valown, bestd, bestid);
                    share(P, SP, nullptr, r, true);
                    return hipSuccess;
                };
                if (int rc = phase(c, m, "lzani_cluster_run: Leiden's moving phase still moves nodes after 64 * n + 64 rounds", move_round, rounds, moved, comms)) return rc;
                out.move_rounds += rounds; out.moves += moved; moved_in_iteration += moved;
                if (comms == m) break;                  // every community is one level node
                hipLaunchKernelGGL(k_ld_refine_init, nodes, threads, 0, c->stream, m, s, R, SR, cntr, ownw);
                if (L) hipLaunchKernelGGL(k_ld_wp, entries, threads, 0, c->stream, lkey, lq, L, m, P, ownw);
                hipLaunchKernelGGL(k_ld_well, nodes, threads, 0, c->stream, m, g, s, P, SP, ownw, well);
                const ClLdRefine rf{g, s, P, R, SP, SR, cntr, well, ext};
                auto refine_round = [&](u32 r) -> hipError_t {
                    if (hipError_t e = cluster_table_clear(c, t.S, t.key, {{t.val, 0}})) return e;
                    if (hipError_t e = hipMemsetAsync(ext, 0, (size_t)m * 8, c->stream)) return e;
                    if (L) hipLaunchKernelGGL(k_ld_refine_insert, entries, threads, 0, c->stream, lkey, lq, L, m, P, R, t, ext, ctl);
                    hipLaunchKernelGGL(k_ld_refine_node, nodes, threads, 0, c->stream, m, bestd, bestid, cd, cv);
                    hipLaunchKernelGGL(k_ld_refine_bestd, slots, threads, 0, c->stream, t, m, rf, bestd);
                    hipLaunchKernelGGL(k_ld_refine_bestid, slots, threads, 0, c->stream, t, m, rf, bestd, bestid);
                    share(R, SR, cntr, r, false);
                    return hipSuccess;
                };
                if (int rc = phase(c, m, "lzani_cluster_run: Leiden's refinement still moves nodes after 64 * n + 64 rounds", refine_round, rounds, merged, comms)) return rc;
                out.refine_rounds += rounds; out.merges += merged;
                if (!moved && !merged) break;           // nothing can change any more
                // aggregation: the R-communities, numbered in ascending order of their smallest member, and the entries between them
                hipLaunchKernelGGL(k_ld_agg_flags, nodes, threads, 0, c->stream, m, R, flag);
                hipLaunchKernelGGL(k_pf_scan, dim3(1), dim3(1024), 0, c->stream, flag, (u64)m, below);
                hipLaunchKernelGGL(k_ld_agg_nodes, nodes, threads, 0, c->stream, m, R, P, SR, below, s2, P2);
                hipLaunchKernelGGL(k_ld_agg_nodeof, all, threads, 0, c->stream, n, m, R, below, node_of);
                const ClLdTable ta{tkey, tval, cluster_table_slots(L)};
                HIPCHK(c, cluster_table_clear(c, ta.S, ta.key, {{ta.val, 0}}));
                HIPCHK(c, hipMemsetAsync(ctl, 0, CL_LD_CTL * sizeof(u32), c->stream));
                if (L) hipLaunchKernelGGL(k_ld_agg_insert, entries, threads, 0, c->stream, lkey, lq, L, m, R, below, ta, ctl);
                const u64* total = compact(c, ta, wkey, wq);
                HIPCHK(c, hipGetLastError());
                u64 m2 = 0, L2 = 0;
                u32 err = 0;
                HIPCHK(c, hipMemcpyAsync(&m2, below.get() + m, 8, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipMemcpyAsync(&L2, total, 8, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipMemcpyAsync(&err, ctl.get() + CL_LD_ERR, 4, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                if (err) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: the contraction table's probe sequence ran out, or an id out of range");
                if (!m2 || m2 > m || L2 > L) return fail(c, LZANI_ERR_DEVICE, "lzani_cluster_run: an aggregated level larger than the level it comes from");
                std::swap(s, s2); std::swap(P, P2);
                m = (u32)m2; L = L2; lkey = wkey; lq = wq;
                HIPCHK(c, hipMemsetAsync(SP, 0, (size_t)m * 4, c->stream));
                hipLaunchKernelGGL(k_ld_sizes, dim3(pf_blocks(m)), threads, 0, c->stream, m, s, P, SP, (u32*)nullptr, (u32*)nullptr);
            }
            // rep_of: the smallest original id of every final community
            hipLaunchKernelGGL(k_ld_final, all, threads, 0, c->stream, n, m, node_of, P, newlab, minm);
            hipLaunchKernelGGL(k_ld_minm, all, threads, 0, c->stream, n, newlab, minm);
            hipLaunchKernelGGL(k_ld_newid, all, threads, 0, c->stream, n, newlab, minm, rep_of, SP, (u32*)nullptr);
            HIPCHK(c, hipGetLastError());
            if (!moved_in_iteration) break;
        }
        // Q of the result on the original graph (k_ld_newid left SP cleared)
        HIPCHK(c, hipMemsetAsync(quality, 0, 8, c->stream));
        hipLaunchKernelGGL(k_ld_sizes, all, threads, 0, c->stream, n, (const u32*)nullptr, rep_of, SP, (u32*)nullptr, (u32*)nullptr);
        if (D) hipLaunchKernelGGL(k_ld_quality_edges, dim3(pf_blocks(D)), threads, 0, c->stream, e0key, e0q, D, n, rep_of, quality);
        hipLaunchKernelGGL(k_ld_quality_nodes, all, threads, 0, c->stream, n, g, SP, quality);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, span.end(c->stream));
        unsigned long long h_quality = 0;
        HIPCHK(c, hipMemcpyAsync(&h_quality, quality, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        float dedup_ms = 0, rounds_ms = 0;
        HIPCHK(c, dedup.elapsed(dedup_ms));
        HIPCHK(c, span.elapsed(rounds_ms));
        out.quality = (int64_t)h_quality; out.dedup_ms = dedup_ms; out.rounds_ms = rounds_ms;
        st.rounds = out.move_rounds + out.refine_rounds;
        return LZANI_OK;
    }
};

// The run of `unit` on the context's edges: the span and the counters, the unit's run (rep_of, rounds, its own info), the
// numbering (cluster_of and the run's part of `info`).  It allocates nothing.
template <class Unit>
int cluster_run_stage(lzani_ctx* c, Unit& unit, ClusterStage& st, lzani_cluster_info& info)
{
    const u32 n = c->cl.info.n;
    const dim3 nodes(pf_blocks(n)), threads(PF_THREADS);
    StreamSpan span;
    HIPCHK(c, span.begin(c->stream));
    HIPCHK(c, hipMemsetAsync(st.counters, 0, CL_COUNTERS * sizeof(u32), c->stream));
    if (int rc = unit.run(c, st)) return rc;
    hipLaunchKernelGGL(k_cl_flags, nodes, threads, 0, c->stream, n, st.rep_of, st.flag, st.size);
    hipLaunchKernelGGL(k_pf_scan, dim3(1), dim3(1024), 0, c->stream, st.flag, (u64)n, st.below);
    hipLaunchKernelGGL(k_cl_number, nodes, threads, 0, c->stream, n, st.rep_of, st.below, st.size, st.cluster_of, st.counters);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, span.end(c->stream));
    u32 h_counters[CL_COUNTERS] = {0, 0};
    u64 clusters = 0;
    HIPCHK(c, hipMemcpyAsync(h_counters, st.counters, sizeof h_counters, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&clusters, st.below.get() + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    HIPCHK(c, span.elapsed(ms));
    info.algo = st.algo; info.rounds = (u32)st.rounds; info.clusters = clusters; info.singletons = h_counters[CL_SINGLETONS];
    info.largest = h_counters[CL_LARGEST]; info.run_ms = ms;
    TRACE("cluster: algo=%d n=%u edges=%llu rounds=%llu clusters=%llu", st.algo, n, (unsigned long long)c->cl.info.edges, (unsigned long long)st.rounds,
          (unsigned long long)clusters);
    return LZANI_OK;
}

// lzani_cluster_run with the unit of its algorithm.  The unit and the stage are allocated whole first: refused, or short of
// memory, with the cluster state as it was.
template <class Unit>
int cluster_run_as(lzani_ctx* c, int algo, uint64_t* n_clusters)
{
    Cluster& k = c->cl;
    Unit unit;
    if (int rc = unit.alloc(c)) return rc;
    ClusterStage st;
    if (int rc = st.alloc(c)) return rc;
    st.algo = algo;
    k.ran = false;
    k.rep_of.reset(); k.cluster_of.reset();                    // the last run's result goes before the run, not before its memory is had
    lzani_cluster_info info = k.info;
    const int rc = cluster_run_stage(c, unit, st, info);
    if (rc != LZANI_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    k.info = info;
    k.specific = unit.info;
    k.rep_of = std::move(st.rep_of); k.cluster_of = std::move(st.cluster_of);
    k.ran = true;
    if (n_clusters) *n_clusters = info.clusters;
    return LZANI_OK;
}

// The info of the last run where that was one of the algorithm whose info struct `Info` is.
template <class Info>
int cluster_specific_info(const lzani_ctx* c, Info* info)
{
    if (!c || !info) return LZANI_ERR_ARG;
    const Info* last = c->cl.begun ? std::get_if<Info>(&c->cl.specific) : nullptr;
    if (!last) return LZANI_ERR_STATE;
    *info = *last;
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
        hipLaunchKernelGGL(k_cl_add_kept, dim3(pf_blocks(K)), dim3(PF_THREADS), 0, c->stream, c->kept.rec, K, k.len, (int)k.info.measure, k.edges,
                           k.info.edges);
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
    switch (algo) {                                            // the one place that knows which unit an algorithm is
    case LZANI_CLUSTER_SET_COVER: return cluster_run_as<CoverUnit>(c, algo, n_clusters);
    case LZANI_CLUSTER_COMPLETE: return cluster_run_as<LinkUnit>(c, algo, n_clusters);
    case LZANI_CLUSTER_LEIDEN: return cluster_run_as<LeidenUnit>(c, algo, n_clusters);
    default: return cluster_run_as<PlainUnit>(c, algo, n_clusters);
    }
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

uint32_t lzani_cluster_cut_lines(const lzani_cluster_cut* cut, const lzani_result* x, const lzani_result* y, uint32_t lines, uint32_t len_a, uint32_t len_b)
{
    if (!cut || !x || !y || !cluster_cut_ok(*cut)) return 0xFFFFFFFFu;
    return cluster_cut_lines(*cut, *x, *y, lines, len_a, len_b);
}

int lzani_cluster_store_begin(lzani_ctx* c, uint32_t n, const uint32_t* report_len)
{
    if (!c) return LZANI_ERR_ARG;
    const std::string fn = "lzani_cluster_store_begin";
    if (!c->gs.n) return fail(c, LZANI_ERR_STATE, fn + ": no genomes set");
    if (!n) return fail(c, LZANI_ERR_ARG, fn + ": no genomes");
    if (!report_len && n != c->gs.n) return fail(c, LZANI_ERR_ARG, fn + ": the genome set's own lengths are those of its n genomes");
    std::vector<u32> own;
    if (!report_len) { own = kept_own_lengths(c); report_len = own.data(); }
    HIPCHK(c, hipSetDevice(c->dev));
    c->cls = ClusterStore{};                                   // the last store goes first
    ClusterStore s;
    HIPCHK(c, s.len.alloc(n));
    HIPCHK(c, hipMemcpyAsync(s.len.get(), report_len, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.info.n = n;
    s.begun = true;
    c->cls = std::move(s);
    return LZANI_OK;
}

int lzani_cluster_store_add_kept(lzani_ctx* c, uint64_t* records_total)
{
    if (!c) return LZANI_ERR_ARG;
    const std::string fn = "lzani_cluster_store_add_kept";
    if (int rc = cluster_store_state(c, fn)) return rc;
    if (!c->kept.done) return fail(c, LZANI_ERR_STATE, fn + ": no kept result (call lzani_run_rows_kept first)");
    if (c->kept.n != c->cls.info.n)
        return fail(c, LZANI_ERR_ARG, fn + ": the kept result is one of " + std::to_string(c->kept.n) + " genomes, the record store of " + std::to_string(c->cls.info.n));
    HIPCHK(c, hipSetDevice(c->dev));
    if (int rc = cluster_store_append(c, c->kept.rec.get(), c->kept.info.kept_pairs, hipMemcpyDeviceToDevice)) return rc;
    if (records_total) *records_total = c->cls.info.records;
    return LZANI_OK;
}

int lzani_debug_cluster_store_add(lzani_ctx* c, const lzani_kept_pair* rec, uint64_t count)
{
    if (!c) return LZANI_ERR_ARG;
    const std::string fn = "lzani_debug_cluster_store_add";
    if (int rc = cluster_store_state(c, fn)) return rc;
    if (count && !rec) return fail(c, LZANI_ERR_ARG, fn + ": null records");
    static_assert(sizeof(lzani_kept_pair) == 36, "lzani_kept_pair is nine 32-bit fields");
    for (uint64_t i = 0; i < count; ++i)
        if (!(rec[i].a < rec[i].b && rec[i].b < c->cls.info.n && rec[i].lines >= 1 && rec[i].lines <= 3))
            return fail(c, LZANI_ERR_ARG, fn + ": a record without a < b < n, or with lines outside 1..3");
    if (!count) return LZANI_OK;
    HIPCHK(c, hipSetDevice(c->dev));
    if (int rc = cluster_store_append(c, (const u32*)rec, count, hipMemcpyHostToDevice)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LZANI_OK;
}

int lzani_cluster_level(lzani_ctx* c, int measure, const lzani_cluster_cut* cut, uint64_t* edges)
{
    if (!c) return LZANI_ERR_ARG;
    const std::string fn = "lzani_cluster_level";
    if (int rc = cluster_store_state(c, fn)) return rc;
    if (!cut) return fail(c, LZANI_ERR_ARG, fn + ": null cut");
    if (!cluster_cut_ok(*cut)) return fail(c, LZANI_ERR_ARG, fn + ": a minimum of the cut is not a number, or its reserved word is not 0");
    if (!cluster_measure_known(measure)) return fail(c, LZANI_ERR_ARG, fn + ": unknown measure");
    if (!cluster_launch_covers(c->cls.info.records)) return fail(c, LZANI_ERR_ARG, fn + ": more records than one launch covers");
    HIPCHK(c, hipSetDevice(c->dev));
    c->cl = Cluster{};                                         // the last state goes first
    Cluster k;
    const int rc = cluster_level_run(c, k, measure, *cut);
    if (rc != LZANI_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    k.begun = true;
    c->cl = std::move(k);
    if (edges) *edges = c->cl.info.edges;
    return LZANI_OK;
}

int lzani_debug_cluster_edges(lzani_ctx* c, uint64_t first, uint64_t count, lzani_cluster_edge* out)
{
    if (!c) return LZANI_ERR_ARG;
    const std::string fn = "lzani_debug_cluster_edges";
    if (int rc = cluster_state(c, fn)) return rc;
    const u64 E = c->cl.info.edges;
    if (first > E || count > E - first) return fail(c, LZANI_ERR_ARG, fn + ": the range lies past the end of the edges");
    if (!count) return LZANI_OK;
    if (!out) return fail(c, LZANI_ERR_ARG, fn + ": null output");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipMemcpy(out, c->cl.edges.get() + first, (size_t)count * sizeof(lzani_cluster_edge), hipMemcpyDeviceToHost));
    return LZANI_OK;
}

int lzani_get_cluster_store_info(const lzani_ctx* c, lzani_cluster_store_info* info)
{
    if (!c || !info) return LZANI_ERR_ARG;
    if (!c->cls.begun) return LZANI_ERR_STATE;
    *info = c->cls.info;
    return LZANI_OK;
}

int lzani_get_cluster_level_info(const lzani_ctx* c, lzani_cluster_level_info* info)
{
    if (!c || !info) return LZANI_ERR_ARG;
    if (!c->cl.begun || !c->cl.from_level) return LZANI_ERR_STATE;
    *info = c->cl.level;
    return LZANI_OK;
}

int lzani_get_cluster_cover_info(const lzani_ctx* c, lzani_cluster_cover_info* info) { return cluster_specific_info(c, info); }
int lzani_get_cluster_link_info(const lzani_ctx* c, lzani_cluster_link_info* info) { return cluster_specific_info(c, info); }
int lzani_get_cluster_leiden_info(const lzani_ctx* c, lzani_cluster_leiden_info* info) { return cluster_specific_info(c, info); }

}  // extern "C"
