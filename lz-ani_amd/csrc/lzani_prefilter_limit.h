// lzani_prefilter_limit.h -- host side of the prefilter's limit stage (include/lzani.h states the definition): every
// limiting genome keeps its N best pairs of the context's current prefilter result.  The entry points are
// lzani_prefilter_limit, lzani_get_prefilter_limit_info, the pure lzani_prefilter_limit_host and the test hook
// lzani_debug_prefilter_set.  Included by lzani_hip.hip only, behind lzani_prefilter.h; of that file it uses pf_blocks and
// pf_chunks, of lzani_hip.hip lzani_ctx (which holds the Prefilter), fail, HIPCHK, sort_keys and sort_scratch_bytes, of
// lzani_devmem.h DevMem and StreamSpan.  The kernels are the k_pfl_* of lzani_kernels_prefilter.h and k_pf_scan, the sorts
// lzani_sort.hip's.
//
// A post-stage: the result lies in Prefilter::tiles (per tile ids and shared, row_off on the host) and is replaced by one
// tile over all rows.  Order of work (PfLimit::run), E entries, n genomes, Dk directed keys (2 E; cross form E):
//   the tiles' entries side by side (several tiles only) and row_off on the device
//   row_of[e]; the score keys ~q << 32 | e in CSR order; their sort by the bits [32, 64)
//   the directed keys g << 32 | i and the degrees; their sort by the bits [32, 32 + bits(n)); the scan of the degrees
//   the marks of every list's first N; the genomes cut
//   per row the survivors counted, scanned, row_off read back once; ids and shared of the survivors written.
//
// What the stage reads and writes per entry (the sorts apart: 24 B per key and pass, four passes over E keys and
// ceil(bits(n) / 8) passes over Dk keys).  Several tiles: 8 B read, 8 B written.  row_of: 4 B written.  Score keys:
// 12 B read at the entry's index, two |K| words gathered, 8 B written.  Directed keys: 8 B read in order, two words
// gathered at the entry (one in the cross form), 16 B written (cross: 8 B), two integer atomic adds (cross: one).  Marks,
// per directed key: 8 B read in order, one start word and one sorted key gathered, at most one byte stored.  Rows: one byte
// read twice, and per survivor 8 B read and 8 B written.  Per genome: a degree, two offsets, two counts.
#pragma once

namespace {

constexpr u64 PF_LIMIT_MAX_ENTRIES = 0x7FFFFFF7ull;     // 2^31 - 9: twice as many keys fit one sort call of 2^32 - 17

// What the two functions that take caller arrays check; the reason in msg.
int pf_limit_check(u32 n, u32 n_ref, const u32* kmers_of, const u64* row_off, const u32* ids, const u32* shared, std::string& msg)
{
    auto bad = [&](const std::string& m) { msg = m; return (int)LZANI_ERR_ARG; };
    if (!n || !kmers_of || !row_off) return bad("empty input");
    if (n_ref >= n) return bad("n_ref must be 0 (all pairs) or 1 .. n - 1");
    if (row_off[0] != 0) return bad("row_off must start at 0");
    for (u32 a = 0; a < n; ++a)
        if (row_off[a + 1] < row_off[a]) return bad("row_off descends at row " + std::to_string(a));
    const u64 E = row_off[n];
    if (E > PF_LIMIT_MAX_ENTRIES) return bad("more than 2^31 - 9 entries");
    if (E && (!ids || !shared)) return bad("null entries");
    for (u32 a = 0; a < n; ++a)
        for (u64 e = row_off[a]; e < row_off[a + 1]; ++e) {
            const u32 b = ids[e];
            auto at = [&]() { return " (row " + std::to_string(a) + ", entry " + std::to_string(e) + ")"; };
            if (b >= n) return bad("an id is not below n" + at());
            if (b <= a) return bad("an id is not above its row" + at());
            if (e > row_off[a] && ids[e - 1] >= b) return bad("the ids of a row do not ascend strictly" + at());
            if (n_ref && !(a < n_ref && b >= n_ref)) return bad("the cross form holds pairs a < n_ref <= b only" + at());
            if (!shared[e]) return bad("shared is 0" + at());
            if (shared[e] > std::min(kmers_of[a], kmers_of[b])) return bad("shared is above min(|K|)" + at());
        }
    return LZANI_OK;
}

// The rule by its definition, on checked arrays: the list of every limiting genome sorted by (q descending, partner
// ascending), its first N marked.
void pf_limit_host_impl(u32 n, u32 n_ref, const u32* kmers_of, const u64* row_off, const u32* ids, const u32* shared, u32 N, uint8_t* keep)
{
    struct Item { u32 nq, h; u64 e; };                  // ~q, the partner, the entry
    const u64 E = row_off[n];
    std::vector<u64> start((size_t)n + 1, 0);
    auto limiting = [&](u32 g) { return !n_ref || g >= n_ref; };
    for (u32 a = 0; a < n; ++a)
        for (u64 e = row_off[a]; e < row_off[a + 1]; ++e) {
            if (limiting(a)) ++start[(size_t)a + 1];
            if (limiting(ids[e])) ++start[(size_t)ids[e] + 1];
        }
    for (u32 g = 0; g < n; ++g) start[(size_t)g + 1] += start[g];
    std::vector<Item> list((size_t)start[n]);
    std::vector<u64> fill(start.begin(), start.end() - 1);
    for (u32 a = 0; a < n; ++a)
        for (u64 e = row_off[a]; e < row_off[a + 1]; ++e) {
            const u32 b = ids[e], nq = ~pf_limit_score(shared[e], kmers_of[a], kmers_of[b]);
            if (limiting(a)) list[(size_t)fill[a]++] = Item{nq, b, e};
            if (limiting(b)) list[(size_t)fill[b]++] = Item{nq, a, e};
        }
    std::fill(keep, keep + E, (uint8_t)0);
    for (u32 g = 0; g < n; ++g) {
        const auto lo = list.begin() + (ptrdiff_t)start[g], hi = list.begin() + (ptrdiff_t)start[(size_t)g + 1];
        std::sort(lo, hi, [](const Item& x, const Item& y) { return x.nq != y.nq ? x.nq < y.nq : x.h < y.h; });
        for (auto it = lo; it != hi && (u64)(it - lo) < (u64)N; ++it) keep[it->e] = 1;
    }
}

// The workspace of a run, allocated whole before the result is touched.
struct PfLimitWork {
    DevMem<u32> ids, shared;              // the tiles' entries side by side (several tiles only)
    DevMem<u64> rowoff;                   // the result's row offsets (n + 1)
    DevMem<u32> row_of;                   // per entry: its row
    DevMem<unsigned long long> ka, kb, kq;        // ka: the score keys, then the directed keys; kb: the directed keys sorted; kq: the score keys sorted
    DevMem<unsigned char> scratch, survive;
    DevMem<u32> deg, rowcnt, cut;         // per genome: its list's length; per row: its survivors; the genomes cut
    DevMem<u64> start, outoff;            // the scans of deg and of rowcnt (n + 1 each)
    u64 bytes() const
    {
        return ids.bytes() + shared.bytes() + rowoff.bytes() + row_of.bytes() + ka.bytes() + kb.bytes() + kq.bytes() + scratch.bytes() + survive.bytes() +
               deg.bytes() + rowcnt.bytes() + cut.bytes() + start.bytes() + outoff.bytes();
    }
};

struct PfLimit {
    lzani_ctx* c; Prefilter& pf; const u32 N;
    const u32 n, n_ref;
    const u64 E, Dk;                      // entries; directed keys
    const int gbits;                      // of a genome id
    PfLimitWork w;
    StreamSpan span;
    lzani_prefilter_limit_info info{};

    PfLimit(lzani_ctx* c_, u32 N_)
        : c(c_), pf(c_->pf), N(N_), n(pf.n), n_ref(pf.cross ? pf.cinfo.n_ref : 0u), E(pf.info.entries), Dk(n_ref ? E : 2 * E), gbits(std::max(1, ceil_log2(n))) {}

    bool one_tile() const { return pf.tiles.size() == 1 && pf.row_off[pf.tiles[0].r0] == 0 && pf.row_off[pf.tiles[0].r1] == E; }

    int alloc()
    {
        size_t need1 = 0, need2 = 0;
        if (int rc = sort_scratch_bytes(c, (size_t)E, 1, 32, 64, "lzani_prefilter_limit: sort", need1)) return rc;
        if (int rc = sort_scratch_bytes(c, (size_t)Dk, 1, 32, 32 + gbits, "lzani_prefilter_limit: sort", need2)) return rc;
        if (!one_tile()) { HIPCHK(c, w.ids.alloc((size_t)E)); HIPCHK(c, w.shared.alloc((size_t)E)); }
        HIPCHK(c, w.rowoff.alloc((size_t)n + 1)); HIPCHK(c, w.row_of.alloc((size_t)E));
        HIPCHK(c, w.ka.alloc((size_t)Dk)); HIPCHK(c, w.kb.alloc((size_t)Dk)); HIPCHK(c, w.kq.alloc((size_t)E));
        HIPCHK(c, w.scratch.alloc(std::max(need1, need2))); HIPCHK(c, w.survive.alloc((size_t)E));
        HIPCHK(c, w.deg.alloc(n)); HIPCHK(c, w.rowcnt.alloc(n)); HIPCHK(c, w.cut.alloc(1));
        HIPCHK(c, w.start.alloc((size_t)n + 1)); HIPCHK(c, w.outoff.alloc((size_t)n + 1));
        return LZANI_OK;
    }

    int run(PrefilterTile& out, std::vector<u64>& h_off, u32& cut)
    {
        const dim3 threads(PF_THREADS), entries(pf_blocks(E)), directed(pf_blocks(Dk)), nodes(pf_blocks(n)), rows((n + PF_THREADS / 64 - 1) / (PF_THREADS / 64));
        hipStream_t s = c->stream;
        HIPCHK(c, span.begin(s));
        const u32 *ids = nullptr, *shared = nullptr;
        if (one_tile()) { ids = pf.tiles[0].ids; shared = pf.tiles[0].shared; }
        else {
            for (const PrefilterTile& t : pf.tiles) {
                const u64 at = pf.row_off[t.r0], cnt = pf.row_off[t.r1] - at;
                if (!cnt) continue;
                HIPCHK(c, hipMemcpyAsync(w.ids.get() + at, t.ids.get(), (size_t)cnt * 4, hipMemcpyDeviceToDevice, s));
                HIPCHK(c, hipMemcpyAsync(w.shared.get() + at, t.shared.get(), (size_t)cnt * 4, hipMemcpyDeviceToDevice, s));
            }
            ids = w.ids; shared = w.shared;
        }
        HIPCHK(c, hipMemcpyAsync(w.rowoff, pf.row_off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemsetAsync(w.deg, 0, (size_t)n * 4, s));
        HIPCHK(c, hipMemsetAsync(w.survive, 0, (size_t)E, s));
        HIPCHK(c, hipMemsetAsync(w.cut, 0, 4, s));
        // ---- the entries by score
        hipLaunchKernelGGL(k_pfl_rowof, rows, threads, 0, s, (const u64*)w.rowoff.get(), n, w.row_of.get());
        hipLaunchKernelGGL(k_pfl_keys, entries, threads, 0, s, (const u32*)w.row_of.get(), ids, shared, E, (const u32*)pf.kmers_of.get(), w.ka.get());
        HIPCHK(c, hipGetLastError());
        if (int rc = sort_keys(c, w.scratch, w.ka.get(), w.kq.get(), (size_t)E, 1, 32, 64, "lzani_prefilter_limit: sort", false)) return rc;
        // ---- every limiting genome's list in order
        hipLaunchKernelGGL((n_ref ? k_pfl_directed<true> : k_pfl_directed<false>), entries, threads, 0, s, (const unsigned long long*)w.kq.get(), E,
                           (const u32*)w.row_of.get(), ids, w.ka.get(), w.deg.get());
        HIPCHK(c, hipGetLastError());
        if (int rc = sort_keys(c, w.scratch, w.ka.get(), w.kb.get(), (size_t)Dk, 1, 32, 32 + gbits, "lzani_prefilter_limit: sort", false)) return rc;
        hipLaunchKernelGGL(k_pf_scan, dim3(1), dim3(1024), 0, s, (const u32*)w.deg.get(), (u64)n, w.start.get());
        hipLaunchKernelGGL(k_pfl_mark, directed, threads, 0, s, (const unsigned long long*)w.kb.get(), Dk, (const u64*)w.start.get(), N,
                           (const unsigned long long*)w.kq.get(), w.survive.get());
        hipLaunchKernelGGL(k_pfl_cut, nodes, threads, 0, s, (const u32*)w.deg.get(), n, N, w.cut.get());
        // ---- the survivors, row by row
        hipLaunchKernelGGL(k_pfl_rows<false>, rows, threads, 0, s, (const u64*)w.rowoff.get(), n, (const unsigned char*)w.survive.get(), ids, shared,
                           w.rowcnt.get(), (const u64*)nullptr, (u32*)nullptr, (u32*)nullptr);
        hipLaunchKernelGGL(k_pf_scan, dim3(1), dim3(1024), 0, s, (const u32*)w.rowcnt.get(), (u64)n, w.outoff.get());
        HIPCHK(c, hipGetLastError());
        h_off.resize((size_t)n + 1);
        HIPCHK(c, hipMemcpyAsync(h_off.data(), w.outoff, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(&cut, w.cut, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        if (h_off[n] > E) return fail(c, LZANI_ERR_DEVICE, "lzani_prefilter_limit: more survivors than entries");
        out.r0 = 0; out.r1 = n;
        HIPCHK(c, out.ids.alloc((size_t)h_off[n]));
        HIPCHK(c, out.shared.alloc((size_t)h_off[n]));
        hipLaunchKernelGGL(k_pfl_rows<true>, rows, threads, 0, s, (const u64*)w.rowoff.get(), n, (const unsigned char*)w.survive.get(), ids, shared,
                           w.rowcnt.get(), (const u64*)w.outoff.get(), out.ids.get(), out.shared.get());
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, span.end(s));
        float ms = 0;
        HIPCHK(c, span.elapsed(ms));                             // (waits for the end: the stream is idle behind it)
        info.limit_ms = ms;
        return LZANI_OK;
    }
};

int prefilter_limit_impl(lzani_ctx* c, u32 N, uint64_t* n_entries)
{
    if (!c) return LZANI_ERR_ARG;
    if (!c->pf.done) return fail(c, LZANI_ERR_STATE, "lzani_prefilter_limit: no prefilter result (call lzani_prefilter first)");
    if (!N) return fail(c, LZANI_ERR_ARG, "lzani_prefilter_limit: max_per_genome must be at least 1");
    if (c->pf.info.entries > PF_LIMIT_MAX_ENTRIES)
        return fail(c, LZANI_ERR_ARG, "lzani_prefilter_limit: " + std::to_string(c->pf.info.entries) + " entries; the stage takes at most 2^31 - 9");
    HIPCHK(c, hipSetDevice(c->dev));
    PfLimit L(c, N);
    Prefilter& pf = c->pf;
    L.info.max_per_genome = N;
    L.info.limiting = L.n_ref ? L.n - L.n_ref : L.n;
    L.info.entries_in = L.info.entries_out = L.E;
    if (L.E) {                                                   // (no entry: nothing to rank, the result stays as it is)
        PrefilterTile out;
        std::vector<u64> h_off;
        u32 cut = 0;
        int rc = L.alloc();
        if (rc == LZANI_OK) { L.info.workspace_bytes = L.w.bytes(); rc = L.run(out, h_off, cut); }
        if (rc != LZANI_OK) { (void)hipStreamSynchronize(c->stream); return rc; }     // (the unlimited result is as it was)
        pf.tiles.clear();
        pf.tiles.push_back(std::move(out));
        pf.row_off = std::move(h_off);
        pf.info.entries = pf.row_off[L.n];
        L.info.entries_out = pf.info.entries;
        L.info.genomes_cut = cut;
    }
    pf.limited = true;
    pf.linfo = L.info;
    if (n_entries) *n_entries = pf.info.entries;
    TRACE("prefilter limit: N=%u entries %llu -> %llu, %llu genomes cut", N, (unsigned long long)L.info.entries_in, (unsigned long long)L.info.entries_out,
          (unsigned long long)L.info.genomes_cut);
    return LZANI_OK;
}

}  // namespace

extern "C" {

int lzani_prefilter_limit(lzani_ctx* c, uint32_t max_per_genome, uint64_t* n_entries) { return prefilter_limit_impl(c, max_per_genome, n_entries); }

int lzani_get_prefilter_limit_info(const lzani_ctx* c, lzani_prefilter_limit_info* info)
{
    if (!c || !info) return LZANI_ERR_ARG;
    if (!c->pf.done || !c->pf.limited) return LZANI_ERR_STATE;
    *info = c->pf.linfo;
    return LZANI_OK;
}

int lzani_prefilter_limit_host(uint32_t n, uint32_t n_ref, const uint32_t* kmers_of, const uint64_t* row_off, const uint32_t* ids, const uint32_t* shared,
                               uint32_t max_per_genome, uint8_t* keep)
{
    std::string msg;
    if (int rc = pf_limit_check(n, n_ref, kmers_of, row_off, ids, shared, msg)) return rc;
    if (!max_per_genome || (row_off[n] && !keep)) return LZANI_ERR_ARG;
    pf_limit_host_impl(n, n_ref, kmers_of, row_off, ids, shared, max_per_genome, keep);
    return LZANI_OK;
}

int lzani_debug_prefilter_set(lzani_ctx* c, uint32_t n, uint32_t n_ref, const uint32_t* kmers_of, const uint64_t* row_off, const uint32_t* ids,
                              const uint32_t* shared)
{
    if (!c) return LZANI_ERR_ARG;
    std::string msg;
    if (int rc = pf_limit_check(n, n_ref, kmers_of, row_off, ids, shared, msg)) return fail(c, rc, "lzani_debug_prefilter_set: " + msg);
    HIPCHK(c, hipSetDevice(c->dev));
    c->pf = Prefilter{};                                         // the last result goes first: two need not fit
    const u64 E = row_off[n];
    Prefilter pf;
    PrefilterTile tile;
    tile.r0 = 0; tile.r1 = n;
    HIPCHK(c, pf.kmers_of.alloc(n));
    HIPCHK(c, tile.ids.alloc((size_t)E));
    HIPCHK(c, tile.shared.alloc((size_t)E));
    HIPCHK(c, hipMemcpy(pf.kmers_of, kmers_of, (size_t)n * 4, hipMemcpyHostToDevice));
    if (E) {
        HIPCHK(c, hipMemcpy(tile.ids, ids, (size_t)E * 4, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(tile.shared, shared, (size_t)E * 4, hipMemcpyHostToDevice));
    }
    pf.n = n;
    pf.cross = n_ref != 0; pf.cinfo.n_ref = n_ref; pf.cinfo.n_query = n_ref ? n - n_ref : 0;
    pf.info.entries = E; pf.info.tiles = 1;
    pf.bin_lo = {0, PF_BINS};
    pf.row_off.assign(row_off, row_off + (size_t)n + 1);
    pf.tiles.push_back(std::move(tile));
    pf.done = true;
    c->pf = std::move(pf);
    return LZANI_OK;
}

}  // extern "C"
