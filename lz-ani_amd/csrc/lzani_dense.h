// lzani_dense.h -- host side of the dense-row stage of a run: the candidates of every pair of a batch from the presence
// matrix of the batch's references (lzani_kernels_cand.h) instead of a probe per query position or a join per pair, and,
// where a batch holds few, long pairs, those pairs by several waves each (lzani_kernels_split.h).  Included by
// lzani_hip.hip only, between the run's types and its pair launch; of that file it uses lzani_ctx (which holds the
// CandScratch), RunCtx / Batch / RunPlan / Knobs / RowFacts, fail, HIPCHK, TRACE, raise_lds, sort_keys and launch_row, of
// lzani_index.h gtab, slot_bytes, ensure_slabs and for_slices.  The pure decisions -- the batches, the split / LPT rule,
// the bytes of a slab slot -- are lzani_run_plan.h.
// Host only: not among the sources a run-time compile embeds (lzani_rtc.h).
//
// Order of work:
//   plan_bitmaps       once per run (plan_run): whether the rows qualify, what a batch may hold (index slabs + the bitmaps of
//                      its pairs within the memory there is), the matrix, pair table and bitmap buffers, the batches
//   per batch (run_batch), behind its index build:
//     choose_split_lpt   the split / LPT rule of the batch (choose_split), the candidate counts' buffer, cleared
//     candidate_stage    group by group of pm_group references: pair table (query lists), matrix (k_pm_from_index, or
//                        cleared + k_pm_build), k_pm_cand -> bitmaps and counts; then the ticket order (k_lpt_keys + sort)
//     sink_candidates    test hook only: the batch's bitmaps and counts to the host
//     run_split          from launch_pairs, where the rule chose the split: which pairs to cut (by their counts), the
//                        checkpoints, rounds of segments + stitch until every pair is finished
//
// What it holds between batches and runs: CandScratch (lzani_ctx::cs) -- matrix, pair table, bitmaps, counts and ticket
// keys, the split's buffers.  Every buffer only grows (DevMem::reserve); all of them go with the genome set
// (lzani_set_genomes), or together when the matrix, the pair table or the bitmaps cannot be had (plan_bitmaps: the run
// then takes the probe / join form, which needs none of them).
#pragma once

namespace {

// Test hook (lzani_debug_run_candidates): host copies of every batch's candidate bitmaps -- the first `words` words of each
// pair -- and, where the batch counted them, its pairs' candidate counts; indexed by the run's pair offset.
struct CandSink { u32* cbits; u64 words; u32* pcount; u32 counted_batches; };

// Dense rows: the candidates of every pair of a batch come from the presence matrix of its references
// (lzani_kernels_cand.h) instead of a probe per query position (viral sizes) or a join of sorted k-mer lists per pair
// (long genomes), where the rows qualify; a batch is then also bounded by what the candidate bitmaps of its pairs take,
// and the index slabs are sized for such a batch.  p.pm stays clear where the rows do not qualify or do not fit (a genome
// set this large: the probe / join form, batch by batch), and where a buffer (matrix, pair table, bitmaps) cannot be had
// after all -- the sizing is an estimate, and an allocation may fail on a fragmented heap: the bitmap buffers are then
// released (the probe / join form needs none of them).
int plan_bitmaps(lzani_ctx* c, const RunGenomes& g, const Knobs& k, const RowFacts& f, u32 n_rows, const u64* row_off, bool lists, bool regions, RunPlan& p)
{
    // (from 32 rows on where the probe form with tag words is the alternative; from 8 rows where it is the rounds of the
    // first kernel: genomes whose tags do not fit a tag byte -- 260 kbp to 2 Mbp at mal 15, viral sizes at mal 13+.
    // Below, the matrix -- 16 GB to clear at 30 key bits -- costs more than it saves.)
    // Long genomes (the join is the alternative: 210 ms for the 56 pairs of 8 x 5 Mbp against 149 by bitmaps, 92 with the
    // pairs cut into segments): from two rows on.
    const u32 min_rows = k.pm_min_rows ? (u32)std::max(1, *k.pm_min_rows) : c->gs.lay.join_mode ? 2u : c->gs.lay.tw_stride ? 32u : 8u;
    // Query lists qualify when they are dense where they are: a query that occurs in a group of rows should meet a
    // good part of it (one matrix row read serves all its pairs of the group) -- the row x column blocks of a tiled
    // all2all do, the few relatives a kmer-db filter leaves per row do not.  No query twice in a row (one bitmap each).
    // (Measured in round 4 on the related workload, families of 50 in length order -- 16 pairs per query and group:
    // the pair kernel gains 18 % from the bitmaps, the candidate stage costs more than that; against the ROUNDS of the
    // first kernel -- no tag words: long k-mers on mid-size genomes -- the bitmaps win from two pairs per query on.)
    const u64 min_share = k.pm_min_share.value_or(c->gs.lay.tw_stride ? 48 : 2);
    const bool lists_ok = !lists || (!f.lists_dup && f.n_pairs >= min_share * f.lists_involved);
    if (!(!regions && lists_ok && c->gs.tab.kmL && c->gs.lay.bk_stride && c->P.mqd + c->P.mrd <= 128 && c->gs.geo.kb <= 30 &&
          g.n >= 2 && n_rows >= min_rows && k.pm))
        return LZANI_OK;
    u64 max_row = 0;
    for (u32 r = 0; r < n_rows; ++r) max_row = std::max<u64>(max_row, row_off[r + 1] - row_off[r]);
    p.pm_tiles = (u32)(((u64)p.Lmax + c->P.mrd + 320 + PM_TILE - 1) / PM_TILE);
    p.cb_words = (u64)p.pm_tiles * PM_TILE_WORDS;
    p.pm_group = p.pm_bits <= 27 ? (u32)PM_GROUP : 128u;                    // 64-byte rows up to 2^27 of them (8 GB), 16-byte rows beyond (16 GB at 2^30)
    const size_t m_bytes = ((size_t)1 << p.pm_bits) * (p.pm_group / 8);
    const size_t x_bytes = lists ? ((size_t)g.n * p.pm_group + 2 * (size_t)g.n + 64) * 4 : 0;   // pair table, query flags, list, count
    const size_t per_pair = (size_t)p.cb_words * 4;
    const double avg_row = (double)f.n_pairs / n_rows;
    const size_t per_slot = (size_t)slot_bytes(c->gs).total();
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    // what this run may lay out anew: the free memory and what the context holds from earlier runs -- ITS slabs
    // included, which is why slabs larger than this run wants are released below (ensure_slabs never shrinks them:
    // an earlier run with sparse rows may have grown them to 60 % of the memory)
    const size_t pool = free_b + (size_t)c->sl.slots * per_slot + c->cs.d_pm_cbits.bytes() + c->cs.d_pm.bytes() + c->cs.d_pm_pidx.bytes();
    const size_t cap = k.pm_max_bytes.value_or(std::min((size_t)64 << 30, total_b / 4));
    const double room = pool * 0.85 - (double)m_bytes - (double)x_bytes;
    u64 fit = room > 0 ? (u64)(room / ((double)per_slot + avg_row * (double)per_pair)) : 0;     // rows: a slab + its pairs' bitmaps each
    fit = std::min<u64>(fit, std::min<u32>(n_rows, c->gs.lay.max_slots));
    u64 cap_pairs = std::min<u64>((u64)(cap / per_pair), 0xFFFFFFF0ull);                           // pair indexes of a batch are 32 bits
    cap_pairs = std::min<u64>(cap_pairs, (u64)((double)fit * avg_row) + max_row);
    if (fit < std::min<u32>(8, n_rows) || cap_pairs < max_row) return LZANI_OK;
    if (c->sl.slots > fit) c->sl = IndexSlabs{};                                     // (counted as available above)
    if (!got(c->cs.d_pm.reserve(m_bytes / 4)) || !got(c->cs.d_pm_pidx.reserve(x_bytes / 4))) {
        TRACE("candidate bitmaps: no memory for the matrix / pair table, falling back");
        c->cs = CandScratch{};
        return LZANI_OK;
    }
    const int rc = ensure_slabs(c, (u32)fit);
    if (rc == LZANI_ERR_NOMEM) { c->cs = CandScratch{}; return LZANI_OK; }
    if (rc) return rc;
    u32 rows_cap = c->sl.slots;
    if (!lists) {                                            // dense rows: whole groups of references, if there are several batches
        u64 r = std::min<u64>(rows_cap, cap_pairs / (u64)(g.n - 1));
        if (r < n_rows && r > p.pm_group) r -= r % p.pm_group;
        rows_cap = (u32)std::max<u64>(r, 1);
    }
    size_t need = (size_t)cut_batches(n_rows, row_off, rows_cap, cap_pairs, p.bstart) * p.cb_words * 4;
    if (k.pm_fail_cbits) need = (size_t)1 << 60;                          // tests: the fallback
    if (!got(c->cs.d_pm_cbits.reserve(need / 4))) {
        TRACE("candidate bitmaps: no memory for %zu bytes of bitmaps, falling back", need);
        c->cs = CandScratch{};
        return LZANI_OK;
    }
    p.pm = true;
    return LZANI_OK;
}

// The split / LPT choice of the batch's pair launch (choose_split, lzani_run_plan.h) and the buffer of the candidate
// counts it wants, cleared.  (Candidate bitmaps only: no regions, mqd + mrd <= 128.)
int choose_split_lpt(RunCtx& r, Batch& bt)
{
    lzani_ctx* c = r.c;
    const u64 bp = bt.e1 - bt.e0;
    const SplitChoice ch = choose_split(bp, (u64)r.max_blocks * 4, r.p.cb_words, r.p.Lmax + c->P.mrd,
                                        SplitKnobs{r.k.split, r.k.lpt, r.k.split_s, r.k.split_seglen});
    bt.split_S = ch.split_S; bt.split_seglen = ch.split_seglen; bt.lpt = ch.lpt;
    if (bt.lpt && c->cs.d_lpt_cnt.capacity() < bp) {
        c->cs.d_lpt_cnt.reset(); c->cs.d_lpt_keys.reset();    // (both released before either is made anew)
        if (!got(c->cs.d_lpt_cnt.alloc(bp)) || !got(c->cs.d_lpt_keys.alloc(2 * bp))) {
            c->cs.d_lpt_cnt.reset(); c->cs.d_lpt_keys.reset();
            bt.lpt = false;                                   // (placement only: the run goes on without it)
        }
    }
    if (bt.lpt) HIPCHK(c, hipMemsetAsync(c->cs.d_lpt_cnt, 0, (size_t)bp * 4, c->stream));
    return LZANI_OK;
}

// The instantiations of the two matrix kernels by the words of a matrix row (rw: 4, 8, 12 or 16).
using PmFromIndexFn = decltype(&k_pm_from_index<4>);
PmFromIndexFn pm_from_index_fn(u32 rw)
{
    switch (rw) {
    case 4: return k_pm_from_index<4>;
    case 8: return k_pm_from_index<8>;
    case 12: return k_pm_from_index<12>;
    default: return k_pm_from_index<16>;
    }
}
using PmCandFn = decltype(&k_pm_cand<1>);
PmCandFn pm_cand_fn(u32 rw)
{
    switch (rw / 4) {
    case 1: return k_pm_cand<1>;
    case 2: return k_pm_cand<2>;
    case 3: return k_pm_cand<3>;
    default: return k_pm_cand<4>;
    }
}

// The candidate bitmaps of the batch's pairs, group by group of pm_group references; then the ticket order of its queues.
int candidate_stage(RunCtx& r, Batch& bt)
{
    lzani_ctx* c = r.c;
    const RunPlan& p = r.p;
    const int pm_bits = p.pm_bits;
    const u32 n = r.g.n;                                     // genomes of the run's table
    for (u32 g0 = 0; g0 < bt.rows; g0 += p.pm_group) {
        PmArgs pg;
        pg.G = gtab(c);
        pg.ref_ids = r.d_ref + bt.k0; pg.row_off = r.d_off + bt.k0;
        pg.slot0 = g0; pg.rows = std::min<u32>(p.pm_group, bt.rows - g0);
        pg.M = c->cs.d_pm; pg.rw = ((pg.rows + 127) / 128) * 4; pg.mmask = (u32)lowmask(pm_bits); pg.rshift = c->gs.geo.kb - pm_bits;
        pg.mal = c->P.mal; pg.mrd = c->P.mrd;
        pg.cbits = c->cs.d_pm_cbits; pg.cb_words = p.cb_words; pg.e0 = bt.e0; pg.n = n; pg.q0 = 0;
        pg.query_ids = r.d_q; pg.pidx = nullptr; pg.qflag = pg.qlist = pg.qcount = nullptr;
        pg.pcount = bt.lpt ? c->cs.d_lpt_cnt : nullptr;
        if (r.query_ids) {                                   // the lists of the group's rows -> pair table + the queries involved
            const size_t tab = (size_t)n * 32 * pg.rw;
            pg.pidx = c->cs.d_pm_pidx; pg.qflag = c->cs.d_pm_pidx + (size_t)n * p.pm_group; pg.qlist = pg.qflag + n; pg.qcount = pg.qlist + n;
            HIPCHK(c, hipMemsetAsync(pg.pidx, 0xFF, tab * 4, c->stream));
            HIPCHK(c, hipMemsetAsync(pg.qflag, 0, ((size_t)2 * n + 1) * 4, c->stream));
            hipLaunchKernelGGL(k_pm_pairs, dim3(pg.rows), dim3(256), 0, c->stream, pg);
        }
        // the matrix: from the group's indexes, chunk by chunk through LDS (long genomes: no global atomics, no clearing),
        // or by one atomicOr per text position into the cleared matrix
        const int tbits = c->gs.geo.kb - c->gs.geo.dirbits;
        // (chunks of 64 KB: two blocks = 32 waves a CU; with 128 KB chunks, one block a CU, the matrix of 128 x 5 Mbp took 3 ms more)
        const int rcl = std::min(pm_bits, pg.rw <= 4 ? 12 : pg.rw <= 8 ? 11 : 10);
        const bool from_index = c->gs.geo.tagmask == (u32)lowmask(tbits) && pm_bits == c->gs.geo.kb && rcl >= tbits &&
                                r.k.pm_from_index.value_or(pm_bits > 24);
        if (from_index) {
            c->run.pmfi_launches += 1;
            const size_t fl = ((size_t)pg.rw << rcl) * 4;
            const PmFromIndexFn kfi = pm_from_index_fn(pg.rw);
            { int rc = raise_lds(c, kfi, 128 * 1024); if (rc) return rc; }
            hipLaunchKernelGGL(kfi, dim3(1u << (pm_bits - rcl)), dim3(1024), fl, c->stream, pg, c->sl.d_dirz, c->sl.d_ent, c->gs.dir_stride, c->gs.ent_stride,
                               tbits, c->gs.geo.posbits, rcl);
        } else {
            HIPCHK(c, hipMemsetAsync(c->cs.d_pm, 0, ((size_t)1 << pm_bits) * pg.rw * 4, c->stream));
            hipLaunchKernelGGL(k_pm_build, dim3((u32)std::min<u64>(((u64)c->gs.Tmax + 255) / 256, 64), pg.rows), dim3(256), 0, c->stream, pg, c->gs.Tmax);
        }
        const u32 rp = 32 * pg.rw;
        const size_t lds = (size_t)(PM_TILE_WORDS * (rp + 1) + rp) * 4;
        const PmCandFn kc = pm_cand_fn(pg.rw);
        { int rc = raise_lds(c, kc, (size_t)(PM_TILE_WORDS * (PM_GROUP + 1) + PM_GROUP) * 4); if (rc) return rc; }      // (what a full group takes)
        // (query lists: one row of blocks per query that occurs in the group -- counted here, the device list is
        // k_pm_pairs' -- not per genome: 20,000 genomes x 44 tiles of blocks that find nothing to do were most of
        // the candidate stage of a filtered run)
        u32 nq = n;
        if (r.query_ids) {
            if (r.grp_seen.size() != n) r.grp_seen.assign(n, 0xFFFFFFFFu);
            const u32 stamp = ++r.grp_stamp;
            nq = 0;
            for (u64 e = r.row_off[bt.k0 + g0]; e < r.row_off[bt.k0 + g0 + pg.rows]; ++e)
                if (r.grp_seen[r.query_ids[e]] != stamp) { r.grp_seen[r.query_ids[e]] = stamp; ++nq; }
        }
        for_slices(nq, [&](u32 q0, u32 cnt) {
            pg.q0 = q0;
            c->run.pmc_launches += 1;
            hipLaunchKernelGGL(kc, dim3(p.pm_tiles, cnt), dim3(PM_CAND_THREADS), lds, c->stream, pg);
        });
        c->run.tm.cand_launches += 2;
    }
    if (!bt.lpt || c->cs.d_lpt_cnt == nullptr) bt.split_S = 0;   // (no candidate counts after all -- their buffer could not be had: no split)
    if (bt.lpt && bt.split_S < 2) {                            // the ticket order of the batch's queues
        const u64 bp = bt.e1 - bt.e0;
        QueueBounds qbv;
        for (int x = 0; x <= NQUEUES; ++x) qbv.v[x] = bt.qb[x];
        hipLaunchKernelGGL(k_lpt_keys, dim3((u32)std::min<u64>((bp + 255) / 256, 4096)), dim3(256), 0, c->stream,
                           r.d_qorder + bt.k0, r.d_qcum + bt.k0 + bt.b, qbv, r.d_off + bt.k0, bt.e0, c->cs.d_lpt_cnt, c->cs.d_lpt_keys, bt.rows, bp);
        if (int rc = sort_keys(c, c->gs.d_jtmp, c->cs.d_lpt_keys, c->cs.d_lpt_keys + bp, bp, 1, 32, 56, "ticket order: radix sort", true)) return rc;
    }
    HIPCHK(c, hipGetLastError());
    return LZANI_OK;
}

// Few, long pairs: several waves a pair (lzani_kernels_split.h) -- the checkpoints, then rounds of segments until the stitch
// has every pair.  row: the mode-0 row of the batch's k_split in PAIR_KERNELS (choose_pair_kernel), mode 1 the row behind it.
// The buffers are CandScratch's, grown here and kept: a batch of the same or a smaller size allocates nothing.  Where
// their last use is ordered: everything that touches them -- the memsets below, the two uploads, k_split (cuts, heavy, its
// work list, outs, the ticket counter), k_split_stitch (cuts, outs, done, the counters, the next round's list) -- is work of the context's one stream, and the last of it, the final round's stitch, lies before the
// hipStreamSynchronize that ends that round (the host reads the counters there).  So the next batch's memsets are ordered
// behind every earlier use by the stream alone, a buffer that has to grow is released by hipFree, which waits for the
// device, and nothing outside this function reads them: the device-wide wait of the per-batch hipFree was not relied on.
int run_split(RunCtx& r, const Batch& bt, const PairArgs& pa, int row)
{
    lzani_ctx* c = r.c;
    CandScratch& cs = c->cs;
    c->run.pm_launches += 1;
    c->run.split_launches += 1;
    const u32 npb = (u32)(bt.e1 - bt.e0), S = bt.split_S;
    const size_t n_seg = (size_t)npb * S;
    HIPCHK(c, cs.d_sp_cuts.reserve(n_seg));
    HIPCHK(c, cs.d_sp_outs.reserve(n_seg));
    HIPCHK(c, cs.d_sp_work.reserve(n_seg));
    HIPCHK(c, cs.d_sp_next.reserve(n_seg));
    HIPCHK(c, cs.d_sp_cnt.reserve(12));
    HIPCHK(c, cs.d_sp_done.reserve(npb));
    HIPCHK(c, cs.d_sp_heavy.reserve(npb));
    HIPCHK(c, hipMemsetAsync(cs.d_sp_cnt.get(), 0, 48, c->stream));
    HIPCHK(c, hipMemsetAsync(cs.d_sp_done.get(), 0, npb, c->stream));
    HIPCHK(c, hipMemsetAsync(cs.d_sp_cuts.get(), 0xFF, n_seg * sizeof(SplitStart), c->stream));      // (cut 0 of every pair: no checkpoint)
    SplitArgs sa;
    sa.pa = pa; sa.rows = bt.rows; sa.n_pairs = npb; sa.S = S; sa.seglen = bt.split_seglen;
    sa.cuts = cs.d_sp_cuts.get(); sa.outs = cs.d_sp_outs.get(); sa.work = cs.d_sp_work.get(); sa.work_next = cs.d_sp_next.get();
    sa.counters = cs.d_sp_cnt.get(); sa.done = cs.d_sp_done.get(); sa.heavy = cs.d_sp_heavy.get();
    sa.reg = c->P.reg; sa.last_round = 0;
    auto launch = [&](int mode, u32 items) {
        sa.n_work = items;
        void* kargs[] = {&sa};
        return launch_row(c, row + mode, dim3((u32)std::min<u64>(((u64)items + 3) / 4, r.max_blocks)), dim3(256), kargs);
    };
    // which pairs to cut: the ones with many anchor candidates (related: a candidate at every other position; a chance
    // pair has one in a hundred and is scanned whole, by its segment 0 with the null chain at work) -- heaviest first
    u32 items = 0, n_heavy = 0;
    {
        std::vector<u32> cnt(npb);
        HIPCHK(c, hipMemcpyAsync(cnt.data(), cs.d_lpt_cnt, (size_t)npb * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        // (every pair by default: at a wave or two per SIMD a chance pair of 5 Mbp takes nearly as long as a related one;
        // LZANI_SPLIT_ALL=0 cuts the pairs with a candidate at one position in 32 and more only)
        const u32 thr = !r.k.split_all ? (u32)r.p.cb_words : r.k.split_thr;
        std::vector<u32> order(npb);
        for (u32 k = 0; k < npb; ++k) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](u32 x, u32 y) { return cnt[x] > cnt[y]; });
        std::vector<unsigned char> heavy(npb, 0);
        std::vector<u32> all;
        all.reserve((size_t)npb * 2);
        for (u32 k : order) if (cnt[k] >= thr) { heavy[k] = 1; ++n_heavy; for (u32 sg = 0; sg < S; ++sg) all.push_back(k * S + sg); }
        for (u32 k : order) if (cnt[k] < thr) all.push_back(k * S);
        items = (u32)all.size();
        HIPCHK(c, hipMemcpyAsync(cs.d_sp_heavy.get(), heavy.data(), npb, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(cs.d_sp_work.get(), all.data(), all.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));            // (the vectors leave scope)
        TRACE("split: %u pairs, %u of them cut into %u segments (candidates >= %u)", npb, n_heavy, S, thr);
    }
    HIPCHK(c, launch(0, npb * (S - 1)));                    // the checkpoints
    u32* cur = cs.d_sp_work.get(); u32* nxt = cs.d_sp_next.get();
    auto t_round = std::chrono::steady_clock::now();
    // (a chain of void segments costs a round each: more segments, more rounds allowed; LZANI_SPLIT_GIVE_UP: a diagnostic switch)
    const int give_up = std::max(0, r.k.split_give_up.value_or(6 + (int)S / 4));
    c->run.split_cut += n_heavy;
    u32 last[12] = {0};
    for (int round = 0; round < give_up + 4 && items; ++round) {
        HIPCHK(c, hipMemsetAsync(cs.d_sp_cnt.get(), 0, 8, c->stream));     // tickets, next round's items (the finished pairs' count stays)
        sa.work = cur; sa.work_next = nxt;
        HIPCHK(c, launch(1, items));
        sa.last_round = round >= give_up;
        hipLaunchKernelGGL(k_split_stitch, dim3((npb + 255) / 256), dim3(256), 0, c->stream, sa);
        u32 cnt[12] = {0};
        HIPCHK(c, hipMemcpyAsync(cnt, cs.d_sp_cnt.get(), 48, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->run.split_items += items;
        c->run.split_rounds = std::max(c->run.split_rounds, (u32)round + 1);
        std::copy(cnt, cnt + 12, last);
        const auto t_now = std::chrono::steady_clock::now();
        TRACE("split: round %d ran %u segments in %.1f ms, %u pairs finished, %u segments to run again (void so far, by cause: look-back cut short %u, kept/dropped %u, dropped/kept %u, floor %u, guess %u, chain %u)",
              round, items, std::chrono::duration<double, std::milli>(t_now - t_round).count(), cnt[2], cnt[1], cnt[4], cnt[5], cnt[6], cnt[7], cnt[8], cnt[9]);
        t_round = t_now;
        items = cnt[1];
        std::swap(cur, nxt);
        if (items == 0 && cnt[2] != npb) return fail(c, LZANI_ERR_DEVICE, "split pairs: the stitch left pairs behind");
    }
    if (items) return fail(c, LZANI_ERR_DEVICE, "split pairs: no end of rounds");
    // (the stitch's counters run through the batch's rounds: the last round's copy is the batch's sum)
    for (int k = 0; k < 6; ++k) c->run.split_void[k] += last[4 + k];
    c->run.split_resumed += last[10]; c->run.split_given_up += last[11];
    return LZANI_OK;
}

// Test hook: the batch's candidate bitmaps (and counts) into the run's CandSink, after its candidate stage.
int sink_candidates(RunCtx& r, const Batch& bt)
{
    lzani_ctx* c = r.c;
    CandSink& s = *r.sink;
    const u64 bp = bt.e1 - bt.e0, w = std::min<u64>(s.words, r.p.cb_words);
    if (s.cbits && w)
        HIPCHK(c, hipMemcpy2DAsync(s.cbits + bt.e0 * s.words, s.words * 4, c->cs.d_pm_cbits, r.p.cb_words * 4, w * 4, bp,
                                   hipMemcpyDeviceToHost, c->stream));
    if (s.pcount && bt.lpt && c->cs.d_lpt_cnt) {
        HIPCHK(c, hipMemcpyAsync(s.pcount + bt.e0, c->cs.d_lpt_cnt, bp * 4, hipMemcpyDeviceToHost, c->stream));
        s.counted_batches += 1;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LZANI_OK;
}

}  // namespace
