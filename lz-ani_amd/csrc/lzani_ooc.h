// lzani_ooc.h -- genome sets larger than the device: block uploads and the tiled run.  Included by lzani_hip.hip only,
// after run_rows_impl, which every tile calls on its own genome table; of that file it uses lzani_ctx, RunGenomes, check_rows,
// RunRecord, RegionSink, fail, HIPCHK and TRACE, of lzani_index.h for_slices, pack_genomes and launch_kmers.  The block plan
// and the footprint of a genome (plan_blocks_impl, ooc_genome_bytes) are lzani_set_plan.h; the decisions of a tiled run --
// the steps below, every tile's local tables, the tables of an upload -- are lzani_tile_plan.h, and this file is their driver.
//
// A set whose genome tables (packed texts, N masks, k-mer words, join lists) do not fit a genome-memory limit stays on
// the host (1 B per base).  Its genomes are cut, in id order, into contiguous blocks of at most limit / 2 bytes of
// tables each; the device holds two of them at a time, half A (the reference block) and half B (a query block).
// A run goes tile by tile over (reference block i, query block j): each tile is a run_rows_impl call on a local genome
// table of A's genomes (local ids 0 .. nA-1) and B's (nA ..), and its results are scattered to their CSR positions.
//
// Order of a run (what lzani_get_residency counts, and what a caller can predict):
//   reference blocks ascending, those with rows only; block i goes to A -- no upload if A holds it, the two halves
//   trade places if B holds it, else one upload;
//   then its query blocks: i itself first (its queries are in A), then the block B holds if it has pairs of these rows,
//   then the others ascending; every block that B does not hold yet is one upload.
// The halves keep their blocks from run to run; lzani_set_genomes starts a fresh GenomeSet (the context's `gs`, which owns
// the host copy, the resident region and the upload staging) and so empties them.
#pragma once

namespace {

// Results of a tile (local CSR order) -> their places in the caller's CSR order: pos[e] for the tile's pair e.
__global__ void k_scatter_pairs(const int* __restrict__ src, int* __restrict__ dst, const u64* __restrict__ pos, u64 n)
{
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const u64 d = 3 * pos[e];
    dst[d] = src[3 * e];
    dst[d + 1] = src[3 * e + 1];
    dst[d + 2] = src[3 * e + 2];
}

// Region records of a tile: `pair` is the tile's CSR position; it becomes the caller's.
__global__ void k_remap_regions(lzani_region* __restrict__ r, u64 n, const u64* __restrict__ pos)
{
    const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) r[k].pair = pos[r[k].pair];
}

// What the plan's genome tables are made from (lzani_tile_plan.h), of the context's set.
TileSet tile_set_of(const GenomeSet& gs)
{
    return TileSet{gs.blk_first, gs.L, gs.nmoff, gs.h_hasN, gs.h_codeoff, gs.half_words, gs.half_genomes};
}

// The upload of an out-of-core set: block b from the host copy into half h -- staging, k_pack and k_kmers on the
// block's genomes only (pack_genomes / launch_kmers of lzani_index.h, slice by slice), by the tables of
// plan_tile_upload.  Timed into res.upload_ms.
int ooc_upload(lzani_ctx* c, u32 b, int h)
{
    c->gs.half_block[h] = -1;                                     // (until the upload is complete)
    const u32 cnt = c->gs.blk_first[b + 1] - c->gs.blk_first[b], hg = c->gs.half_genomes;
    const TileUpload u = plan_tile_upload(tile_set_of(c->gs), b, h);
    StreamSpan span;
    float ms = 0;
    HIPCHK(c, span.begin(c->stream));
    if (u.bases) HIPCHK(c, hipMemcpyAsync(c->gs.d_stage, c->gs.h_codes.data() + u.code0, u.bases, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->gs.d_up_tab, u.tab.data(), u.tab.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->gs.d_up_L, u.Ls.data(), u.Ls.size() * 4, hipMemcpyHostToDevice, c->stream));
    const int Tb = ref_text_len(u.Lmax, c->P.mrd);
    const GenomeTables& t = c->gs.tab;
    for_slices(cnt, [&](u32 k0, u32 k) {
        pack_genomes(c, c->gs.d_stage, c->gs.d_up_tab, t.t2, t.nm, c->gs.d_up_tab + hg, c->gs.d_up_L, c->gs.d_up_L + hg, Tb, k0, k);
        if (t.kmL) launch_kmers(c, GenomeTab{t.t2, t.nm, c->gs.d_up_tab + hg, c->gs.d_up_L, t.kmL, t.kmS, c->gs.d_up_L + hg + k0}, Tb, k0, k);
    });
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, span.end(c->stream));
    HIPCHK(c, span.elapsed(ms));                                  // (also: the upload's host tables leave scope)
    c->res.upload_ms += ms;
    c->res.uploads += 1;
    c->gs.half_block[h] = (int)b;
    return LZANI_OK;
}

// The tiled run: the contract of run_rows_impl, with the results written to d_out (device, caller's CSR order) and / or
// h_out (host), regions to rs with `pair` in the caller's CSR order.  The steps, the row tables of a reference block's
// tiles and a tile's genome table are the plan's (lzani_tile_plan.h); here they are copied, launched, waited for, counted.
int run_rows_tiled(lzani_ctx* c, u32 n_rows, const u32* ref_ids, const u64* row_off, const u32* query_ids,
                   int* d_out, lzani_result* h_out, const RegionSink* rs)
{
    c->run = RunRecord{};
    c->res = Residency{};
    if (n_rows == 0) return LZANI_OK;
    RowFacts rf;
    const int rc0 = check_rows(c, run_genomes_of(c), n_rows, ref_ids, row_off, query_ids, rf);
    if (rc0 || rf.n_pairs == 0) return rc0;
    HIPCHK(c, hipSetDevice(c->dev));

    const TileRows rows{n_rows, ref_ids, row_off, query_ids};
    const std::vector<u32> bof = block_of_genomes(c->gs.blk_first);
    Halves halves{{c->gs.half_block[0], c->gs.half_block[1]}, c->gs.half_a};      // the state now; after the plan, the state the steps lead to
    const std::vector<TileStep> steps = plan_tile_steps(c->gs.blk_first, bof, rows, halves);

    RunRecord tot;
    u64 reg_done = 0;
    DevMem<lzani_result> d_res;                            // grow as the tiles need
    DevMem<u64> d_pos;
    std::vector<lzani_result> h_res;
    std::vector<TileTable> tiles;
    for (const TileStep& s : steps) {
        plan_tile_tables(c->gs.blk_first, bof, rows, s, tiles);
        c->gs.half_a = s.half_a;
        if (s.a == TILE_A_UPLOADS) { int rc = ooc_upload(c, s.i, s.half_a); if (rc) return rc; }
        for (const TileStep::Query& sq : s.q) {
            const int hB = s.half_a ^ 1;
            if (sq.b_upload) { int rc = ooc_upload(c, sq.j, hB); if (rc) return rc; }
            c->res.peak = std::max<u64>(c->res.peak, c->gs.blk_bytes[s.i] + (c->gs.half_block[hB] >= 0 ? c->gs.blk_bytes[c->gs.half_block[hB]] : 0));
            const TileTable& t = tiles[sq.j];
            const TileGenomes g = plan_tile_genomes(tile_set_of(c->gs), s.i, sq.j, s.half_a);
            const u64 tp = t.pairs();
            HIPCHK(c, hipMemcpyAsync(c->gs.tab.L, g.L.data(), g.L.size() * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(c->gs.tab.hasN, g.hasN.data(), g.hasN.size() * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(c->gs.tab.nmoff, g.nmoff.data(), g.nmoff.size() * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, d_res.reserve(tp));
            if (d_out || rs) {
                HIPCHK(c, d_pos.reserve(tp));
                HIPCHK(c, hipMemcpyAsync(d_pos.get(), t.pos.data(), tp * 8, hipMemcpyHostToDevice, c->stream));
            }
            HIPCHK(c, hipStreamSynchronize(c->stream));            // (the copies above read pageable host vectors: they are done before the tile's run begins)
            if (c->gs.lay.join_mode) c->gs.jl = JoinLists{};                   // (made again for this tile's table, if its form needs them)
            const int rc = run_rows_impl(c, RunGenomes{(u32)g.L.size(), g.L.data()}, (u32)t.rows.size(), t.lref.data(), t.off.data(), t.lq.data(),
                                         (int*)d_res.get(), rs);
            if (c->gs.lay.join_mode) c->gs.jl = JoinLists{};
            if (rc) return rc;
            c->res.tiles += 1;
            tot += c->run;
            if (d_out) {
                hipLaunchKernelGGL(k_scatter_pairs, dim3((u32)((tp + 255) / 256)), dim3(256), 0, c->stream, (const int*)d_res.get(), d_out, d_pos.get(), tp);
                HIPCHK(c, hipGetLastError());
            }
            if (h_out) {
                h_res.resize(tp);
                HIPCHK(c, hipMemcpyAsync(h_res.data(), d_res.get(), tp * sizeof(lzani_result), hipMemcpyDeviceToHost, c->stream));
            }
            if (rs) {
                unsigned long long cnt = 0;
                HIPCHK(c, hipMemcpyAsync(&cnt, rs->d_count, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                const u64 lo = std::min<u64>(reg_done, rs->capacity), hi = std::min<u64>(cnt, rs->capacity);
                if (hi > lo) {
                    hipLaunchKernelGGL(k_remap_regions, dim3((u32)((hi - lo + 255) / 256)), dim3(256), 0, c->stream, rs->d_regions + lo, hi - lo, d_pos.get());
                    HIPCHK(c, hipGetLastError());
                }
                reg_done = cnt;
            }
            HIPCHK(c, hipStreamSynchronize(c->stream));            // (the host tables of the tile leave scope)
            if (h_out) for (u64 e = 0; e < tp; ++e) h_out[t.pos[e]] = h_res[e];
        }
    }
    assert(halves.a == c->gs.half_a && halves.block[0] == c->gs.half_block[0] && halves.block[1] == c->gs.half_block[1]);
    c->run = tot;
    TRACE("out-of-core run: %u tiles, %llu block uploads (%.1f ms)", c->res.tiles, (unsigned long long)c->res.uploads, c->res.upload_ms);
    return LZANI_OK;
}

// lzani_set_genomes for a set that does not stay in-core: it keeps a host copy of its codes and the device region of
// the two halves; the blocks are uploaded by the runs.
int ooc_set_genomes(lzani_ctx* c, u32 n, const uint8_t* const* codes, const uint32_t* len)
{
    const u32 nb = (u32)c->gs.blk_first.size() - 1;
    try {
        c->gs.h_codeoff.assign((size_t)n + 1, 0);
        for (u32 g = 0; g < n; ++g) c->gs.h_codeoff[g + 1] = c->gs.h_codeoff[g] + len[g];
        c->gs.h_codes.resize(c->gs.h_codeoff[n]);
        c->gs.h_hasN.assign(n, 0);
    } catch (const std::bad_alloc&) {
        return fail(c, LZANI_ERR_NOMEM, "lzani_set_genomes: host copy of an out-of-core genome set");
    }
    for (u32 g = 0; g < n; ++g) {
        if (len[g]) memcpy(c->gs.h_codes.data() + c->gs.h_codeoff[g], codes[g], len[g]);
        c->gs.h_hasN[g] = std::any_of(codes[g], codes[g] + len[g], [](uint8_t v) { return v >= 4; });
    }
    c->gs.all_nfree = std::none_of(c->gs.h_hasN.begin(), c->gs.h_hasN.end(), [](int v) { return v != 0; });
    u64 max_bases = 0;
    for (u32 b = 0; b < nb; ++b) {
        const u32 g0 = c->gs.blk_first[b], g1 = c->gs.blk_first[b + 1];
        c->gs.half_words = std::max<u64>(c->gs.half_words, (g1 < n ? c->gs.nmoff[g1] : c->gs.total_nm) - c->gs.nmoff[g0]);
        c->gs.half_genomes = std::max<u32>(c->gs.half_genomes, g1 - g0);
        max_bases = std::max<u64>(max_bases, c->gs.h_codeoff[g1] - c->gs.h_codeoff[g0]);
    }
    const u64 hw = c->gs.half_words, hg = c->gs.half_genomes;
    GenomeTables t;                                               // (moved into the set whole, or not at all)
    DevMem<uint8_t> stage;
    DevMem<u64> up_tab;
    DevMem<int> up_L;
    HIPCHK(c, t.t2.alloc(2 * hw * 2));
    HIPCHK(c, t.nm.alloc(2 * hw));
    if (kmer_words_of(c->P)) {
        HIPCHK(c, t.kmL.alloc(2 * hw * 64));
        HIPCHK(c, t.kmS.alloc(2 * hw * 64));
    }
    HIPCHK(c, t.nmoff.alloc(2 * hg));
    HIPCHK(c, t.L.alloc(2 * hg));
    HIPCHK(c, t.hasN.alloc(2 * hg));
    HIPCHK(c, stage.alloc(max_bases));
    HIPCHK(c, up_tab.alloc(2 * hg));
    HIPCHK(c, up_L.alloc(2 * hg));
    c->gs.tab = std::move(t);
    c->gs.d_stage = std::move(stage); c->gs.d_up_tab = std::move(up_tab); c->gs.d_up_L = std::move(up_L);
    c->gs.total_nm = 2 * hw;                                          // (lzani_get_layout: the resident region's bytes)
    c->gs.kmers_ready = true;                                         // (made by every block upload)
    c->gs.ooc = true;
    c->gs.n = n;
    TRACE("set_genomes: out-of-core, n=%u blocks=%u limit=%llu half=%llu words", n, nb, (unsigned long long)c->gs.mem_limit, (unsigned long long)hw);
    return LZANI_OK;
}

}  // namespace
