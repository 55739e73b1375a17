// lzani_index.h -- host side of the index stage: everything between lzani_set_genomes and a batch's pair launch.  The
// in-core genome upload, the index slabs, the k-mer words and the join lists of a genome set, the index build of a batch's
// references, and the two index test hooks.  Included by lzani_hip.hip only, behind the context and Knobs; of that file it
// uses lzani_ctx (which holds the GenomeSet, its JoinLists and the IndexSlabs), Knobs, fail, HIPCHK, TRACE, raise_lds and
// sort_keys.  The pure decisions -- the form of the index, the footprints, the slot count of the slabs -- are
// lzani_set_plan.h, the bytes of a slab slot lzani_run_plan.h; the kernels are lzani_kernels_index.h.
// Host only: not among the sources a run-time compile embeds (lzani_rtc.h).
//
// Order of work:
//   upload_genomes   lzani_set_genomes, in-core set: tables, the codes through two pinned staging buffers, k_pack
//                    (an out-of-core set packs block by block: ooc_upload of lzani_ooc.h, by the same launches)
//   first run after lzani_set_genomes:
//     ensure_kmers   the k-mer words of every genome (timed: kmers_ms)
//     ensure_join    join form only: the sorted k-mer lists (their time is added to kmers_ms) -- before ...
//     ensure_slabs   ... the slabs, which take 60 % of what is left, at most a slot per row of the run
//   per batch (run_batch): build_indexes into slots 0 .. rows-1
// The two index test hooks of the C-ABI (lzani_debug_get_index, lzani_debug_index_slab) are defined at the end of this file.
#pragma once

namespace {

// A launch per slice of at most 32,768 genomes (gridDim.y is limited to 65535): f(first genome, genomes).
template <class F>
void for_slices(u32 n, F&& f)
{
    for (u32 g0 = 0; g0 < n; g0 += 32768) f(g0, std::min<u32>(32768, n - g0));
}

GenomeTab gtab(const lzani_ctx* c)
{
    const GenomeTables& t = c->gs.tab;
    return GenomeTab{t.t2, t.nm, t.nmoff, t.L, t.kmL, t.kmS, t.hasN};
}

// One slice of k_pack: `cnt` genomes from g0 on, codes[codeoff[g]] -> packed text and N mask at nmoff[g], hasN[g] set
// where a genome holds an N.  Tmax: the longest text among them.
void pack_genomes(lzani_ctx* c, const uint8_t* codes, const u64* codeoff, u64* t2, u64* nm, const u64* nmoff, const int* L, int* hasN,
                  int Tmax, u32 g0, u32 cnt)
{
    hipLaunchKernelGGL(k_pack, dim3((u32)((text_wordsN(Tmax) + 127) / 128), cnt), dim3(128), 0, c->stream,
                       codes, codeoff + g0, t2, nm, nmoff + g0, L + g0, hasN + g0, c->P.mrd, cnt);
}

// One slice of k_kmers: the k-mer words of `cnt` genomes of G from g0 on, into the set's k-mer arrays.
void launch_kmers(lzani_ctx* c, GenomeTab G, int Tmax, u32 g0, u32 cnt)
{
    G.nmoff += g0; G.L += g0;
    hipLaunchKernelGGL(k_kmers, dim3((Tmax + 255) / 256, cnt), dim3(256), 0, c->stream,
                       G, c->gs.tab.kmL, c->gs.tab.kmS, c->P.mal, c->P.msl, c->P.mrd, Tmax);
}

// lzani_set_genomes for a set that stays in-core: the tables, the codes of every genome, k_pack.
int upload_genomes(lzani_ctx* c, u32 n, const uint8_t* const* codes, const uint32_t* len, const std::vector<u64>& codeoff, u64 total_codes)
{
    const u64 total_nm = c->gs.total_nm;
    DevMem<uint8_t> d_codes;
    DevMem<u64> d_codeoff;
    HIPCHK(c, d_codes.alloc(total_codes));
    HIPCHK(c, d_codeoff.alloc(n));
    {
        GenomeTables t;                                       // (moved into the set whole, or not at all)
        HIPCHK(c, t.t2.alloc(total_nm * 2));
        HIPCHK(c, t.nm.alloc(total_nm));
        HIPCHK(c, t.nmoff.alloc(n));
        HIPCHK(c, t.L.alloc(n));
        HIPCHK(c, t.hasN.alloc(n));
        HIPCHK(c, hipMemset(t.hasN, 0, (size_t)n * 4));
        if (kmer_words_of(c->P)) {
            HIPCHK(c, t.kmL.alloc(total_nm * 64));
            HIPCHK(c, t.kmS.alloc(total_nm * 64));
        }
        c->gs.tab = std::move(t);
    }
    // The caller's sequences are separate host buffers: they go up through two pinned 64 MB staging buffers, the
    // copy of one overlapping the fill of the other (the 4 GB of config 5 take as long as the PCIe link needs).
    {
        const u64 chunk = 64ull << 20;
        PinMem<uint8_t> pin[2];
        DevEvent done[2];
        hipError_t e = hipSuccess;
        for (int k = 0; k < 2 && e == hipSuccess; ++k) {
            e = pin[k].alloc(chunk);
            if (e == hipSuccess) e = done[k].create(hipEventDisableTiming);
        }
        u64 at = 0;                                               // codes staged so far
        u32 g = 0; u64 goff = 0;                                  // next genome / offset inside it
        for (int k = 0; e == hipSuccess && at < total_codes; k ^= 1) {
            e = hipEventSynchronize(done[k]);                     // the previous copy out of this buffer (no-op the first time)
            u64 fill = 0;
            while (g < n && fill < chunk) {
                const u64 take = std::min<u64>(chunk - fill, (u64)len[g] - goff);
                if (take) memcpy(pin[k] + fill, codes[g] + goff, take);
                fill += take; goff += take;
                if (goff == len[g]) { ++g; goff = 0; }
            }
            if (e == hipSuccess) e = hipMemcpyAsync(d_codes.get() + at, pin[k], fill, hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) e = hipEventRecord(done[k], c->stream);
            at += fill;
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? LZANI_ERR_NOMEM : LZANI_ERR_DEVICE, std::string("staging the sequences: ") + hipGetErrorString(e));
    }
    HIPCHK(c, hipMemcpy(d_codeoff, codeoff.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->gs.tab.nmoff, c->gs.nmoff.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->gs.tab.L, c->gs.L.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    c->gs.n = n;
    for_slices(n, [&](u32 g0, u32 cnt) {
        pack_genomes(c, d_codes, d_codeoff, c->gs.tab.t2, c->gs.tab.nm, c->gs.tab.nmoff, c->gs.tab.L, c->gs.tab.hasN, c->gs.Tmax, g0, cnt);
    });
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    {
        std::vector<int> hn(n);
        HIPCHK(c, hipMemcpy(hn.data(), c->gs.tab.hasN, (size_t)n * 4, hipMemcpyDeviceToHost));
        c->gs.all_nfree = std::all_of(hn.begin(), hn.end(), [](int v) { return v == 0; });
    }
    TRACE("set_genomes: n=%u Tmax=%d dirbits=%d posbits=%d tagmask=%x", n, c->gs.Tmax, c->gs.geo.dirbits, c->gs.geo.posbits, c->gs.geo.tagmask);
    return LZANI_OK;
}

// The bytes of one index slab slot of the set (lzani_run_plan.h): the tables, and the keys of the sort-based build.
SlabBytes slot_bytes(const GenomeSet& gs)
{
    return slab_bytes_per_slot(gs.dir_stride, gs.ent_stride, gs.lay.bk_stride, gs.lay.tw_stride, gs.lay.fl_stride, gs.lay.sort_build, (u64)gs.Tmax);
}

int ensure_slabs(lzani_ctx* c, u32 want_rows)
{
    const SetLayout& f = c->gs.lay;
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    const u32 slots = slab_slot_count(free_b, c->sl.slots, slot_bytes(c->gs).total(), want_rows, f.max_slots);
    if (slots <= c->sl.slots) return LZANI_OK;
    c->sl = IndexSlabs{};                              // released first: two generations need not fit
    IndexSlabs s;
    HIPCHK(c, s.d_dirz.alloc((size_t)slots * c->gs.dir_stride));
    HIPCHK(c, s.d_ent.alloc((size_t)slots * c->gs.ent_stride));
    if (f.bk_stride) HIPCHK(c, s.d_bk.alloc((size_t)slots * f.bk_stride));
    if (f.tw_stride) HIPCHK(c, s.d_tw.alloc((size_t)slots * f.tw_stride));
    if (f.tw_stride) {
        HIPCHK(c, s.d_fl.alloc((size_t)slots * f.fl_stride));
        if (!f.fl_stride) HIPCHK(c, hipMemset(s.d_fl, 0xFF, 4));
    }
    HIPCHK(c, s.d_status.alloc(slots));
    if (f.sort_build) {
        HIPCHK(c, s.d_ikeys_in.alloc((size_t)slots * c->gs.Tmax));
        HIPCHK(c, s.d_ikeys.alloc((size_t)slots * c->gs.Tmax));
        HIPCHK(c, s.d_icnt.alloc(slots));
        HIPCHK(c, s.d_ibase.alloc(slots));
    }
    s.slots = slots;
    c->sl = std::move(s);
    return LZANI_OK;
}

// Join form: the k-mer list of every genome as a query, sorted by (genome, bucket) -- k_join_keys + the radix sort of lzani_sort.hip,
// once per run, behind k_kmers (it is part of the path's work like the k-mer words it is made from).
// the resident part of the join lists (the sorted keys: 8 B per forward position), allocated before the index slabs are
// sized so that those see what is really left
int alloc_join_lists(lzani_ctx* c, const RunGenomes& g)
{
    const u32 n = g.n;
    if (c->gs.jl.keys) return LZANI_OK;
    JoinLists jl;                                        // (moved into the set whole, or not at all)
    jl.h_koff.assign((size_t)n + 1, 0);
    for (u32 x = 0; x < n; ++x) jl.h_koff[x + 1] = jl.h_koff[x] + (u64)g.L[x];
    HIPCHK(c, jl.koff.alloc((size_t)n + 1));
    HIPCHK(c, jl.soff.alloc((size_t)n + 1));
    HIPCHK(c, jl.cnt.alloc(n));
    HIPCHK(c, jl.keys.alloc(jl.h_koff[n]));
    HIPCHK(c, hipMemcpyAsync(jl.koff, jl.h_koff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    c->gs.jl = std::move(jl);
    return LZANI_OK;
}

int build_join_lists(lzani_ctx* c, const RunGenomes& g)
{
    const u32 n = g.n;
    int rc0 = alloc_join_lists(c, g);
    if (rc0) return rc0;
    // the unsorted keys live for the duration of the sort only (as much again as the lists themselves)
    DevMem<unsigned long long> keys_in;
    HIPCHK(c, keys_in.alloc(c->gs.jl.h_koff[n]));
    int Lmax = 0;
    for (u32 x = 0; x < n; ++x) Lmax = std::max(Lmax, g.L[x]);
    // An invalid key is all ones; the sort looks at the bits [posbits, shift_g + gbits) only, so no real genome number may
    // be all ones in gbits bits, or its keys with the all-ones hash would be indistinguishable from the invalid keys of
    // the genomes before it (found by the fuzz at n = 4: genome 3 lost the k-mers of its last bucket)
    const int shift_g = c->gs.geo.kb + c->gs.geo.posbits, gbits = ceil_log2((u64)n + 1);
    HIPCHK(c, hipMemsetAsync(c->gs.jl.cnt, 0, (size_t)n * 4, c->stream));
    if (Lmax > 0)
        for_slices(n, [&](u32 g0, u32 cnt) {
            GenomeTab G = gtab(c);
            G.nmoff += g0; G.L += g0;
            // (the genome number of the key is global: the kernel adds g0 through the offset tables it is given)
            hipLaunchKernelGGL(k_join_keys, dim3((Lmax + 4095) / 4096, cnt), dim3(256), 0, c->stream, G, c->gs.jl.koff + g0, keys_in,
                               c->gs.jl.cnt + g0, shift_g, c->gs.geo.posbits, Lmax, g0);
        });
    HIPCHK(c, hipGetLastError());
    std::vector<u32> valid(n);
    HIPCHK(c, hipMemcpyAsync(valid.data(), c->gs.jl.cnt, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // sort in groups of whole genomes below 2^30 keys; invalid keys (all ones) end up behind the group's valid ones
    std::vector<u64> soff((size_t)n + 1, 0);
    for (u32 g0 = 0; g0 < n;) {
        u32 g1 = g0;
        u64 keys = 0;
        while (g1 < n && (g1 == g0 || keys + (u64)g.L[g1] <= (1ull << 30))) keys += (u64)g.L[g1++];
        if (keys > 0x7FFFFFF0ull) return fail(c, LZANI_ERR_ARG, "join lists: a genome of more than 2^31 positions");
        u64 at = c->gs.jl.h_koff[g0];
        for (u32 x = g0; x < g1; ++x) { soff[x] = at; at += valid[x]; }
        if (g1 == n) soff[n] = at;
        if (keys)
            if (int rc = sort_keys(c, c->gs.d_jtmp, keys_in + c->gs.jl.h_koff[g0], c->gs.jl.keys + c->gs.jl.h_koff[g0], keys, 1, c->gs.geo.posbits, shift_g + gbits,
                                   "join lists: radix sort", false))
                return rc;
        g0 = g1;
    }
    // (a genome's list ends after its valid keys -- d_jcnt -- not where the next list begins: between two groups sit the
    // invalid keys of the first)
    HIPCHK(c, hipMemcpyAsync(c->gs.jl.soff, soff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));        // (before keys_in is released)
    c->run.tm.index_launches += 2;
    return LZANI_OK;
}

// Per-genome k-mer words (and, for long genomes, the sorted join lists made from them): once per genome set, by the
// first run after lzani_set_genomes -- before its index slabs are sized, so that the slabs see what the lists and the
// sort's temporaries have left -- and kept for the runs that follow (they depend on the genomes and the parameters
// only).  Timed on their own (lzani_timing.kmers_ms).  They belong to the set, not to a run: made for gs.n genomes, in-core
// only (out-of-core, every block upload makes its own and kmers_ready is set from the start).
int ensure_kmers(lzani_ctx* c)
{
    if (!c->gs.tab.kmL || c->gs.kmers_ready) return LZANI_OK;
    HIPCHK(c, c->km_span.begin(c->stream));
    for_slices(c->gs.n, [&](u32 g0, u32 cnt) { launch_kmers(c, gtab(c), c->gs.Tmax, g0, cnt); });
    HIPCHK(c, hipGetLastError());
    c->run.tm.index_launches += 1;
    HIPCHK(c, c->km_span.end(c->stream));
    c->gs.kmers_ready = true;
    c->km_timed = true;
    return LZANI_OK;
}

// The sorted join lists of a long-genome set (join form of candidate detection): made by the first run that needs them
// -- dense rows take their candidates from the presence matrix instead -- and kept like the k-mer words they are made
// from; their time is part of that run's kmers_ms.
int ensure_join(lzani_ctx* c, const RunGenomes& g)
{
    if (!c->gs.lay.join_mode || c->gs.jl.ready) return LZANI_OK;
    StreamSpan span;
    float ms = 0;
    HIPCHK(c, span.begin(c->stream));
    if (int rc = build_join_lists(c, g)) return rc;
    HIPCHK(c, span.end(c->stream));
    HIPCHK(c, span.elapsed(ms));
    c->join_ms_pending = ms;
    c->gs.jl.ready = true;
    return LZANI_OK;
}

// Index build of `rows` references (device list d_ref_ids) into slots 0..rows-1.
// with_tw = false: the sort-based build leaves the tag words out (a batch whose pairs read candidate bitmaps never probes them:
// 8.6 GB less to write per 128 x 5 Mbp references)
int build_indexes(lzani_ctx* c, const Knobs& k, const u32* d_ref_ids, u32 rows, bool with_filter = true, bool with_tw = true)
{
    const SetLayout& f = c->gs.lay;
    IdxArgs ia;
    ia.G = gtab(c);
    ia.ref_ids = d_ref_ids;
    ia.dirz = c->sl.d_dirz; ia.ent = c->sl.d_ent;
    ia.dir_stride = c->gs.dir_stride; ia.ent_stride = c->gs.ent_stride;
    ia.mal = c->P.mal; ia.mrd = c->P.mrd; ia.geo = c->gs.geo; ia.todo = nullptr;
    const u32 nb = 1u << c->gs.geo.dirbits;
    { int rc = ensure_kmers(c); if (rc) return rc; }
    if (f.fl_stride && with_filter) {                  // (only the block kernel reads it)
        HIPCHK(c, hipMemsetAsync(c->sl.d_fl, 0, (size_t)rows * f.fl_stride * 4, c->stream));
        hipLaunchKernelGGL(k_idx_filter, dim3((u32)std::min<u64>(((u64)c->gs.Tmax + 255) / 256, 64), rows), dim3(256), 0, c->stream,
                           ia, c->sl.d_fl, f.fl_stride, f.fmask, c->gs.Tmax);
        c->run.tm.index_launches += 1;
    }
    if (f.sort_build) {
        c->sl.index_build = LZANI_INDEX_BUILD_SORT;
        // keys -> radix sort, every slot a segment of its own (lzani_sort.hip) -> the tables in one streaming pass.  A key is
        // hash || position; a position without a k-mer is all ones and sorts behind the slot's keys by the one bit above the hash.
        const int shift_slot = c->gs.geo.kb + c->gs.geo.posbits;
        const u64 Tm = (u64)c->gs.Tmax;
        const u32 group = 1;
        HIPCHK(c, hipMemsetAsync(c->sl.d_icnt, 0, (size_t)rows * 4, c->stream));
        hipLaunchKernelGGL(k_idx_keys, dim3((u32)((Tm + 4095) / 4096), rows), dim3(256), 0, c->stream, ia, c->sl.d_ikeys_in, c->sl.d_icnt, c->gs.Tmax, shift_slot);
        if (int rc = sort_keys(c, c->gs.d_jtmp, c->sl.d_ikeys_in, c->sl.d_ikeys, Tm, rows, c->gs.geo.posbits, shift_slot + 1, "index build: radix sort", true)) return rc;
        hipLaunchKernelGGL(k_idx_base, dim3((rows + 255) / 256), dim3(256), 0, c->stream, c->sl.d_icnt, c->sl.d_ibase, rows, group, Tm);
        hipLaunchKernelGGL(k_idx_from_sorted, dim3((u32)std::min<u64>((Tm + 255) / 256, 8192), rows), dim3(256), 0, c->stream,
                           ia, c->sl.d_ikeys, c->sl.d_icnt, c->sl.d_ibase, c->sl.d_bk, with_tw ? c->sl.d_tw : nullptr, f.bk_stride, f.tw_stride);
        HIPCHK(c, hipGetLastError());
        c->run.tm.index_launches += 4;
        return LZANI_OK;
    }
    const bool lds_build = c->gs.tab.kmL && c->gs.geo.dirbits <= k.lds_index_max_dirbits && k.lds_index;
    c->sl.index_build = lds_build ? LZANI_INDEX_BUILD_LDS : LZANI_INDEX_BUILD_ATOMICS;
    // blocks per slot of the global-atomics kernels: the whole range when they build every slot, a handful when
    // they only pick up what k_idx_build left (usually nothing)
    const u32 gx_pos = lds_build ? 16u : (u32)((c->gs.Tmax + 255) / 256), gx_bkt = lds_build ? 16u : (nb + 255) / 256;
    dim3 gp(gx_pos, rows);
    if (lds_build) {
        // one block per reference, everything through LDS; a slot that does not fit (status != 0) falls through
        // to the global-atomics kernels below, which skip every other slot
        const size_t lds = (size_t)(IDX_RANGE / 2 + IDX_STAGE) * 4;
        { int rc = raise_lds(c, k_idx_build, lds); if (rc) return rc; }
        HIPCHK(c, hipMemsetAsync(c->sl.d_status, 0, (size_t)rows * 4, c->stream));
        hipLaunchKernelGGL(k_idx_build, dim3(rows), dim3(1024), lds, c->stream, ia, c->sl.d_bk, c->sl.d_tw, f.bk_stride, f.tw_stride, c->sl.d_status);
        ia.todo = c->sl.d_status;
        hipLaunchKernelGGL(k_idx_zero, dim3(gx_bkt, rows), dim3(256), 0, c->stream, c->sl.d_dirz, c->gs.dir_stride, nb, ia.todo);
    } else HIPCHK(c, hipMemsetAsync(c->sl.d_dirz, 0, (size_t)rows * c->gs.dir_stride * 4, c->stream));
    hipLaunchKernelGGL(k_idx_count, gp, dim3(256), 0, c->stream, ia, c->gs.Tmax);
    hipLaunchKernelGGL(k_idx_scan, dim3(rows), dim3(1024), 0, c->stream, c->sl.d_dirz, c->gs.dir_stride, nb, ia.todo);
    hipLaunchKernelGGL(k_idx_fill, gp, dim3(256), 0, c->stream, ia, c->gs.Tmax);
    hipLaunchKernelGGL(k_idx_sort, dim3(gx_bkt, rows), dim3(256), 0, c->stream,
                       c->sl.d_dirz, c->sl.d_ent, c->gs.dir_stride, c->gs.ent_stride, nb, ia.todo, 0);
    if (c->sl.d_bk)
        hipLaunchKernelGGL(k_idx_buckets, dim3(gx_bkt, rows), dim3(256), 0, c->stream,
                           c->sl.d_dirz, c->sl.d_ent, c->sl.d_bk, c->sl.d_tw, c->gs.dir_stride, c->gs.ent_stride, f.bk_stride, f.tw_stride,
                           nb, c->gs.geo.posbits, ia.todo);
    HIPCHK(c, hipGetLastError());
    c->run.tm.index_launches += 4;
    return LZANI_OK;
}

// What the two index test hooks below do first: slabs for `rows`, the ids up, the run's own build_indexes into slots 0 .. rows-1, and the wait for it.
int debug_build_slab(lzani_ctx* c, u32 rows, const u32* ref_ids, bool with_filter, bool with_tw)
{
    HIPCHK(c, hipSetDevice(c->dev));
    int rc = ensure_slabs(c, rows);
    if (rc) return rc;
    if (c->sl.slots < rows) return fail(c, LZANI_ERR_ARG, "lzani_debug_index_slab: more rows than index slabs");
    DevMem<u32> d_ref;
    HIPCHK(c, d_ref.alloc(rows));
    HIPCHK(c, hipMemcpy(d_ref.get(), ref_ids, (size_t)rows * 4, hipMemcpyHostToDevice));
    rc = build_indexes(c, Knobs{}, d_ref, rows, with_filter, with_tw);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LZANI_OK;
}

}  // namespace

// Test hook: one genome's packed text and N mask, and slot 0 of the one-row slab -- the directory and the entries it counts.
int lzani_debug_get_index(lzani_ctx* c, uint32_t id, uint64_t* t2, uint64_t* nm, uint32_t* dirz,
                          uint32_t* ent, uint32_t* n_ent, uint32_t* geom)
{
    if (!c) return LZANI_ERR_ARG;
    if (!c->gs.n || id >= c->gs.n) return fail(c, LZANI_ERR_ARG, "lzani_debug_get_index: bad id");
    if (c->gs.ooc) return fail(c, LZANI_ERR_STATE, "lzani_debug_get_index: the genome is not resident (out-of-core set)");
    if (int rc = debug_build_slab(c, 1, &id, true, true)) return rc;
    int T = ref_text_len(c->gs.L[id], c->P.mrd);
    size_t wn = text_wordsN(T);
    if (nm) HIPCHK(c, hipMemcpy(nm, c->gs.tab.nm + c->gs.nmoff[id], wn * 8, hipMemcpyDeviceToHost));
    if (t2) HIPCHK(c, hipMemcpy(t2, c->gs.tab.t2 + 2 * c->gs.nmoff[id], wn * 16, hipMemcpyDeviceToHost));
    std::vector<u32> d(c->gs.dir_stride);
    HIPCHK(c, hipMemcpy(d.data(), c->sl.d_dirz, c->gs.dir_stride * 4, hipMemcpyDeviceToHost));
    u32 ne = d[c->gs.dir_stride - 1];
    if (dirz) memcpy(dirz, d.data(), c->gs.dir_stride * 4);
    if (ent && ne) HIPCHK(c, hipMemcpy(ent, c->sl.d_ent, (size_t)ne * 4, hipMemcpyDeviceToHost));
    if (n_ent) *n_ent = ne;
    if (geom) { geom[0] = c->gs.geo.kb; geom[1] = c->gs.geo.dirbits; geom[2] = c->gs.geo.posbits; geom[3] = c->gs.geo.tagmask; }
    return LZANI_OK;
}

// Test hook: the index slabs of one batch of `rows` reference ids, built by the run's own build_indexes into slots 0 .. rows-1.
int lzani_debug_index_slab(lzani_ctx* c, uint32_t rows, const uint32_t* ref_ids, int with_filter, int with_tw,
                           lzani_slab_info* info, uint32_t* dirz, uint32_t* ent, uint32_t* bk, uint32_t* tw, uint32_t* fl,
                           uint32_t* status)
{
    if (!c) return LZANI_ERR_ARG;
    if (!c->gs.n || !rows || !ref_ids || !info) return fail(c, LZANI_ERR_ARG, "lzani_debug_index_slab: bad arguments");
    if (c->gs.ooc) return fail(c, LZANI_ERR_STATE, "lzani_debug_index_slab: the genomes are not resident (out-of-core set)");
    for (u32 k = 0; k < rows; ++k)
        if (ref_ids[k] >= c->gs.n) return fail(c, LZANI_ERR_ARG, "lzani_debug_index_slab: reference id out of range");
    if (int rc = debug_build_slab(c, rows, ref_ids, with_filter != 0, with_tw != 0)) return rc;
    const SetLayout& f = c->gs.lay;
    info->key_bits = c->gs.geo.kb; info->dir_bits = c->gs.geo.dirbits; info->pos_bits = c->gs.geo.posbits; info->tag_mask = c->gs.geo.tagmask;
    info->filter_mask = f.fmask;
    info->build = c->sl.index_build;
    info->dir_stride = c->gs.dir_stride; info->ent_stride = c->gs.ent_stride; info->bk_stride = f.bk_stride;
    // (what this build wrote: the sort build leaves the tag words out without with_tw, every build the filter without with_filter)
    info->tw_stride = (c->sl.index_build != LZANI_INDEX_BUILD_SORT || with_tw) ? f.tw_stride : 0;
    info->fl_stride = with_filter ? f.fl_stride : 0;
    const size_t r = rows;
    if (dirz) HIPCHK(c, hipMemcpy(dirz, c->sl.d_dirz, r * c->gs.dir_stride * 4, hipMemcpyDeviceToHost));
    if (ent) HIPCHK(c, hipMemcpy(ent, c->sl.d_ent, r * c->gs.ent_stride * 4, hipMemcpyDeviceToHost));
    if (bk && info->bk_stride) HIPCHK(c, hipMemcpy(bk, c->sl.d_bk, r * info->bk_stride * 4, hipMemcpyDeviceToHost));
    if (tw && info->tw_stride) HIPCHK(c, hipMemcpy(tw, c->sl.d_tw, r * info->tw_stride * 4, hipMemcpyDeviceToHost));
    if (fl && info->fl_stride) HIPCHK(c, hipMemcpy(fl, c->sl.d_fl, r * info->fl_stride * 4, hipMemcpyDeviceToHost));
    if (status) {
        if (c->sl.index_build == LZANI_INDEX_BUILD_LDS) HIPCHK(c, hipMemcpy(status, c->sl.d_status, r * 4, hipMemcpyDeviceToHost));
        else memset(status, 0, r * 4);
    }
    return LZANI_OK;
}

