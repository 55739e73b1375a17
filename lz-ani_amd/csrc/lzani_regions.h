// lzani_regions.h -- host side of the alignment-region stage (include/lzani.h states the definitions): the checks of made-up
// regions, the stage -- sums, rule, keys of the regions that stay, three stable sorts, gather -- over a finished buffer of raw
// regions, the capacity of that buffer and the one repeat of a run that overflowed it, and the entry points
// (lzani_run_rows_aligned, lzani_regions_fetch, lzani_get_regions_info, lzani_set_region_capacity, lzani_debug_order_regions
// and the pure lzani_regions_host).  Included by lzani_hip.hip only, behind lzani_kept.h; of that file it uses kept_check_rows,
// kept_stage_run and kept_own_lengths, of lzani_hip.hip lzani_ctx (which holds the AlignedRegions), RegionSink, fail, HIPCHK,
// sort_keys and run_rows_any, of lzani_prefilter.h pf_chunks and pf_blocks.  The kernels are lzani_kernels_regions.h.
//
// Order of work (regions_stage_run) on R raw regions of E entries: sums and `has` cleared; k_rg_sums; k_rg_pass; the count
// pass of k_rg_keys, k_pf_scan, and one read-back: K, the regions that stay, and the largest seq_start and length among them;
// two key buffers, the sort's scratch and the result are allocated at K; the write pass; sort by seq_start, rekey, sort by
// maxlen - length, rekey, sort by entry -- each over the bits its field has in this call; k_rg_gather.  Bytes: 32 read per raw
// region by k_rg_sums and again by each pass of k_rg_keys; per region that stays 8 written by the write pass, 16 per radix pass
// (and 8 more read by its histogram), 32 + 8 read and 8 written per rekey, 40 read and 32 written by the gather; per entry 8 of
// sums and 2 bits.
#pragma once

namespace {

constexpr u64 RG_MAX_REGIONS = 0xFFFFFFEFull;     // 2^32 - 17: what one sort takes
constexpr u64 RG_MIN_CAPACITY = 1024;

int regions_check_filter(lzani_ctx* c, const std::string& fn, const lzani_out_filter* f)
{
    if (f && aln_filter_has_nan(*f)) return fail(c, LZANI_ERR_ARG, fn + ": a minimum of the alignment filter is not a number");
    return LZANI_OK;
}

// made-up regions, on the host: their entry is one of the call, they are not empty and no field is negative
int regions_check(lzani_ctx* c, const std::string& fn, const lzani_region* r, u64 count, u64 entries)
{
    if (count > RG_MAX_REGIONS) return fail(c, LZANI_ERR_ARG, fn + ": more regions than one sort takes (2^32 - 17)");
    for (u64 i = 0; i < count; ++i) {
        if (r[i].pair >= entries) return fail(c, LZANI_ERR_ARG, fn + ": a region's pair lies beyond the call's entries (region " + std::to_string(i) + ")");
        if (r[i].ref_start < 0 || r[i].ref_end < 0 || r[i].seq_start < 0 || r[i].seq_end < 0 || r[i].num_matches < 0 || r[i].num_mismatches < 0)
            return fail(c, LZANI_ERR_ARG, fn + ": a region with a negative field (region " + std::to_string(i) + ")");
        if (r[i].seq_end <= r[i].seq_start) return fail(c, LZANI_ERR_ARG, fn + ": an empty region (region " + std::to_string(i) + ")");
    }
    return LZANI_OK;
}

int regions_bits(u64 v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }
u64 regions_passes(int bits) { return (u64)((bits + 7) / 8); }                   // (the radix sort takes 8 bits a pass)

// The stage on d_raw (this context's device, R records, complete on the context's stream or before): fills `g`.  The rows
// passed kept_check_rows; f null: no entry is dropped.
int regions_stage_run(lzani_ctx* c, AlignedRegions& g, u32 n, const u32* aln_len, u32 n_rows, const u32* ref_ids, const u64* row_off, const u32* query_ids,
                      u64 E, const lzani_region* d_raw, u64 R, const lzani_out_filter* f)
{
    g.info.entries = E; g.info.found = R;
    if (R > RG_MAX_REGIONS) return fail(c, LZANI_ERR_ARG, "the region stage: more regions than one sort takes (2^32 - 17)");
    if (!E || !R) { HIPCHK(c, g.rec.alloc(0)); return LZANI_OK; }
    DevMem<u32> d_ref, d_q, d_len, d_blkcnt;
    DevMem<u64> d_off, d_blkoff;
    DevMem<int> d_sums;
    DevMem<unsigned long long> d_has, d_keep, d_counters, ka, kb;
    DevMem<unsigned char> scratch;
    const u64 words = (E + 63) / 64, blocks = pf_chunks(R);
    HIPCHK(c, d_sums.alloc((size_t)E * 2));
    HIPCHK(c, d_has.alloc(words));
    HIPCHK(c, d_keep.alloc(words));
    HIPCHK(c, d_counters.alloc(RG_COUNTERS));
    HIPCHK(c, d_blkcnt.alloc(blocks));
    HIPCHK(c, d_blkoff.alloc(blocks + 1));
    if (f) {                                                   // the rule's tables: the query of an entry and its length
        HIPCHK(c, d_len.alloc(n));
        HIPCHK(c, hipMemcpyAsync(d_len, aln_len, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        if (query_ids) {
            HIPCHK(c, d_q.alloc(E));
            HIPCHK(c, hipMemcpyAsync(d_q, query_ids, (size_t)E * 4, hipMemcpyHostToDevice, c->stream));
        } else {
            HIPCHK(c, d_ref.alloc(n_rows));
            HIPCHK(c, d_off.alloc((size_t)n_rows + 1));
            HIPCHK(c, hipMemcpyAsync(d_ref, ref_ids, (size_t)n_rows * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(d_off, row_off, ((size_t)n_rows + 1) * 8, hipMemcpyHostToDevice, c->stream));
        }
    }
    HIPCHK(c, hipMemsetAsync(d_sums, 0, (size_t)E * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(d_has, 0, (size_t)words * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(d_counters, 0, RG_COUNTERS * sizeof(unsigned long long), c->stream));
    const RgCall call{d_off.get(), d_ref.get(), d_q.get(), d_len.get(), n_rows, f ? 1 : 0, E, f ? *f : lzani_out_filter{}};
    const dim3 threads(PF_THREADS);
    StreamSpan sums_span, sort_span, write_span;
    HIPCHK(c, sums_span.begin(c->stream));
    hipLaunchKernelGGL(k_rg_sums, dim3(pf_blocks(R)), threads, 0, c->stream, d_raw, R, E, d_sums.get(), d_has.get());
    hipLaunchKernelGGL(k_rg_pass, dim3(pf_blocks(E)), threads, 0, c->stream, call, (const int*)d_sums.get(), (const unsigned long long*)d_has.get(), d_keep.get(),
                       d_counters.get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, sums_span.end(c->stream));
    HIPCHK(c, sort_span.begin(c->stream));
    hipLaunchKernelGGL(k_rg_keys<false>, dim3((u32)blocks), threads, 0, c->stream, d_raw, R, (const unsigned long long*)d_keep.get(), E, d_blkcnt.get(),
                       (const u64*)d_blkoff.get(), (unsigned long long*)nullptr, d_counters.get());
    hipLaunchKernelGGL(k_pf_scan, dim3(1), dim3(1024), 0, c->stream, (const u32*)d_blkcnt.get(), blocks, d_blkoff.get());
    HIPCHK(c, hipGetLastError());
    u64 K = 0;
    unsigned long long counters[RG_COUNTERS] = {};
    HIPCHK(c, hipMemcpyAsync(&K, d_blkoff.get() + blocks, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(counters, d_counters, sizeof counters, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (K > R) return fail(c, LZANI_ERR_DEVICE, "the region stage: more regions stay than there are");
    g.info.kept = K; g.info.entries_with_regions = counters[RG_WITH]; g.info.entries_dropped = counters[RG_DROPPED];
    const int bits[3] = {regions_bits(counters[RG_MAX_START]), regions_bits(counters[RG_MAX_LEN]), regions_bits(E - 1)};
    const u32 maxlen = (u32)counters[RG_MAX_LEN];
    size_t need = 0;
    for (int b : bits) {
        size_t x = 0;
        if (int rc = sort_scratch_bytes(c, (size_t)K, 1, 32, 32 + b, "the region stage: sort", x)) return rc;
        need = std::max(need, x);
    }
    HIPCHK(c, g.rec.alloc((size_t)K));                         // the exact size, known before the buffer is made
    if (K) {
        HIPCHK(c, ka.alloc((size_t)K));
        HIPCHK(c, kb.alloc((size_t)K));
        HIPCHK(c, scratch.alloc(need));
        const dim3 kept_blocks(pf_blocks(K));
        hipLaunchKernelGGL(k_rg_keys<true>, dim3((u32)blocks), threads, 0, c->stream, d_raw, R, (const unsigned long long*)d_keep.get(), E, d_blkcnt.get(),
                           (const u64*)d_blkoff.get(), ka.get(), d_counters.get());
        HIPCHK(c, hipGetLastError());
        // by seq_start, then (the sorts are stable) by maxlen - length, then by the entry: only the bits each field has here
        if (int rc = sort_keys(c, scratch, ka, kb, (size_t)K, 1, 32, 32 + bits[0], "the region stage: sort", false)) return rc;
        hipLaunchKernelGGL(k_rg_rekey<1>, kept_blocks, threads, 0, c->stream, d_raw, kb.get(), K, maxlen);
        if (int rc = sort_keys(c, scratch, kb, ka, (size_t)K, 1, 32, 32 + bits[1], "the region stage: sort", false)) return rc;
        hipLaunchKernelGGL(k_rg_rekey<2>, kept_blocks, threads, 0, c->stream, d_raw, ka.get(), K, maxlen);
        if (int rc = sort_keys(c, scratch, ka, kb, (size_t)K, 1, 32, 32 + bits[2], "the region stage: sort", false)) return rc;
        HIPCHK(c, hipGetLastError());
        g.info.sort_passes = regions_passes(bits[0]) + regions_passes(bits[1]) + regions_passes(bits[2]);
    }
    HIPCHK(c, sort_span.end(c->stream));
    HIPCHK(c, write_span.begin(c->stream));
    if (K) {
        hipLaunchKernelGGL(k_rg_gather, dim3(pf_blocks(K)), threads, 0, c->stream, d_raw, (const unsigned long long*)kb.get(), K, g.rec.get());
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, write_span.end(c->stream));
    float ms[3] = {0, 0, 0};
    HIPCHK(c, sums_span.elapsed(ms[0]));
    HIPCHK(c, sort_span.elapsed(ms[1]));
    HIPCHK(c, write_span.elapsed(ms[2]));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    g.info.sums_ms = ms[0]; g.info.sort_ms = ms[1]; g.info.write_ms = ms[2];
    g.info.workspace_bytes = d_ref.bytes() + d_q.bytes() + d_len.bytes() + d_blkcnt.bytes() + d_off.bytes() + d_blkoff.bytes() + d_sums.bytes() + d_has.bytes() +
                             d_keep.bytes() + d_counters.bytes() + ka.bytes() + kb.bytes() + scratch.bytes();
    TRACE("regions: entries=%llu found=%llu kept=%llu with=%llu dropped=%llu passes=%llu", (unsigned long long)E, (unsigned long long)R, (unsigned long long)K,
          counters[RG_WITH], counters[RG_DROPPED], (unsigned long long)g.info.sort_passes);
    return LZANI_OK;
}

// An upper bound of the regions of a call's entries: a region is at least reg long in the query and a pair's regions are
// disjoint there, so the entry (ref a, query b) has at most floor((L_b + mrd) / max(reg, 1)) of them.  With
// reg < 1 it is no bound; the run is then repeated once with the exact count, like any run that overflows.
u64 regions_bound(const lzani_ctx* c, u32 n_rows, const u32* ref_ids, const u64* row_off, const u32* query_ids)
{
    const u32 n = c->gs.n;
    const u64 reg = (u64)std::max(c->P.reg, 1);
    auto term = [&](u32 b) { return ((u64)c->gs.L[b] + (u64)c->P.mrd) / reg; };
    u64 sum = 0;
    if (query_ids) { for (u64 e = 0; e < row_off[n_rows]; ++e) sum += term(query_ids[e]); return sum; }
    u64 all = 0;
    for (u32 b = 0; b < n; ++b) all += term(b);
    for (u32 k = 0; k < n_rows; ++k) sum += all - term(ref_ids[k]);
    return sum;
}

// The first capacity of a call: the forced one, or the smallest of the bound, what an eighth of the free device memory
// holds and what the sort takes, and at least RG_MIN_CAPACITY.
int regions_capacity(lzani_ctx* c, u32 n_rows, const u32* ref_ids, const u64* row_off, const u32* query_ids, u64& cap)
{
    if (c->region_cap) { cap = std::min(c->region_cap, RG_MAX_REGIONS); return LZANI_OK; }
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    cap = std::min({regions_bound(c, n_rows, ref_ids, row_off, query_ids), (u64)free_b / 8 / sizeof(lzani_region), RG_MAX_REGIONS});
    cap = std::max(cap, RG_MIN_CAPACITY);
    return LZANI_OK;
}

// lzani_run_rows_aligned behind its checks: the run (twice where the first capacity was too small), the results to the host,
// the kept stage and the region stage into fresh groups that become the context's on success.
int aligned_run(lzani_ctx* c, u32 n_rows, const u32* ref_ids, const u64* row_off, const u32* query_ids, lzani_result* out, const lzani_out_filter* kept_filter,
                const u32* report_len, const lzani_out_filter* aln_filter, const u32* aln_len, const std::vector<u32>& row_of, const KeptRows& kr)
{
    const u64 E = kr.entries;
    DevMem<lzani_result> d_res;
    DevMem<lzani_region> d_raw;
    DevMem<unsigned long long> d_count;
    HIPCHK(c, d_res.alloc(E));
    HIPCHK(c, d_count.alloc(1));
    u64 cap = 0, runs = 0;
    unsigned long long cnt = 0;
    if (int rc = regions_capacity(c, n_rows, ref_ids, row_off, query_ids, cap)) return rc;
    for (;;) {
        HIPCHK(c, d_raw.alloc(cap));
        HIPCHK(c, hipMemset(d_count.get(), 0, sizeof(unsigned long long)));
        const RegionSink rs{d_raw.get(), d_count.get(), cap};
        ++runs;
        if (int rc = run_rows_any(c, n_rows, ref_ids, row_off, query_ids, (int*)d_res.get(), nullptr, nullptr, &rs)) return rc;
        HIPCHK(c, hipMemcpy(&cnt, d_count.get(), sizeof cnt, hipMemcpyDeviceToHost));
        if (cnt <= cap) break;
        if (runs == 2) return fail(c, LZANI_ERR_DEVICE, "lzani_run_rows_aligned: the repeated run found more regions than the first");
        if (cnt > RG_MAX_REGIONS) return fail(c, LZANI_ERR_ARG, "lzani_run_rows_aligned: more regions than one sort takes (2^32 - 17)");
        cap = cnt;                                             // the exact count: the one repeat
    }
    if (out && E) HIPCHK(c, hipMemcpy(out, d_res.get(), (size_t)E * sizeof(lzani_result), hipMemcpyDeviceToHost));
    Kept k;
    if (kept_filter) {
        if (int rc = kept_stage_run(c, k, c->gs.n, report_len, n_rows, ref_ids, row_off, query_ids, row_of, kr, (const int*)d_res.get(), *kept_filter)) return rc;
        k.done = true;
    }
    d_res.reset();
    AlignedRegions g;
    if (int rc = regions_stage_run(c, g, c->gs.n, aln_len, n_rows, ref_ids, row_off, query_ids, E, d_raw.get(), cnt, aln_filter)) return rc;
    g.info.capacity = cap; g.info.runs = runs;
    g.done = true;
    d_raw.reset();                                             // the raw buffer goes before the call returns
    if (k.done) c->kept = std::move(k);
    c->rg = std::move(g);
    return LZANI_OK;
}

// lzani_debug_order_regions behind its checks: the made-up regions to the device, then the stage.
int order_uploaded(lzani_ctx* c, AlignedRegions& g, u32 n, const u32* aln_len, u32 n_rows, const u32* ref_ids, const u64* row_off, const u32* query_ids, u64 E,
                   const lzani_region* regions, u64 count, const lzani_out_filter* f)
{
    DevMem<lzani_region> d_raw;
    HIPCHK(c, d_raw.alloc(count));
    if (count) HIPCHK(c, hipMemcpy(d_raw.get(), regions, (size_t)count * sizeof(lzani_region), hipMemcpyHostToDevice));
    return regions_stage_run(c, g, n, aln_len, n_rows, ref_ids, row_off, query_ids, E, d_raw.get(), count, f);
}

}  // namespace

extern "C" {

int lzani_regions_host(uint32_t n, const uint32_t* aln_len, uint32_t n_rows, const uint32_t* ref_ids, const uint64_t* row_off, const uint32_t* query_ids,
                       const lzani_region* regions, uint64_t count, const lzani_out_filter* f, lzani_region* out, uint64_t* n_out, lzani_regions_info* info)
{
    const std::string fn = "lzani_regions_host";
    if (!n || !aln_len || !n_out || (n_rows && (!ref_ids || !row_off)) || (count && !regions)) return LZANI_ERR_ARG;
    *n_out = 0;
    if (regions_check_filter(nullptr, fn, f)) return LZANI_ERR_ARG;
    std::vector<u32> row_of;
    KeptRows kr;
    if (kept_check_rows(nullptr, fn, n, n_rows, ref_ids, row_off, query_ids, row_of, kr)) return LZANI_ERR_ARG;
    if (kr.entries > 0xFFFFFFFFull) return LZANI_ERR_ARG;
    if (regions_check(nullptr, fn, regions, count, kr.entries)) return LZANI_ERR_ARG;
    lzani_regions_info o{};
    o.entries = kr.entries; o.found = count;
    std::vector<u64> order;
    aln_host_counts cnt;
    aln_host_order(n_rows, ref_ids, row_off, query_ids, aln_len, regions, count, f, order, cnt);      // (the statement itself: lzani_aln_rule.h)
    o.entries_with_regions = cnt.entries_with_regions; o.entries_dropped = cnt.entries_dropped; o.kept = order.size();
    if (out) for (size_t j = 0; j < order.size(); ++j) out[j] = regions[order[j]];
    *n_out = order.size();
    if (info) *info = o;
    return LZANI_OK;
}

int lzani_set_region_capacity(lzani_ctx* c, uint64_t regions)
{
    if (!c) return LZANI_ERR_ARG;
    c->region_cap = regions;
    return LZANI_OK;
}

int lzani_run_rows_aligned(lzani_ctx* c, uint32_t n_rows, const uint32_t* ref_ids, const uint64_t* row_off, const uint32_t* query_ids, lzani_result* out,
                           const lzani_out_filter* kept_filter, const uint32_t* report_len, const lzani_out_filter* aln_filter, const uint32_t* aln_len,
                           uint64_t* n_kept, uint64_t* n_regions)
{
    if (!c) return LZANI_ERR_ARG;
    const std::string fn = "lzani_run_rows_aligned";
    if (n_rows && (!ref_ids || !row_off)) return fail(c, LZANI_ERR_ARG, fn + ": null argument");
    if (!c->gs.n) return fail(c, LZANI_ERR_STATE, fn + ": no genomes set");
    if (kept_filter) if (int rc = kept_check_filter(c, fn, kept_filter)) return rc;
    if (int rc = regions_check_filter(c, fn, aln_filter)) return rc;
    std::vector<u32> row_of, own;
    KeptRows kr;
    if (int rc = kept_check_rows(c, fn, c->gs.n, n_rows, ref_ids, row_off, query_ids, row_of, kr)) return rc;
    if (kr.entries > 0xFFFFFFFFull) return fail(c, LZANI_ERR_ARG, fn + ": 2^32 or more entries in one call");
    if (!report_len || !aln_len) own = kept_own_lengths(c);
    if (!report_len) report_len = own.data();
    if (!aln_len) aln_len = own.data();
    HIPCHK(c, hipSetDevice(c->dev));
    c->kept = Kept{};                                          // the last results go first: two need not fit
    c->rg = AlignedRegions{};
    const int rc = aligned_run(c, n_rows, ref_ids, row_off, query_ids, out, kept_filter, report_len, aln_filter, aln_len, row_of, kr);
    if (rc != LZANI_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    if (n_kept) *n_kept = c->kept.done ? c->kept.info.kept_pairs : 0;
    if (n_regions) *n_regions = c->rg.info.kept;
    return LZANI_OK;
}

int lzani_debug_order_regions(lzani_ctx* c, uint32_t n, const uint32_t* aln_len, uint32_t n_rows, const uint32_t* ref_ids, const uint64_t* row_off,
                              const uint32_t* query_ids, const lzani_region* regions, uint64_t count, const lzani_out_filter* f, uint64_t* n_regions)
{
    if (!c) return LZANI_ERR_ARG;
    const std::string fn = "lzani_debug_order_regions";
    if (!n || !aln_len || (n_rows && (!ref_ids || !row_off)) || (count && !regions)) return fail(c, LZANI_ERR_ARG, fn + ": null argument");
    if (int rc = regions_check_filter(c, fn, f)) return rc;
    std::vector<u32> row_of;
    KeptRows kr;
    if (int rc = kept_check_rows(c, fn, n, n_rows, ref_ids, row_off, query_ids, row_of, kr)) return rc;
    if (kr.entries > 0xFFFFFFFFull) return fail(c, LZANI_ERR_ARG, fn + ": 2^32 or more entries in one call");
    if (int rc = regions_check(c, fn, regions, count, kr.entries)) return rc;
    HIPCHK(c, hipSetDevice(c->dev));
    c->rg = AlignedRegions{};
    AlignedRegions g;
    const int rc = order_uploaded(c, g, n, aln_len, n_rows, ref_ids, row_off, query_ids, kr.entries, regions, count, f);
    if (rc != LZANI_OK) {                                      // as where a run's stage runs short: neither result is left
        (void)hipStreamSynchronize(c->stream);
        c->kept = Kept{};
        return rc;
    }
    g.info.capacity = count; g.info.runs = 0;
    g.done = true;
    c->rg = std::move(g);
    if (n_regions) *n_regions = c->rg.info.kept;
    return LZANI_OK;
}

int lzani_regions_fetch(lzani_ctx* c, uint64_t first, uint64_t count, lzani_region* out)
{
    if (!c) return LZANI_ERR_ARG;
    if (!c->rg.done) return fail(c, LZANI_ERR_STATE, "lzani_regions_fetch: no regions result (call lzani_run_rows_aligned first)");
    const u64 K = c->rg.info.kept;
    if (first > K || count > K - first) return fail(c, LZANI_ERR_ARG, "lzani_regions_fetch: the range lies past the end of the regions");
    if (!count) return LZANI_OK;
    if (!out) return fail(c, LZANI_ERR_ARG, "lzani_regions_fetch: null output");
    static_assert(sizeof(lzani_region) == 32, "lzani_region is one 64-bit and six 32-bit fields");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipMemcpy(out, c->rg.rec.get() + first, (size_t)count * sizeof(lzani_region), hipMemcpyDeviceToHost));
    c->rg.info.bytes_to_host += count * sizeof(lzani_region);
    return LZANI_OK;
}

int lzani_get_regions_info(const lzani_ctx* c, lzani_regions_info* info)
{
    if (!c || !info) return LZANI_ERR_ARG;
    if (!c->rg.done) return LZANI_ERR_STATE;
    *info = c->rg.info;
    return LZANI_OK;
}

}  // extern "C"
