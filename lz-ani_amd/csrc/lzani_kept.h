// lzani_kept.h -- host side of the output filter on the device (include/lzani.h states the definitions): the checks of the
// kept forms, the stage -- count, scan, write over the directed entries of a finished result buffer -- and the entry points
// (lzani_run_rows_kept, lzani_kept_fetch, lzani_filter_results_device, lzani_debug_filter_results, lzani_get_kept_info and the
// pure lzani_out_filter_lines).  Included by lzani_hip.hip only, behind lzani_prefilter.h; of that file it uses lzani_ctx
// (which holds the Kept), fail, HIPCHK and run_rows_any, of lzani_prefilter.h pf_chunks, of lzani_devmem.h DevMem and
// StreamSpan.  The kernels are lzani_kernels_outfilter.h; the group's form is in lzani_multi.h.
//
// Order of work (kept_stage): the previous result is dropped (two need not fit); the call's tables go to the device --
// ref_ids, row_off, query_ids, row_of[n] (the row of every genome that is a reference of the call), the reported lengths;
// the count pass gives the kept pairs per block of PF_CHUNK entries, the scan their offsets and the exact total; the record
// buffer is allocated at that size; the write pass fills it in entry order.  What the stage reads per leading entry: its own
// result and its mate's (12 B each, the mate's by a gather), two lengths, and the row tables on the way; what it writes:
// 36 B per kept pair.
#pragma once

namespace {

// What the checks find beside errors.
struct KeptRows { u64 entries = 0, leading = 0; };

// The preconditions of the kept forms, on the host before anything runs: the row table of lzani_run_rows (ids below n, row_off
// from 0 and monotone, dense rows of n - 1), and beyond it distinct ref_ids and strictly ascending lists.  row_of[n] is made
// on the way.
int kept_check_rows(lzani_ctx* c, const std::string& fn, u32 n, u32 n_rows, const u32* ref_ids, const u64* row_off, const u32* query_ids,
                    std::vector<u32>& row_of, KeptRows& kr)
{
    row_of.assign(n, OF_NO_ROW);
    if (!n_rows) return LZANI_OK;
    if (row_off[0] != 0) return fail(c, LZANI_ERR_ARG, fn + ": row_off[0] must be 0");
    for (u32 k = 0; k < n_rows; ++k) {
        const u32 a = ref_ids[k];
        if (a >= n) return fail(c, LZANI_ERR_ARG, fn + ": reference id out of range");
        if (row_of[a] != OF_NO_ROW) return fail(c, LZANI_ERR_ARG, fn + ": ref_ids must be distinct (genome " + std::to_string(a) + " leads two rows)");
        row_of[a] = k;
        if (row_off[k + 1] < row_off[k]) return fail(c, LZANI_ERR_ARG, fn + ": row_off not monotone");
        const u64 cnt = row_off[k + 1] - row_off[k];
        if (!query_ids) {
            if (cnt != (u64)n - 1) return fail(c, LZANI_ERR_ARG, fn + ": dense row must have n-1 queries");
            kr.leading += (u64)n - 1 - a;
            continue;
        }
        for (u64 e = row_off[k]; e < row_off[k + 1]; ++e) {
            const u32 q = query_ids[e];
            if (q >= n) return fail(c, LZANI_ERR_ARG, fn + ": query id out of range");
            if (e > row_off[k] && q <= query_ids[e - 1])
                return fail(c, LZANI_ERR_ARG, fn + ": the query ids of a row must ascend strictly (row " + std::to_string(k) + ")");
            kr.leading += q > a;
        }
    }
    kr.entries = row_off[n_rows];
    return LZANI_OK;
}

int kept_check_filter(lzani_ctx* c, const std::string& fn, const lzani_out_filter* f)
{
    if (!f) return fail(c, LZANI_ERR_ARG, fn + ": null filter");
    if (out_filter_has_nan(*f)) return fail(c, LZANI_ERR_ARG, fn + ": a minimum of the filter is not a number");
    return LZANI_OK;
}

// The stage on d_results (this context's device, row_off[n_rows] results, complete on the context's stream or before): fills
// `k`.  The rows passed kept_check_rows, which made row_of.
int kept_stage_run(lzani_ctx* c, Kept& k, u32 n, const u32* report_len, u32 n_rows, const u32* ref_ids, const u64* row_off, const u32* query_ids,
                   const std::vector<u32>& row_of, const KeptRows& kr, const int* d_results, const lzani_out_filter& f)
{
    k.n = n;
    k.info.entries = kr.entries; k.info.leading = kr.leading;
    const u64 E = kr.entries;
    if (!E) { HIPCHK(c, k.rec.alloc(0)); return LZANI_OK; }
    DevMem<u32> d_ref, d_q, d_rowof, d_len, d_blkcnt;
    DevMem<u64> d_off, d_blkoff;
    DevMem<unsigned long long> d_counters;
    const u64 blocks = pf_chunks(E);
    HIPCHK(c, d_ref.alloc(n_rows));
    HIPCHK(c, d_off.alloc((size_t)n_rows + 1));
    HIPCHK(c, d_rowof.alloc(n));
    HIPCHK(c, d_len.alloc(n));
    HIPCHK(c, d_blkcnt.alloc(blocks));
    HIPCHK(c, d_blkoff.alloc(blocks + 1));
    HIPCHK(c, d_counters.alloc(OF_COUNTERS));
    if (query_ids) HIPCHK(c, d_q.alloc(E));
    HIPCHK(c, hipMemcpyAsync(d_ref, ref_ids, (size_t)n_rows * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_off, row_off, ((size_t)n_rows + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_rowof, row_of.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_len, report_len, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if (query_ids) HIPCHK(c, hipMemcpyAsync(d_q, query_ids, (size_t)E * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_counters, 0, OF_COUNTERS * sizeof(unsigned long long), c->stream));
    const OfCall call{d_results, d_off.get(), d_ref.get(), query_ids ? d_q.get() : nullptr, d_rowof.get(), d_len.get(), n_rows, n, f};
    StreamSpan span;
    HIPCHK(c, span.begin(c->stream));
    hipLaunchKernelGGL(k_of_kept<false>, dim3((u32)blocks), dim3(PF_THREADS), 0, c->stream, call, E, d_blkcnt.get(), (const u64*)d_blkoff.get(), (u32*)nullptr, d_counters.get());
    hipLaunchKernelGGL(k_pf_scan, dim3(1), dim3(1024), 0, c->stream, (const u32*)d_blkcnt.get(), blocks, d_blkoff.get());
    HIPCHK(c, hipGetLastError());
    u64 total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, d_blkoff.get() + blocks, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, k.rec.alloc((size_t)total * 9));                 // the exact size, known before the buffer is made
    if (total) {
        hipLaunchKernelGGL(k_of_kept<true>, dim3((u32)blocks), dim3(PF_THREADS), 0, c->stream, call, E, d_blkcnt.get(), (const u64*)d_blkoff.get(), k.rec.get(), d_counters.get());
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, span.end(c->stream));
    unsigned long long counters[OF_COUNTERS] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(counters, d_counters, sizeof counters, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    HIPCHK(c, span.elapsed(ms));
    k.info.filter_ms = ms;
    k.info.unpaired = counters[OF_UNPAIRED]; k.info.kept_lines = counters[OF_LINES]; k.info.kept_pairs = total;
    TRACE("out-filter: entries=%llu leading=%llu unpaired=%llu kept=%llu lines=%llu", (unsigned long long)E, (unsigned long long)kr.leading,
          (unsigned long long)k.info.unpaired, (unsigned long long)total, (unsigned long long)k.info.kept_lines);
    return LZANI_OK;
}

// kept_stage_run into a fresh Kept that becomes the context's on success; a failure synchronises the stream and leaves the
// context without a kept result (the caller dropped the last one) and otherwise unchanged.
int kept_stage(lzani_ctx* c, u32 n, const u32* report_len, u32 n_rows, const u32* ref_ids, const u64* row_off, const u32* query_ids,
               const std::vector<u32>& row_of, const KeptRows& kr, const int* d_results, const lzani_out_filter& f, uint64_t* n_kept)
{
    Kept k;
    const int rc = kept_stage_run(c, k, n, report_len, n_rows, ref_ids, row_off, query_ids, row_of, kr, d_results, f);
    if (rc != LZANI_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    k.done = true;
    c->kept = std::move(k);
    if (n_kept) *n_kept = c->kept.info.kept_pairs;
    return LZANI_OK;
}

// the genome set's own lengths, as the stage takes them
std::vector<u32> kept_own_lengths(const lzani_ctx* c) { return std::vector<u32>(c->gs.L.begin(), c->gs.L.end()); }

}  // namespace

extern "C" {

uint32_t lzani_out_filter_lines(const lzani_out_filter* f, const lzani_result* x, const lzani_result* y, uint32_t len_a, uint32_t len_b)
{
    if (!f || !x || !y || out_filter_has_nan(*f)) return 0xFFFFFFFFu;
    return out_filter_lines(*f, *x, *y, len_a, len_b);
}

int lzani_filter_results_device(lzani_ctx* c, uint32_t n, const uint32_t* report_len, uint32_t n_rows, const uint32_t* ref_ids, const uint64_t* row_off,
                                const uint32_t* query_ids, const void* d_results, const lzani_out_filter* f, uint64_t* n_kept)
{
    if (!c) return LZANI_ERR_ARG;
    const std::string fn = "lzani_filter_results_device";
    if (!n || !report_len || (n_rows && (!ref_ids || !row_off))) return fail(c, LZANI_ERR_ARG, fn + ": null argument");
    if (int rc = kept_check_filter(c, fn, f)) return rc;
    std::vector<u32> row_of;
    KeptRows kr;
    if (int rc = kept_check_rows(c, fn, n, n_rows, ref_ids, row_off, query_ids, row_of, kr)) return rc;
    if (kr.entries && !d_results) return fail(c, LZANI_ERR_ARG, fn + ": null results");
    HIPCHK(c, hipSetDevice(c->dev));
    c->kept = Kept{};                                          // the last result goes first: two need not fit
    return kept_stage(c, n, report_len, n_rows, ref_ids, row_off, query_ids, row_of, kr, (const int*)d_results, *f, n_kept);
}

int lzani_debug_filter_results(lzani_ctx* c, uint32_t n, const uint32_t* report_len, uint32_t n_rows, const uint32_t* ref_ids, const uint64_t* row_off,
                               const uint32_t* query_ids, const lzani_result* results, const lzani_out_filter* f, uint64_t* n_kept)
{
    if (!c) return LZANI_ERR_ARG;
    const u64 E = n_rows && row_off ? row_off[n_rows] : 0;
    if (E && !results) return fail(c, LZANI_ERR_ARG, "lzani_debug_filter_results: null results");
    HIPCHK(c, hipSetDevice(c->dev));
    DevMem<lzani_result> d_res;
    if (const hipError_t e = d_res.alloc(E); e != hipSuccess) {
        c->kept = Kept{};                                      // as where the stage itself runs short: no kept result, not the last call's
        HIPCHK(c, e);
    }
    if (E) HIPCHK(c, hipMemcpy(d_res.get(), results, (size_t)E * sizeof(lzani_result), hipMemcpyHostToDevice));
    return lzani_filter_results_device(c, n, report_len, n_rows, ref_ids, row_off, query_ids, d_res.get(), f, n_kept);
}

int lzani_run_rows_kept(lzani_ctx* c, uint32_t n_rows, const uint32_t* ref_ids, const uint64_t* row_off, const uint32_t* query_ids,
                        const lzani_out_filter* f, const uint32_t* report_len, uint64_t* n_kept)
{
    if (!c) return LZANI_ERR_ARG;
    const std::string fn = "lzani_run_rows_kept";
    if (n_rows && (!ref_ids || !row_off)) return fail(c, LZANI_ERR_ARG, fn + ": null argument");
    if (!c->gs.n) return fail(c, LZANI_ERR_STATE, fn + ": no genomes set");
    if (int rc = kept_check_filter(c, fn, f)) return rc;
    std::vector<u32> row_of, own;
    KeptRows kr;
    if (int rc = kept_check_rows(c, fn, c->gs.n, n_rows, ref_ids, row_off, query_ids, row_of, kr)) return rc;
    if (!report_len) { own = kept_own_lengths(c); report_len = own.data(); }
    HIPCHK(c, hipSetDevice(c->dev));
    c->kept = Kept{};
    DevMem<lzani_result> d_res;
    HIPCHK(c, d_res.alloc(kr.entries));
    if (int rc = run_rows_any(c, n_rows, ref_ids, row_off, query_ids, (int*)d_res.get(), nullptr, nullptr, nullptr)) return rc;
    return kept_stage(c, c->gs.n, report_len, n_rows, ref_ids, row_off, query_ids, row_of, kr, (const int*)d_res.get(), *f, n_kept);
}

int lzani_kept_fetch(lzani_ctx* c, uint64_t first, uint64_t count, lzani_kept_pair* out)
{
    if (!c) return LZANI_ERR_ARG;
    if (!c->kept.done) return fail(c, LZANI_ERR_STATE, "lzani_kept_fetch: no kept result (call lzani_run_rows_kept first)");
    const u64 K = c->kept.info.kept_pairs;
    if (first > K || count > K - first) return fail(c, LZANI_ERR_ARG, "lzani_kept_fetch: the range lies past the end of the kept pairs");
    if (!count) return LZANI_OK;
    if (!out) return fail(c, LZANI_ERR_ARG, "lzani_kept_fetch: null output");
    static_assert(sizeof(lzani_kept_pair) == 36, "lzani_kept_pair is nine 32-bit fields");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipMemcpy(out, c->kept.rec.get() + 9 * first, (size_t)count * 36, hipMemcpyDeviceToHost));
    c->kept.info.bytes_to_host += count * 36;
    return LZANI_OK;
}

int lzani_get_kept_info(const lzani_ctx* c, lzani_kept_info* info)
{
    if (!c || !info) return LZANI_ERR_ARG;
    if (!c->kept.done) return LZANI_ERR_STATE;
    *info = c->kept.info;
    return LZANI_OK;
}

}  // extern "C"
