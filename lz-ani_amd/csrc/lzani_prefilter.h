// lzani_prefilter.h -- host side of the k-mer prefilter: the slice plan, the pass plan, the pass / tile driver and the
// entry points (lzani_prefilter, _cross, _codes, _codes_cross, the fetch and the info calls).  Included by lzani_hip.hip
// only, after lzani_ooc.h; of that file it uses lzani_ctx (which holds the Prefilter), fail, HIPCHK and sort_keys, of
// lzani_index.h gtab and for_slices, of lzani_set_plan.h env_u64, of lzani_devmem.h DevEvent.  The kernels are
// lzani_kernels_prefilter.h, the sort is lzani_sort.hip's.
//
// The stage computes, for every pair of genomes, how many sampled canonical k-mers they share, and keeps the pairs
// above the thresholds as CSR rows.  The cross form (n_ref > 0) does so for the n_ref reference rows against the
// n - n_ref query columns only.  The genomes come from the resident set, or (PfStream) from the caller's host memory,
// slice by slice through one staging buffer.  A KEY SWEEP is one run of a key kernel over all genomes.
//
// Order of work (PfRun::run):
//   count sweep over the whole set: kept windows per chunk, their total Pv; the window cap; one pass or several
//   several passes only: histogram sweep (windows per bin of the k-mer space), the pass plan, the windows of each pass
//   workspace for the fullest pass (ka, kb, sort scratch)
//   PfRun::tiles_and_passes: tile of matrix rows outer, pass inner.  A pass's postings are built by three sweeps
//     (count of its windows, canonical keys -> sorted dictionary, rank keys -> sorted postings), added into the tile
//     (count_tile), and after the tile's last pass its kept entries are compacted into a PrefilterTile.  With one pass the
//     postings are built once, before the tiles, and every tile counts from them
//     Sparse counting (include/lzani.h): the pair table stands where the matrix tile stands -- alloc_table / count_sparse /
//     compact_sparse beside alloc_tile / count_tile / compact_tile -- and the tiles come from PfTiles' halving rule
//   totals, stage times.
//
// What the counters count:
//   info.positions / distinct_kmers / postings / entries   kept windows, distinct k-mers and postings of the set (the sums
//       over one tile's passes), kept pairs;  info.tiles  PrefilterTiles made
//   info.keys_ms, sort_ms, count_ms, compact_ms; pinfo.hist_ms; sinfo.upload_ms   device time between event pairs (PfClock)
//   pinfo.key_sweeps  W: 1 with no kept window, 3 with one pass and any number of tiles, 2 + 3 T P' with several (T tiles,
//       P' passes that hold a window);  pinfo.passes, largest_pass, cap, workspace_bytes (ka + kb + sort scratch)
//   sinfo.slice_uploads / staged_bytes  slices copied into the staging buffer: a sweep walks the slices up or down in
//       turn and does not copy the one the buffer holds, so W sweeps over S slices upload W (S - 1) + 1
//   cinfo.tile_rows / matrix_bytes  the tile of the cross matrix.
//   spinfo (sparse counting)  attempts, pass_runs, slots, table_bytes, pairs_seen, max_fill; info.tiles then counts the
//       finished tiles, and with several passes W = 2 + 3 pass_runs.
#pragma once
#include "lzani_sparse_plan.h"

namespace {

// Device time of the prefilter's stages (and of the streamed form's slice copies): pairs of events on the context's stream,
// summed per stage at the end.
enum { PF_ST_KEYS = 0, PF_ST_SORT = 1, PF_ST_COUNT = 2, PF_ST_COMPACT = 3, PF_ST_UPLOAD = 4, PF_ST_HIST = 5, PF_STAGES = 6 };
constexpr u64 PF_MAX_PASS_WINDOWS = 0xFFFFFFEFull;       // what one pass may hold: the u32 run offsets of its postings, and lzani_sort_keys' limit
struct PfClock {
    hipStream_t stream;
    std::vector<DevEvent> ev;             // begin, end, begin, end, ...
    std::vector<int> stage;
    explicit PfClock(hipStream_t s) : stream(s) {}
    hipError_t mark()
    {
        DevEvent e;
        const hipError_t rc = e.create();
        if (rc != hipSuccess) return rc;
        ev.push_back(std::move(e));
        return hipEventRecord(ev.back(), stream);
    }
    hipError_t begin(int st) { stage.push_back(st); return mark(); }
    hipError_t end() { return mark(); }
    hipError_t collect(double ms[PF_STAGES])
    {
        for (size_t k = 0; k + 1 < ev.size(); k += 2) {
            float t = 0;
            hipError_t rc = hipEventSynchronize(ev[k + 1]);
            if (rc == hipSuccess) rc = hipEventElapsedTime(&t, ev[k], ev[k + 1]);
            if (rc != hipSuccess) return rc;
            ms[stage[k / 2]] += t;
        }
        return hipSuccess;
    }
};
// blocks of PF_CHUNK elements (the key and compaction kernels) / of PF_THREADS threads, one per element, that cover x
u64 pf_chunks(u64 x) { return (x + PF_CHUNK - 1) / PF_CHUNK; }
u32 pf_blocks(u64 x) { return (u32)((x + PF_THREADS - 1) / PF_THREADS); }
// the free device memory now
int pf_free_bytes(lzani_ctx* c, u64& bytes)
{
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));      // (the text of a failure names the call as written here)
    bytes = free_b;
    return LZANI_OK;
}
int pf_sort(lzani_ctx* c, PrefilterWork& w, const unsigned long long* in, unsigned long long* out, size_t n, int b0, int b1)
{
    return sort_keys(c, w.tmp, in, out, n, 1, b0, b1, "lzani_prefilter: sort", false);      // (alloc_keys sized the scratch: it does not grow)
}

// The slice plan of the streamed prefilter (lzani_plan_slices): genomes in id order into contiguous slices; a new slice
// starts where the next genome would take the slice's sum of lengths above slice_bytes (so genomes of length 0 join the
// current one).  first[s] .. first[s + 1] are slice s's genomes.  slice_bytes 0: one slice.  Returns the number of
// slices, or LZANI_ERR_ARG with the reason in msg.
int plan_slices_impl(u32 n, const u32* len, u64 slice_bytes, std::vector<u32>& first, std::string& msg)
{
    if (!n || !len) { msg = "empty input"; return LZANI_ERR_ARG; }
    first.assign(1, 0);
    if (slice_bytes == 0) { first.push_back(n); return 1; }
    u32 Lmax = 0;
    for (u32 g = 0; g < n; ++g) Lmax = std::max(Lmax, len[g]);
    if ((u64)Lmax > slice_bytes) {
        msg = "slice size of " + std::to_string(slice_bytes) + " bytes is below the minimum of " + std::to_string(Lmax) +
              " bytes (a slice must hold the longest genome)";
        return LZANI_ERR_ARG;
    }
    if ((u64)n > 0x7FFFFFFFull) { msg = "too many genomes"; return LZANI_ERR_ARG; }
    u64 cur = 0;
    for (u32 g = 0; g < n; ++g) {
        if (cur + len[g] > slice_bytes) { first.push_back(g); cur = 0; }
        cur += len[g];
    }
    first.push_back(n);
    return (int)first.size() - 1;
}

// The streamed key source of the prefilter (lzani_prefilter_codes): the genomes stay in the caller's host memory, 1 B a
// base, and pass slice by slice through one staging buffer on the device.  A key sweep goes over all slices, up or
// down; the slice the buffer holds already is not copied again.
struct PfStream {
    const uint8_t* const* codes = nullptr;
    const u32* len = nullptr;
    std::vector<u32> first;               // the slice plan
    std::vector<u64> bytes;               // per slice: the sum of its genomes' lengths
    DevMem<unsigned char> stage;          // the largest slice
    DevMem<u64> d_off;                    // per genome: its byte offset in the staging buffer when its slice is there
    DevMem<u32> d_len;
    std::vector<unsigned char> bounce;    // host side of a copy: the genomes' codes put together, a piece at a time
    int staged = -1;                      // the slice in the buffer
    lzani_prefilter_stream_info info{};
};
enum : u64 { PF_BOUNCE_BYTES = 64ull << 20 };

// Slice s into the staging buffer: the codes of its genomes one after the other, through the bounce buffer.
int pf_upload_slice(lzani_ctx* c, PfStream& st, PfClock& clk, u32 s)
{
    u64 at = 0;
    size_t fill = 0;
    auto flush = [&]() -> int {
        if (!fill) return LZANI_OK;
        HIPCHK(c, clk.begin(PF_ST_UPLOAD));
        HIPCHK(c, hipMemcpyAsync(st.stage.get() + at, st.bounce.data(), fill, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, clk.end());
        HIPCHK(c, hipStreamSynchronize(c->stream));            // (the bounce buffer is filled again)
        at += fill;
        fill = 0;
        return LZANI_OK;
    };
    for (u32 g = st.first[s]; g < st.first[s + 1]; ++g) {
        const uint8_t* src = st.codes[g];
        for (u64 left = st.len[g]; left;) {
            const size_t take = (size_t)std::min<u64>(left, st.bounce.size() - fill);
            memcpy(st.bounce.data() + fill, src, take);
            fill += take; src += take; left -= take;
            if (fill == st.bounce.size()) if (int rc = flush()) return rc;
        }
    }
    if (int rc = flush()) return rc;
    st.staged = (int)s;
    ++st.info.slice_uploads;
    st.info.staged_bytes += st.bytes[s];
    return LZANI_OK;
}

// The pass plan of the prefilter (lzani_plan_passes): bin_lo[0 .. P] with bin_lo[0] = 0 and bin_lo[P] = PF_BINS.  Forced:
// P equal ranges.  Automatic: greedy from bin 0, a pass takes bins while its sum of windows stays <= cap.  Returns P, or
// LZANI_ERR_ARG (forced above PF_BINS; a single bin above cap: *bad_bin names it).
int plan_passes_impl(const u64* hist, u64 cap, u32 forced, std::vector<u32>& bin_lo, u32* bad_bin = nullptr)
{
    bin_lo.assign(1, 0);
    if (forced) {
        if (forced > PF_BINS) return LZANI_ERR_ARG;
        for (u32 p = 1; p <= forced; ++p) bin_lo.push_back((u32)((u64)PF_BINS * p / forced));
        return (int)forced;
    }
    if (!hist) return LZANI_ERR_ARG;
    u64 sum = 0;
    for (u32 b = 0; b < PF_BINS; ++b) {
        if (hist[b] > cap) { if (bad_bin) *bad_bin = b; return LZANI_ERR_ARG; }
        if (hist[b] > cap - sum) { bin_lo.push_back(b); sum = 0; }        // (sum <= cap always; a pass holds a bin at least)
        sum += hist[b];
    }
    bin_lo.push_back(PF_BINS);
    return (int)bin_lo.size() - 1;
}

// The instantiations of the two key kernels, [mode][ranged]: of one pass's windows only (ranged) or of all.  PF_HIST is
// never ranged.
#define PF_MODE_TABLE(K) {{K<PF_COUNT, false>, K<PF_COUNT, true>}, {K<PF_CANON, false>, K<PF_CANON, true>}, {K<PF_RANK, false>, K<PF_RANK, true>}, {K<PF_HIST, false>, K<PF_HIST, false>}}
const decltype(&k_pf_keys<PF_COUNT, false>) pf_keys_kernel[4][2] = PF_MODE_TABLE(k_pf_keys);
const decltype(&k_pf_keys_codes<PF_COUNT, false>) pf_keys_codes_kernel[4][2] = PF_MODE_TABLE(k_pf_keys_codes);
#undef PF_MODE_TABLE

// One k-mer pass: the windows whose bin lies in [lo, hi) (ranged; else all windows, and the kernels compute no bin); how
// many it keeps (the whole set's count, or the histogram's sum over its bins), and the distinct k-mers and postings that
// build_postings found.
struct PfPass { bool ranged = false; u32 lo = 0, hi = PF_BINS; u64 windows = 0, D = 0, M = 0; };

// One run of the stage: fills pf (a fresh Prefilter) from the resident genome set, or (st given) from the n genomes of
// the streamed source.  The two differ in where the key sweeps take their genomes from; all behind them is shared.
// n_ref > 0: the cross form -- the matrix is the n_ref reference rows by the n - n_ref query columns, its tiles cover the
// references only, and every set of postings gets its runsplit.
struct PfRun {
    lzani_ctx* c; Prefilter& pf; PrefilterWork& w; lzani_prefilter_info& info; lzani_prefilter_pass_info& pinfo; lzani_prefilter_sparse_info& sp; PfStream* st;
    PfClock clk;
    const GenomeTab G;                    // resident source
    const int k; const u64 sample_max; const u32 min_shared; const double min_ratio;
    const u32 n, n_ref, n_rows, n_cols;   // genomes; cross form: references; the count matrix
    u64 n_chunks = 0, rows = 0;           // chunks of all genomes; the tile's height
    std::vector<u64> h_off;               // a tile's row offsets, read back
    bool sparse = false;                  // the pair table counts, not the matrix tile
    u64 slots = 0, sp_used = 0;           // its slots; those in use after the last count into it

    PfRun(lzani_ctx* c_, Prefilter& pf_, int k_, u64 sample_max_, u32 min_shared_, double min_ratio_, u32 n_, PfStream* st_, u32 n_ref_)
        : c(c_), pf(pf_), w(pf_.work), info(pf_.info), pinfo(pf_.pinfo), sp(pf_.spinfo), st(st_), clk(c_->stream), G(st_ ? GenomeTab{} : gtab(c_)), k(k_), sample_max(sample_max_),
          min_shared(std::max<u32>(min_shared_, 1)), min_ratio(min_ratio_), n(n_), n_ref(n_ref_), n_rows(n_ref_ ? n_ref_ : n_), n_cols(n_ref_ ? n_ - n_ref_ : n_) {}

    u64 len_of(u32 g) const { return st ? (u64)st->len[g] : (u64)c->gs.L[g]; }

    // One key sweep: pass p's windows of all genomes in `mode` (PF_HIST: out is the histogram; PF_RANK: the dictionary is
    // in ka).  A sweep goes over runs of genomes.  Resident: one run, all genomes.  Streamed: a run per slice, the slices in
    // the sweep's direction (the sweeps alternate: up, down, up, ...), each copied unless the buffer holds it.  A run is
    // launched in slices of genomes (for_slices); the two sources differ in the kernel and its arguments.
    int keys(int mode, const PfPass& p, unsigned long long* out)
    {
        const unsigned long long* dict = mode == PF_RANK ? w.ka.get() : nullptr;
        const u64 D = mode == PF_RANK ? p.D : 0;
        const u32 S = st ? (u32)st->first.size() - 1 : 1;
        const bool up = pinfo.key_sweeps++ % 2 == 0;
        for (u32 i = 0; i < S; ++i) {
            const u32 s = up ? i : S - 1 - i;
            if (st && st->staged != (int)s) if (int rc = pf_upload_slice(c, *st, clk, s)) return rc;
            const u32 f = st ? st->first[s] : 0, ns = st ? st->first[s + 1] - f : n;
            u64 lmax = 0;
            for (u32 g = f; g < f + ns; ++g) lmax = std::max(lmax, len_of(g));
            const u32 gx = (u32)pf_chunks(lmax);
            HIPCHK(c, clk.begin(mode == PF_HIST ? PF_ST_HIST : PF_ST_KEYS));
            if (gx) for_slices(ns, [&](u32 y0, u32 cnt) {
                const dim3 gd(gx, cnt);
                if (st)
                    hipLaunchKernelGGL(pf_keys_codes_kernel[mode][p.ranged], gd, dim3(PF_THREADS), 0, c->stream, (const unsigned char*)st->stage.get(), st->bytes[s],
                                       (const u64*)(st->d_off.get() + f), (const u32*)(st->d_len.get() + f), w.cbase.get(), f, y0, k, sample_max, p.lo, p.hi,
                                       w.blkcnt.get(), w.blkoff.get(), dict, D, out);
                else
                    hipLaunchKernelGGL(pf_keys_kernel[mode][p.ranged], gd, dim3(PF_THREADS), 0, c->stream, G, w.cbase.get(), y0, k, c->P.mrd, sample_max, p.lo, p.hi,
                                       w.blkcnt.get(), w.blkoff.get(), dict, D, out);
            });
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, clk.end());
        }
        return LZANI_OK;
    }
    // the total of a scan, read back
    int scan_total(const u32* cnt, u64 cnt_n, u64* off, u64& total)
    {
        hipLaunchKernelGGL(k_pf_scan, dim3(1), dim3(1024), 0, c->stream, cnt, cnt_n, off);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&total, off + cnt_n, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return LZANI_OK;
    }
    // in[0 .. cnt) ascending -> out without adjacent duplicates; their number
    int uniq(const unsigned long long* in, u64 cnt, unsigned long long* out, u32* per_genome, u64& n_out)
    {
        const u32 blocks = (u32)pf_chunks(cnt);
        hipLaunchKernelGGL(k_pf_uniq<false>, dim3(blocks), dim3(PF_THREADS), 0, c->stream, in, cnt, w.ucnt.get(), w.uoff.get(), out, per_genome, n);
        if (int rc = scan_total(w.ucnt, blocks, w.uoff, n_out)) return rc;
        hipLaunchKernelGGL(k_pf_uniq<true>, dim3(blocks), dim3(PF_THREADS), 0, c->stream, in, cnt, w.ucnt.get(), w.uoff.get(), out, per_genome, n);
        HIPCHK(c, hipGetLastError());
        return LZANI_OK;
    }
    // the kept windows of a pass counted per chunk (blkcnt) and scanned (blkoff): where the two key sweeps behind it write
    int count_windows(const PfPass& p, u64& Pw)
    {
        if (int rc = keys(PF_COUNT, p, nullptr)) return rc;
        HIPCHK(c, clk.begin(PF_ST_KEYS));
        if (int rc = scan_total(w.blkcnt, n_chunks, w.blkoff, Pw)) return rc;
        HIPCHK(c, clk.end());
        return LZANI_OK;
    }
    // ka, kb, the uniq counters and the radix scratch for passes of at most `windows` kept windows
    int alloc_keys(u64 windows)
    {
        HIPCHK(c, w.ka.alloc(windows));
        HIPCHK(c, w.kb.alloc(windows));
        HIPCHK(c, w.ucnt.alloc(pf_chunks(windows)));
        HIPCHK(c, w.uoff.alloc(pf_chunks(windows) + 1));
        size_t need1 = 0, need2 = 0;
        if (int rc = sort_scratch_bytes(c, windows, 1, 0, 2 * k, "lzani_prefilter: sort", need1)) return rc;
        if (int rc = sort_scratch_bytes(c, windows, 1, 32, 64, "lzani_prefilter: sort", need2)) return rc;
        HIPCHK(c, w.tmp.alloc(std::max(need1, need2)));
        pinfo.workspace_bytes = w.ka.bytes() + w.kb.bytes() + w.tmp.bytes();
        return LZANI_OK;
    }
    // The pipeline of one pass behind its count_windows (p.windows > 0): dictionary in ka, then the postings in kb and
    // where every rank's begin (runoff, allocated here unless it is large enough); p.D and p.M are their numbers.
    // per_genome: |K(g)| += the genome's distinct k-mers of the pass.  last_sweep: no key sweep follows this pass's.
    int build_postings(PfPass& p, u32* per_genome, bool last_sweep)
    {
        if (int rc = keys(PF_CANON, p, w.ka.get())) return rc;
        // ---- dictionary: the keys sorted, every distinct k-mer once; its place is its rank
        HIPCHK(c, clk.begin(PF_ST_SORT));
        if (int rc = pf_sort(c, w, w.ka, w.kb, p.windows, 0, 2 * k)) return rc;
        if (int rc = uniq(w.kb, p.windows, w.ka, nullptr, p.D)) return rc;
        HIPCHK(c, clk.end());
        // ---- postings: rank << 32 | genome of every kept window, in genome order; a stable sort by rank leaves the genomes of
        // a rank ascending; adjacent duplicates dropped, a run of equal rank lists the genomes that hold the k-mer
        if (int rc = keys(PF_RANK, p, w.kb.get())) return rc;
        if (st && last_sweep) { HIPCHK(c, hipStreamSynchronize(c->stream)); st->stage.reset(); }      // (the last sweep is done: room for the count matrix)
        HIPCHK(c, clk.begin(PF_ST_SORT));
        if (int rc = pf_sort(c, w, w.kb, w.ka, p.windows, 32, 32 + ceil_log2(p.D))) return rc;
        if (int rc = uniq(w.ka, p.windows, w.kb, per_genome, p.M)) return rc;
        const dim3 grid(pf_blocks(p.M));
        HIPCHK(c, w.runoff.reserve(p.D + 1));
        hipLaunchKernelGGL(k_pf_runs, grid, dim3(PF_THREADS), 0, c->stream, w.kb.get(), p.M, w.runoff.get(), p.D);
        if (n_ref) {
            HIPCHK(c, w.runsplit.reserve(p.D + 1));
            hipLaunchKernelGGL(k_pf_split, grid, dim3(PF_THREADS), 0, c->stream, w.kb.get(), p.M, p.D, n_ref, w.runsplit.get());
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, clk.end());
        return LZANI_OK;
    }
    // the dense rule: the rows of a matrix tile in half of the free device memory
    u64 dense_rows(u64 free_b) const { return std::min<u64>(n_rows, std::max<u64>(1, free_b / 2 / ((u64)4 * n_cols))); }
    // the height of the matrix tile from what is free now, and the tile's buffers
    int alloc_tile()
    {
        u64 free_b = 0;
        if (int rc = pf_free_bytes(c, free_b)) return rc;
        rows = dense_rows(free_b);
        if (const auto forced = env_u64("LZANI_PREFILTER_TILE_ROWS")) rows = std::min<u64>(n_rows, std::max<u64>(1, *forced));
        HIPCHK(c, w.mat.alloc(rows * n_cols));
        HIPCHK(c, w.rowcnt.alloc(rows));
        HIPCHK(c, w.rowoff.alloc(rows + 1));
        if (n_ref) { pf.cinfo.tile_rows = (u32)rows; pf.cinfo.matrix_bytes = w.mat.bytes(); }
        return LZANI_OK;
    }
    // the postings in kb (pass p's) added into the tile of rows r0 .. r1; clear: the tile's first pass
    int count_tile(u32 r0, u32 r1, const PfPass& p, bool clear)
    {
        HIPCHK(c, clk.begin(PF_ST_COUNT));
        if (clear) HIPCHK(c, hipMemsetAsync(w.mat, 0, (size_t)(r1 - r0) * n_cols * 4, c->stream));
        hipLaunchKernelGGL((n_ref ? k_pf_count<true> : k_pf_count<false>), dim3(pf_blocks(p.M)), dim3(PF_THREADS), 0, c->stream, w.kb.get(), p.M,
                           w.runoff.get(), p.D, n, r0, r1, w.mat.get(), (const u32*)w.runsplit.get(), n_ref);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, clk.end());
        return LZANI_OK;
    }
    // What compact_tile and compact_sparse end in.  read_rowoff: the offsets of the tile's nr rows, tile-relative, from
    // rowoff into h_off[0 .. nr].  publish_tile: the tile joins the result behind the tiles so far -- its rows' offsets
    // into pf.row_off, its entries (h_off[nr]) into info.entries.
    int read_rowoff(u32 nr)
    {
        h_off.resize((size_t)nr + 1);
        HIPCHK(c, hipMemcpyAsync(h_off.data(), w.rowoff, ((size_t)nr + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return LZANI_OK;
    }
    void publish_tile(PrefilterTile&& tile)
    {
        const u32 nr = tile.r1 - tile.r0;
        for (u32 r = 0; r < nr; ++r) pf.row_off[(size_t)tile.r0 + r + 1] = info.entries + h_off[r + 1];
        info.entries += h_off[nr];                                 // (the kept pairs of the tiles so far)
        pf.tiles.push_back(std::move(tile));
        ++info.tiles;
    }
    // the kept entries of the tile's rows into a PrefilterTile of their own
    int compact_tile(u32 r0, u32 r1)
    {
        const u32 nr = r1 - r0, row_blocks = (nr + PF_THREADS / 64 - 1) / (PF_THREADS / 64);
        HIPCHK(c, clk.begin(PF_ST_COMPACT));
        hipLaunchKernelGGL((n_ref ? k_pf_rows<false, true> : k_pf_rows<false, false>), dim3(row_blocks), dim3(PF_THREADS), 0, c->stream, w.mat.get(), n, r0, r1,
                           pf.kmers_of.get(), min_shared, min_ratio, w.rowcnt.get(), w.rowoff.get(), (u32*)nullptr, (u32*)nullptr, n_ref);
        hipLaunchKernelGGL(k_pf_scan, dim3(1), dim3(1024), 0, c->stream, w.rowcnt.get(), (u64)nr, w.rowoff.get());
        HIPCHK(c, hipGetLastError());
        if (int rc = read_rowoff(nr)) return rc;
        PrefilterTile tile;
        tile.r0 = r0; tile.r1 = r1;
        HIPCHK(c, tile.ids.alloc(h_off[nr]));
        HIPCHK(c, tile.shared.alloc(h_off[nr]));
        hipLaunchKernelGGL((n_ref ? k_pf_rows<true, true> : k_pf_rows<true, false>), dim3(row_blocks), dim3(PF_THREADS), 0, c->stream, w.mat.get(), n, r0, r1,
                           pf.kmers_of.get(), min_shared, min_ratio, w.rowcnt.get(), w.rowoff.get(), tile.ids.get(), tile.shared.get(), n_ref);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, clk.end());
        publish_tile(std::move(tile));
        return LZANI_OK;
    }

    // Which accumulator counts (called where the tile is sized).  Automatic: the matrix wherever the dense rule gives one
    // tile or a tile height is forced, the table where the matrix would need several tiles (a choice, not a measurement).
    int choose_counting()
    {
        sparse = c->pf_counting == LZANI_PF_COUNTING_SPARSE;
        if (c->pf_counting != LZANI_PF_COUNTING_AUTO || env_u64("LZANI_PREFILTER_TILE_ROWS")) return LZANI_OK;
        u64 free_b = 0;
        if (int rc = pf_free_bytes(c, free_b)) return rc;
        sparse = dense_rows(free_b) < n_rows;
        return LZANI_OK;
    }
    // the slots of the pair table from what is free now, and the table's buffers
    int alloc_table()
    {
        u64 free_b = 0;
        if (int rc = pf_free_bytes(c, free_b)) return rc;
        const u64 cells = (u64)n_rows * n_cols;                    // (< 2^64)
        u64 top = 2;                                               // the smallest power of two >= 2 * cells, 2^32 at most
        while (top < ((u64)1 << 32) && top / 2 < cells) top *= 2;
        slots = 0;
        for (u64 s = 2; s <= top && 12 * s <= free_b / 2; s *= 2) slots = s;
        if (const auto forced = env_u64("LZANI_PREFILTER_TABLE_SLOTS")) slots = *forced;      // (checked in run())
        if (!slots) return fail(c, LZANI_ERR_NOMEM, "lzani_prefilter: no room for a pair table of two slots");
        HIPCHK(c, w.sp_keys.alloc(slots));
        HIPCHK(c, w.sp_cnt.alloc(slots));
        HIPCHK(c, w.sp_ctl.alloc(2));
        HIPCHK(c, w.sp_bcnt.alloc(pf_chunks(slots)));
        HIPCHK(c, w.sp_boff.alloc(pf_chunks(slots) + 1));
        sp.sparse = 1; sp.slots = slots; sp.table_bytes = w.sp_keys.bytes() + w.sp_cnt.bytes();
        return LZANI_OK;
    }
    // count_tile into the pair table.  clear: the attempt's first pass.  overflow: the rows r0 .. r1 hold more than
    // slots / 2 pairs (with the passes so far), the attempt is void; else sp_used = the slots in use.
    int count_sparse(u32 r0, u32 r1, const PfPass& p, bool clear, bool& overflow)
    {
        HIPCHK(c, clk.begin(PF_ST_COUNT));
        if (clear) {
            HIPCHK(c, hipMemsetAsync(w.sp_keys, 0xFF, (size_t)slots * 8, c->stream));
            HIPCHK(c, hipMemsetAsync(w.sp_cnt, 0, (size_t)slots * 4, c->stream));
            HIPCHK(c, hipMemsetAsync(w.sp_ctl, 0, 8, c->stream));
        }
        hipLaunchKernelGGL((n_ref ? k_pf_count_sparse<true> : k_pf_count_sparse<false>), dim3(pf_blocks(p.M)), dim3(PF_THREADS), 0, c->stream,
                           w.kb.get(), p.M, w.runoff.get(), p.D, n, r0, r1, w.sp_keys.get(), w.sp_cnt.get(), slots, w.sp_ctl.get(), (const u32*)w.runsplit.get(), n_ref);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, clk.end());
        u32 ctl[2] = {0, 0};
        HIPCHK(c, hipMemcpyAsync(ctl, w.sp_ctl, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        overflow = ctl[PF_SP_OVERFLOW] != 0;
        sp_used = ctl[PF_SP_USED];
        return LZANI_OK;
    }
    // compact_tile from the pair table: the kept keys, sorted (row after row, ascending b), their ids and counts, the rows' offsets
    int compact_sparse(u32 r0, u32 r1)
    {
        const u32 nr = r1 - r0, blocks = (u32)pf_chunks(slots);
        u64 K = 0;
        HIPCHK(c, clk.begin(PF_ST_COMPACT));
        hipLaunchKernelGGL(k_pf_sparse_kept<false>, dim3(blocks), dim3(PF_THREADS), 0, c->stream, w.sp_keys.get(), w.sp_cnt.get(), slots, pf.kmers_of.get(), min_shared,
                           min_ratio, w.sp_bcnt.get(), w.sp_boff.get(), (unsigned long long*)nullptr);
        if (int rc = scan_total(w.sp_bcnt, blocks, w.sp_boff, K)) return rc;
        const int bits = 32 + ceil_log2(n);
        HIPCHK(c, w.sp_kin.reserve(K));
        HIPCHK(c, w.sp_kout.reserve(K));
        PrefilterTile tile;
        tile.r0 = r0; tile.r1 = r1;
        HIPCHK(c, tile.ids.alloc(K));
        HIPCHK(c, tile.shared.alloc(K));
        HIPCHK(c, w.rowoff.reserve((size_t)nr + 1));
        hipLaunchKernelGGL(k_pf_sparse_kept<true>, dim3(blocks), dim3(PF_THREADS), 0, c->stream, w.sp_keys.get(), w.sp_cnt.get(), slots, pf.kmers_of.get(), min_shared,
                           min_ratio, w.sp_bcnt.get(), w.sp_boff.get(), w.sp_kin.get());
        HIPCHK(c, hipGetLastError());
        if (int rc = sort_keys(c, w.sp_tmp, w.sp_kin, w.sp_kout, K, 1, 0, bits, "lzani_prefilter: sort", false)) return rc;
        if (K) hipLaunchKernelGGL(k_pf_sparse_fetch, dim3(pf_blocks(K)), dim3(PF_THREADS), 0, c->stream, w.sp_kout.get(), K, w.sp_keys.get(),
                                  w.sp_cnt.get(), slots, tile.ids.get(), tile.shared.get());
        hipLaunchKernelGGL(k_pf_sparse_rowoff, dim3(nr / PF_THREADS + 1), dim3(PF_THREADS), 0, c->stream, w.sp_kout.get(), K, r0, nr, w.rowoff.get());
        HIPCHK(c, hipGetLastError());
        if (int rc = read_rowoff(nr)) return rc;
        HIPCHK(c, clk.end());
        if (h_off[nr] != K) return fail(c, LZANI_ERR_DEVICE, "lzani_prefilter: the pair table's kept keys lie outside the tile's rows");
        publish_tile(std::move(tile));
        sp.pairs_seen += sp_used;
        sp.max_fill = std::max<u64>(sp.max_fill, sp_used);
        return LZANI_OK;
    }

    // Several passes: the histogram of the kept windows over the bins, the plan (pf.bin_lo), and `passes`: those of the plan
    // that hold a window (an empty one has nothing to add), with their windows.
    int plan_from_histogram(u32 forced, std::vector<PfPass>& passes)
    {
        DevMem<unsigned long long> d_hist;
        std::vector<u64> hist(PF_BINS);
        HIPCHK(c, d_hist.alloc(PF_BINS));
        HIPCHK(c, hipMemsetAsync(d_hist, 0, (size_t)PF_BINS * 8, c->stream));
        if (int rc = keys(PF_HIST, PfPass{}, d_hist.get())) return rc;
        HIPCHK(c, hipMemcpyAsync(hist.data(), d_hist, (size_t)PF_BINS * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        d_hist.reset();
        u32 bad_bin = 0;
        const int np = plan_passes_impl(hist.data(), pinfo.cap, forced, pf.bin_lo, &bad_bin);
        if (np < 0)
            return fail(c, LZANI_ERR_ARG, "lzani_prefilter: bin " + std::to_string(bad_bin) + " of the k-mer passes alone holds " + std::to_string(hist[bad_bin]) +
                                          " sampled k-mer windows, a pass at most " + std::to_string(pinfo.cap) + ": lower sample_max");
        u64 sum = 0;
        for (int p = 0; p < np; ++p) {
            PfPass ps{true, pf.bin_lo[p], pf.bin_lo[p + 1]};
            for (u32 b = ps.lo; b < ps.hi; ++b) ps.windows += hist[b];
            sum += ps.windows;
            pinfo.largest_pass = std::max(pinfo.largest_pass, ps.windows);
            if (ps.windows) passes.push_back(ps);
        }
        if (pinfo.largest_pass > PF_MAX_PASS_WINDOWS)
            return fail(c, LZANI_ERR_ARG, "lzani_prefilter: " + std::to_string(pinfo.largest_pass) + " sampled k-mer windows in one of the forced passes; a pass holds fewer than 2^32");
        if (sum != info.positions) return fail(c, LZANI_ERR_DEVICE, "lzani_prefilter: the passes' windows do not sum to the set's");
        return LZANI_OK;
    }

    // The one driver of one pass and of several: tile of matrix rows outer, pass inner.  What tells the two apart is
    // whether a pass is ranged, and what a caller can observe depends on it in two ways.
    //   Sweeps.  One pass, {0, PF_BINS}, not ranged: its postings are built once, before the tiles, and every tile counts
    //   from them: W = 3 with the count sweep of the whole set, for any number of tiles.  Several, ranged: a pass's
    //   postings do not outlive the next pass's, so every (tile, non-empty pass) rebuilds them: W = 2 + 3 T P'.
    //   What is held while the tile is sized -- the tile's height comes from the free memory.  One pass: ka and the sort
    //   scratch are released first (the postings are in kb); runoff / runsplit were reserved at D + 1.  Several: the whole
    //   workspace of the fullest pass stays, and runoff / runsplit are allocated at largest + 1 (a pass's distinct k-mers
    //   are no more than its windows).  Streamed: the staging buffer goes after the last key sweep and not before -- with
    //   one pass that is before the tile is sized, with several the tile is sized beside it.
    //   Sparse counting: the same loop over PfTiles, with attempts that may be abandoned.  Then a tile's passes can run more
    //   than once, so |K(g)| of a pass goes in where the pass's postings are built for the first time (kmers_in), and the
    //   last key sweep is not known in advance: with several passes the staging buffer is released behind the loop.  With
    //   one pass an abandoned attempt repeats the count only.  W = 2 + 3 pass_runs with several passes.
    // |K(g)| is accumulated once per pass: dense, on the first tile.
    int tiles_and_passes(std::vector<PfPass>& passes)
    {
        const bool rebuild = passes[0].ranged;
        if (int rc = alloc_keys(pinfo.largest_pass)) return rc;
        if (rebuild) {
            HIPCHK(c, w.runoff.alloc(pinfo.largest_pass + 1));
            if (n_ref) HIPCHK(c, w.runsplit.alloc(pinfo.largest_pass + 1));
        } else {
            if (int rc = build_postings(passes[0], pf.kmers_of.get(), true)) return rc;
            w.ka.reset();                                          // (the count matrix may use the room)
            w.tmp.reset();
        }
        const bool with_matrix = n > 1 && (rebuild || passes[0].M);
        if (with_matrix) {
            if (int rc = choose_counting()) return rc;
            if (int rc = sparse ? alloc_table() : alloc_tile()) return rc;
        } else rows = n_rows;
        if (sparse && !rebuild) sp.pass_runs = 1;
        std::vector<char> kmers_in(passes.size(), 0);             // per pass: its |K(g)| is in
        PfTiles tl(n_rows, sparse ? n_rows : rows);
        while (tl.more()) {
            const u32 r0 = tl.r0, r1 = tl.r1();
            tl.attempt();
            bool clear = true, overflow = false;
            for (size_t i = 0; i < passes.size() && !overflow; ++i) {
                PfPass& p = passes[i];
                if (rebuild) {
                    u64 Pw = 0;
                    if (int rc = count_windows(p, Pw)) return rc;
                    if (Pw != p.windows) return fail(c, LZANI_ERR_DEVICE, "lzani_prefilter: a pass's windows differ from the histogram's");
                    if (int rc = build_postings(p, kmers_in[i] ? nullptr : pf.kmers_of.get(), !sparse && r1 == n_rows && i + 1 == passes.size())) return rc;
                    kmers_in[i] = 1;
                    if (sparse) ++sp.pass_runs;
                }
                if (with_matrix) if (int rc = sparse ? count_sparse(r0, r1, p, clear, overflow) : count_tile(r0, r1, p, clear)) return rc;
                clear = false;
            }
            if (overflow) {
                if (!tl.halve())
                    return fail(c, LZANI_ERR_NOMEM, "lzani_prefilter: row " + std::to_string(r0) + " alone shares k-mers with more than " + std::to_string(slots / 2) +
                                                    " genomes, half of the pair table's " + std::to_string(slots) + " slots: count into the matrix (dense counting)");
                continue;
            }
            if (with_matrix) if (int rc = sparse ? compact_sparse(r0, r1) : compact_tile(r0, r1)) return rc;
            tl.finished();
        }
        if (sparse) sp.attempts = tl.attempts;
        if (st && sparse && rebuild) { HIPCHK(c, hipStreamSynchronize(c->stream)); st->stage.reset(); }
        return LZANI_OK;
    }

    int run()
    {
        info.k = k; pf.n = n;
        pf.cross = n_ref != 0; pf.cinfo.n_ref = n_ref; pf.cinfo.n_query = n_ref ? n_cols : 0;
        const std::optional<u64> forced_passes = env_u64("LZANI_PREFILTER_PASSES");
        if (forced_passes && (*forced_passes < 1 || *forced_passes > PF_BINS))
            return fail(c, LZANI_ERR_ARG, "lzani_prefilter: LZANI_PREFILTER_PASSES must be 1 .. " + std::to_string((int)PF_BINS));
        const u32 forced = forced_passes ? (u32)*forced_passes : 0u;
        if (const auto forced_slots = env_u64("LZANI_PREFILTER_TABLE_SLOTS"))
            if (!pf_slots_ok(*forced_slots)) return fail(c, LZANI_ERR_ARG, "lzani_prefilter: LZANI_PREFILTER_TABLE_SLOTS must be a power of two >= 2");

        // chunks of PF_CHUNK forward positions, genome after genome
        std::vector<u64> cbase((size_t)n + 1, 0);
        for (u32 g = 0; g < n; ++g) cbase[g + 1] = cbase[g] + pf_chunks(len_of(g));
        n_chunks = cbase[n];
        HIPCHK(c, w.cbase.alloc((size_t)n + 1));
        HIPCHK(c, w.blkcnt.alloc(n_chunks));
        HIPCHK(c, w.blkoff.alloc(n_chunks + 1));
        HIPCHK(c, pf.kmers_of.alloc(n));
        HIPCHK(c, hipMemcpyAsync(w.cbase, cbase.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(pf.kmers_of, 0, (size_t)n * 4, c->stream));
        pf.row_off.assign((size_t)n + 1, 0);

        // ---- the kept windows of the whole set counted (this sweep always runs); whether they go in one pass
        u64 Pv = 0;
        if (int rc = count_windows(PfPass{}, Pv)) return rc;
        pinfo.cap = PF_MAX_PASS_WINDOWS;
        if (const auto forced_cap = env_u64("LZANI_PREFILTER_MAX_WINDOWS")) pinfo.cap = *forced_cap;
        else {                                                     // a quarter of the free device memory for the 24 B per window (a choice, not a measurement)
            u64 free_b = 0;
            if (int rc = pf_free_bytes(c, free_b)) return rc;
            pinfo.cap = std::min<u64>(pinfo.cap, free_b / 4 / 24);
        }
        info.positions = Pv;
        // ---- the plan.  One pass is {0, PF_BINS} with the unranged kernels and no histogram.  No kept window: no pass runs,
        // and a forced plan is still what is reported
        std::vector<PfPass> passes;
        pf.bin_lo = {0, PF_BINS};
        if (!Pv) {
            if (forced) plan_passes_impl(nullptr, pinfo.cap, forced, pf.bin_lo);
        } else if (forced ? forced == 1 : Pv <= pinfo.cap) {
            if (Pv > PF_MAX_PASS_WINDOWS)
                return fail(c, LZANI_ERR_ARG, "lzani_prefilter: " + std::to_string(Pv) + " sampled k-mer windows in the one forced pass; a pass holds fewer than 2^32");
            passes.push_back(PfPass{false, 0, PF_BINS, Pv});
            pinfo.largest_pass = Pv;
        } else if (int rc = plan_from_histogram(forced, passes))
            return rc;
        if (Pv) if (int rc = tiles_and_passes(passes)) return rc;

        for (const PfPass& p : passes) { info.distinct_kmers += p.D; info.postings += p.M; }
        pinfo.passes = (u32)pf.bin_lo.size() - 1;
        for (size_t g = n_rows; g < n; ++g) pf.row_off[g + 1] = info.entries;      // (cross form: the query rows are empty)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        double ms[PF_STAGES] = {0, 0, 0, 0, 0, 0};
        HIPCHK(c, clk.collect(ms));
        info.keys_ms = ms[PF_ST_KEYS]; info.sort_ms = ms[PF_ST_SORT]; info.count_ms = ms[PF_ST_COUNT]; info.compact_ms = ms[PF_ST_COMPACT];
        pinfo.hist_ms = ms[PF_ST_HIST];
        if (st) st->info.upload_ms = ms[PF_ST_UPLOAD];
        TRACE("prefilter: k=%d positions=%llu distinct=%llu postings=%llu entries=%llu tiles=%u passes=%u sparse=%u attempts=%u slots=%llu", k, (unsigned long long)Pv,
              (unsigned long long)info.distinct_kmers, (unsigned long long)info.postings, (unsigned long long)info.entries, info.tiles, pinfo.passes, sp.sparse,
              sp.attempts, (unsigned long long)sp.slots);
        return LZANI_OK;
    }
};

// ---- what the four entry points share.  `fn` is the caller's name, so that every message reads as before.  The order of
// effects: the argument checks; then the device, and the previous result dropped (two need not fit) before the n_ref check
// and before anything is allocated; a failed run synchronises the stream and leaves the context usable, without a result.
int pf_check_args(lzani_ctx* c, const std::string& fn, int k, double min_ratio)
{
    if (k < 8 || k > 31) return fail(c, LZANI_ERR_ARG, fn + ": k must be 8 .. 31");
    if (!(min_ratio >= 0)) return fail(c, LZANI_ERR_ARG, fn + ": min_ratio must be a number >= 0");
    return LZANI_OK;
}
int pf_drop_last(lzani_ctx* c, const std::string& fn, u32 n, const uint32_t* n_ref)
{
    HIPCHK(c, hipSetDevice(c->dev));
    c->pf = Prefilter{};                                       // the last result goes first: two need not fit
    if (n_ref && (*n_ref == 0 || *n_ref >= n)) return fail(c, LZANI_ERR_ARG, fn + "_cross: n_ref must be 1 .. n - 1");
    return LZANI_OK;
}
int pf_run_and_publish(lzani_ctx* c, int k, u64 sample_max, u32 min_shared, double min_ratio, u32 n, PfStream* st, const uint32_t* n_ref, uint64_t* n_entries)
{
    Prefilter pf;
    const int rc = PfRun(c, pf, k, sample_max, min_shared, min_ratio, n, st, n_ref ? *n_ref : 0).run();
    if (rc != LZANI_OK) { (void)hipStreamSynchronize(c->stream); return rc; }     // (pf and st release what they held)
    pf.work = PrefilterWork{};
    pf.done = true;
    if (st) { pf.streamed = true; pf.sinfo = st->info; }
    c->pf = std::move(pf);
    if (n_entries) *n_entries = c->pf.info.entries;
    return LZANI_OK;
}

// lzani_prefilter (n_ref null) and lzani_prefilter_cross
int prefilter_resident(lzani_ctx* c, int k, uint64_t sample_max, uint32_t min_shared, double min_ratio, const uint32_t* n_ref, uint64_t* n_entries)
{
    if (!c) return LZANI_ERR_ARG;
    if (!c->gs.n) return fail(c, LZANI_ERR_STATE, "lzani_prefilter: no genomes (call lzani_set_genomes first)");
    if (c->gs.ooc) return fail(c, LZANI_ERR_STATE, "lzani_prefilter: the genome set is out-of-core; the prefilter needs it resident");
    if (int rc = pf_check_args(c, "lzani_prefilter", k, min_ratio)) return rc;
    if (int rc = pf_drop_last(c, "lzani_prefilter", c->gs.n, n_ref)) return rc;
    return pf_run_and_publish(c, k, sample_max, min_shared, min_ratio, c->gs.n, nullptr, n_ref, n_entries);
}

// lzani_prefilter_codes (n_ref null) and lzani_prefilter_codes_cross
int prefilter_streamed(lzani_ctx* c, uint32_t n, const uint8_t* const* codes, const uint32_t* len, int k, uint64_t sample_max,
                       uint32_t min_shared, double min_ratio, uint64_t slice_bytes, const uint32_t* n_ref, uint64_t* n_entries)
{
    if (!c) return LZANI_ERR_ARG;
    if (!n || !codes || !len) return fail(c, LZANI_ERR_ARG, "lzani_prefilter_codes: empty input");
    if (int rc = pf_check_args(c, "lzani_prefilter_codes", k, min_ratio)) return rc;
    u64 total = 0, Lmax = 0;
    for (u32 g = 0; g < n; ++g) {
        if (len[g] > 0x3FFFFFFFu - 3u * (u32)c->P.mrd)
            return fail(c, LZANI_ERR_ARG, "lzani_prefilter_codes: sequence too long for 32-bit text positions");
        if (len[g] && !codes[g]) return fail(c, LZANI_ERR_ARG, "lzani_prefilter_codes: null sequence");
        total += len[g];
        Lmax = std::max<u64>(Lmax, len[g]);
    }
    if (int rc = pf_drop_last(c, "lzani_prefilter_codes", n, n_ref)) return rc;
    if (const auto forced = env_u64("LZANI_PREFILTER_SLICE_BYTES")) slice_bytes = *forced;
    if (slice_bytes == 0) {                                    // automatic: an eighth of the free device memory (a choice, not a measurement)
        u64 free_b = 0;
        if (int rc = pf_free_bytes(c, free_b)) return rc;
        slice_bytes = std::max<u64>(1, std::min<u64>(total, std::max<u64>(Lmax, free_b / 8)));
    }
    PfStream st;
    st.codes = codes; st.len = len;
    std::string msg;
    const int S = plan_slices_impl(n, len, slice_bytes, st.first, msg);
    if (S < 0) return fail(c, S, "lzani_prefilter_codes: " + msg);
    std::vector<u64> off(n);
    st.bytes.assign((size_t)S, 0);
    for (int s = 0; s < S; ++s)
        for (u32 g = st.first[s]; g < st.first[s + 1]; ++g) { off[g] = st.bytes[s]; st.bytes[s] += len[g]; }
    const u64 cap = *std::max_element(st.bytes.begin(), st.bytes.end());
    st.info.slices = (uint32_t)S;
    st.info.stage_bytes = cap;
    HIPCHK(c, st.stage.alloc(cap));
    HIPCHK(c, st.d_off.alloc(n));
    HIPCHK(c, st.d_len.alloc(n));
    HIPCHK(c, hipMemcpyAsync(st.d_off, off.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(st.d_len, len, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    st.bounce.resize((size_t)std::max<u64>(1, std::min<u64>(cap, PF_BOUNCE_BYTES)));
    return pf_run_and_publish(c, k, sample_max, min_shared, min_ratio, n, &st, n_ref, n_entries);
}

}  // namespace

extern "C" {

int lzani_prefilter(lzani_ctx* c, int k, uint64_t sample_max, uint32_t min_shared, double min_ratio, uint64_t* n_entries)
{
    return prefilter_resident(c, k, sample_max, min_shared, min_ratio, nullptr, n_entries);
}

int lzani_prefilter_cross(lzani_ctx* c, int k, uint64_t sample_max, uint32_t min_shared, double min_ratio, uint32_t n_ref, uint64_t* n_entries)
{
    return prefilter_resident(c, k, sample_max, min_shared, min_ratio, &n_ref, n_entries);
}

int lzani_plan_slices(uint32_t n, const uint32_t* len, uint64_t slice_bytes, uint32_t* slice_of)
{
    std::vector<u32> first;
    std::string msg;
    const int ns = plan_slices_impl(n, len, slice_bytes, first, msg);
    if (ns > 0 && slice_of)
        for (int s = 0; s < ns; ++s) std::fill(slice_of + first[s], slice_of + first[s + 1], (uint32_t)s);
    return ns;
}

int lzani_prefilter_codes(lzani_ctx* c, uint32_t n, const uint8_t* const* codes, const uint32_t* len, int k, uint64_t sample_max,
                          uint32_t min_shared, double min_ratio, uint64_t slice_bytes, uint64_t* n_entries)
{
    return prefilter_streamed(c, n, codes, len, k, sample_max, min_shared, min_ratio, slice_bytes, nullptr, n_entries);
}

int lzani_prefilter_codes_cross(lzani_ctx* c, uint32_t n, const uint8_t* const* codes, const uint32_t* len, int k, uint64_t sample_max,
                                uint32_t min_shared, double min_ratio, uint64_t slice_bytes, uint32_t n_ref, uint64_t* n_entries)
{
    return prefilter_streamed(c, n, codes, len, k, sample_max, min_shared, min_ratio, slice_bytes, &n_ref, n_entries);
}

int lzani_get_prefilter_cross_info(const lzani_ctx* c, lzani_prefilter_cross_info* info)
{
    if (!c || !info) return LZANI_ERR_ARG;
    if (!c->pf.done || !c->pf.cross) return LZANI_ERR_STATE;
    *info = c->pf.cinfo;
    return LZANI_OK;
}

int lzani_get_prefilter_stream_info(const lzani_ctx* c, lzani_prefilter_stream_info* info)
{
    if (!c || !info) return LZANI_ERR_ARG;
    if (!c->pf.done || !c->pf.streamed) return LZANI_ERR_STATE;
    *info = c->pf.sinfo;
    return LZANI_OK;
}

int lzani_get_prefilter_pass_info(const lzani_ctx* c, lzani_prefilter_pass_info* info)
{
    if (!c || !info) return LZANI_ERR_ARG;
    if (!c->pf.done) return LZANI_ERR_STATE;
    *info = c->pf.pinfo;
    return LZANI_OK;
}

int lzani_prefilter_pass_plan(const lzani_ctx* c, uint32_t* bin_lo)
{
    if (!c) return LZANI_ERR_ARG;
    if (!c->pf.done) return LZANI_ERR_STATE;
    if (bin_lo) std::copy(c->pf.bin_lo.begin(), c->pf.bin_lo.end(), bin_lo);
    return (int)c->pf.bin_lo.size() - 1;
}

int lzani_set_prefilter_counting(lzani_ctx* c, int mode)
{
    if (!c) return LZANI_ERR_ARG;
    if (mode != LZANI_PF_COUNTING_AUTO && mode != LZANI_PF_COUNTING_DENSE && mode != LZANI_PF_COUNTING_SPARSE)
        return fail(c, LZANI_ERR_ARG, "lzani_set_prefilter_counting: the mode is LZANI_PF_COUNTING_AUTO, _DENSE or _SPARSE");
    c->pf_counting = mode;
    return LZANI_OK;
}

int lzani_get_prefilter_sparse_info(const lzani_ctx* c, lzani_prefilter_sparse_info* info)
{
    if (!c || !info) return LZANI_ERR_ARG;
    if (!c->pf.done) return LZANI_ERR_STATE;
    *info = c->pf.spinfo;
    return LZANI_OK;
}

int lzani_plan_sparse_tiles(uint32_t n_rows, const uint64_t* row_pairs, uint64_t slots, uint32_t* tile_r0, uint32_t* attempts)
{
    std::vector<u32> first;
    u32 att = 0;
    const int nt = plan_sparse_tiles_impl(n_rows, row_pairs, slots, first, att);
    if (nt > 0 && tile_r0) std::copy(first.begin(), first.end(), tile_r0);
    if (nt > 0 && attempts) *attempts = att;
    return nt;
}

int lzani_plan_passes(const uint64_t* hist, uint64_t cap, uint32_t forced, uint32_t* bin_lo)
{
    std::vector<u32> lo;
    const int np = plan_passes_impl(hist, cap, forced, lo);
    if (np > 0 && bin_lo) std::copy(lo.begin(), lo.end(), bin_lo);
    return np;
}

int lzani_prefilter_fetch(lzani_ctx* c, uint32_t* kmers_of, uint64_t* row_off, uint32_t* ids, uint32_t* shared)
{
    if (!c) return LZANI_ERR_ARG;
    if (!c->pf.done) return fail(c, LZANI_ERR_STATE, "lzani_prefilter_fetch: no prefilter result (call lzani_prefilter first)");
    HIPCHK(c, hipSetDevice(c->dev));
    const Prefilter& pf = c->pf;
    const u32 n = pf.n;
    // everything into buffers of our own first: the caller's are written only on success
    std::vector<u32> h_k(kmers_of ? n : 0), h_ids(ids ? pf.info.entries : 0), h_sh(shared ? pf.info.entries : 0);
    if (kmers_of) HIPCHK(c, hipMemcpy(h_k.data(), pf.kmers_of, (size_t)n * 4, hipMemcpyDeviceToHost));
    for (const PrefilterTile& t : pf.tiles) {
        const u64 at = pf.row_off[t.r0], cnt = pf.row_off[t.r1] - at;
        if (!cnt) continue;
        if (ids) HIPCHK(c, hipMemcpy(h_ids.data() + at, t.ids, (size_t)cnt * 4, hipMemcpyDeviceToHost));
        if (shared) HIPCHK(c, hipMemcpy(h_sh.data() + at, t.shared, (size_t)cnt * 4, hipMemcpyDeviceToHost));
    }
    if (kmers_of) memcpy(kmers_of, h_k.data(), h_k.size() * 4);
    if (row_off) memcpy(row_off, pf.row_off.data(), pf.row_off.size() * 8);
    if (ids && !h_ids.empty()) memcpy(ids, h_ids.data(), h_ids.size() * 4);
    if (shared && !h_sh.empty()) memcpy(shared, h_sh.data(), h_sh.size() * 4);
    return LZANI_OK;
}

int lzani_get_prefilter_info(const lzani_ctx* c, lzani_prefilter_info* info)
{
    if (!c || !info) return LZANI_ERR_ARG;
    if (!c->pf.done) return LZANI_ERR_STATE;
    *info = c->pf.info;
    return LZANI_OK;
}

}  // extern "C"
