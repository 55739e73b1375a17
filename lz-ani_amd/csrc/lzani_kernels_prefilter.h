// lzani_kernels_prefilter.h -- device kernels of the k-mer prefilter (lzani_prefilter): the shared canonical k-mer count
// of every genome pair of the resident set, i.e. what the reference's CFilter::load_filter reads from a kmer-db file.
// Included by lzani_hip.hip only (after lzani_tables.h).  Exact integer work:
//   k_pf_keys     one thread per forward position: canonical, sampled k-mer (pf_canon / pf_keep over kmer_at of both
//                 strands) -- counted per block, then written compacted in position order; a third pass writes
//                 rank << 32 | genome  with the k-mer's rank found in the sorted dictionary.  RANGED: only the windows of
//                 one k-mer pass, pf_bin(k-mer) in [bin_lo, bin_hi).  A fourth mode adds every kept window into the
//                 histogram of the PF_BINS bins (per block in LDS, then one atomic add per non-empty bin)
//   k_pf_keys_codes  the same keys from raw symbol codes in a staging buffer (lzani_prefilter_codes: genomes that are not
//                 resident), staged and packed in LDS; the other strand arithmetically from the forward value
//   pf_compact    count, then write, of a block's PF_CHUNK elements (the block sum and the block rank of lzani_block.h):
//                 the one skeleton of k_pf_uniq and k_pf_sparse_kept, which say what is kept and where it is put
//   k_pf_uniq     a sorted array without its adjacent duplicates: the dictionary of distinct k-mers from the sorted keys,
//                 the postings from the sorted (rank, genome) keys
//   k_pf_scan     exclusive prefix of per-block / per-row counts (one block; the arrays are 1/4096 of the data)
//   k_pf_runs     where the postings of every rank begin
//   k_pf_split    cross form: where the postings of every rank pass from the references (genome < n_ref) to the queries
//   pf_walk       the posting walker, a wave per 64 postings: for every posting (rank, a) of the row tile, one add per later
//                 posting (rank, b) of the same run, the lanes side by side over b.  CROSS: a is a reference, the b's are
//                 the run's queries only, and the tile is n_ref rows of n - n_ref columns.  Its two accumulators:
//   k_pf_count        PfMatrixAcc: an add is one atomic add to count[a][b] of the matrix tile
//   k_pf_count_sparse PfTableAcc (sparse counting): an add inserts the pair's key into the pair table by linear probing
//                 and adds to its slot; bounded, with an overflow word for a table too small, polled before every a
//   k_pf_rows     a wave per matrix row: the kept entries counted, then written in ascending b
//   k_pf_sparse_kept / _fetch / _rowoff  the table's kept keys, and behind their sort the ids and counts of the sorted keys
//                 and where every row of the tile begins
//   k_pfl_*       the limit stage over a finished result (lzani_prefilter_limit.h): an entry's row, the score keys, the
//                 directed keys and degrees, the survivor marks, the genomes cut, and the surviving entries of every row
// No kernel waits for another block.  The sorts between them are lzani_sort_keys (lzani_sort.hip).
#pragma once
#include "lzani_block.h"
#include "lzani_prefilter_defs.h"

namespace lzani {

enum { PF_THREADS = 256, PF_PER_THREAD = 16, PF_CHUNK = PF_THREADS * PF_PER_THREAD };
enum { PF_COUNT = 0, PF_CANON = 1, PF_RANK = 2, PF_HIST = 3 };

// The canonical k-mer of the window at forward position p of genome g, if the window exists, holds no N and is sampled.
__device__ __forceinline__ bool pf_key_at(const GenomeTab& G, u32 g, int L, int p, int k, int mrd, u64 sample_max, u64& key)
{
    if (p > L - k) return false;
    const u64 o = G.nmoff[g];
    const TextView R = ref_view(G.t2 + 2 * o, G.nm + o, L, mrd, false);
    u64 f, r;
    if (!kmer_at(R, p, k, f) || !kmer_at(R, R.rc0 + L - p - k, k, r)) return false;
    key = pf_canon(f, r);
    return pf_keep(key, sample_max);
}

// index of key in the ascending dictionary (it is there)
__device__ __forceinline__ u32 pf_find(const unsigned long long* __restrict__ dict, u64 D, u64 key)
{
    u64 lo = 0, hi = D;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (dict[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (u32)lo;
}

// Whether a kept k-mer belongs to the pass of bins [lo, hi).  Not RANGED: every one does, and nothing is computed.
template <bool RANGED>
__device__ __forceinline__ bool pf_in_pass(u64 key, u32 lo, u32 hi)
{
    if (!RANGED) return true;
    const u32 b = pf_bin(key);
    return b >= lo && b < hi;
}

// PF_HIST: the block's histogram in LDS cleared / added into hist[PF_BINS], the empty bins left out.
__device__ __forceinline__ void pf_hist_clear(u32* s_hist)
{
    for (int i = threadIdx.x; i < PF_BINS; i += PF_THREADS) s_hist[i] = 0;
    __syncthreads();
}
__device__ __forceinline__ void pf_hist_flush(const u32* s_hist, unsigned long long* __restrict__ hist)
{
    __syncthreads();
    for (int i = threadIdx.x; i < PF_BINS; i += PF_THREADS) {
        const u32 c = s_hist[i];
        if (c) atomicAdd(&hist[i], (unsigned long long)c);
    }
}

// The tail the two key kernels share.  pf_emit: one window of every thread of the block (ok: it is kept and of the pass,
// key: its canonical k-mer) -- COUNT: counted in `mine`; HIST: added to the block's histogram; CANON / RANK: written at
// out[base + its rank among the block's kept windows of this step], and base moves past them.  Every thread of the block
// calls it (block_rank holds barriers).
template <int MODE>
__device__ __forceinline__ void pf_emit(bool ok, u64 key, u32 g, const unsigned long long* __restrict__ dict, u64 D, unsigned long long* __restrict__ out,
                                        u64& base, u32& mine, u32* s_w, u32* s_hist)
{
    if (MODE == PF_COUNT) mine += ok;
    else if (MODE == PF_HIST) { if (ok) atomicAdd(&s_hist[pf_bin(key)], 1u); }
    else {
        u32 tot;
        const u32 r = block_rank<PF_THREADS>(ok, s_w, tot);
        if (ok) out[base + r] = MODE == PF_CANON ? key : ((u64)pf_find(dict, D, key) << 32) | (u64)g;
        base += tot;
    }
}
// pf_keys_end: the block's epilogue -- COUNT: the threads' counts reduced into blkcnt[blk] (*s_cnt was cleared before a
// barrier); HIST: the block's histogram flushed into out.
template <int MODE>
__device__ __forceinline__ void pf_keys_end(u32 mine, u32* __restrict__ blkcnt, u64 blk, u32* s_cnt, const u32* s_hist, unsigned long long* __restrict__ out)
{
    if (MODE == PF_COUNT) {
        block_sum(mine, s_cnt);
        if (threadIdx.x == 0) blkcnt[blk] = *s_cnt;
    }
    if (MODE == PF_HIST) pf_hist_flush(s_hist, out);
}

// Block (x, y) = chunk x of PF_CHUNK forward positions of genome g0 + y; its number in the count / offset arrays is
// cbase[g] + x.  COUNT: blkcnt[block] = kept windows.  CANON / RANK: they are written from blkoff[block] on, in position
// order -- the canonical k-mer, or  rank in dict << 32 | genome.  RANGED: of the kept windows only those of the pass
// [bin_lo, bin_hi).  HIST (never RANGED): out is the histogram u64[PF_BINS]; blkcnt / blkoff are not touched.
template <int MODE, bool RANGED>
__global__ void __launch_bounds__(PF_THREADS) k_pf_keys(GenomeTab G, const u64* __restrict__ cbase, u32 g0, int k, int mrd, u64 sample_max,
                                                        u32 bin_lo, u32 bin_hi, u32* __restrict__ blkcnt, const u64* __restrict__ blkoff,
                                                        const unsigned long long* __restrict__ dict, u64 D, unsigned long long* __restrict__ out)
{
    __shared__ u32 s_w[PF_THREADS / 64];
    __shared__ u32 s_cnt;
    __shared__ u32 s_hist[MODE == PF_HIST ? PF_BINS : 1];
    const u32 g = g0 + blockIdx.y;
    const int L = G.L[g];
    const u64 chunk0 = (u64)blockIdx.x * PF_CHUNK;
    if (chunk0 >= (u64)L) return;
    const u64 blk = cbase[g] + blockIdx.x;
    u64 base = MODE == PF_COUNT || MODE == PF_HIST ? 0 : blkoff[blk];
    u32 mine = 0;
    if (MODE == PF_COUNT) { if (threadIdx.x == 0) s_cnt = 0; __syncthreads(); }
    if (MODE == PF_HIST) pf_hist_clear(s_hist);
    for (int it = 0; it < PF_PER_THREAD; ++it) {
        if (chunk0 + (u64)it * PF_THREADS >= (u64)L) break;              // (the same for the whole block)
        const u64 p = chunk0 + (u64)it * PF_THREADS + threadIdx.x;
        u64 key = 0;
        const bool ok = p < (u64)L && pf_key_at(G, g, L, (int)p, k, mrd, sample_max, key) && pf_in_pass<RANGED>(key, bin_lo, bin_hi);
        pf_emit<MODE>(ok, key, g, dict, D, out, base, mine, s_w, s_hist);
    }
    pf_keys_end<MODE>(mine, blkcnt, blk, &s_cnt, s_hist, out);
}

// k_pf_keys for genomes that are not resident (lzani_prefilter_codes): their raw symbol codes, 1 B each, lie one after the
// other in a staging buffer, at any byte offset.  Block (x, y) = chunk x of genome y0 + y OF THE SLICE (soff / slen: its
// byte offset in the buffer and its length); its global id, for cbase and the PF_RANK keys, is gfirst + y0 + y.  The
// block brings the codes of its chunk and of the k - 1 symbols behind it -- cut at the genome's end, so that no window
// sees the next genome's codes -- into LDS with aligned 16-byte loads, packs them there (pf_pack16), and every thread
// forms its windows from LDS (pf_window; the other strand by pf_rc_of).  Same counts, same keys in the same order as
// k_pf_keys.  slice_bytes: the bytes of the buffer that hold the slice; none beyond is read.
enum { PF_GROUPS = PF_CHUNK / 16 + 4 };           // groups of 16 symbols: PF_CHUNK + 30 symbols, and the two groups pf_window reads on
template <int MODE, bool RANGED>
__global__ void __launch_bounds__(PF_THREADS) k_pf_keys_codes(const unsigned char* __restrict__ stage, u64 slice_bytes, const u64* __restrict__ soff,
                                                              const u32* __restrict__ slen, const u64* __restrict__ cbase, u32 gfirst, u32 y0, int k,
                                                              u64 sample_max, u32 bin_lo, u32 bin_hi, u32* __restrict__ blkcnt, const u64* __restrict__ blkoff,
                                                              const unsigned long long* __restrict__ dict, u64 D, unsigned long long* __restrict__ out)
{
    __shared__ uint4 s_raw[PF_GROUPS];            // the codes as they lie in the buffer, from the 16-byte boundary before the chunk
    __shared__ u32 s_t2[PF_GROUPS];
    __shared__ unsigned short s_nm[PF_GROUPS];
    __shared__ u32 s_w[PF_THREADS / 64];
    __shared__ u32 s_cnt;
    __shared__ u32 s_hist[MODE == PF_HIST ? PF_BINS : 1];
    const u32 y = y0 + blockIdx.y;
    const u32 g = gfirst + y;
    const int L = (int)slen[y];
    const u64 chunk0 = (u64)blockIdx.x * PF_CHUNK;
    if (chunk0 >= (u64)L) return;
    const int cnt = (int)(((u64)L - chunk0) < (u64)(PF_CHUNK + k - 1) ? ((u64)L - chunk0) : (u64)(PF_CHUNK + k - 1));      // symbols staged
    const u64 b0 = soff[y] + chunk0;
    const u64 a0 = b0 & ~15ULL;
    const int shift = (int)(b0 & 15ULL);
    const int n16 = (shift + cnt + 15) >> 4;      // <= (15 + PF_CHUNK + 30 + 15) / 16 < PF_GROUPS
    for (int i = threadIdx.x; i < n16; i += PF_THREADS) {
        const u64 a = a0 + 16ULL * (u64)i;
        uint4 v;
        if (a + 16 <= slice_bytes) v = *reinterpret_cast<const uint4*>(stage + a);
        else {                                    // the slice's last bytes
            u32 wd[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 16; ++j) if (a + j < slice_bytes) wd[j >> 2] |= (u32)stage[a + j] << (8 * (j & 3));
            v = make_uint4(wd[0], wd[1], wd[2], wd[3]);
        }
        s_raw[i] = v;
    }
    __syncthreads();
    const unsigned char* raw = reinterpret_cast<const unsigned char*>(s_raw) + shift;
    for (int j = threadIdx.x; j < PF_GROUPS; j += PF_THREADS) {
        const int left = cnt - 16 * j;
        u32 sym, nb;
        pf_pack16(raw + 16 * j, left < 0 ? 0 : (left > 16 ? 16 : left), sym, nb);
        s_t2[j] = sym;
        s_nm[j] = (unsigned short)nb;
    }
    if (MODE == PF_COUNT && threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    if (MODE == PF_HIST) pf_hist_clear(s_hist);
    const u64 blk = cbase[g] + blockIdx.x;
    u64 base = MODE == PF_COUNT || MODE == PF_HIST ? 0 : blkoff[blk];
    u32 mine = 0;
    for (int it = 0; it < PF_PER_THREAD; ++it) {
        if (chunk0 + (u64)it * PF_THREADS >= (u64)L) break;              // (the same for the whole block)
        const int q = it * PF_THREADS + (int)threadIdx.x;
        u64 f = 0, key = 0;
        bool ok = chunk0 + (u64)q + (u64)k <= (u64)L && pf_window(s_t2, s_nm, q, k, f);
        if (ok) { key = pf_canon(f, pf_rc_of(f, k)); ok = pf_keep(key, sample_max) && pf_in_pass<RANGED>(key, bin_lo, bin_hi); }
        pf_emit<MODE>(ok, key, g, dict, D, out, base, mine, s_w, s_hist);
    }
    pf_keys_end<MODE>(mine, blkcnt, blk, &s_cnt, s_hist, out);
}

// Count, then write: block b takes the PF_CHUNK elements from b * PF_CHUNK on of n, and of those that item.kept(i, v)
// keeps (v: what it read of element i) it counts them (blkcnt[b]), or (WRITE) hands each to item.put(at, v), at = blkoff[b]
// + its rank among the block's kept elements, in the order of i.  The whole block calls it, once.
template <bool WRITE, class Item>
__device__ __forceinline__ void pf_compact(u64 n, u32* __restrict__ blkcnt, const u64* __restrict__ blkoff, Item item)
{
    __shared__ u32 s_w[PF_THREADS / 64];
    __shared__ u32 s_cnt;
    const u64 i0 = (u64)blockIdx.x * PF_CHUNK;
    u64 base = WRITE ? blkoff[blockIdx.x] : 0;
    u32 mine = 0;
    if (!WRITE) { if (threadIdx.x == 0) s_cnt = 0; __syncthreads(); }
    for (int it = 0; it < PF_PER_THREAD; ++it) {
        if (i0 + (u64)it * PF_THREADS >= n) break;                       // (the same for the whole block)
        const u64 i = i0 + (u64)it * PF_THREADS + threadIdx.x;
        u64 v = 0;
        const bool ok = i < n && item.kept(i, v);
        if (!WRITE) mine += ok;
        else {
            u32 tot;
            const u32 r = block_rank<PF_THREADS>(ok, s_w, tot);
            if (ok) item.put(base + r, v);
            base += tot;
        }
    }
    if (!WRITE) {
        block_sum(mine, &s_cnt);
        if (threadIdx.x == 0) blkcnt[blockIdx.x] = s_cnt;
    }
}

// in[0 .. n) ascending: the elements that differ from their predecessor, counted or written by pf_compact.  per_genome
// (WRITE, may be null): += 1 at the low 32 bits of every element written.
struct PfUniqItem {
    const unsigned long long* __restrict__ in;
    unsigned long long* __restrict__ out;
    u32* __restrict__ per_genome;
    u32 n_genomes;
    __device__ __forceinline__ bool kept(u64 i, u64& v) const { v = in[i]; return i == 0 || in[i - 1] != v; }
    __device__ __forceinline__ void put(u64 at, u64 v) const
    {
        out[at] = v;
        if (per_genome && (u32)v < n_genomes) atomicAdd(&per_genome[(u32)v], 1u);
    }
};
template <bool WRITE>
__global__ void __launch_bounds__(PF_THREADS) k_pf_uniq(const unsigned long long* __restrict__ in, u64 n, u32* __restrict__ blkcnt,
                                                        const u64* __restrict__ blkoff, unsigned long long* __restrict__ out,
                                                        u32* __restrict__ per_genome, u32 n_genomes)
{
    pf_compact<WRITE>(n, blkcnt, blkoff, PfUniqItem{in, out, per_genome, n_genomes});
}

// off[0 .. n] = exclusive prefix of cnt[0 .. n), the total at off[n].  One block.
__global__ void __launch_bounds__(1024) k_pf_scan(const u32* __restrict__ cnt, u64 n, u64* __restrict__ off)
{
    __shared__ u64 s_wsum[16];
    __shared__ u64 s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (u64 base = 0; base < n; base += 1024) {
        const u64 idx = base + threadIdx.x;
        const u64 before = block_scan_step<u64>(idx < n ? cnt[idx] : 0, s_wsum, &s_carry);
        if (idx < n) off[idx] = before;
    }
    if (threadIdx.x == 0) off[n] = s_carry;
}

// post[0 .. M) = rank << 32 | genome, ascending, every rank below D present: runoff[r] = first posting of rank r, runoff[D] = M.
__global__ void __launch_bounds__(PF_THREADS) k_pf_runs(const unsigned long long* __restrict__ post, u64 M, u32* __restrict__ runoff, u64 D)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i == 0) runoff[D] = (u32)M;
    if (i >= M) return;
    const u64 r = post[i] >> 32;
    if (r < D && (i == 0 || (post[i - 1] >> 32) != r)) runoff[r] = (u32)i;
}

// Cross form (lzani_prefilter_cross): a run lists its genomes ascending, the references (genome < n_ref) before the
// queries.  runsplit[r] = the first posting of run r whose genome is >= n_ref, runoff[r + 1] where it has none;
// runsplit[D] = M.  One thread per posting, and exactly one posting of a run writes the run's entry: its first one if
// that is a query, a query behind a reference, or its last one (index + 1) if that is a reference.
__global__ void __launch_bounds__(PF_THREADS) k_pf_split(const unsigned long long* __restrict__ post, u64 M, u64 D, u32 n_ref, u32* __restrict__ runsplit)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i == 0) runsplit[D] = (u32)M;
    if (i >= M) return;
    const u64 key = post[i];
    const u64 r = key >> 32;
    if (r >= D) return;
    if ((u32)key >= n_ref) {
        if (i == 0 || (post[i - 1] >> 32) != r || (u32)post[i - 1] < n_ref) runsplit[r] = (u32)i;
    } else if (i + 1 == M || (post[i + 1] >> 32) != r) runsplit[r] = (u32)(i + 1);
}

// The posting walker: for every pair of postings (rank, a), (rank, b) with r0 <= a < r1 and a < b, one acc.add(b).
// A wave takes 64 consecutive postings as its a's, one after the other, the lanes over the rest of a's run: a k-mer that
// every genome holds is spread over n / 64 waves, and a wave's adds of one step belong to one row a.
// CROSS: the rows are references, r1 <= n_ref, the columns the n - n_ref queries: a posting is active iff it is a
// reference of the tile and its run holds a query, the lanes go over the run's queries, [runsplit[rank], end), and the
// column handed to add is b - n_ref.
// The accumulator says what an add does.  Before each a, acc.go(): false ends the walk for the whole wave (every lane
// gets the same answer).  acc.row(a): the adds that follow belong to row a.  acc.add(c): column c of that row += 1;
// false ends this lane's part of the run and nothing else.
template <bool CROSS, class Acc>
__device__ __forceinline__ void pf_walk(const unsigned long long* __restrict__ post, u64 M, const u32* __restrict__ runoff, u64 D, u32 n, u32 r0, u32 r1,
                                        const u32* __restrict__ runsplit, u32 n_ref, Acc acc)
{
    const int lane = threadIdx.x & 63;
    const u64 w0 = (((u64)blockIdx.x * PF_THREADS + threadIdx.x) >> 6) << 6;      // the wave's first posting
    const u64 i = w0 + lane;
    u32 a = 0, end = 0, from = 0;
    bool act = false;
    if (i < M) {
        const u64 key = post[i];
        const u64 rank = key >> 32;
        a = (u32)key;
        if (rank < D && a >= r0 && a < r1) {
            const u64 e = runoff[rank + 1];
            end = (u32)(e < M ? e : M);
            if (CROSS) {
                from = runsplit[rank];                         // (a < r1 <= n_ref: the split lies behind i)
                act = from < end;
            } else
                act = (u64)end > i + 1;
        }
    }
    const u32 c0 = CROSS ? n_ref : 0u, nc = n - c0;            // the first column's genome; columns
    u64 todo = __builtin_amdgcn_ballot_w64(act);
    while (todo) {
        if (!acc.go()) return;
        const int l = ctz64(todo);
        todo &= todo - 1;
        const u32 el = __shfl(end, l);
        acc.row(__shfl(a, l));
        for (u64 j = (CROSS ? (u64)__shfl(from, l) : w0 + l + 1) + lane; j < (u64)el; j += 64) {
            const u32 c = (u32)post[j] - c0;                   // (CROSS, a genome below n_ref: wraps beyond nc)
            if (c < nc && !acc.add(c)) break;
        }
    }
}

// The matrix tile as the walker's accumulator: mat[(a - r0) * cols + c] += 1, cols = n (CROSS: n - n_ref) columns a row.
struct PfMatrixAcc {
    u32* __restrict__ mat;
    u32 r0, cols;
    u32* row_;
    __device__ __forceinline__ bool go() const { return true; }
    __device__ __forceinline__ void row(u32 a) { row_ = mat + (u64)(a - r0) * cols; }
    __device__ __forceinline__ bool add(u32 c) const { atomicAdd(&row_[c], 1u); return true; }
};
template <bool CROSS>
__global__ void __launch_bounds__(PF_THREADS) k_pf_count(const unsigned long long* __restrict__ post, u64 M, const u32* __restrict__ runoff, u64 D,
                                                         u32 n, u32 r0, u32 r1, u32* __restrict__ mat, const u32* __restrict__ runsplit, u32 n_ref)
{
    pf_walk<CROSS>(post, M, runoff, D, n, r0, r1, runsplit, n_ref, PfMatrixAcc{mat, r0, CROSS ? n - n_ref : n, nullptr});
}

// kept: shared >= min_shared (>= 1) and shared / min(|a|, |b|) >= min_ratio, in IEEE double division
__device__ __forceinline__ bool pf_kept(u32 s, u32 ka, u32 kb, u32 min_shared, double min_ratio)
{
    if (s < min_shared) return false;
    return (double)s / (double)(ka < kb ? ka : kb) >= min_ratio;
}

// A wave per row a of the tile: the kept entries b > a counted (rowcnt[a - r0]) or written from rowoff[a - r0] on
// (tile-relative), in ascending b.  CROSS: the row holds the n - n_ref queries, column c is b = n_ref + c.
template <bool WRITE, bool CROSS>
__global__ void __launch_bounds__(PF_THREADS) k_pf_rows(const u32* __restrict__ mat, u32 n, u32 r0, u32 r1, const u32* __restrict__ kmers_of,
                                                        u32 min_shared, double min_ratio, u32* __restrict__ rowcnt, const u64* __restrict__ rowoff,
                                                        u32* __restrict__ ids, u32* __restrict__ shared, u32 n_ref)
{
    const int lane = threadIdx.x & 63;
    const u64 wave = ((u64)blockIdx.x * PF_THREADS + threadIdx.x) >> 6;
    if (wave >= (u64)(r1 - r0)) return;
    const u32 a = r0 + (u32)wave;
    const u32 c0 = CROSS ? n_ref : 0u;                          // the row's first column is genome c0
    const u32* __restrict__ m = mat + wave * (n - c0);
    const u32 ka = kmers_of[a];
    u64 base = WRITE ? rowoff[wave] : 0;
    u32 cnt = 0;
    for (u64 b0 = CROSS ? (u64)n_ref : (u64)a + 1; b0 < n; b0 += 64) {
        const u64 b = b0 + lane;
        u32 s = 0;
        bool ok = false;
        if (b < n) { s = m[b - c0]; ok = pf_kept(s, ka, kmers_of[b], min_shared, min_ratio); }
        const u64 mask = __builtin_amdgcn_ballot_w64(ok);
        if (WRITE && ok) {
            const u64 at = base + (u64)__popcll(mask & ((1ULL << lane) - 1ULL));
            ids[at] = (u32)b;
            shared[at] = s;
        }
        base += (u64)__popcll(mask);
        cnt += (u32)__popcll(mask);
    }
    if (!WRITE && lane == 0) rowcnt[wave] = cnt;
}

// ---- Sparse counting: the pair table in place of the matrix tile.  S slots (a power of two) of keys[S] (u64) and cnt[S]
// (u32); the key of a pair is  a << 32 | b  with global genome ids (a < b; CROSS: a < n_ref <= b), PF_SP_EMPTY (all ones,
// no pair's key) marks a free slot; a key's home is pf_splitmix64(key) & (S - 1), collisions go on to the next slot and
// wrap at S.  A slot's key changes once, from empty to its final value.  ctl[PF_SP_USED] = slots claimed,
// ctl[PF_SP_OVERFLOW] != 0: the tile's pairs are more than S / 2 and the attempt is void.

constexpr u64 PF_SP_EMPTY = ~0ULL;
enum { PF_SP_USED = 0, PF_SP_OVERFLOW = 1 };

__device__ __forceinline__ void pf_sp_give_up(u32* __restrict__ ctl) { __hip_atomic_store(&ctl[PF_SP_OVERFLOW], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// += 1 at the slot of `key`, which is claimed where the key is new.  At most S probe steps; none waits for another lane.
// The pre-read goes past the L1 (a relaxed agent-scope load): what it may still return is an empty that has been taken
// since, never a wrong key, and then the compare-and-swap's old value decides.  The claim that finds S / 2 slots in use
// already, and a probe sequence that runs out, raise the overflow word: false, and the lane adds no more.
__device__ __forceinline__ bool pf_sp_add(unsigned long long* __restrict__ keys, u32* __restrict__ cnt, u64 S, u32* __restrict__ ctl, u64 key)
{
    const u64 mask = S - 1;
    u64 slot = pf_splitmix64(key) & mask;
    for (u64 step = 0; step < S; ++step, slot = (slot + 1) & mask) {
        u64 cur = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == PF_SP_EMPTY) {
            cur = atomicCAS(&keys[slot], (unsigned long long)PF_SP_EMPTY, (unsigned long long)key);
            if (cur == PF_SP_EMPTY) {                          // the slot is this lane's
                if ((u64)atomicAdd(&ctl[PF_SP_USED], 1u) >= S / 2) { pf_sp_give_up(ctl); return false; }
                cur = key;
            }
        }
        if (cur == key) { atomicAdd(&cnt[slot], 1u); return true; }
    }
    pf_sp_give_up(ctl);
    return false;
}

// The pair table as the walker's accumulator: an add inserts the pair's key  a << 32 | c0 + c  (c0: the genome of column
// 0) and its slot's count goes up by one.  A wave reads the overflow word before every a and leaves where it is raised,
// whatever lane saw it; a lane whose add fails ends its run.
struct PfTableAcc {
    unsigned long long* __restrict__ keys;
    u32* __restrict__ cnt;
    u64 S;
    u32* __restrict__ ctl;
    u32 c0;
    u64 hi_;
    __device__ __forceinline__ bool go() const
    {
        const u32 ovf = __hip_atomic_load(&ctl[PF_SP_OVERFLOW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return !__builtin_amdgcn_ballot_w64(ovf != 0);
    }
    __device__ __forceinline__ void row(u32 a) { hi_ = (u64)a << 32; }
    __device__ __forceinline__ bool add(u32 c) const { return pf_sp_add(keys, cnt, S, ctl, hi_ | (u32)(c0 + c)); }
};
template <bool CROSS>
__global__ void __launch_bounds__(PF_THREADS) k_pf_count_sparse(const unsigned long long* __restrict__ post, u64 M, const u32* __restrict__ runoff, u64 D,
                                                                u32 n, u32 r0, u32 r1, unsigned long long* __restrict__ keys, u32* __restrict__ cnt, u64 S,
                                                                u32* __restrict__ ctl, const u32* __restrict__ runsplit, u32 n_ref)
{
    pf_walk<CROSS>(post, M, runoff, D, n, r0, r1, runsplit, n_ref, PfTableAcc{keys, cnt, S, ctl, CROSS ? n_ref : 0u, 0});
}

// The kept slots of the table, counted or written by pf_compact: the keys of the occupied slots whose count passes
// pf_kept.  The order is the table's, the sort behind it makes it the result's.
struct PfTableItem {
    const unsigned long long* __restrict__ keys;
    const u32* __restrict__ cnt;
    const u32* __restrict__ kmers_of;
    u32 min_shared;
    double min_ratio;
    unsigned long long* __restrict__ out;
    __device__ __forceinline__ bool kept(u64 i, u64& key) const
    {
        key = keys[i];
        return key != PF_SP_EMPTY && pf_kept(cnt[i], kmers_of[(u32)(key >> 32)], kmers_of[(u32)key], min_shared, min_ratio);
    }
    __device__ __forceinline__ void put(u64 at, u64 key) const { out[at] = key; }
};
template <bool WRITE>
__global__ void __launch_bounds__(PF_THREADS) k_pf_sparse_kept(const unsigned long long* __restrict__ keys, const u32* __restrict__ cnt, u64 S,
                                                               const u32* __restrict__ kmers_of, u32 min_shared, double min_ratio,
                                                               u32* __restrict__ blkcnt, const u64* __restrict__ blkoff, unsigned long long* __restrict__ out)
{
    pf_compact<WRITE>(S, blkcnt, blkoff, PfTableItem{keys, cnt, kmers_of, min_shared, min_ratio, out});
}

// sorted[0 .. K): the kept keys ascending, i.e. row after row with ascending b.  ids[i] = b, shared[i] = the count of the
// key's slot, found by the probe sequence of the insert (the key is in the table; S steps at most).
__global__ void __launch_bounds__(PF_THREADS) k_pf_sparse_fetch(const unsigned long long* __restrict__ sorted, u64 K, const unsigned long long* __restrict__ keys,
                                                                const u32* __restrict__ cnt, u64 S, u32* __restrict__ ids, u32* __restrict__ shared)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= K) return;
    const u64 key = sorted[i], mask = S - 1;
    u64 slot = pf_splitmix64(key) & mask;
    u32 s = 0;
    for (u64 step = 0; step < S; ++step, slot = (slot + 1) & mask) {
        const u64 cur = keys[slot];
        if (cur == key) { s = cnt[slot]; break; }
        if (cur == PF_SP_EMPTY) break;
    }
    ids[i] = (u32)key;
    shared[i] = s;
}

// A thread per row of the tile and one more: rowoff[r] = how many sorted keys lie below (r0 + r) << 32, r = 0 .. nr.
__global__ void __launch_bounds__(PF_THREADS) k_pf_sparse_rowoff(const unsigned long long* __restrict__ sorted, u64 K, u32 r0, u32 nr, u64* __restrict__ rowoff)
{
    const u64 r = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (r > (u64)nr) return;
    const u64 key = ((u64)r0 + r) << 32;
    u64 lo = 0, hi = K;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (sorted[mid] < key) lo = mid + 1; else hi = mid;
    }
    rowoff[r] = lo;
}

// ---- The limit stage (lzani_prefilter_limit.h): every limiting genome keeps its N best pairs.  E entries in CSR order
// (rowoff[n + 1], ids, shared), e < 2^31; no kernel waits for another block, and the only atomics are integer adds whose
// order cannot show.

// A wave per row a: row_of[e] = a for the row's entries, so that the passes over the entries find an entry's row at its
// own index.
__global__ void __launch_bounds__(PF_THREADS) k_pfl_rowof(const u64* __restrict__ rowoff, u32 n, u32* __restrict__ row_of)
{
    const int lane = threadIdx.x & 63;
    const u64 a = ((u64)blockIdx.x * PF_THREADS + threadIdx.x) >> 6;
    if (a >= (u64)n) return;
    const u64 e1 = rowoff[a + 1];
    for (u64 e = rowoff[a] + lane; e < e1; e += 64) row_of[e] = (u32)a;
}

// A thread per entry e, in CSR order: key[e] = ~q << 32 | e with q = pf_limit_score of the entry's pair -- ascending keys
// are descending scores.
__global__ void __launch_bounds__(PF_THREADS) k_pfl_keys(const u32* __restrict__ row_of, const u32* __restrict__ ids, const u32* __restrict__ shared, u64 E,
                                                         const u32* __restrict__ kmers_of, unsigned long long* __restrict__ key)
{
    const u64 e = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (e >= E) return;
    const u32 q = pf_limit_score(shared[e], kmers_of[row_of[e]], kmers_of[ids[e]]);
    key[e] = ((u64)(~q) << 32) | e;
}

// A thread per position i of the keys sorted by score: the directed keys  g << 32 | i  of the entry's limiting endpoints
// -- both (at 2 i and 2 i + 1), or (CROSS) the query alone (at i) -- and deg[g] += 1 for each.
template <bool CROSS>
__global__ void __launch_bounds__(PF_THREADS) k_pfl_directed(const unsigned long long* __restrict__ sorted, u64 E, const u32* __restrict__ row_of,
                                                             const u32* __restrict__ ids, unsigned long long* __restrict__ dkey, u32* __restrict__ deg)
{
    const u64 i = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= E) return;
    const u32 e = (u32)sorted[i];
    const u32 b = ids[e];
    if (CROSS) dkey[i] = ((u64)b << 32) | i;
    else {
        const u32 a = row_of[e];
        reinterpret_cast<ulonglong2*>(dkey)[i] = make_ulonglong2(((u64)a << 32) | i, ((u64)b << 32) | i);
        atomicAdd(&deg[a], 1u);
    }
    atomicAdd(&deg[b], 1u);
}

// A thread per directed key, sorted by genome (a genome's keys then ascend in i: its list in order).  start[g]: where the
// keys of g begin.  The first N of a genome mark their entry: survive[e] = 1, a plain store of the same value by whoever
// gets there.
__global__ void __launch_bounds__(PF_THREADS) k_pfl_mark(const unsigned long long* __restrict__ dsorted, u64 Dk, const u64* __restrict__ start, u32 max_per_genome,
                                                         const unsigned long long* __restrict__ sorted, unsigned char* __restrict__ survive)
{
    const u64 p = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    if (p >= Dk) return;
    const u64 key = dsorted[p];
    if (p - start[(u32)(key >> 32)] < (u64)max_per_genome) survive[(u32)sorted[(u32)key]] = 1;
}

// A thread per genome: *cut += the genomes whose list is longer than N (one atomic add per block that has one).
__global__ void __launch_bounds__(PF_THREADS) k_pfl_cut(const u32* __restrict__ deg, u32 n, u32 max_per_genome, u32* __restrict__ cut)
{
    __shared__ u32 s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const u64 g = (u64)blockIdx.x * PF_THREADS + threadIdx.x;
    block_sum(g < (u64)n && deg[g] > max_per_genome ? 1u : 0u, &s_cnt);
    if (threadIdx.x == 0 && s_cnt) atomicAdd(cut, s_cnt);
}

// k_pf_rows over the entries instead of the matrix: a wave per row a, its surviving entries counted (rowcnt[a]) or written
// from out_off[a] on, in the row's order.
template <bool WRITE>
__global__ void __launch_bounds__(PF_THREADS) k_pfl_rows(const u64* __restrict__ rowoff, u32 n, const unsigned char* __restrict__ survive,
                                                         const u32* __restrict__ ids, const u32* __restrict__ shared, u32* __restrict__ rowcnt,
                                                         const u64* __restrict__ out_off, u32* __restrict__ out_ids, u32* __restrict__ out_shared)
{
    const int lane = threadIdx.x & 63;
    const u64 a = ((u64)blockIdx.x * PF_THREADS + threadIdx.x) >> 6;
    if (a >= (u64)n) return;
    const u64 e1 = rowoff[a + 1];
    u64 base = WRITE ? out_off[a] : 0;
    u32 cnt = 0;
    for (u64 e0 = rowoff[a]; e0 < e1; e0 += 64) {
        const u64 e = e0 + lane;
        const bool ok = e < e1 && survive[e] != 0;
        const u64 mask = __builtin_amdgcn_ballot_w64(ok);
        if (WRITE && ok) {
            const u64 at = base + (u64)__popcll(mask & ((1ULL << lane) - 1ULL));
            out_ids[at] = ids[e];
            out_shared[at] = shared[e];
        }
        base += (u64)__popcll(mask);
        cnt += (u32)__popcll(mask);
    }
    if (!WRITE && lane == 0) rowcnt[a] = cnt;
}

}  // namespace lzani
