// lzani_multi.h -- the multi-GPU layer of the C-ABI (include/lzani.h, "sharding over GPUs").  Included by
// lzani_hip.hip only, after the single-GPU entry points it builds on.
//
// What shards is the reference's own work unit, the reference ROW (one index build, many queries;
// /root/reference/src/lz_matcher.cpp:196-255): rows are independent, the packed genome set is replicated on
// every GPU (10k x 40 kbp = 0.3 GB of text + 6.4 GB of k-mer words against 288 GB of HBM), and the only
// exchange is ONE gather of the per-pair int32[3] records after the compute -- RCCL over xGMI.
//
//   lzani_partition_rows / lzani_row_costs   rows -> shards: cyclic for equal-cost (dense) rows, greedy
//                                            longest-processing-time for the ragged rows of a kmer-db filter
//   lzani_comm_*                             one process per GPU (torchrun, MPI...): ncclCommInitRank from a
//                                            unique id the caller distributes, ncclAllGather of padded shards
//                                            or grouped ncclSend/ncclRecv of ragged shards to a root
//   lzani_group_*                            one process, n GPUs (`lz-ani --gpus n`): a context per device, ncclCommInitAll;
//                                            lzani_group_run_rows in stages: check the rows -> deal them and make the ONE
//                                            shard plan (lzani_shard_plan.h: free of HIP, tested on the CPU through
//                                            lzani_plan_gather) -> ensure the buffers -> run the shards, a host thread per device
//                                            -> grouped ncclSend/ncclRecv to device 0 -> scatter kernel into CSR order, ONE copy out
//                                            lzani_group_run_rows_kept: the same stages up to the scatter kernel, then the output
//                                            filter's stage (lzani_kept.h) on the CSR-ordered buffer, on the first device's context
//                                            and stream; the copy out of the full results is left out
//                                            lzani_group_cluster_*: the cluster stage (lzani_cluster.h) on that context, its
//                                            record store and levels included
#pragma once
#include <rccl/rccl.h>

#include <numeric>
#include <thread>

#include "lzani_shard_plan.h"

struct lzani_group {
    std::vector<lzani_ctx*> ctx;
    std::vector<int> devs;
    std::vector<ncclComm_t> comms;      // one per device; empty when the group has one device or is a rehearsal
    bool rehearsal = false;             // the same device listed more than once: shards move by device copies
    std::string err;
    double gather_ms = 0;
    // buffers of lzani_group_run_rows, kept from call to call and grown when a call needs more (a tiled all2all makes ten
    // calls of the same size: no allocation after the first): the gathered / CSR-ordered results on the first device, a
    // shard buffer per peer, the scatter table, and two pinned staging buffers for the copy out
    DevMem<lzani_result> d_all, d_final;
    std::vector<DevMem<lzani_result>> d_shard;    // [0] stays empty (the first device writes into d_all); [d] lives on device d
    DevMem<unsigned long long> d_tab;
    PinMem<char> h_stage[2];
    DevEvent ev_stage[2], ev_gather[2];   // (ev_gather: made with the group; gather_ms is from before the gather to after the scatter kernel)
};
enum : size_t { GROUP_STAGE_BYTES = (size_t)32 << 20 };

namespace {

#define RCCLCHK(c, call)                                                                              \
    do {                                                                                              \
        ncclResult_t r_ = (call);                                                                     \
        if (r_ != ncclSuccess) return fail(c, LZANI_ERR_DEVICE, std::string(#call) + ": " + ncclGetErrorString(r_)); \
    } while (0)
#define GHIPCHK(g, call)                                                                              \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return gfail(g, e_ == hipErrorOutOfMemory ? LZANI_ERR_NOMEM : LZANI_ERR_DEVICE,           \
                         std::string("gather / copy out: ") + hipGetErrorString(e_));                 \
    } while (0)

// Rows of a gathered buffer (shard order) -> the caller's CSR order.  One block per row.
__global__ void k_scatter_rows(const int* __restrict__ src, int* __restrict__ dst, const u64* __restrict__ src_off,
                               const u64* __restrict__ dst_off, const u64* __restrict__ count)
{
    const u64 s = 3 * src_off[blockIdx.x], d = 3 * dst_off[blockIdx.x], n = 3 * count[blockIdx.x];
    for (u64 k = threadIdx.x; k < n; k += blockDim.x) dst[d + k] = src[s + k];
}

// ---- the stages of lzani_group_run_rows; each reports through gfail (GHIPCHK: HIPCHK for the group's gather and copy out)
int gfail(lzani_group* g, int code, const std::string& msg) { if (g) g->err = msg; return code; }
thread_local std::string t_group_create_err;      // why the last lzani_group_create of this thread failed (there is no group to hold it)

// f(d) -> an LZANI_* code, for every device at once (threads for devices 1 .. n - 1, device 0 on the caller's); the first error wins
template <class F> int on_every_device(lzani_group* g, F f)
{
    std::vector<int> rc(g->ctx.size(), LZANI_OK);
    std::vector<std::thread> th;
    auto one = [&](size_t d) { rc[d] = f(d); };
    for (size_t d = 1; d < g->ctx.size(); ++d) th.emplace_back(one, d);
    one(0);
    for (auto& t : th) t.join();
    for (size_t d = 0; d < g->ctx.size(); ++d)
        if (rc[d] != LZANI_OK) return gfail(g, rc[d], "device " + std::to_string(g->devs[d]) + ": " + lzani_last_error(g->ctx[d]));
    return LZANI_OK;
}

struct GroupRun {                       // one lzani_group_run_rows call on its way through the stages
    u32 n_rows; const u32* ref_ids; const u64* row_off; const u32* query_ids; lzani_result* out; u64 n_pairs = 0;   // (the caller's)
    bool kept = false;                  // lzani_group_run_rows_kept: no host output, the results end on the first device
    ShardPlan plan;                     // what every device gets, and the scatter table
    std::vector<int*> d_shard;          // where every device writes its shard ([0]: in place in d_all)
};

int group_check_rows(lzani_group* g, GroupRun& r)
{
    if (!r.ref_ids || !r.row_off) return gfail(g, LZANI_ERR_ARG, "lzani_group_run_rows: null argument");
    r.n_pairs = r.n_rows ? r.row_off[r.n_rows] : 0;
    if (r.n_pairs && !r.out && !r.kept) return gfail(g, LZANI_ERR_ARG, "lzani_group_run_rows: null output");
    g->gather_ms = 0;
    const u32 n = g->ctx[0]->gs.n;
    if (!n) return gfail(g, LZANI_ERR_STATE, "lzani_group_run_rows: no genomes set");
    for (u32 k = 0; k < r.n_rows; ++k)
        if (r.ref_ids[k] >= n || r.row_off[k + 1] < r.row_off[k]) return gfail(g, LZANI_ERR_ARG, "lzani_group_run_rows: bad row table");
    if (r.query_ids)
        for (u64 e = 0; e < r.n_pairs; ++e) if (r.query_ids[e] >= n) return gfail(g, LZANI_ERR_ARG, "lzani_group_run_rows: query id out of range");
    return LZANI_OK;
}

// rows -> devices: cyclic for dense rows, LPT on the row costs for query lists; then the one shard plan
int group_partition_rows(lzani_group* g, GroupRun& r)
{
    const GenomeSet& gs = g->ctx[0]->gs;
    const u32 nd = (u32)g->ctx.size();
    std::vector<u32> part(r.n_rows);
    std::vector<u64> cost(r.query_ids ? r.n_rows : 0);
    if (r.query_ids) {
        std::vector<u32> len(gs.L.begin(), gs.L.end());
        int rc = lzani_row_costs(r.n_rows, r.ref_ids, r.row_off, r.query_ids, gs.n, len.data(), cost.data());
        if (rc != LZANI_OK) return gfail(g, rc, "lzani_group_run_rows: row costs");
    }
    lzani_partition_rows(r.n_rows, r.query_ids ? cost.data() : nullptr, nd, part.data());
    if (!plan_shards(r.n_rows, r.ref_ids, r.row_off, r.query_ids, part.data(), nd, r.plan)) return gfail(g, LZANI_ERR_ARG, "lzani_group_run_rows: gather plan");
    return LZANI_OK;
}

// device 0 holds the gathered buffer (its own shard is written in place) and the CSR-ordered copy: grown, never shrunk
int group_ensure_buffers(lzani_group* g, GroupRun& r)
{
    const hipError_t e = hipSetDevice(g->ctx[0]->dev);
    if (e != hipSuccess) return gfail(g, LZANI_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    if (g->d_final.capacity() < std::max<u64>(r.n_pairs, 1)) {
        g->d_all.reset(); g->d_final.reset();                    // (both released before either is made anew; a failure leaves none)
        if (!got(g->d_all.alloc(r.n_pairs)) || !got(g->d_final.alloc(r.n_pairs))) {
            g->d_all.reset();
            return gfail(g, LZANI_ERR_NOMEM, "lzani_group_run_rows: result buffers on device 0");
        }
    }
    g->d_shard.resize(g->ctx.size());                            // (a peer's shard buffer is made on its own thread, below)
    r.d_shard.assign(g->ctx.size(), nullptr); r.d_shard[0] = (int*)g->d_all.get();
    return LZANI_OK;
}

int group_run_shards(lzani_group* g, GroupRun& r)
{
    return on_every_device(g, [&](size_t d) -> int {
        lzani_ctx* c = g->ctx[d];
        const Shard& s = r.plan.shard[d];
        if (s.rows.empty()) { c->run.tm = lzani_timing{}; return LZANI_OK; }   // no row for this device
        if (d && g->d_shard[d].capacity() < std::max<u64>(s.pairs(), 1)) {
            if (hipSetDevice(c->dev) != hipSuccess) return LZANI_ERR_DEVICE;
            if (!got(g->d_shard[d].alloc(s.pairs()))) return fail(c, LZANI_ERR_NOMEM, "lzani_group_run_rows: the device's shard buffer");
        }
        if (d) r.d_shard[d] = (int*)g->d_shard[d].get();
        static const u32 none = 0;                             // (lists that are all empty are still lists, not dense rows: never null)
        const u32* q = !r.query_ids ? nullptr : s.q.empty() ? &none : s.q.data();
        return lzani_run_rows_device(c, (u32)s.ref.size(), s.ref.data(), s.off.data(), q, r.d_shard[d]);
    });
}

// the gather: every peer's shard to device 0 (grouped ncclSend / ncclRecv over xGMI)
int group_gather(lzani_group* g, const GroupRun& r)
{
    lzani_ctx* c0 = g->ctx[0];
    const u32 nd = (u32)g->ctx.size();
    const std::vector<Shard>& sh = r.plan.shard;
    GHIPCHK(g, hipSetDevice(c0->dev));
    GHIPCHK(g, hipEventRecord(g->ev_gather[0], c0->stream));
    if (!g->comms.empty()) {
        ncclResult_t rn = ncclGroupStart();
        for (u32 d = 1; d < nd && rn == ncclSuccess; ++d) {
            const size_t cnt = (size_t)sh[d].pairs() * 3;
            if (!cnt) continue;
            hipSetDevice(g->ctx[d]->dev);
            rn = ncclSend(r.d_shard[d], cnt, ncclInt32, 0, g->comms[d], g->ctx[d]->stream);
            hipSetDevice(c0->dev);
            if (rn == ncclSuccess) rn = ncclRecv(r.d_shard[0] + 3 * sh[d].base, cnt, ncclInt32, (int)d, g->comms[0], c0->stream);
        }
        ncclResult_t r2 = ncclGroupEnd();
        if (rn == ncclSuccess) rn = r2;
        if (rn != ncclSuccess) return gfail(g, LZANI_ERR_DEVICE, std::string("RCCL gather: ") + ncclGetErrorString(rn));
    } else {
        for (u32 d = 1; d < nd; ++d)                         // rehearsal on one device: plain device copies
            if (sh[d].pairs() && hipMemcpyAsync(r.d_shard[0] + 3 * sh[d].base, r.d_shard[d], sh[d].pairs() * 12, hipMemcpyDeviceToDevice, c0->stream) != hipSuccess)
                return gfail(g, LZANI_ERR_DEVICE, "device copy of a shard failed");
    }
    return LZANI_OK;
}

// shard order -> the caller's CSR order on device 0 (d_final), on the first context's stream
int group_scatter(lzani_group* g, const GroupRun& r)
{
    if (!r.n_rows) return LZANI_OK;
    lzani_ctx* c0 = g->ctx[0];
    const std::vector<u64>& tab = r.plan.tab;
    int* const d_final = (int*)g->d_final.get();
    GHIPCHK(g, g->d_tab.reserve(tab.size()));
    unsigned long long* const d_tab = g->d_tab;
    GHIPCHK(g, hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, c0->stream));
    hipLaunchKernelGGL(k_scatter_rows, dim3(r.n_rows), dim3(256), 0, c0->stream, r.d_shard[0], d_final, (const u64*)d_tab, (const u64*)d_tab + r.n_rows, (const u64*)d_tab + 2 * (size_t)r.n_rows);
    GHIPCHK(g, hipGetLastError());
    GHIPCHK(g, hipEventRecord(g->ev_gather[1], c0->stream));
    return LZANI_OK;
}

// the end of a group run: every device's stream drained, the gather's time read
int group_finish(lzani_group* g, const GroupRun& r)
{
    if (!r.n_rows) return LZANI_OK;
    lzani_ctx* c0 = g->ctx[0];
    GHIPCHK(g, hipStreamSynchronize(c0->stream));
    hipError_t e = hipSuccess;
    for (size_t d = 1; d < g->ctx.size() && e == hipSuccess; ++d) { hipSetDevice(g->ctx[d]->dev); e = hipStreamSynchronize(g->ctx[d]->stream); }
    hipSetDevice(c0->dev);                             // (the calling thread leaves with device 0 current, as it came)
    GHIPCHK(g, e);
    float ms = 0;
    if (hipEventElapsedTime(&ms, g->ev_gather[0], g->ev_gather[1]) == hipSuccess) g->gather_ms = ms;
    return LZANI_OK;
}

// the one device-to-host copy of the CSR-ordered results
int group_copy_out(lzani_group* g, const GroupRun& r)
{
    if (!r.n_rows) return LZANI_OK;
    lzani_ctx* c0 = g->ctx[0];
    const int* const d_final = (const int*)g->d_final.get();
    // the copy out: through two pinned staging buffers that take turns -- the device-to-host copy of one piece flies
    // while the host moves the piece before it into the caller's (pageable) buffer
    for (int k = 0; k < 2; ++k) {
        if (!g->h_stage[k]) GHIPCHK(g, g->h_stage[k].alloc(GROUP_STAGE_BYTES));
        if (!g->ev_stage[k]) GHIPCHK(g, g->ev_stage[k].create(hipEventDisableTiming));
    }
    const size_t total = (size_t)r.n_pairs * 12;
    size_t issued = 0, moved = 0, len[2] = {0, 0};
    for (int k = 0; issued < total || moved < total; k ^= 1) {
        if (len[k]) {                                  // the piece this buffer holds: wait for it, hand it over
            GHIPCHK(g, hipEventSynchronize(g->ev_stage[k]));
            memcpy((char*)r.out + moved, g->h_stage[k], len[k]);
            moved += len[k];
            len[k] = 0;
        }
        if (issued < total) {
            len[k] = std::min<size_t>(GROUP_STAGE_BYTES, total - issued);
            GHIPCHK(g, hipMemcpyAsync(g->h_stage[k], (const char*)d_final + issued, len[k], hipMemcpyDeviceToHost, c0->stream));
            GHIPCHK(g, hipEventRecord(g->ev_stage[k], c0->stream));
            issued += len[k];
        }
    }
    return LZANI_OK;
}

}  // namespace

static void comm_release(lzani_ctx* c)
{
    if (c->comm) { ncclCommDestroy((ncclComm_t)c->comm); c->comm = nullptr; }
}

extern "C" {

// ---- rows -> shards ---------------------------------------------------------------------------------
int lzani_row_costs(uint32_t n_rows, const uint32_t* ref_ids, const uint64_t* row_off, const uint32_t* query_ids,
                    uint32_t n, const uint32_t* len, uint64_t* cost)
{
    if (!ref_ids || !row_off || !len || !cost) return LZANI_ERR_ARG;
    u64 total = 0;
    if (!query_ids) for (u32 g = 0; g < n; ++g) total += len[g];
    for (u32 k = 0; k < n_rows; ++k) {
        if (ref_ids[k] >= n) return LZANI_ERR_ARG;
        u64 c = (u64)LZANI_ROW_COST_REF_WEIGHT * len[ref_ids[k]];
        if (!query_ids) c += total - len[ref_ids[k]];
        else
            for (u64 e = row_off[k]; e < row_off[k + 1]; ++e) {
                if (query_ids[e] >= n) return LZANI_ERR_ARG;
                c += len[query_ids[e]];
            }
        cost[k] = c;
    }
    return LZANI_OK;
}

int lzani_partition_rows(uint32_t n_rows, const uint64_t* row_cost, uint32_t n_parts, uint32_t* part_of_row)
{
    if (!n_parts || (n_rows && !part_of_row)) return LZANI_ERR_ARG;
    if (!row_cost) {                                          // equal rows: cyclic in the given (length-descending) order
        for (u32 k = 0; k < n_rows; ++k) part_of_row[k] = k % n_parts;
        return LZANI_OK;
    }
    // greedy LPT: heaviest row first onto the least loaded shard (ties: earlier row, lower shard) -- the 4/3 rule
    std::vector<u32> order(n_rows);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](u32 a, u32 b) { return row_cost[a] > row_cost[b]; });
    typedef std::pair<u64, u32> Load;                          // (load, shard): a min-heap
    std::vector<Load> heap;
    for (u32 p = 0; p < n_parts; ++p) heap.emplace_back(0, p);
    auto cmp = [](const Load& a, const Load& b) { return a > b; };
    std::make_heap(heap.begin(), heap.end(), cmp);
    for (u32 k : order) {
        std::pop_heap(heap.begin(), heap.end(), cmp);
        Load& l = heap.back();
        part_of_row[k] = l.second;
        l.first += row_cost[k];
        std::push_heap(heap.begin(), heap.end(), cmp);
    }
    return LZANI_OK;
}

// ---- one process per GPU ------------------------------------------------------------------------------
int lzani_comm_unique_id(uint8_t* id)
{
    if (!id) return LZANI_ERR_ARG;
    static_assert(sizeof(ncclUniqueId) == LZANI_UNIQUE_ID_BYTES, "unique id size");
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) return LZANI_ERR_DEVICE;
    memcpy(id, &u, sizeof u);
    return LZANI_OK;
}

int lzani_comm_init(lzani_ctx* c, uint32_t n_ranks, uint32_t rank, const uint8_t* id)
{
    if (!c) return LZANI_ERR_ARG;
    if (!id || !n_ranks || rank >= n_ranks) return fail(c, LZANI_ERR_ARG, "lzani_comm_init: bad rank / id");
    if (c->comm) return fail(c, LZANI_ERR_STATE, "lzani_comm_init: communicator exists already");
    HIPCHK(c, hipSetDevice(c->dev));
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    ncclComm_t comm = nullptr;
    RCCLCHK(c, ncclCommInitRank(&comm, (int)n_ranks, u, (int)rank));
    c->comm = comm; c->n_ranks = n_ranks; c->rank = rank;
    return LZANI_OK;
}

int lzani_comm_allgather(lzani_ctx* c, const void* d_send, void* d_recv, uint64_t n_results)
{
    if (!c) return LZANI_ERR_ARG;
    if (!c->comm) return fail(c, LZANI_ERR_STATE, "lzani_comm_allgather: no communicator (lzani_comm_init)");
    if (n_results && (!d_send || !d_recv)) return fail(c, LZANI_ERR_ARG, "lzani_comm_allgather: null buffer");
    HIPCHK(c, hipSetDevice(c->dev));
    RCCLCHK(c, ncclAllGather(d_send, d_recv, (size_t)n_results * 3, ncclInt32, (ncclComm_t)c->comm, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LZANI_OK;
}

int lzani_comm_gatherv(lzani_ctx* c, const void* d_send, void* d_recv, const uint64_t* counts, uint32_t root)
{
    if (!c) return LZANI_ERR_ARG;
    if (!c->comm) return fail(c, LZANI_ERR_STATE, "lzani_comm_gatherv: no communicator (lzani_comm_init)");
    if (!counts || root >= c->n_ranks) return fail(c, LZANI_ERR_ARG, "lzani_comm_gatherv: bad argument");
    HIPCHK(c, hipSetDevice(c->dev));
    ncclComm_t comm = (ncclComm_t)c->comm;
    if (c->rank == root) {
        if (!d_recv) return fail(c, LZANI_ERR_ARG, "lzani_comm_gatherv: null receive buffer on the root");
        u64 off = 0;
        for (u32 p = 0; p < root; ++p) off += counts[p];
        if (counts[root] && (int*)d_recv + 3 * off != d_send)          // the root's own shard
            HIPCHK(c, hipMemcpyAsync((int*)d_recv + 3 * off, d_send, counts[root] * 12, hipMemcpyDeviceToDevice, c->stream));
        ncclResult_t r = ncclGroupStart();
        off = 0;
        for (u32 p = 0; p < c->n_ranks && r == ncclSuccess; ++p) {
            if (p != root && counts[p]) r = ncclRecv((int*)d_recv + 3 * off, (size_t)counts[p] * 3, ncclInt32, (int)p, comm, c->stream);
            off += counts[p];
        }
        const ncclResult_t r2 = ncclGroupEnd();
        RCCLCHK(c, r);
        RCCLCHK(c, r2);
    } else if (counts[c->rank])
        RCCLCHK(c, ncclSend(d_send, (size_t)counts[c->rank] * 3, ncclInt32, (int)root, comm, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LZANI_OK;
}

// ---- one process, n GPUs ------------------------------------------------------------------------------
// The shard plan of lzani_group_run_rows (lzani_shard_plan.h states the rule) in flat arrays: testable without a GPU.
int lzani_plan_gather(uint32_t n_rows, const uint64_t* row_off, const uint32_t* part_of_row, uint32_t n_parts,
                      uint64_t* shard_base, uint64_t* src, uint64_t* dst, uint64_t* cnt, uint32_t* row_of_entry)
{
    if (!n_parts || (n_rows && (!row_off || !part_of_row)) || !shard_base || (n_rows && (!src || !dst || !cnt))) return LZANI_ERR_ARG;
    ShardPlan p;
    if (!plan_shards(n_rows, nullptr, row_off, nullptr, part_of_row, n_parts, p)) return LZANI_ERR_ARG;
    shard_base[0] = 0;
    for (u32 d = 0; d < n_parts; ++d) shard_base[d + 1] = p.shard[d].base + p.shard[d].pairs();
    if (row_of_entry) for (const Shard& sh : p.shard) row_of_entry = std::copy(sh.rows.begin(), sh.rows.end(), row_of_entry);
    const u64* t = p.tab.data();
    std::copy(t, t + n_rows, src); std::copy(t + n_rows, t + 2 * (size_t)n_rows, dst); std::copy(t + 2 * (size_t)n_rows, t + 3 * (size_t)n_rows, cnt);
    return LZANI_OK;
}

void lzani_group_destroy(lzani_group* g)
{
    if (!g) return;
    for (size_t d = 1; d < g->d_shard.size(); ++d)                  // a shard buffer is released with its device current
        if (g->d_shard[d]) { hipSetDevice(g->ctx[d]->dev); g->d_shard[d].reset(); }
    if (!g->ctx.empty()) hipSetDevice(g->ctx[0]->dev);
    g->d_all.reset(); g->d_final.reset(); g->d_tab.reset();         // (on the first device; the pinned buffers go with the group)
    for (auto& e : g->ev_stage) e.reset();
    for (auto& e : g->ev_gather) e.reset();
    for (auto cm : g->comms) if (cm) ncclCommDestroy(cm);
    for (auto c : g->ctx) lzani_destroy(c);
    delete g;
}

// (a null group: the reason the last lzani_group_create of the calling thread failed, if it did)
const char* lzani_group_last_error(const lzani_group* g)
{
    return g ? g->err.c_str() : (t_group_create_err.empty() ? "null group" : t_group_create_err.c_str());
}

int lzani_group_create(const lzani_params* p, uint32_t n_devices, const int* device_ids, lzani_group** out)
{
    t_group_create_err.clear();
    if (!p || !out || !n_devices || !device_ids) { t_group_create_err = "lzani_group_create: null argument"; return LZANI_ERR_ARG; }
    *out = nullptr;
    lzani_group* g = new (std::nothrow) lzani_group();
    if (!g) return LZANI_ERR_NOMEM;
    g->devs.assign(device_ids, device_ids + n_devices);
    for (u32 d = 0; d < n_devices; ++d) {
        lzani_ctx* c = nullptr;
        int rc = lzani_create(p, device_ids[d], &c);
        if (rc != LZANI_OK) {
            t_group_create_err = "lzani_create on device " + std::to_string(device_ids[d]) + " failed with code " + std::to_string(rc) +
                                 (rc == LZANI_ERR_PARAMS ? " (LZ parameters outside the supported envelope)" : rc == LZANI_ERR_DEVICE ? " (no such HIP device, or its stream could not be made)" :
                                  rc == LZANI_ERR_NOMEM ? " (out of memory)" : "");
            lzani_group_destroy(g);
            return rc;
        }
        g->ctx.push_back(c);
    }
    hipSetDevice(g->ctx[0]->dev);                               // (gather_ms is timed between two events of the first device)
    for (auto& e : g->ev_gather) if (e.create() != hipSuccess) { t_group_create_err = "hipEventCreate failed"; lzani_group_destroy(g); return LZANI_ERR_DEVICE; }
    std::vector<int> sorted(g->devs);
    std::sort(sorted.begin(), sorted.end());
    g->rehearsal = std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end();
    if (n_devices > 1 && !g->rehearsal) {
        g->comms.assign(n_devices, nullptr);
        ncclResult_t r = ncclCommInitAll(g->comms.data(), (int)n_devices, g->devs.data());
        if (r != ncclSuccess) {
            t_group_create_err = std::string("ncclCommInitAll: ") + ncclGetErrorString(r);
            g->comms.clear();
            lzani_group_destroy(g);
            return LZANI_ERR_DEVICE;
        }
    }
    *out = g;
    return LZANI_OK;
}

int lzani_group_set_genomes(lzani_group* g, uint32_t n, const uint8_t* const* codes, const uint32_t* len)
{
    if (!g) return LZANI_ERR_ARG;
    return on_every_device(g, [&](size_t d) { return lzani_set_genomes(g->ctx[d], n, codes, len); });
}

int lzani_group_run_rows(lzani_group* g, uint32_t n_rows, const uint32_t* ref_ids, const uint64_t* row_off,
                         const uint32_t* query_ids, lzani_result* out)
{
    if (!g) return LZANI_ERR_ARG;
    GroupRun r{n_rows, ref_ids, row_off, query_ids, out};
    int rc = group_check_rows(g, r);
    if (rc == LZANI_OK) rc = group_partition_rows(g, r);
    if (rc == LZANI_OK) rc = group_ensure_buffers(g, r);
    if (rc == LZANI_OK) rc = group_run_shards(g, r);
    if (rc == LZANI_OK) rc = group_gather(g, r);
    if (rc == LZANI_OK) rc = group_scatter(g, r);
    if (rc == LZANI_OK) rc = group_copy_out(g, r);
    if (rc == LZANI_OK) rc = group_finish(g, r);
    return rc;
}

int lzani_group_run_rows_kept(lzani_group* g, uint32_t n_rows, const uint32_t* ref_ids, const uint64_t* row_off,
                              const uint32_t* query_ids, const lzani_out_filter* f, const uint32_t* report_len, uint64_t* n_kept)
{
    if (!g) return LZANI_ERR_ARG;
    lzani_ctx* c0 = g->ctx[0];
    const std::string fn = "lzani_group_run_rows_kept";
    auto of_c0 = [&](int rc) { return rc == LZANI_OK ? rc : gfail(g, rc, lzani_last_error(c0)); };
    GroupRun r{n_rows, ref_ids, row_off, query_ids, nullptr};
    r.kept = true;
    int rc = group_check_rows(g, r);
    if (rc != LZANI_OK) return rc;
    if (int e = of_c0(kept_check_filter(c0, fn, f))) return e;
    std::vector<u32> row_of, own;
    KeptRows kr;
    if (int e = of_c0(kept_check_rows(c0, fn, c0->gs.n, n_rows, ref_ids, row_off, query_ids, row_of, kr))) return e;
    if (!report_len) { own = kept_own_lengths(c0); report_len = own.data(); }
    GHIPCHK(g, hipSetDevice(c0->dev));
    c0->kept = Kept{};                                          // the last result goes first: two need not fit
    rc = group_partition_rows(g, r);
    if (rc == LZANI_OK) rc = group_ensure_buffers(g, r);
    if (rc == LZANI_OK) rc = group_run_shards(g, r);
    if (rc == LZANI_OK) rc = group_gather(g, r);
    if (rc == LZANI_OK) rc = group_scatter(g, r);
    if (rc == LZANI_OK) rc = group_finish(g, r);
    if (rc != LZANI_OK) return rc;
    return of_c0(kept_stage(c0, c0->gs.n, report_len, n_rows, ref_ids, row_off, query_ids, row_of, kr, (const int*)g->d_final.get(), *f, n_kept));
}

int lzani_group_kept_fetch(lzani_group* g, uint64_t first, uint64_t count, lzani_kept_pair* out)
{
    if (!g) return LZANI_ERR_ARG;
    const int rc = lzani_kept_fetch(g->ctx[0], first, count, out);
    return rc == LZANI_OK ? rc : gfail(g, rc, lzani_last_error(g->ctx[0]));
}

int lzani_group_get_kept_info(const lzani_group* g, lzani_kept_info* info)
{
    if (!g) return LZANI_ERR_ARG;
    return lzani_get_kept_info(g->ctx[0], info);
}

// The cluster stage for the group (lzani_cluster.h): on the first device's context, where the group's kept results are.
int lzani_group_cluster_begin(lzani_group* g, uint32_t n, const uint32_t* report_len, int measure)
{
    if (!g) return LZANI_ERR_ARG;
    const int rc = lzani_cluster_begin(g->ctx[0], n, report_len, measure);
    return rc == LZANI_OK ? rc : gfail(g, rc, lzani_last_error(g->ctx[0]));
}

int lzani_group_cluster_add_kept(lzani_group* g, uint64_t* edges_total)
{
    if (!g) return LZANI_ERR_ARG;
    const int rc = lzani_cluster_add_kept(g->ctx[0], edges_total);
    return rc == LZANI_OK ? rc : gfail(g, rc, lzani_last_error(g->ctx[0]));
}

int lzani_group_cluster_run(lzani_group* g, int algo, uint64_t* n_clusters)
{
    if (!g) return LZANI_ERR_ARG;
    const int rc = lzani_cluster_run(g->ctx[0], algo, n_clusters);
    return rc == LZANI_OK ? rc : gfail(g, rc, lzani_last_error(g->ctx[0]));
}

int lzani_group_cluster_fetch(lzani_group* g, uint32_t* rep_of, uint32_t* cluster_of)
{
    if (!g) return LZANI_ERR_ARG;
    const int rc = lzani_cluster_fetch(g->ctx[0], rep_of, cluster_of);
    return rc == LZANI_OK ? rc : gfail(g, rc, lzani_last_error(g->ctx[0]));
}

int lzani_group_get_cluster_info(const lzani_group* g, lzani_cluster_info* info)
{
    if (!g) return LZANI_ERR_ARG;
    return lzani_get_cluster_info(g->ctx[0], info);
}

int lzani_group_get_cluster_cover_info(const lzani_group* g, lzani_cluster_cover_info* info)
{
    if (!g) return LZANI_ERR_ARG;
    return lzani_get_cluster_cover_info(g->ctx[0], info);
}

int lzani_group_get_cluster_link_info(const lzani_group* g, lzani_cluster_link_info* info)
{
    if (!g) return LZANI_ERR_ARG;
    return lzani_get_cluster_link_info(g->ctx[0], info);
}

int lzani_group_set_cluster_leiden(lzani_group* g, double resolution, int iterations)
{
    if (!g) return LZANI_ERR_ARG;
    const int rc = lzani_set_cluster_leiden(g->ctx[0], resolution, iterations);
    return rc == LZANI_OK ? rc : gfail(g, rc, lzani_last_error(g->ctx[0]));
}

int lzani_group_get_cluster_leiden_info(const lzani_group* g, lzani_cluster_leiden_info* info)
{
    if (!g) return LZANI_ERR_ARG;
    return lzani_get_cluster_leiden_info(g->ctx[0], info);
}

// The cluster levels for the group: the record store and the levels on the first device's context.
int lzani_group_cluster_store_begin(lzani_group* g, uint32_t n, const uint32_t* report_len)
{
    if (!g) return LZANI_ERR_ARG;
    const int rc = lzani_cluster_store_begin(g->ctx[0], n, report_len);
    return rc == LZANI_OK ? rc : gfail(g, rc, lzani_last_error(g->ctx[0]));
}

int lzani_group_cluster_store_add_kept(lzani_group* g, uint64_t* records_total)
{
    if (!g) return LZANI_ERR_ARG;
    const int rc = lzani_cluster_store_add_kept(g->ctx[0], records_total);
    return rc == LZANI_OK ? rc : gfail(g, rc, lzani_last_error(g->ctx[0]));
}

int lzani_group_cluster_level(lzani_group* g, int measure, const lzani_cluster_cut* cut, uint64_t* edges)
{
    if (!g) return LZANI_ERR_ARG;
    const int rc = lzani_cluster_level(g->ctx[0], measure, cut, edges);
    return rc == LZANI_OK ? rc : gfail(g, rc, lzani_last_error(g->ctx[0]));
}

int lzani_group_get_cluster_store_info(const lzani_group* g, lzani_cluster_store_info* info)
{
    if (!g) return LZANI_ERR_ARG;
    return lzani_get_cluster_store_info(g->ctx[0], info);
}

int lzani_group_get_cluster_level_info(const lzani_group* g, lzani_cluster_level_info* info)
{
    if (!g) return LZANI_ERR_ARG;
    return lzani_get_cluster_level_info(g->ctx[0], info);
}

int lzani_group_set_genome_memory(lzani_group* g, uint64_t bytes)
{
    if (!g) return LZANI_ERR_ARG;
    for (auto c : g->ctx) lzani_set_genome_memory(c, bytes);
    return LZANI_OK;
}

int lzani_group_get_residency(const lzani_group* g, uint32_t device_index, lzani_residency_info* info)
{
    if (!g || device_index >= g->ctx.size() || !info) return LZANI_ERR_ARG;
    return lzani_get_residency(g->ctx[device_index], info);
}

int lzani_group_get_timing(const lzani_group* g, uint32_t device_index, lzani_timing* t, double* gather_ms)
{
    if (!g || device_index >= g->ctx.size() || !t) return LZANI_ERR_ARG;
    *t = g->ctx[device_index]->run.tm;
    if (gather_ms) *gather_ms = g->gather_ms;
    return LZANI_OK;
}

}  // extern "C"
