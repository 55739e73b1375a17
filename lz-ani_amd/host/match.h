// match.h -- the stages of the `lz-ani` host binary that call the engine: the device k-mer filter, the matching drivers
// (whole, --out-alignment, tiled), the -V 2 reporters, the alignment file and the cluster file.  Uses cli.h (P), engine.h
// (the binding and the owners), emit.h (the table, the records, the writer) and ingest.h (genomes, filter rows).
//
// Stage sequence: CLZMatcher::run_all2all (/root/reference/src/lz_matcher.cpp:582-617); the matching stage is one call per
// block of rows into the C-ABI of include/lzani.h.
#pragma once
#include <chrono>
#include <condition_variable>
#include <deque>
#include <future>
#include <thread>

#include "../csrc/lzani_aln_rule.h"
#include "../csrc/lzani_cluster_plan.h"
#include "cli.h"
#include "engine.h"

struct AlnRegion { uint32_t ref, qry; lzani_region r; };

static void genome_views(const vector<Genome>& g, vector<const uint8_t*>& ptr, vector<uint32_t>& len)   // the genomes as the C-ABI takes them
{
    ptr.resize(g.size()); len.resize(g.size());
    for (size_t i = 0; i < g.size(); ++i) { ptr[i] = g[i].codes.data(); len[i] = (uint32_t)g[i].codes.size(); }
}

// The devices of a run over the genomes g, for the group and the --out-alignment shards alike: at most --gpus of them,
// P.device + d, or what LZANI_DEVICE_LIST names (rehearsals: "0,0,0")
static vector<int> device_list(const vector<Genome>& g)
{
    const int ng = max(1, min<int>(P.gpus, (int)max<size_t>(g.size(), 1)));
    vector<int> devs;
    if (const char* e = getenv("LZANI_DEVICE_LIST")) for (const auto& x : split(e, ',')) devs.push_back(atoi(x.c_str()));
    else for (int d = 0; d < ng; ++d) devs.push_back(P.device + d);
    if (devs.empty()) devs.push_back(P.device);
    return devs;
}

static bool matching_failed(const string& why)
{
    cerr << "LZ matching failed: " << why << endl;
    return false;
}

// The group on the run's devices, with the genomes on every device.
static bool open_group(Group& G, const vector<Genome>& g)
{
    vector<const uint8_t*> ptr; vector<uint32_t> len;
    genome_views(g, ptr, len);
    G.devs = device_list(g);
    const auto t_a = chrono::steady_clock::now();
    const int rc = G.E.group_create(&P.lz, (uint32_t)G.devs.size(), G.devs.data(), &G.p);
    if (rc != LZANI_OK) return matching_failed("lzani_group_create failed with code " + to_string(rc) + ": " + G.E.group_last_error(nullptr));
    const auto t_b = chrono::steady_clock::now();
    G.E.group_set_genome_memory(G, P.gpu_mem);
    if (G.E.group_set_genomes(G, (uint32_t)g.size(), ptr.data(), len.data()) != LZANI_OK) return matching_failed(G.E.group_last_error(G));
    G.secs[0] = chrono::duration<double>(t_b - t_a).count();
    G.secs[1] = chrono::duration<double>(chrono::steady_clock::now() - t_b).count();
    return true;
}

// -V 2: what one GPU did (summed: a tiled all2all's sums over its calls, the k-mer words inside the candidate figure)
static void print_gpu_timing(int dev, const lzani_timing& t, bool summed, const double* gather)
{
    cerr << "GPU " << dev << ": " << t.pairs << " pairs, index " << t.index_ms << " ms, ";
    if (summed) cerr << "k-mer words + candidate stage ";
    else cerr << "k-mer words " << t.kmers_ms << " ms, candidate stage ";
    cerr << t.cand_ms << " ms, pair kernel " << t.pairs_ms << " ms" << (gather ? ", gather " + to_string(*gather) + " ms" : string()) << "\n";
}

// -V 2 with --gpu-mem or an out-of-core set: how the genome set of a device was held (lzani_get_residency); a tiled
// all2all passes its sums over its calls
static void print_residency(int dev, const lzani_residency_info& r, uint64_t tiles, uint64_t uploads, double upload_ms)
{
    if (!P.gpu_mem && r.blocks <= 1) return;
    cerr << "genome set on device " << dev << ": " << (r.blocks > 1 ? "out-of-core" : "in-core") << ", " << r.blocks << " block(s), " << tiles
         << " tile(s), " << uploads << " block upload(s), upload " << upload_ms << " ms, limit " << r.limit << " bytes, peak resident "
         << r.peak_resident_bytes << " bytes\n";
}

// -V 2 after an untiled group run: every device's timing and residency
static void print_group_devices(const Group& G)
{
    for (int d = 0; d < (int)G.devs.size(); ++d) {
        lzani_timing t; lzani_residency_info ri; double gather = 0;
        if (G.E.group_get_timing(G, (uint32_t)d, &t, &gather) == LZANI_OK) print_gpu_timing(G.devs[d], t, false, d == 0 && G.devs.size() > 1 ? &gather : nullptr);
        if (G.E.group_get_residency(G, (uint32_t)d, &ri) == LZANI_OK) print_residency(G.devs[d], ri, ri.tiles, ri.block_uploads, ri.upload_ms);
    }
}

// -V 2: the one line of the device's output filter (a tiled all2all: the sums over its blocks)
static void print_kept(const lzani_kept_info& k)
{
    cerr << "out-filter on the device: " << k.kept_pairs << " pairs, " << k.kept_lines << " lines kept of " << k.leading << " pairs, " << k.unpaired
         << " unpaired, " << k.filter_ms << " ms\n";
}

// -V 2 after the one group call of an untiled run
static void print_engine_line(const Group& G, double matching_secs)
{
    cerr << "engine: create " << G.secs[0] << " s, genomes to the device " << G.secs[1] << " s, matching " << matching_secs << " s\n";
}

// --flt-kmers: the filter rows from the device k-mer prefilter on the first device, for the genomes in their reordered
// ids: a context of its own, the stage with min_shared 1 and the threshold as min_ratio, the kept pairs; symmetrised into
// flt.rows like a kmer-db file's.  Without --gpu-mem the genomes become the context's set and lzani_prefilter runs on
// them; with it -- or where that set went out-of-core or did not fit -- the genomes stay in host memory and
// lzani_prefilter_codes streams them through a staging buffer of at most --gpu-mem bytes (automatic without).  n_ref > 0
// (query2ref): the cross form of either, the kept pairs of the references 0 .. n_ref - 1 with the queries behind them.
// --flt-kmers-counting goes to the context before the stage runs.  --flt-kmers-max-seqs: lzani_prefilter_limit cuts the
// result of whichever of the four calls made it, before it is fetched.
static bool kmer_filter(const Engine& E, const vector<Genome>& g, Filter& flt, uint32_t n_ref = 0)
{
    const uint32_t n = (uint32_t)g.size();
    vector<const uint8_t*> ptr; vector<uint32_t> len;
    genome_views(g, ptr, len);
    if (P.flt_max_seqs)
        if (const char* sym = E.missing_limit()) { cerr << "Missing symbol " << sym << " (--flt-kmers-max-seqs needs it)" << endl; return false; }
    Context ctx(E);
    auto fresh = [&]() {                                                  // a new context, configured
        ctx.reset();
        const int rc = E.create(&P.lz, P.device, &ctx.p);
        if (rc != LZANI_OK) { cerr << "K-mer filter failed: lzani_create failed with code " << rc << endl; return false; }
        E.set_prefilter_counting(ctx, P.flt_counting);
        return true;
    };
    auto resident = [&](uint64_t* kept) {
        return n_ref ? E.prefilter_cross(ctx, P.flt_k, sample_max_of(P.flt_fraction), 1, P.filter_thr, n_ref, kept)
                     : E.prefilter(ctx, P.flt_k, sample_max_of(P.flt_fraction), 1, P.filter_thr, kept);
    };
    auto codes = [&](uint64_t slice, uint64_t* kept) {
        return n_ref ? E.prefilter_codes_cross(ctx, n, ptr.data(), len.data(), P.flt_k, sample_max_of(P.flt_fraction), 1, P.filter_thr, slice, n_ref, kept)
                     : E.prefilter_codes(ctx, n, ptr.data(), len.data(), P.flt_k, sample_max_of(P.flt_fraction), 1, P.filter_thr, slice, kept);
    };
    if (!fresh()) return false;
    uint64_t kept = 0;
    vector<uint64_t> row_off((size_t)n + 1, 0);
    vector<uint32_t> ids;
    bool streamed = P.gpu_mem != 0;
    int rc;
    if (streamed) rc = codes(P.gpu_mem, &kept);
    else {
        rc = E.set_genomes(ctx, n, ptr.data(), len.data());
        if (rc == LZANI_OK) rc = resident(&kept);
        if (rc == LZANI_ERR_STATE || rc == LZANI_ERR_NOMEM) {             // the set went out-of-core, or does not fit: a fresh context, streamed
            if (!fresh()) return false;
            streamed = true;
            rc = codes(0, &kept);
        }
    }
    if (rc == LZANI_OK && P.flt_max_seqs) rc = E.prefilter_limit(ctx, P.flt_max_seqs, &kept);
    if (rc == LZANI_OK) { ids.resize(kept); rc = E.prefilter_fetch(ctx, nullptr, row_off.data(), ids.data(), nullptr); }
    if (rc != LZANI_OK) { cerr << "K-mer filter failed: " << E.last_error(ctx) << endl; return false; }
    lzani_prefilter_info pi;
    lzani_prefilter_stream_info si;
    lzani_prefilter_pass_info ps;
    lzani_prefilter_sparse_info sp;
    lzani_prefilter_limit_info li;
    string stream_note, sparse_note, limit_note;
    if (P.flt_max_seqs && E.get_prefilter_limit_info(ctx, &li) == LZANI_OK) {
        ostringstream ss;
        ss << "; max-seqs " << li.max_per_genome << ": " << li.entries_out << " of " << li.entries_in << " pairs stay, " << li.genomes_cut << " of " << li.limiting
           << " sequences cut, limit " << li.limit_ms << " ms";
        limit_note = ss.str();
    }
    if (E.get_prefilter_sparse_info(ctx, &sp) == LZANI_OK && sp.sparse)                   // (the tiles are in the line already)
        sparse_note = "; sparse counting: " + to_string(sp.attempts) + " attempt(s), " + to_string(sp.slots) + " slots";
    if (streamed && E.get_prefilter_stream_info(ctx, &si) == LZANI_OK) {
        ostringstream ss;
        ss << "; streamed: " << si.slices << " slice(s), " << si.slice_uploads << " upload(s), upload " << si.upload_ms << " ms, staging " << si.stage_bytes << " bytes";
        stream_note = ss.str();
    }
    if (E.get_prefilter_pass_info(ctx, &ps) == LZANI_OK && ps.passes > 1) stream_note += "; " + to_string(ps.passes) + " passes";
    if (n_ref) stream_note += "; " + to_string(n_ref) + " x " + to_string(n - n_ref);
    if (P.verbosity >= 2 && E.get_prefilter_info(ctx, &pi) == LZANI_OK)
        cerr << "k-mer filter on device " << P.device << ": k " << pi.k << ", " << pi.positions << " sampled windows, " << pi.distinct_kmers
             << " distinct k-mers, " << pi.postings << " postings, " << pi.entries << " kept pairs, " << pi.tiles << " tile(s); keys " << pi.keys_ms
             << " ms, sorts " << pi.sort_ms << " ms, counting " << pi.count_ms << " ms, compaction " << pi.compact_ms << " ms" << sparse_note << stream_note << limit_note << "\n";
    flt.names.clear();
    filter_from_pairs(n, row_off, ids, flt);
    return true;
}

// The alignment file (store_alignment, lz_matcher.cpp:102-169): one BLAST-tab-like row per region.  Both paths write
// through it, region by region in the file's order: pairs in (reference, query) order, the rows of one pair in
// calc_regions order (length desc, seq_start asc).
struct AlnWriter {
    ofstream o;
    string line;
    char num[64];
    bool open()
    {
        o.open(P.out_aln, ios::binary);
        if (!o.is_open()) { cerr << "Cannot open output file: " << P.out_aln << endl; return false; }
        o << "query\treference\tpident\talnlen\tqstart\tqend\trstart\trend\tnt_match\tnt_mismatch\n";
        return true;
    }
    void put(const vector<Genome>& g, uint32_t r, uint32_t q, const lzani_region& x)
    {
        const int len1 = (int)g[r].codes.size(), rc_corr = 2 * len1 + 2 * P.lz.max_dist_in_ref + 1;
        const int length = x.seq_end - x.seq_start;
        line.clear();
        line += g[q].name; line += '\t'; line += g[r].name; line += '\t';
        line.append(num, real_to_chars(100.0 * x.num_matches / length, num, 6)); line += '\t';
        auto field = [&](long v, char sep) { line += to_string(v); line += sep; };
        field(length, '\t'); field(1 + x.seq_start, '\t'); field(x.seq_end, '\t');
        if (x.ref_start < len1) { field(1 + x.ref_start, '\t'); field(x.ref_end, '\t'); }
        else { field(rc_corr - (1 + x.ref_start), '\t'); field(rc_corr - x.ref_end, '\t'); }
        field(x.num_matches, '\t'); field(x.num_mismatches, '\n');
        o.write(line.data(), (streamsize)line.size());
    }
    bool close() { o.close(); return !o.fail(); }
};

// The host path of --out-alignment: the regions of every shard, as match_regions left them, through the library's host
// statement of the region stage (lzani_regions_host: the rule over the region sums -- the part of --out-filter that applies
// here -- and the file's order).  The call it is given lists the pairs that own a region, in (reference, query) order.  A
// library without the symbol: lzani::aln_host_order (lzani_aln_rule.h), the header function that lzani_regions_host itself calls.
static bool store_alignment(const Engine& E, const vector<Genome>& g, vector<AlnRegion>& regs)
{
    AlnWriter W;
    if (!W.open()) return false;
    const uint32_t n = (uint32_t)g.size();
    vector<uint64_t> keys(regs.size());
    for (size_t k = 0; k < regs.size(); ++k) keys[k] = (uint64_t)regs[k].ref << 32 | regs[k].qry;
    sort(keys.begin(), keys.end());
    keys.erase(unique(keys.begin(), keys.end()), keys.end());
    vector<uint32_t> ref_ids, query_ids(keys.size()), len(n);
    vector<uint64_t> row_off(1, 0);
    for (size_t e = 0; e < keys.size(); ++e) {
        if (e == 0 || keys[e] >> 32 != keys[e - 1] >> 32) { if (e) row_off.push_back(e); ref_ids.push_back((uint32_t)(keys[e] >> 32)); }
        query_ids[e] = (uint32_t)keys[e];
    }
    if (!keys.empty()) row_off.push_back(keys.size());
    for (uint32_t i = 0; i < n; ++i) len[i] = (uint32_t)g[i].codes.size();
    vector<lzani_region> raw(regs.size()), out(regs.size());
    for (size_t k = 0; k < regs.size(); ++k) {
        raw[k] = regs[k].r;
        raw[k].pair = (uint64_t)(lower_bound(keys.begin(), keys.end(), (uint64_t)regs[k].ref << 32 | regs[k].qry) - keys.begin());
    }
    // the part of --out-filter that applies here; a NaN minimum drops nothing and the other minima apply (lzani_regions_host
    // refuses a NaN: -inf says the same)
    lzani_out_filter f = out_filter_minima();
    for (double* m : {&f.min_gani, &f.min_ani, &f.min_qcov}) if (*m != *m) *m = -numeric_limits<double>::infinity();
    const lzani_out_filter* rule = P.flt_mask != 0 ? &f : nullptr;
    uint64_t n_out = 0;
    if (E.regions_host && n) {
        if (E.regions_host(n, len.data(), (uint32_t)ref_ids.size(), ref_ids.data(), row_off.data(), query_ids.data(), raw.data(), raw.size(), rule, out.data(), &n_out,
                           nullptr) != LZANI_OK) { cerr << "Ordering the alignment regions failed" << endl; return false; }
    } else {                                                    // an older library: the statement itself, the header function that call is made of
        vector<uint64_t> order;
        lzani::aln_host_counts cnt;
        lzani::aln_host_order((uint32_t)ref_ids.size(), ref_ids.data(), row_off.data(), query_ids.data(), len.data(), raw.data(), raw.size(), rule, order, cnt);
        for (uint64_t i : order) out[n_out++] = raw[i];
    }
    if (P.verbosity >= 2) cerr << "alignment regions on the host: " << n_out << " of " << raw.size() << " regions stay\n";
    for (uint64_t k = 0; k < n_out; ++k) W.put(g, (uint32_t)(keys[out[k].pair] >> 32), (uint32_t)keys[out[k].pair], out[k]);
    return W.close();
}

// --cluster-out: one line per genome in the order of the ids file, its id and its cluster number or its representative's id.
// A level of --cluster-level writes the same lines into its own file.
static bool write_clusters(const vector<Genome>& g, const vector<uint32_t>& rep_of, const vector<uint32_t>& cluster_of, const string& fn = P.cluster_out)
{
    ofstream o(fn, ios::binary);
    if (!o.is_open()) { cerr << "Cannot open output file: " << fn << endl; return false; }
    o << "object\t" << (P.cluster_reps ? "representative" : "cluster") << "\n";
    for (size_t i = 0; i < g.size(); ++i) {
        o << g[i].name << '\t';
        if (P.cluster_reps) o << g[rep_of[i]].name; else o << cluster_of[i];
        o << '\n';
    }
    o.close();
    return !o.fail();
}

// The device path of --cluster: an empty edge set before the kept calls, the edges of each kept call added behind it
// (run_block), and at the end the run, the fetch and the file.  With --cluster-cut or --cluster-level (P.levels_on()): an
// empty record store before the kept calls, the records of each kept call added behind it, and at the end, for every level in
// order, the level's edges from the store under its cut, then the run, the fetch and the level's file.
static bool clustering_failed(const Group& G)
{
    cerr << "Clustering failed: " << G.E.group_last_error(G) << endl;
    return false;
}
static bool cluster_begin(const Group& G, const vector<uint32_t>& rlen)
{
    if (P.levels_on()) return G.E.group_cluster_store_begin(G, (uint32_t)rlen.size(), rlen.data()) == LZANI_OK || clustering_failed(G);
    return G.E.group_cluster_begin(G, (uint32_t)rlen.size(), rlen.data(), P.cluster_measure) == LZANI_OK || clustering_failed(G);
}
// the run of `algo` on the edges there are, the fetch, what -V 2 says of the run, and the file
static bool cluster_run_to_file(const Group& G, const vector<Genome>& g, int algo, const string& fn)
{
    vector<uint32_t> rep_of(g.size()), cluster_of(g.size());
    if (algo == LZANI_CLUSTER_LEIDEN && G.E.group_set_cluster_leiden(G, P.leiden_resolution, P.leiden_iterations) != LZANI_OK) return clustering_failed(G);
    if (G.E.group_cluster_run(G, algo, nullptr) != LZANI_OK || G.E.group_cluster_fetch(G, rep_of.data(), cluster_of.data()) != LZANI_OK)
        return clustering_failed(G);
    lzani_cluster_info ci;
    if (P.verbosity >= 2 && G.E.group_get_cluster_info(G, &ci) == LZANI_OK)
        cerr << "clusters on the device: " << ci.clusters << " of " << ci.n << " sequences (" << ci.singletons << " singletons, the largest of " << ci.largest
             << ") from " << ci.edges << " pairs, " << ci.rounds << " round(s), add " << ci.add_ms << " ms, run " << ci.run_ms << " ms\n";
    lzani_cluster_cover_info cv;
    if (P.verbosity >= 2 && G.E.group_get_cluster_cover_info && G.E.group_get_cluster_cover_info(G, &cv) == LZANI_OK)
        cerr << "set cover: " << cv.distinct_edges << " distinct pairs (" << cv.duplicate_edges << " given again), unique " << cv.dedup_ms << " ms, rounds "
             << cv.rounds_ms << " ms, workspace " << cv.workspace_bytes << " bytes\n";
    lzani_cluster_link_info lk;
    if (P.verbosity >= 2 && G.E.group_get_cluster_link_info && G.E.group_get_cluster_link_info(G, &lk) == LZANI_OK)
        cerr << "complete linkage: " << lk.distinct_edges << " distinct pairs (" << lk.duplicate_edges << " given again), " << lk.merges << " merges, table of "
             << lk.table_slots << " slots, first insert " << lk.dedup_ms << " ms, rounds " << lk.rounds_ms << " ms, workspace " << lk.workspace_bytes << " bytes\n";
    lzani_cluster_leiden_info ld;
    if (P.verbosity >= 2 && G.E.group_get_cluster_leiden_info && G.E.group_get_cluster_leiden_info(G, &ld) == LZANI_OK)
        cerr << "Leiden: " << ld.distinct_edges << " distinct pairs (" << ld.duplicate_edges << " given again), " << ld.iterations << " iterations, " << ld.levels
             << " levels, " << ld.move_rounds << " moving and " << ld.refine_rounds << " refinement rounds, " << ld.moves << " moves, " << ld.merges
             << " merges, quality " << ld.quality << " / 2^20 (distinct " << ld.dedup_ms << " ms, rounds " << ld.rounds_ms << " ms)\n";
    return write_clusters(g, rep_of, cluster_of, fn);
}
static bool cluster_finish(const Group& G, const vector<Genome>& g)
{
    if (!P.levels_on()) return cluster_run_to_file(G, g, P.cluster_algo, P.cluster_out);
    lzani_cluster_store_info si;
    if (P.verbosity >= 2 && G.E.group_get_cluster_store_info(G, &si) == LZANI_OK)
        cerr << "cluster record store on the device: " << si.records << " records of " << si.n << " sequences, " << si.record_bytes << " bytes, add " << si.add_ms << " ms\n";
    for (size_t k = 0; k < P.levels.size(); ++k) {
        const Params::Level& lv = P.levels[k];
        if (G.E.group_cluster_level(G, P.cluster_measure, &lv.cut, nullptr) != LZANI_OK) return clustering_failed(G);
        lzani_cluster_level_info li;
        if (P.verbosity >= 2 && G.E.group_get_cluster_level_info(G, &li) == LZANI_OK)
            cerr << "cluster level " << k << " on the device (" << lv.out << "): " << li.records_in << " records in, " << li.edges_out << " edges out, lines "
                 << li.lines_in << " -> " << li.lines_out << ", level " << li.level_ms << " ms\n";
        if (!cluster_run_to_file(G, g, lv.algo, lv.out)) return false;
    }
    return true;
}

// The host path of --cluster: the records of the table's pairs of which the filter keeps a line, by the sequential statement.
// level (--cluster-cut, --cluster-level): of those records the lines that stay under the level's cut (cluster_cut_lines), into
// the level's file; null: the clustering of --cluster alone.
static bool cluster_on_host(const vector<Genome>& g, const PairTable& T, const EmitParams& ep, const Params::Level* level = nullptr)
{
    const vector<uint32_t> len = report_lengths(g, ep.mrd);
    const int algo = level ? level->algo : P.cluster_algo;
    vector<lzani_cluster_edge> edges;
    for (uint32_t a = 0; a < T.n; ++a)
        for_pairs_led_by(T, a, [&](uint32_t b, const lzani_result& X, const lzani_result& Y) {
            const lzani_kept_pair k = make_record(len, ep, a, b, X, Y);
            const uint32_t lines = level ? lzani::cluster_cut_lines(level->cut, k.x, k.y, k.lines, len[a], len[b]) : k.lines;
            if (lines) edges.push_back(lzani_cluster_edge{a, b, lzani::cluster_weight(P.cluster_measure, k.x, k.y, lines, len[a], len[b])});
        });
    vector<uint32_t> rep_of(g.size()), cluster_of(g.size());
    uint32_t k = 0;
    auto run = [&]() {
        if (algo != LZANI_CLUSTER_LEIDEN)
            return lzani::cluster_host((uint32_t)g.size(), edges.data(), edges.size(), algo, rep_of.data(), cluster_of.data(), &k);
        // Leiden with the resolution and the iterations asked for (cluster_host runs the defaults)
        if (int rc = lzani::cluster_leiden_host((uint32_t)g.size(), edges.data(), edges.size(), P.leiden_resolution, P.leiden_iterations, rep_of.data(), nullptr)) return rc;
        k = lzani::cluster_number((uint32_t)g.size(), rep_of.data(), cluster_of.data());
        return (int)LZANI_OK;
    };
    if (!g.empty() && run() != LZANI_OK) {
        cerr << "Clustering failed" << endl;
        return false;
    }
    if (P.verbosity >= 2) cerr << "clusters on the host: " << k << " of " << g.size() << " sequences from " << edges.size() << " pairs\n";
    return write_clusters(g, rep_of, cluster_of, level ? level->out : P.cluster_out);
}

// A block of rows as the engine takes it: CSR over ids, q null for dense rows (every id but the row's own).
struct RowBlock { uint32_t n_rows; const uint32_t* rows; const uint64_t* off; const uint32_t* q; };

// One group call for a block of rows: into `out` (lzani_group_run_rows), or, where out is null, the kept form with the
// output filter and the printed lengths rlen (lzani_group_run_rows_kept), n_kept records of which stay in the group, and
// behind it the block's cluster edges (--cluster), or with levels its records into the store.  whole: the call is the run's only one, and -V 2 says what it took.
static bool run_block(const Group& G, const RowBlock& b, lzani_result* out, const vector<uint32_t>& rlen, uint64_t& n_kept, bool whole)
{
    const lzani_out_filter f = out_filter_minima();
    n_kept = 0;
    const auto t_c = chrono::steady_clock::now();
    const int rc = out ? G.E.group_run_rows(G, b.n_rows, b.rows, b.off, b.q, out)
                       : G.E.group_run_rows_kept(G, b.n_rows, b.rows, b.off, b.q, &f, rlen.data(), &n_kept);
    if (whole && P.verbosity >= 2) print_engine_line(G, chrono::duration<double>(chrono::steady_clock::now() - t_c).count());
    if (rc != LZANI_OK) return matching_failed(G.E.group_last_error(G));
    // before the next kept call replaces the records: their edges, or (levels) the records themselves into the store
    if (!out && P.cluster && (P.levels_on() ? G.E.group_cluster_store_add_kept(G, nullptr) : G.E.group_cluster_add_kept(G, nullptr)) != LZANI_OK) return clustering_failed(G);
    return true;
}

// Records first .. first + count - 1 of the group's last kept call.
static bool fetch_kept(const Group& G, uint64_t first, vector<lzani_kept_pair>& rec)
{
    return G.E.group_kept_fetch(G, first, rec.size(), rec.data()) == LZANI_OK || matching_failed(G.E.group_last_error(G));
}

// --out-alignment: the per-pair region lists are variable-length, so every shard comes back through host memory
// (lzani_run_rows_regions, a context per entry of the device list); the rows are dealt by the group's partition.
static bool match_regions(const Engine& E, const vector<Genome>& g, const vector<uint32_t>& ref_ids, PairTable& T, vector<AlnRegion>& aln)
{
    const uint32_t n = (uint32_t)g.size();
    const vector<int> devs = device_list(g);
    vector<const uint8_t*> ptr; vector<uint32_t> len;
    genome_views(g, ptr, len);
    vector<uint32_t> part(n);
    vector<uint64_t> cost(T.dense ? 0 : n);
    if (!T.dense) E.row_costs(n, ref_ids.data(), T.row_off.data(), T.query_ids.data(), n, len.data(), cost.data());
    E.partition_rows(n, T.dense ? nullptr : cost.data(), (uint32_t)devs.size(), part.data());
    vector<string> errs(devs.size());
    mutex mtx;
    auto shard = [&](int d) {
        Context ctx(E);
        int rc = E.create(&P.lz, devs[d], &ctx.p);
        if (rc != LZANI_OK) { errs[d] = "lzani_create failed with code " + to_string(rc) + (rc == LZANI_ERR_PARAMS ? " (LZ parameters outside the supported envelope)" : ""); return; }
        E.set_genome_memory(ctx, P.gpu_mem);
        rc = E.set_genomes(ctx, n, ptr.data(), len.data());
        vector<uint32_t> rows, query_ids;
        vector<uint64_t> row_off(1, 0);
        for (uint32_t r = 0; r < n; ++r) {
            if (part[r] != (uint32_t)d) continue;
            rows.push_back(r);
            if (!T.dense) query_ids.insert(query_ids.end(), T.query_ids.begin() + (ptrdiff_t)T.row_off[r], T.query_ids.begin() + (ptrdiff_t)T.row_off[r + 1]);
            row_off.push_back(row_off.back() + T.row_size(r));
        }
        vector<lzani_result> out(row_off.back());
        vector<lzani_region> regs;
        uint64_t cap = max<uint64_t>(1024, row_off.back() / 4), cnt = 0;
        while (rc == LZANI_OK) {
            regs.resize(cap);
            rc = E.run_rows_regions(ctx, (uint32_t)rows.size(), rows.data(), row_off.data(), T.dense ? nullptr : query_ids.data(),
                                    out.data(), regs.data(), cap, &cnt);
            if (rc != LZANI_OK || cnt <= cap) break;
            cap = cnt;
        }
        if (rc != LZANI_OK) { errs[d] = E.last_error(ctx); return; }
        regs.resize(cnt);
        for (size_t k = 0; k < rows.size(); ++k)
            copy(out.begin() + (ptrdiff_t)row_off[k], out.begin() + (ptrdiff_t)row_off[k + 1], T.res.begin() + (ptrdiff_t)T.row_off[rows[k]]);
        lock_guard<mutex> lck(mtx);
        for (const auto& x : regs) {
            size_t k = upper_bound(row_off.begin(), row_off.end(), x.pair) - row_off.begin() - 1;
            aln.push_back(AlnRegion{rows[k], T.id_at(rows[k], x.pair - row_off[k]), x});
        }
        if (P.verbosity >= 2) {
            lzani_timing t; lzani_residency_info ri;
            if (E.get_timing(ctx, &t) == LZANI_OK) print_gpu_timing(devs[d], t, false, nullptr);
            if (E.get_residency(ctx, &ri) == LZANI_OK) print_residency(devs[d], ri, ri.tiles, ri.block_uploads, ri.upload_ms);
        }
    };
    vector<thread> th;
    for (int d = 1; d < (int)devs.size(); ++d) th.emplace_back(shard, d);
    shard(0);
    for (auto& t : th) t.join();
    for (auto& e : errs) if (!e.empty()) return matching_failed(e);
    return true;
}

// -V 2: the one line of the device's region stage
static void print_regions(const lzani_regions_info& r)
{
    cerr << "alignment regions on the device: " << r.kept << " of " << r.found << " regions stay, " << r.entries_dropped << " of " << r.entries_with_regions
         << " pairs dropped, capacity " << r.capacity << ", " << r.runs << " run(s), " << r.sort_passes << " sort passes, sums " << r.sums_ms << " ms, sorts "
         << r.sort_ms << " ms, gather " << r.write_ms << " ms, workspace " << r.workspace_bytes << " bytes\n";
}

// --out-alignment on one device (lzani_run_rows_aligned): one run leaves the results -- in T, or with `kept` as the kept
// records of the output filter, written here as do_matching writes them -- and the regions of the pairs that pass the
// alignment's rule, in the file's order; the alignment file is written while they are fetched, in pieces of a million (32 MB).
static bool match_aligned(const Engine& E, const vector<Genome>& g, const vector<uint32_t>& ref_ids, PairTable& T, const EmitParams& ep, bool kept)
{
    const uint32_t n = (uint32_t)g.size();
    vector<const uint8_t*> ptr; vector<uint32_t> len;
    genome_views(g, ptr, len);
    const int dev = device_list(g)[0];
    Context ctx(E);
    const auto t_a = chrono::steady_clock::now();
    int rc = E.create(&P.lz, dev, &ctx.p);
    if (rc != LZANI_OK) return matching_failed("lzani_create failed with code " + to_string(rc) + (rc == LZANI_ERR_PARAMS ? " (LZ parameters outside the supported envelope)" : ""));
    const auto t_b = chrono::steady_clock::now();
    E.set_genome_memory(ctx, P.gpu_mem);
    if (E.set_genomes(ctx, n, ptr.data(), len.data()) != LZANI_OK) return matching_failed(E.last_error(ctx));
    const auto t_c = chrono::steady_clock::now();
    static const uint32_t no_ids[1] = {0};
    const uint32_t* q = T.dense ? nullptr : T.query_ids.empty() ? no_ids : T.query_ids.data();
    const vector<uint32_t> rlen = report_lengths(g, ep.mrd);
    const lzani_out_filter f = out_filter_minima();
    uint64_t n_kept = 0, n_regs = 0;
    rc = E.run_rows_aligned(ctx, n, ref_ids.data(), T.row_off.data(), q, kept ? nullptr : T.res.data(), kept ? &f : nullptr, rlen.data(),
                            P.flt_mask != 0 ? &f : nullptr, nullptr, &n_kept, &n_regs);
    if (rc != LZANI_OK) return matching_failed(E.last_error(ctx));
    if (P.verbosity >= 2) {
        cerr << "engine: create " << chrono::duration<double>(t_b - t_a).count() << " s, genomes to the device " << chrono::duration<double>(t_c - t_b).count()
             << " s, matching " << chrono::duration<double>(chrono::steady_clock::now() - t_c).count() << " s\n";
        lzani_timing t; lzani_residency_info ri; lzani_kept_info ki; lzani_regions_info gi;
        if (E.get_timing(ctx, &t) == LZANI_OK) print_gpu_timing(dev, t, false, nullptr);
        if (E.get_residency(ctx, &ri) == LZANI_OK) print_residency(dev, ri, ri.tiles, ri.block_uploads, ri.upload_ms);
        if (kept && E.get_kept_info(ctx, &ki) == LZANI_OK) print_kept(ki);
        if (E.get_regions_info(ctx, &gi) == LZANI_OK) print_regions(gi);
    }
    if (kept) {
        if (P.verbosity >= 1) cerr << "Storing results" << endl;
        ResultWriter W;
        if (!W.open(g, ep)) return false;
        vector<lzani_kept_pair> rec;
        for (uint64_t first = 0; first < n_kept; first += rec.size()) {
            rec.resize((size_t)min<uint64_t>(n_kept - first, 1u << 20));
            if (E.kept_fetch(ctx, first, rec.size(), rec.data()) != LZANI_OK) return matching_failed(E.last_error(ctx));
            W.emit_kept(g, rec.data(), rec.size());
        }
        if (!W.close()) return false;
    }
    AlnWriter A;
    if (!A.open()) return false;
    vector<lzani_region> regs;
    uint32_t row = 0;                                           // the regions come by ascending entry: the row only moves on
    for (uint64_t first = 0; first < n_regs; first += regs.size()) {
        regs.resize((size_t)min<uint64_t>(n_regs - first, 1u << 20));
        if (E.regions_fetch(ctx, first, regs.size(), regs.data()) != LZANI_OK) return matching_failed(E.last_error(ctx));
        for (const lzani_region& x : regs) {
            while (x.pair >= T.row_off[row + 1]) ++row;
            A.put(g, ref_ids[row], T.id_at(row, x.pair - T.row_off[row]), x);
        }
    }
    return A.close();
}

// do_matching (lz_matcher.cpp:172-277).  The reference's workers pull reference rows off an atomic counter and
// run one CParser each; here the whole row table goes to the engine in one call: lzani_group_run_rows deals
// the rows over the GPUs of the group (cyclic for dense rows, LPT for filtered ones), runs them, gathers the
// shards over RCCL on the first GPU and copies the results out once, CSR-aligned with T.
// kept: the output filter on the device -- the same rows (the filter's lists sorted by the caller, lists_ascend) through
// lzani_group_run_rows_kept with the printed lengths; T keeps its layout and no results, and the kept records -- in the
// order of the output file -- are written here, in pieces of a million (36 MB) as they are fetched.
// aln (--out-alignment): the regions of every pair as well, by match_regions (the host path: they come back unordered, for
// store_alignment); aln_dev: by match_aligned instead, which writes the alignment file, and with `kept` the result files, itself.
static bool do_matching(const Engine& E, const vector<Genome>& g, Filter& flt, PairTable& T, const EmitParams& ep, bool kept, vector<AlnRegion>* aln, bool aln_dev)
{
    const uint32_t n = (uint32_t)g.size();
    if (P.verbosity >= 1) cerr << "All2all sparse" << endl;
    if (flt.empty()) T.init_dense(n, !kept);
    else { T.init_sparse(flt.rows, !kept); vector<vector<uint32_t>>().swap(flt.rows); }   // the reference clears filter rows as it goes (266-267)
    vector<uint32_t> ref_ids(n);
    for (uint32_t i = 0; i < n; ++i) ref_ids[i] = i;
    if (aln_dev) return match_aligned(E, g, ref_ids, T, ep, kept);
    if (aln) return match_regions(E, g, ref_ids, T, *aln);

    // (kept: lists that are all empty are still lists, never null; the table form has always passed them as they are, and the
    // engine then refuses them as dense rows of the wrong size)
    static const uint32_t no_ids[1] = {0};
    const RowBlock all{n, ref_ids.data(), T.row_off.data(), T.dense ? nullptr : kept && T.query_ids.empty() ? no_ids : T.query_ids.data()};
    Group G(E);
    if (!open_group(G, g)) return false;
    const vector<uint32_t> rlen = report_lengths(g, ep.mrd);   // the lengths the TSV prints
    uint64_t n_kept = 0;
    if (kept && P.cluster && !cluster_begin(G, rlen)) return false;
    if (!run_block(G, all, kept ? nullptr : T.res.data(), rlen, n_kept, true)) return false;
    if (P.verbosity >= 2) {
        print_group_devices(G);
        lzani_kept_info ki;
        if (kept && E.group_get_kept_info(G, &ki) == LZANI_OK) print_kept(ki);
    }
    if (!kept) return true;
    if (P.cluster && !cluster_finish(G, g)) return false;
    if (P.verbosity >= 1) cerr << "Storing results" << endl;
    ResultWriter W;
    if (!W.open(g, ep)) return false;
    vector<lzani_kept_pair> rec;
    for (uint64_t first = 0; first < n_kept; first += rec.size()) {
        rec.resize((size_t)min<uint64_t>(n_kept - first, 1u << 20));
        if (!fetch_kept(G, first, rec)) return false;
        W.emit_kept(g, rec.data(), rec.size());
    }
    return W.close();
}

// Dense all2all, tiled: the matrix goes to the engine in row x column blocks -- block A = the rows of A against the
// queries from A on, plus the rows behind A against the queries of A -- so that after block A every pair {a in A, b > a}
// is there in both directions, which is all the text of the reference rows A needs (store_results, lz_matcher.cpp:
// 371-567, walks the pairs the same way, after ALL of do_matching): an emitter thread formats and writes the rows of A
// while the GPUs work on the next block.  Every directed pair is still computed exactly once; the file is byte for
// byte the one the untiled run writes.
// kept: the output filter on the device -- every block's call is lzani_group_run_rows_kept, whose records are exactly the
// pairs {a in A, b > a} of which a line passes, in the file's order (the block holds both directions of each); they are
// fetched behind the call and written by the emitter thread while the next block runs, and the table T is not made.
static bool do_matching_tiled(const Engine& E, const vector<Genome>& g, PairTable& T, const EmitParams& ep, uint32_t tile, bool kept)
{
    const uint32_t n = (uint32_t)g.size();
    if (P.verbosity >= 1) cerr << "All2all sparse" << endl;
    if (!kept) T.init_dense(n);
    Group G(E);
    if (!open_group(G, g)) return false;
    const vector<int>& devs = G.devs;

    ResultWriter W;
    if (!W.open(g, ep)) return false;
    // emitter: the row blocks in order, as they complete
    mutex mtx;
    condition_variable cv;
    deque<pair<uint32_t, uint32_t>> ready;
    deque<vector<lzani_kept_pair>> ready_kept;                  // kept: the records of the finished blocks
    bool done = false;
    thread emitter([&]() {
        for (;;) {
            pair<uint32_t, uint32_t> blk;
            vector<lzani_kept_pair> rec;
            {
                unique_lock<mutex> lk(mtx);
                cv.wait(lk, [&]() { return done || !ready.empty() || !ready_kept.empty(); });
                if (ready.empty() && ready_kept.empty()) return;
                if (kept) { rec = move(ready_kept.front()); ready_kept.pop_front(); }
                else { blk = ready.front(); ready.pop_front(); }
            }
            if (kept) W.emit_kept(g, rec.data(), rec.size());
            else W.emit_rows(g, T, blk.first, blk.second);
        }
    });
    lzani_kept_info k_sum{};
    vector<lzani_timing> t_sum(devs.size(), lzani_timing{});   // (cand_ms: the k-mer words and the candidate stage)
    vector<uint64_t> r_tiles(devs.size(), 0), r_uploads(devs.size(), 0);
    vector<double> r_upload_ms(devs.size(), 0);
    double t_gather = 0;
    // Three sets of buffers: while the GPUs run block k, one host thread lays out the row lists of block k + 1 and another
    // moves the results of block k - 1 into the table and hands its rows to the emitter.
    struct Block { uint32_t a0 = 0, a1 = 0; vector<uint32_t> rows, q; vector<uint64_t> off; vector<lzani_result> out; };
    Block blk[3];
    const uint32_t n_blocks = (n + tile - 1) / tile;
    auto build = [&](uint32_t k) {
        Block& B = blk[k % 3];
        B.a0 = k * tile; B.a1 = min(n, B.a0 + tile);
        B.rows.clear(); B.q.clear(); B.off.assign(1, 0);
        for (uint32_t r = B.a0; r < n; ++r) {
            const size_t before = B.q.size();
            if (r < B.a1) { for (uint32_t x = B.a0; x < n; ++x) if (x != r) B.q.push_back(x); }
            else for (uint32_t x = B.a0; x < B.a1; ++x) B.q.push_back(x);
            if (B.q.size() == before) continue;
            B.rows.push_back(r);
            B.off.push_back(B.q.size());
        }
        if (!kept) B.out.resize(B.q.size());
    };
    auto post = [&](uint32_t k) {
        Block& B = blk[k % 3];
        for (size_t i = 0; i < B.rows.size(); ++i) {              // into the dense table: row r, query x at x - (x > r)
            const uint32_t r = B.rows[i];
            lzani_result* dst = T.res.data() + T.row_off[r];
            for (uint64_t e = B.off[i]; e < B.off[i + 1]; ++e) { const uint32_t x = B.q[e]; dst[x < r ? x : x - 1] = B.out[e]; }
        }
        { lock_guard<mutex> lk(mtx); ready.emplace_back(B.a0, B.a1); }
        cv.notify_one();
    };
    // --cluster: every unordered pair lies in exactly one block, whose kept call adds its edges
    bool ok = !(kept && P.cluster) || cluster_begin(G, W.lengths());
    future<void> f_build, f_post;
    build(0);
    for (uint32_t k = 0; k < n_blocks && ok; ++k) {
        Block& B = blk[k % 3];
        if (k + 1 < n_blocks) f_build = async(launch::async, build, k + 1);
        if (!B.rows.empty()) {
            uint64_t n_kept = 0;
            ok = run_block(G, RowBlock{(uint32_t)B.rows.size(), B.rows.data(), B.off.data(), B.q.data()}, kept ? nullptr : B.out.data(), W.lengths(), n_kept, false);
            if (kept && ok) {
                vector<lzani_kept_pair> rec((size_t)n_kept);
                lzani_kept_info ki;
                if (!fetch_kept(G, 0, rec)) ok = false;
                else if (E.group_get_kept_info(G, &ki) != LZANI_OK) ok = matching_failed(E.group_last_error(G));
                else {
                    k_sum.entries += ki.entries; k_sum.leading += ki.leading; k_sum.unpaired += ki.unpaired; k_sum.kept_pairs += ki.kept_pairs;
                    k_sum.kept_lines += ki.kept_lines; k_sum.filter_ms += ki.filter_ms;
                    { lock_guard<mutex> lk(mtx); ready_kept.push_back(move(rec)); }
                    cv.notify_one();
                }
            }
            for (size_t d = 0; d < devs.size() && ok; ++d) {
                lzani_timing t; double gather = 0;
                if (E.group_get_timing(G, (uint32_t)d, &t, &gather) == LZANI_OK) {
                    t_sum[d].index_ms += t.index_ms; t_sum[d].pairs_ms += t.pairs_ms; t_sum[d].cand_ms += t.cand_ms + t.kmers_ms; t_sum[d].pairs += t.pairs;
                    if (d == 0) t_gather += gather;
                }
                lzani_residency_info ri;
                if (E.group_get_residency(G, (uint32_t)d, &ri) == LZANI_OK) { r_tiles[d] += ri.tiles; r_uploads[d] += ri.block_uploads; r_upload_ms[d] += ri.upload_ms; }
            }
        }
        if (f_build.valid()) f_build.get();
        if (f_post.valid()) f_post.get();                         // (block k - 1 is out of its buffers before block k + 2 is laid out in them)
        if (ok && !kept) f_post = async(launch::async, post, k);
    }
    if (f_post.valid()) f_post.get();
    if (kept && P.cluster && ok) ok = cluster_finish(G, g);
    { lock_guard<mutex> lk(mtx); done = true; }
    cv.notify_one();
    if (P.verbosity >= 2 && ok) {
        cerr << "LZ matching done (" << (n + tile - 1) / tile << " blocks of " << tile << " rows); the last rows are being written" << endl;
        for (size_t d = 0; d < devs.size(); ++d) print_gpu_timing(devs[d], t_sum[d], true, d == 0 && devs.size() > 1 ? &t_gather : nullptr);
        for (size_t d = 0; d < devs.size(); ++d) {
            lzani_residency_info ri;
            if (E.group_get_residency(G, (uint32_t)d, &ri) == LZANI_OK) print_residency(devs[d], ri, r_tiles[d], r_uploads[d], r_upload_ms[d]);
        }
        if (kept) print_kept(k_sum);
    }
    emitter.join();
    return W.close() && ok;
}

// The filter's rows sorted (as PairTable::init_sparse would sort them); whether every row then ascends strictly, which the
// engine's kept form asks for (a kmer-db file that names a pair twice: the filter stays on the host).
static bool lists_ascend(Filter& flt)
{
    bool strict = true;
    for (auto& row : flt.rows) {
        sort(row.begin(), row.end());
        strict = strict && adjacent_find(row.begin(), row.end()) == row.end();
    }
    return strict;
}
