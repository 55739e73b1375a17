// lz-ani (MI355X build) -- the reference's command line on top of the HIP pair engine.
//
// Drop-in surface: /root/reference/src/lz-ani.cpp:39-355 (modes, flags, defaults, exit codes) and the
// stage sequence of CLZMatcher::run_all2all (/root/reference/src/lz_matcher.cpp:582-617):
//   load sequences -> load filter -> check names -> reorder -> LZ matching -> store results.
// The matching stage is one call per GPU into the C-ABI of include/lzani.h (liblzani_hip.so, loaded
// with dlopen so that this binary builds and its ingest/emit code is testable without ROCm present).
// Extras over the reference: --flt-kmers <k> <thr> (the filter rows made on the GPU from the genomes themselves, in place
// of a kmer-db file), the mode query2ref (--query-fasta / --query-txt / --query-dir: a query set against the reference set
// of --in-*, the cross pairs only), --gpus <n> (rows dealt cyclically over n GPUs), --device <id>, --gpu-mem <size>
// (genome-memory limit per GPU: larger sets run out-of-core, in tiles of genome blocks; with --flt-kmers the filter then
// streams the genomes from host memory in slices of at most that size),
// and the test seams --results-out / --results-in (raw int triples of the matching stage).
// --out-filter on a two-TSV output is applied on the device (lzani_group_run_rows_kept): only the pairs of which a line
// passes come back, and the table of all pairs is never made; LZANI_OUT_FILTER=host keeps the filter on the host.
// --out-alignment on one device goes through the region stage (lzani_run_rows_aligned): the regions of the pairs that pass the
// alignment's rule come back in the file's order and are written as they are fetched; with an --out-filter and no --cluster
// the same call is the kept call.  LZANI_OUT_ALN=host, --gpus above 1 and an older library keep the regions' order on the host.
// --cluster <single|greedy-first|greedy-best|set-cover|complete-linkage|leiden-cpm> clusters the pairs the output filter keeps (include/lzani.h,
// "clustering the kept pairs") and writes one line per genome to --cluster-out: on the device where the filter is applied there
// (lzani_group_cluster_*), else by the sequential statement of lzani_cluster_plan.h over the emitter's own lines.
// --cluster-cut <par> <value> cuts the pairs of the --cluster level further at cluster time, and --cluster-level <algorithm>
// <file_name> <cuts> adds a clustering of the same run with a cut and a file of its own (include/lzani.h, "cluster levels"):
// on the device the kept records go into a record store and every level is made from it; the TSV and the ids file never
// depend on either flag.
// This file keeps the raw seams, the stage sequence and main; cli.h holds the command line, engine.h the binding of the
// engine, match.h the stages that call it, emit.h the result files and ingest.h the inputs.
#include "match.h"

// test seams: the matching stage's integers as text, "ref query mat lit comp" per directed pair
static bool write_raw(const string& fn, const PairTable& T)
{
    ofstream o(fn);
    if (!o.is_open()) return false;
    for (uint32_t r = 0; r < T.n; ++r)
        for (uint64_t j = 0; j < T.row_size(r); ++j) {
            const lzani_result& x = T.at(r, j);
            o << r << ' ' << T.id_at(r, j) << ' ' << x.sym_in_matches << ' ' << x.sym_in_literals << ' ' << x.no_components << '\n';
        }
    return true;
}
static bool read_raw(const string& fn, size_t n, PairTable& T)
{
    ifstream in(fn);
    if (!in.is_open()) { cerr << "Cannot open file: " << fn << endl; return false; }
    struct Rec { uint32_t q; lzani_result r; };
    vector<vector<Rec>> rows(n);
    size_t r; Rec x;
    while (in >> r >> x.q >> x.r.sym_in_matches >> x.r.sym_in_literals >> x.r.no_components) { if (r >= n || x.q >= n) return false; rows[r].push_back(x); }
    vector<vector<uint32_t>> ids(n);
    for (size_t k = 0; k < n; ++k) {
        stable_sort(rows[k].begin(), rows[k].end(), [](const Rec& a, const Rec& b) { return a.q < b.q; });
        for (auto& e : rows[k]) ids[k].push_back(e.q);
    }
    T.init_sparse(ids);
    for (size_t k = 0; k < n; ++k) for (size_t j = 0; j < rows[k].size(); ++j) T.res[T.row_off[k] + j] = rows[k][j].r;
    return true;
}

static bool run_all2all()
{
    using clk = chrono::high_resolution_clock;
    vector<pair<clk::time_point, string>> times{{clk::now(), ""}};
    auto stamp = [&](const char* s) { times.emplace_back(clk::now(), s); };

    if (P.verbosity >= 1) cerr << "Loading sequences\n";
    vector<Genome> g;
    if (P.multisample ? !load_multifasta(P.inputs, g) : !load_fasta(P.inputs, (uint32_t)P.lz.max_dist_in_ref, g)) return false;
    if (P.verbosity >= 2) cerr << g.size() << endl;
    vector<Genome> qry;                                     // query2ref: the queries, through the same loader
    if (P.query2ref) {
        if (P.multisample ? !load_multifasta(P.query_inputs, qry) : !load_fasta(P.query_inputs, (uint32_t)P.lz.max_dist_in_ref, qry)) return false;
        if (P.verbosity >= 2) cerr << qry.size() << endl;
        if (g.empty() || qry.empty()) { cerr << "query2ref needs at least one reference and one query sequence" << endl; return false; }
    }
    stamp("Loading sequences");

    Filter flt;
    if (!P.filter_fn.empty()) {
        if (P.verbosity >= 1) cerr << "Loading filter data" << endl;
        if (!load_filter(P.filter_fn, P.filter_thr, flt)) return false;
        if (P.verbosity >= 1) cerr << "Filter size: " << flt.size() << endl;
    }
    stamp("Loading filter");

    if (!flt.empty()) {                                     // compare_sequences (lz_matcher.cpp:43-75)
        bool same = flt.names.size() == g.size();
        for (size_t i = 0; same && i < g.size(); ++i) same = flt.names[i] == g[i].name;
        if (!same) {
            cerr << "seq_sn.size(): " << g.size() << endl << "flt_sn.size(): " << flt.names.size() << endl;
            cerr << (flt.names.size() != g.size() ? "Input sequences and filter sequences sets are of different size!"
                                                  : "Input sequences and filter sequences are different!") << endl;
            return false;
        }
    }
    stamp("Comparing sequence and filter compatibility");

    if (P.verbosity >= 1) cerr << "Reordering sequences" << endl;
    auto map = reorder(g);
    if (!flt.empty()) { if (P.verbosity >= 1) cerr << "Reordering filter" << endl; reorder_filter(flt, map); }
    // query2ref: each side in its own order; the ids are the references, then the queries
    const uint32_t n_ref = P.query2ref ? (uint32_t)g.size() : 0;
    if (P.query2ref) {
        reorder(qry);
        g.insert(g.end(), make_move_iterator(qry.begin()), make_move_iterator(qry.end()));
        qry.clear();
    }
    stamp("Reordering sequences");

    Engine E;
    bool engine_loaded = false;
    if (P.flt_kmers) {
        if (P.verbosity >= 1) cerr << "Building k-mer filter" << endl;
        if (!E.load()) return false;
        engine_loaded = true;
        if (!kmer_filter(E, g, flt, n_ref)) return false;
        if (P.verbosity >= 1) cerr << "Filter size: " << flt.size() << endl;
        stamp("K-mer filter");
    } else if (P.query2ref) {                               // every cross pair, as the kept pairs of a prefilter that drops none
        const uint32_t n = (uint32_t)g.size();
        vector<uint64_t> row_off((size_t)n + 1);
        vector<uint32_t> ids((size_t)n_ref * (n - n_ref));
        for (uint32_t a = 0; a <= n; ++a) row_off[a] = (uint64_t)min(a, n_ref) * (n - n_ref);
        for (size_t e = 0; e < ids.size(); ++e) ids[e] = n_ref + (uint32_t)(e % (n - n_ref));
        filter_from_pairs(n, row_off, ids, flt);
    }

    EmitParams ep;
    ep.out_name = P.out; ep.ids_name = P.out_ids; ep.single_txt = P.single_txt; ep.in_percent = P.in_percent;
    ep.comps = P.comps; ep.filter = out_filter_minima(); ep.filtered = P.flt_mask != 0;
    ep.threads = P.threads; ep.mrd = P.lz.max_dist_in_ref;
    if (P.single_txt) ep.params_dump = params_dump();

    // A large dense all2all runs tiled, the result rows of a block written while the next block is matched
    // (LZANI_TILE_ROWS: rows per block, 0 = never; LZANI_TILE_MIN: genomes from which on)
    uint32_t tile = 1024, tile_min = 4096;
    if (const char* e = getenv("LZANI_TILE_ROWS")) tile = (uint32_t)max(0, atoi(e));
    if (const char* e = getenv("LZANI_TILE_MIN")) tile_min = (uint32_t)max(0, atoi(e));
    const bool tiled = tile > 0 && P.results_in.empty() && P.out_aln.empty() && flt.empty() && g.size() >= tile_min && g.size() > tile;

    PairTable results;
    bool stored = tiled;                                    // the result files are written already
    bool clustered = false;                                 // ... and so is the cluster file (the device path)
    if (!P.results_in.empty()) { if (!read_raw(P.results_in, g.size(), results)) return false; }
    else {
        if (!engine_loaded && !E.load()) return false;
        // --out-filter on the device where it applies to the TSV, the library has the stage and the filter's lists are sets
        bool leiden = false;                                // a level is one of leiden-cpm
        for (const auto& lv : P.levels) leiden = leiden || lv.algo == LZANI_CLUSTER_LEIDEN;
        const bool ascend = lists_ascend(flt);
        // --out-alignment through the device's region stage: one device, a library with the stage, lists that are sets
        const bool aln_dev = out_aln_on_device() && E.has_aligned() && ascend && device_list(g).size() == 1;
        // (with --out-alignment the kept call is the aligned call; with --cluster as well, the filter and the clusters stay on the host)
        const bool kept = out_filter_on_device() && E.has_kept() && ascend && (!P.cluster || (leiden ? E.has_leiden() : E.has_cluster()))
                          && (P.out_aln.empty() || (aln_dev && !P.cluster));
        if (kept && P.cluster && P.levels_on())
            if (const char* sym = E.missing_levels()) { cerr << "Missing symbol " << sym << " (--cluster-cut and --cluster-level need it)" << endl; return false; }
        clustered = kept && P.cluster;
        if (tiled) {
            if (P.verbosity >= 1) cerr << "Storing results (row blocks, while the matching goes on)" << endl;
            if (!do_matching_tiled(E, g, results, ep, tile, kept)) return false;
        } else {
            vector<AlnRegion> aln;
            if (!do_matching(E, g, flt, results, ep, kept, P.out_aln.empty() ? nullptr : &aln, aln_dev)) return false;
            if (!P.out_aln.empty() && !aln_dev && !store_alignment(E, g, aln)) return false;
            stored = kept;                                  // the kept form writes its records as it fetches them
        }
    }
    stamp(stored ? "LZ matching + storing results" : "LZ matching");
    if (!P.results_out.empty() && !write_raw(P.results_out, results)) return false;

    if (P.cluster && !clustered) {
        if (!P.levels_on()) { if (!cluster_on_host(g, results, ep)) return false; }
        else for (const auto& lv : P.levels) if (!cluster_on_host(g, results, ep, &lv)) return false;
    }

    if (!stored) {
        if (P.verbosity >= 1) cerr << "Storing results" << endl;
        if (!store_results(g, results, ep)) return false;
        stamp("Storing results");
    }

    if (P.verbosity > 1) {
        ifstream st("/proc/self/status");
        for (string ln; getline(st, ln);) if (ln.rfind("VmHWM:", 0) == 0) cerr << "Peak RSS " << ln.substr(6) << "\n";
        cerr << "Timings\n";
        for (size_t i = 1; i < times.size(); ++i) cerr << times[i].second << " : " << chrono::duration<double>(times[i].first - times[i - 1].first).count() << "s\n";
        cerr << "Total time: " << chrono::duration<double>(times.back().first - times.front().first).count() << "s\n";
    }
    return true;
}

int main(int argc, char** argv)
{
    P.lz = lzani_params{11, 7, 40, 40, 35, 15, 7, 3};
    parse_output_format("standard");
    if (!parse_params(argc, argv)) return 0;                  // the reference returns 0 here too (lz-ani.cpp:341-342)
    if (argc == 2) return 0;                                  // --version
    if (P.threads == 0) { P.threads = thread::hardware_concurrency(); if (!P.threads) P.threads = 1; }
    if (!run_all2all()) { cerr << "Run failed" << endl; exit(1); }
    return 0;
}
