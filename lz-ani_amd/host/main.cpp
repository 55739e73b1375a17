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
// --cluster <single|greedy-first|greedy-best> clusters the pairs the output filter keeps (include/lzani.h, "clustering the
// kept pairs") and writes one line per genome to --cluster-out: on the device where the filter is applied there
// (lzani_group_cluster_*), else by the sequential statement of lzani_cluster_plan.h over the emitter's own lines.
#include <dlfcn.h>

#include <chrono>
#include <condition_variable>
#include <deque>
#include <cstdlib>
#include <fstream>
#include <future>
#include <iterator>
#include <sstream>
#include <thread>

#include "emit.h"
#include "ingest.h"

using namespace host;
using namespace std;

static const char* VER = "1.2.3";
static const char* INFO = "lz-ani 1.2.3 (2024-11-02) by Sebastian Deorowicz, Adam Gudys -- MI355X (gfx950) HIP engine";

struct Params {
    uint32_t verbosity = 1, threads = 0;
    lzani_params lz;
    bool multisample = true, in_percent = false, single_txt = false;
    double filter_thr = 0;
    vector<string> inputs;
    bool query2ref = false;                                 // mode query2ref: the genomes of query_inputs against those of inputs
    vector<string> query_inputs;
    bool query_given = false;                               // a --query-* flag was read
    string out, out_ids, out_aln, filter_fn, out_format = "standard";
    vector<Comp> comps;
    uint64_t flt_mask = 0;
    double flt_vals[16] = {0};
    int gpus = 1, device = 0;
    uint64_t gpu_mem = 0;                                   // --gpu-mem: genome-memory limit per GPU (0: automatic)
    string results_out, results_in;
    bool flt_kmers = false;                                 // --flt-kmers: the filter rows come from the device k-mer prefilter
    int flt_k = 0;
    string flt_fraction_arg;                                // --flt-kmers-fraction as given; checked after the flags are read
    double flt_fraction = 1;
    string flt_counting_arg;                                // --flt-kmers-counting as given; checked after the flags are read
    int flt_counting = LZANI_PF_COUNTING_AUTO;
    string cluster_arg, cluster_out, cluster_measure_arg;  // --cluster, --cluster-out, --cluster-measure as given
    bool cluster = false, cluster_reps = false;             // --cluster given; --cluster-representatives
    int cluster_algo = LZANI_CLUSTER_SINGLE, cluster_measure = LZANI_CLUSTER_TANI;
};

static Params P;

static string parse_output_format(const string& of)          // params.h:169-198
{
    P.comps.clear();
    vector<string> names;
    for (const auto& x : split(of, ',')) {
        auto m = comp_metas().find(x);
        if (m == comp_metas().end()) names.push_back(x);
        else for (const auto& y : split(m->second, ',')) names.push_back(y);
    }
    for (const auto& x : names) {
        auto p = comp_names().find(x);
        if (p == comp_names().end()) return x;
        P.comps.push_back(p->second);
    }
    return "";
}

// --gpu-mem: bytes, with an optional K, M or G suffix (powers of 1024); false for anything else
static bool parse_size(const string& v, uint64_t& out)
{
    size_t k = 0;
    uint64_t x = 0;
    while (k < v.size() && isdigit((unsigned char)v[k])) {
        const uint64_t d = (uint64_t)(v[k++] - '0');
        if (x > (UINT64_MAX - d) / 10) return false;
        x = x * 10 + d;
    }
    if (k == 0) return false;
    int shift = 0;
    if (k + 1 == v.size()) {
        const char u = (char)toupper((unsigned char)v[k]);
        shift = u == 'K' ? 10 : u == 'M' ? 20 : u == 'G' ? 30 : -1;
        if (shift < 0) return false;
    } else if (k != v.size()) return false;
    if (shift && x > (UINT64_MAX >> shift)) return false;
    out = x << shift;
    return true;
}

static void usage()
{
    cerr << INFO << "\n"
         << "Tool for rapid determination of similarities among sets of DNA sequences\n"
         << "Usage:\nlz-ani <mode> [options]\nModes:\n  all2all                        - all to all\n"
         << "  query2ref                      - every query (--query-*) against every reference (--in-*): the cross pairs only\n"
         << "Options - input specification:\n"
         << "      --in-fasta <file_name>     - FASTA file (for multisample-fasta mode)\n"
         << "      --in-txt <file_name>       - text file with FASTA file names\n"
         << "      --in-dir <path>            - directory with FASTA files\n"
         << "      --query-fasta <file_name>  - query2ref: FASTA file with the queries\n"
         << "      --query-txt <file_name>    - query2ref: text file with the queries' FASTA file names\n"
         << "      --query-dir <path>         - query2ref: directory with the queries' FASTA files\n"
         << "      --multisample-fasta <bool> - multi sample FASTA input (default: true)\n"
         << "      --flt-kmerdb <fn> <float>  - filtering file (kmer-db output) and threshold\n"
         << "      --flt-kmers <k> <float>    - filter built on the GPU instead of read from a file: pairs whose shared canonical k-mers (8 <= k <= 31)\n"
         << "                                   are at least <float> of the smaller genome's k-mer set (not with --flt-kmerdb)\n"
         << "      --flt-kmers-fraction <float> - fraction of the k-mers sampled for --flt-kmers, in (0, 1] (default: 1)\n"
         << "      --flt-kmers-counting <auto|dense|sparse> - where --flt-kmers counts shared k-mers: a matrix of all pairs, or a table of\n"
         << "                                   the pairs that share one (default: auto, the table where the matrix needs several tiles)\n"
         << "Options - output specification:\n"
         << "  -o, --out <file_name>          - output file name\n"
         << "      --out-ids <file_name>      - output file name for ids file (optional)\n"
         << "      --out-alignment <file_name>- output file name for ids file (optional)\n"
         << "      --out-in-percent <bool>    - output in percent (default: false)\n"
         << "      --out-type <type>          - one of:\n"
         << "                                   tsv - two tsv files with: results defined by --out-format and sequence ids (default)\n"
         << "                                   single-txt - combined results in single txt file\n"
         << "      --out-format <type>        - comma-separated list of values: \n"
         << "                                   query,reference,qidx,ridx,qlen,rlen,tani,gani,ani,qcov,rcov,len_ratio,nt_match,nt_mismatch,num_alns\n"
         << "                                   you can include also meta-names:\n";
    for (auto& kv : comp_metas()) cerr << "                                   " << kv.first << "=" << kv.second << "\n";
    cerr << "                                   (default: standard)\n"
         << "      --out-filter <par> <float> - store only results with <par> (can be: tani, gani, ani, cov) at least <float>; can be used multiple times\n"
         << "      --cluster <algorithm>      - all2all: cluster the pairs that --out-filter keeps; one of single (connected components),\n"
         << "                                   greedy-first (first representative, as CD-HIT), greedy-best (most similar representative, as UCLUST)\n"
         << "      --cluster-out <file_name>  - output file of --cluster: one line per sequence, its id and its cluster number\n"
         << "      --cluster-measure <type>   - the similarity greedy-best compares: tani, gani or ani (default: tani)\n"
         << "      --cluster-representatives  - write the representative's id instead of the cluster number\n"
         << "Options - LZ-parsing-related:\n"
         << "  -a, --mal <int>                - min. anchor length (default: 11)\n"
         << "  -s, --msl <int>                - min. seed length (default: 7)\n"
         << "  -r, --mrd <int>                - max. dist. between approx. matches in reference (default: 40)\n"
         << "  -q, --mqd <int>                - max. dist. between approx. matches in query (default: 40)\n"
         << "  -g, --reg <int>                - min. considered region length (default: 35)\n"
         << "      --aw <int>                 - approx. window length (default: 15)\n"
         << "      --am <int>                 - max. no. of mismatches in approx. window (default: 7)\n"
         << "      --ar <int>                 - min. length of run ending approx. extension (default: 3)\n"
         << "Options - other:\n"
         << "  -t, --threads <int>            - no of host threads; 0 means auto-detect (default: 0)\n"
         << "  -V, --verbose <int>            - verbosity level (default: 1)\n"
         << "      --gpus <int>               - number of GPUs to shard the reference rows over (default: 1)\n"
         << "      --gpu-mem <size>           - genome-memory limit per GPU in bytes, suffix K/M/G allowed; larger genome sets\n"
         << "                                   stay in host memory and run in tiles of genome blocks (default: 0 = automatic);\n"
         << "                                   with --flt-kmers also the size of the filter's staging buffer: the genomes are\n"
         << "                                   then streamed from host memory in slices of at most <size> bytes\n"
         << "      --device <int>             - first HIP device ordinal (default: 0)\n";
}

static bool parse_bool(const char* v, bool& out) { if (v == "true"s) out = true; else if (v == "false"s) out = false; else return false; return true; }

// Mirrors parse_params (lz-ani.cpp:105-336), including its return/exit conventions.
static bool parse_params(int argc, char** argv)
{
    if (argc == 2 && argv[1] == "--version"s) { cerr << VER << endl; return true; }
    if (argc < 3) { usage(); return false; }
    if (argv[1] == "query2ref"s) P.query2ref = true;
    else if (argv[1] != "all2all"s) { cerr << "Unknown mode: " << argv[1] << endl; usage(); return false; }
    lzani_params& z = P.lz;
    for (int i = 2; i < argc;) {
        string par = argv[i];
        auto has = [&](int k) { return i + k < argc; };
        const bool qry = par.rfind("--query-", 0) == 0;       // the same three sources for either side
        vector<string>& inputs = qry ? P.query_inputs : P.inputs;
        const string src = qry ? "--in-" + par.substr(8) : par;
        if (qry && has(1)) P.query_given = true;
        if (src == "--in-txt" && has(1)) {
            ifstream ifs(argv[i + 1]);
            if (!ifs.is_open()) { cerr << "Cannot open file: " << argv[i + 1] << endl; return false; }
            inputs.assign(istream_iterator<string>(ifs), istream_iterator<string>());
            if (inputs.empty()) return false;
            i += 2;
        } else if (src == "--in-dir" && has(1)) {
            try {
                inputs.clear();
                for (const auto& fs : filesystem::directory_iterator(filesystem::path(argv[i + 1]))) inputs.push_back(fs.path().string());
            } catch (...) { cerr << "Non-existing directory: " << argv[i + 1] << endl; return false; }
            if (inputs.empty()) return false;
            i += 2;
        } else if (src == "--in-fasta" && has(1)) { inputs.assign(1, argv[i + 1]); i += 2; }
        else if ((par == "-o" || par == "--out") && has(1)) { P.out = argv[i + 1]; i += 2; }
        else if (par == "--out-ids" && has(1)) { P.out_ids = argv[i + 1]; i += 2; }
        else if (par == "--out-alignment" && has(1)) { P.out_aln = argv[i + 1]; i += 2; }
        else if ((par == "-t" || par == "--threads") && has(1)) { P.threads = (uint32_t)atoi(argv[i + 1]); i += 2; }
        else if ((par == "-s" || par == "--msl") && has(1)) { z.min_seed_len = atoi(argv[i + 1]); i += 2; }
        else if ((par == "-a" || par == "--mal") && has(1)) { z.min_anchor_len = atoi(argv[i + 1]); i += 2; }
        else if ((par == "-r" || par == "--mrd") && has(1)) { z.max_dist_in_ref = atoi(argv[i + 1]); i += 2; }
        else if ((par == "-q" || par == "--mqd") && has(1)) { z.max_dist_in_query = atoi(argv[i + 1]); i += 2; }
        else if ((par == "-g" || par == "--reg") && has(1)) { z.min_region_len = atoi(argv[i + 1]); i += 2; }
        else if (par == "--aw" && has(1)) { z.approx_window = atoi(argv[i + 1]); i += 2; }
        else if (par == "--am" && has(1)) { z.approx_mismatches = atoi(argv[i + 1]); i += 2; }
        else if (par == "--ar" && has(1)) { z.approx_run_len = atoi(argv[i + 1]); i += 2; }
        else if (par == "--flt-kmerdb" && has(2)) { P.filter_fn = argv[i + 1]; P.filter_thr = atof(argv[i + 2]); i += 3; }
        else if (par == "--flt-kmers" && has(2)) { P.flt_kmers = true; P.flt_k = atoi(argv[i + 1]); P.filter_thr = atof(argv[i + 2]); i += 3; }
        else if (par == "--flt-kmers-fraction" && has(1)) { P.flt_fraction_arg = argv[i + 1]; i += 2; }
        else if (par == "--flt-kmers-counting" && has(1)) { P.flt_counting_arg = argv[i + 1]; i += 2; }
        else if ((par == "-V" || par == "--verbose") && has(1)) { P.verbosity = (uint32_t)atoi(argv[i + 1]); i += 2; }
        else if (par == "--out-type" && has(1)) {
            string t = argv[i + 1];
            if (t == "single-txt") P.single_txt = true;
            else if (t == "tsv") P.single_txt = false;
            else { cerr << "Unknown output-type: " << t << endl; usage(); exit(0); }
            i += 2;
        } else if (par == "--out-format" && has(1)) {
            string bad = parse_output_format(argv[i + 1]);
            if (!bad.empty()) { cerr << "Unknown output-format component: " << bad; return false; }
            P.out_format = argv[i + 1];
            i += 2;
        } else if (par == "--out-filter" && has(2)) {
            static const map<string, Comp> flt = {{"tani", Comp::tani}, {"gani", Comp::gani}, {"ani", Comp::ani}, {"qcov", Comp::qcov}, {"rcov", Comp::rcov}};
            auto p = flt.find(argv[i + 1]);
            if (p == flt.end()) { cerr << "Unknown output-filter component: " << argv[i + 1] << " " << argv[i + 2] << endl; return false; }
            P.flt_mask |= 1ull << (uint32_t)p->second;
            P.flt_vals[(int)p->second] = atof(argv[i + 2]);
            i += 3;
        } else if (par == "--multisample-fasta" && has(1)) {
            if (!parse_bool(argv[i + 1], P.multisample)) { cerr << "Unknown value for --multisample-fasta: " << argv[1] << endl; return false; }
            i += 2;
        } else if (par == "--out-in-percent" && has(1)) {
            if (!parse_bool(argv[i + 1], P.in_percent)) { cerr << "Unknown value for --out-in-percent: " << argv[1] << endl; return false; }
            i += 2;
        } else if (par == "--gpus" && has(1)) { P.gpus = max(1, atoi(argv[i + 1])); i += 2; }
        else if (par == "--gpu-mem" && has(1)) {
            if (!parse_size(argv[i + 1], P.gpu_mem)) {
                cerr << "Invalid value for --gpu-mem: " << argv[i + 1] << " (bytes, with an optional K, M or G suffix)" << endl;
                exit(1);
            }
            i += 2;
        }
        else if (par == "--device" && has(1)) { P.device = atoi(argv[i + 1]); i += 2; }
        else if (par == "--results-out" && has(1)) { P.results_out = argv[i + 1]; i += 2; }
        else if (par == "--results-in" && has(1)) { P.results_in = argv[i + 1]; i += 2; }
        else if (par == "--cluster" && has(1)) { P.cluster = true; P.cluster_arg = argv[i + 1]; i += 2; }
        else if (par == "--cluster-out" && has(1)) { P.cluster_out = argv[i + 1]; i += 2; }
        else if (par == "--cluster-measure" && has(1)) { P.cluster_measure_arg = argv[i + 1]; i += 2; }
        else if (par == "--cluster-representatives") { P.cluster_reps = true; i += 1; }
        else { cerr << "Unknown parameter: " << argv[i] << endl; usage(); exit(1); }
    }
    // query2ref: what it does not take, and what only it takes
    if (P.query2ref && !P.filter_fn.empty()) { cerr << "--flt-kmerdb cannot be used with query2ref (use --flt-kmers)" << endl; exit(1); }
    if (!P.query2ref && P.query_given) { cerr << "--query-fasta, --query-txt and --query-dir belong to the mode query2ref" << endl; exit(1); }
    if (P.query2ref && P.query_inputs.empty()) { cerr << "Query file names not provided (--query-fasta, --query-txt or --query-dir)" << endl; exit(1); }
    // The device k-mer prefilter: refused here, before any input is read
    if (P.flt_kmers && !P.filter_fn.empty()) { cerr << "--flt-kmers and --flt-kmerdb cannot be used together" << endl; exit(1); }
    if (P.flt_kmers && (P.flt_k < 8 || P.flt_k > 31)) {
        cerr << "Unsupported value: --flt-kmers " << P.flt_k << " (k-mer lengths 8 .. 31 are supported)" << endl;
        exit(1);
    }
    if (!P.flt_fraction_arg.empty() && !parse_fraction(P.flt_fraction_arg.c_str(), P.flt_fraction)) {
        cerr << "Invalid value for --flt-kmers-fraction: " << P.flt_fraction_arg << " (a number in (0, 1])" << endl;
        exit(1);
    }
    if (!P.flt_counting_arg.empty()) {
        if (P.flt_counting_arg == "auto") P.flt_counting = LZANI_PF_COUNTING_AUTO;
        else if (P.flt_counting_arg == "dense") P.flt_counting = LZANI_PF_COUNTING_DENSE;
        else if (P.flt_counting_arg == "sparse") P.flt_counting = LZANI_PF_COUNTING_SPARSE;
        else {
            cerr << "Invalid value for --flt-kmers-counting: " << P.flt_counting_arg << " (auto, dense or sparse)" << endl;
            exit(1);
        }
    }
    // --cluster: refused here, before any input is read
    if (!P.cluster && (!P.cluster_out.empty() || !P.cluster_measure_arg.empty() || P.cluster_reps)) {
        cerr << "--cluster-out, --cluster-measure and --cluster-representatives belong to --cluster" << endl;
        exit(1);
    }
    if (P.cluster) {
        static const map<string, int> algos = {{"single", LZANI_CLUSTER_SINGLE}, {"greedy-first", LZANI_CLUSTER_GREEDY_FIRST}, {"greedy-best", LZANI_CLUSTER_GREEDY_BEST}};
        static const map<string, int> measures = {{"tani", LZANI_CLUSTER_TANI}, {"gani", LZANI_CLUSTER_GANI}, {"ani", LZANI_CLUSTER_ANI}};
        const auto a = algos.find(P.cluster_arg);
        if (a == algos.end()) { cerr << "Unknown value for --cluster: " << P.cluster_arg << " (single, greedy-first or greedy-best)" << endl; exit(1); }
        P.cluster_algo = a->second;
        const auto m = measures.find(P.cluster_measure_arg.empty() ? "tani" : P.cluster_measure_arg);
        if (m == measures.end()) { cerr << "Unknown value for --cluster-measure: " << P.cluster_measure_arg << " (tani, gani or ani)" << endl; exit(1); }
        P.cluster_measure = m->second;
        if (P.cluster_out.empty()) { cerr << "--cluster needs --cluster-out <file_name>" << endl; exit(1); }
        if (P.query2ref) { cerr << "--cluster belongs to the mode all2all (query2ref compares two sets)" << endl; exit(1); }
        if (P.single_txt) { cerr << "--cluster cannot be used with --out-type single-txt (it takes no output filter)" << endl; exit(1); }
        if (!P.flt_mask) { cerr << "--cluster needs an --out-filter: the pairs it keeps are the edges of the graph" << endl; exit(1); }
    }
    if (P.inputs.empty()) { cerr << "Input file names not provided\n"; return false; }
    // The engine's parameter envelope (lz-ani_amd/csrc/lzani_layout.h: params_supported).  The reference accepts any
    // ints here (lz-ani.cpp:205-260); values outside the envelope are refused before any file is read.
    struct { const char* flag; int v, lo, hi; } env[] = {
        {"--msl", z.min_seed_len, 1, 32}, {"--mal", z.min_anchor_len, 1, 32}, {"--mrd", z.max_dist_in_ref, 0, 1 << 20},
        {"--mqd", z.max_dist_in_query, 0, 64}, {"--aw", z.approx_window, 1, 64}, {"--ar", z.approx_run_len, -(1 << 30), 64},
        {"--am", z.approx_mismatches, 0, 1 << 30}};
    for (auto& e : env)
        if (e.v < e.lo || e.v > e.hi) {
            cerr << "Unsupported value: " << e.flag << " " << e.v << " (this engine supports " << e.lo << " .. " << e.hi << ")" << endl;
            exit(1);
        }
    if (P.verbosity >= 2 && (z.min_anchor_len > 15 || z.min_seed_len > 15))
        cerr << "Note: --mal / --msl above 15: the engine runs without per-genome k-mer words (generic path, several times slower)" << endl;
    return true;
}

static string params_dump()                                   // CParams::str(), params.h:120-157
{
    stringstream ss;
    const lzani_params& z = P.lz;
    ss << "[params]" << endl
       << "min_anchor_len             : " << z.min_anchor_len << endl
       << "min_seed_len               : " << z.min_seed_len << endl
       << "max_dist_in_ref            : " << z.max_dist_in_ref << endl
       << "max_dist_in_query          : " << z.max_dist_in_query << endl
       << "min_region_len             : " << z.min_region_len << endl
       << "approx_window              : " << z.approx_window << endl
       << "approx_mismatches          : " << z.approx_mismatches << endl
       << "approx_run_len             : " << z.approx_run_len << endl
       << "multisample_fasta          : " << boolalpha << P.multisample << noboolalpha << endl
       << "filter_thr                 : " << P.filter_thr << endl
       << "output_format              : " << P.out_format << endl
       << "output_in_percent          : " << boolalpha << P.in_percent << noboolalpha << endl
       << "no_threads                 : " << P.threads << endl
       << "output_file_name           : " << P.out << endl
       << "output_ids_file_name       : " << P.out_ids << endl
       << "output_alignment_file_name : " << P.out_ids << endl
       << "filter_file_name           : " << P.filter_fn << endl
       << "input_file_names           : ";
    for (size_t i = 0; i + 1 < P.inputs.size(); ++i) ss << P.inputs[i] << ", ";
    ss << P.inputs.back() << endl;
    return ss.str();
}

// ---- the engine, bound at run time -----------------------------------------------------------
struct Engine {
    void* so = nullptr;
    int (*create)(const lzani_params*, int, lzani_ctx**) = nullptr;
    void (*destroy)(lzani_ctx*) = nullptr;
    const char* (*last_error)(const lzani_ctx*) = nullptr;
    int (*set_genomes)(lzani_ctx*, uint32_t, const uint8_t* const*, const uint32_t*) = nullptr;
    int (*get_timing)(const lzani_ctx*, lzani_timing*) = nullptr;
    int (*run_rows_regions)(lzani_ctx*, uint32_t, const uint32_t*, const uint64_t*, const uint32_t*, lzani_result*, lzani_region*,
                            uint64_t, uint64_t*) = nullptr;
    int (*row_costs)(uint32_t, const uint32_t*, const uint64_t*, const uint32_t*, uint32_t, const uint32_t*, uint64_t*) = nullptr;
    int (*partition_rows)(uint32_t, const uint64_t*, uint32_t, uint32_t*) = nullptr;
    int (*group_create)(const lzani_params*, uint32_t, const int*, lzani_group**) = nullptr;
    void (*group_destroy)(lzani_group*) = nullptr;
    const char* (*group_last_error)(const lzani_group*) = nullptr;
    int (*group_set_genomes)(lzani_group*, uint32_t, const uint8_t* const*, const uint32_t*) = nullptr;
    int (*group_run_rows)(lzani_group*, uint32_t, const uint32_t*, const uint64_t*, const uint32_t*, lzani_result*) = nullptr;
    int (*group_get_timing)(const lzani_group*, uint32_t, lzani_timing*, double*) = nullptr;
    int (*set_genome_memory)(lzani_ctx*, uint64_t) = nullptr;
    int (*get_residency)(const lzani_ctx*, lzani_residency_info*) = nullptr;
    int (*group_set_genome_memory)(lzani_group*, uint64_t) = nullptr;
    int (*group_get_residency)(const lzani_group*, uint32_t, lzani_residency_info*) = nullptr;
    int (*prefilter)(lzani_ctx*, int, uint64_t, uint32_t, double, uint64_t*) = nullptr;
    int (*prefilter_fetch)(lzani_ctx*, uint32_t*, uint64_t*, uint32_t*, uint32_t*) = nullptr;
    int (*get_prefilter_info)(const lzani_ctx*, lzani_prefilter_info*) = nullptr;
    int (*prefilter_codes)(lzani_ctx*, uint32_t, const uint8_t* const*, const uint32_t*, int, uint64_t, uint32_t, double, uint64_t, uint64_t*) = nullptr;
    int (*get_prefilter_stream_info)(const lzani_ctx*, lzani_prefilter_stream_info*) = nullptr;
    int (*get_prefilter_pass_info)(const lzani_ctx*, lzani_prefilter_pass_info*) = nullptr;
    int (*prefilter_cross)(lzani_ctx*, int, uint64_t, uint32_t, double, uint32_t, uint64_t*) = nullptr;
    int (*prefilter_codes_cross)(lzani_ctx*, uint32_t, const uint8_t* const*, const uint32_t*, int, uint64_t, uint32_t, double, uint64_t, uint32_t, uint64_t*) = nullptr;
    int (*set_prefilter_counting)(lzani_ctx*, int) = nullptr;
    int (*get_prefilter_sparse_info)(const lzani_ctx*, lzani_prefilter_sparse_info*) = nullptr;
    // the output filter on the device: bound where the library has it (an older one: the filter stays on the host)
    int (*group_run_rows_kept)(lzani_group*, uint32_t, const uint32_t*, const uint64_t*, const uint32_t*, const lzani_out_filter*, const uint32_t*, uint64_t*) = nullptr;
    int (*group_kept_fetch)(lzani_group*, uint64_t, uint64_t, lzani_kept_pair*) = nullptr;
    int (*group_get_kept_info)(const lzani_group*, lzani_kept_info*) = nullptr;
    bool has_kept() const { return group_run_rows_kept && group_kept_fetch && group_get_kept_info; }
    // the cluster stage: bound where the library has it (an older one: the clusters are made on the host)
    int (*group_cluster_begin)(lzani_group*, uint32_t, const uint32_t*, int) = nullptr;
    int (*group_cluster_add_kept)(lzani_group*, uint64_t*) = nullptr;
    int (*group_cluster_run)(lzani_group*, int, uint64_t*) = nullptr;
    int (*group_cluster_fetch)(lzani_group*, uint32_t*, uint32_t*) = nullptr;
    int (*group_get_cluster_info)(const lzani_group*, lzani_cluster_info*) = nullptr;
    bool has_cluster() const { return group_cluster_begin && group_cluster_add_kept && group_cluster_run && group_cluster_fetch && group_get_cluster_info; }
    bool load(const char* argv0)
    {
        vector<string> cand;
        if (const char* e = getenv("LZANI_LIB")) cand.push_back(e);
        error_code ec;
        auto self = filesystem::canonical("/proc/self/exe", ec);
        if (!ec) { cand.push_back((self.parent_path() / "liblzani_hip.so").string()); cand.push_back((self.parent_path().parent_path() / "liblzani_hip.so").string()); }
        (void)argv0;
        cand.push_back("liblzani_hip.so");
        for (auto& c : cand) if ((so = dlopen(c.c_str(), RTLD_NOW | RTLD_LOCAL))) break;
        if (!so) { cerr << "Cannot load liblzani_hip.so (the HIP engine; there is no CPU fallback): " << dlerror() << endl; return false; }
#define BIND(f) f = reinterpret_cast<decltype(f)>(dlsym(so, "lzani_" #f)); if (!f) { cerr << "Missing symbol lzani_" #f << endl; return false; }
        BIND(create) BIND(destroy) BIND(last_error) BIND(set_genomes) BIND(get_timing) BIND(run_rows_regions)
        BIND(row_costs) BIND(partition_rows)
        BIND(group_create) BIND(group_destroy) BIND(group_last_error) BIND(group_set_genomes) BIND(group_run_rows) BIND(group_get_timing)
        BIND(set_genome_memory) BIND(get_residency) BIND(group_set_genome_memory) BIND(group_get_residency)
        BIND(prefilter) BIND(prefilter_fetch) BIND(get_prefilter_info) BIND(prefilter_codes) BIND(get_prefilter_stream_info) BIND(get_prefilter_pass_info)
        BIND(prefilter_cross) BIND(prefilter_codes_cross) BIND(set_prefilter_counting) BIND(get_prefilter_sparse_info)
#undef BIND
#define BIND(f) f = reinterpret_cast<decltype(f)>(dlsym(so, "lzani_" #f));
        BIND(group_run_rows_kept) BIND(group_kept_fetch) BIND(group_get_kept_info)
        BIND(group_cluster_begin) BIND(group_cluster_add_kept) BIND(group_cluster_run) BIND(group_cluster_fetch) BIND(group_get_cluster_info)
#undef BIND
        return true;
    }
};

struct AlnRegion { uint32_t ref, qry; lzani_region r; };

static void genome_views(const vector<Genome>& g, vector<const uint8_t*>& ptr, vector<uint32_t>& len)   // the genomes as the C-ABI takes them
{
    ptr.resize(g.size()); len.resize(g.size());
    for (size_t i = 0; i < g.size(); ++i) { ptr[i] = g[i].codes.data(); len[i] = (uint32_t)g[i].codes.size(); }
}

// The devices of a run on ng GPUs, for the group and the --out-alignment shards alike: P.device + d, or what LZANI_DEVICE_LIST names (rehearsals: "0,0,0")
static vector<int> device_list(int ng)
{
    vector<int> devs;
    if (const char* e = getenv("LZANI_DEVICE_LIST")) for (const auto& x : split(e, ',')) devs.push_back(atoi(x.c_str()));
    else for (int d = 0; d < ng; ++d) devs.push_back(P.device + d);
    if (devs.empty()) devs.push_back(P.device);
    return devs;
}

// A group on devs with the genomes on every device; secs (optional): the seconds of the create and of the genomes.
static bool open_group(const Engine& E, const vector<Genome>& g, lzani_group*& grp, const vector<int>& devs, double* secs = nullptr)
{
    vector<const uint8_t*> ptr; vector<uint32_t> len;
    genome_views(g, ptr, len);
    const auto t_a = chrono::steady_clock::now();
    int rc = E.group_create(&P.lz, (uint32_t)devs.size(), devs.data(), &grp);
    if (rc != LZANI_OK) { cerr << "LZ matching failed: lzani_group_create failed with code " << rc << ": " << E.group_last_error(nullptr) << endl; return false; }
    const auto t_b = chrono::steady_clock::now();
    E.group_set_genome_memory(grp, P.gpu_mem);
    rc = E.group_set_genomes(grp, (uint32_t)g.size(), ptr.data(), len.data());
    if (rc != LZANI_OK) { cerr << "LZ matching failed: " << E.group_last_error(grp) << endl; E.group_destroy(grp); return false; }
    if (secs) { secs[0] = chrono::duration<double>(t_b - t_a).count(); secs[1] = chrono::duration<double>(chrono::steady_clock::now() - t_b).count(); }
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

// --flt-kmers: the filter rows from the device k-mer prefilter on the first device, for the genomes in their reordered
// ids: a context of its own, the stage with min_shared 1 and the threshold as min_ratio, the kept pairs; symmetrised into
// flt.rows like a kmer-db file's.  Without --gpu-mem the genomes become the context's set and lzani_prefilter runs on
// them; with it -- or where that set went out-of-core or did not fit -- the genomes stay in host memory and
// lzani_prefilter_codes streams them through a staging buffer of at most --gpu-mem bytes (automatic without).  n_ref > 0
// (query2ref): the cross form of either, the kept pairs of the references 0 .. n_ref - 1 with the queries behind them.
// --flt-kmers-counting goes to the context before the stage runs.
static bool kmer_filter(const Engine& E, const vector<Genome>& g, Filter& flt, uint32_t n_ref = 0)
{
    const uint32_t n = (uint32_t)g.size();
    auto resident = [&](lzani_ctx* ctx, uint64_t* kept) {
        return n_ref ? E.prefilter_cross(ctx, P.flt_k, sample_max_of(P.flt_fraction), 1, P.filter_thr, n_ref, kept)
                     : E.prefilter(ctx, P.flt_k, sample_max_of(P.flt_fraction), 1, P.filter_thr, kept);
    };
    auto codes = [&](lzani_ctx* ctx, const vector<const uint8_t*>& ptr, const vector<uint32_t>& len, uint64_t slice, uint64_t* kept) {
        return n_ref ? E.prefilter_codes_cross(ctx, n, ptr.data(), len.data(), P.flt_k, sample_max_of(P.flt_fraction), 1, P.filter_thr, slice, n_ref, kept)
                     : E.prefilter_codes(ctx, n, ptr.data(), len.data(), P.flt_k, sample_max_of(P.flt_fraction), 1, P.filter_thr, slice, kept);
    };
    vector<const uint8_t*> ptr; vector<uint32_t> len;
    genome_views(g, ptr, len);
    lzani_ctx* ctx = nullptr;
    int rc = E.create(&P.lz, P.device, &ctx);
    if (rc != LZANI_OK) { cerr << "K-mer filter failed: lzani_create failed with code " << rc << endl; return false; }
    uint64_t kept = 0;
    vector<uint64_t> row_off((size_t)n + 1, 0);
    vector<uint32_t> ids;
    bool streamed = P.gpu_mem != 0;
    E.set_prefilter_counting(ctx, P.flt_counting);
    if (streamed) rc = codes(ctx, ptr, len, P.gpu_mem, &kept);
    else {
        rc = E.set_genomes(ctx, n, ptr.data(), len.data());
        if (rc == LZANI_OK) rc = resident(ctx, &kept);
        if (rc == LZANI_ERR_STATE || rc == LZANI_ERR_NOMEM) {             // the set went out-of-core, or does not fit: a fresh context, streamed
            E.destroy(ctx);
            ctx = nullptr;
            rc = E.create(&P.lz, P.device, &ctx);
            if (rc != LZANI_OK) { cerr << "K-mer filter failed: lzani_create failed with code " << rc << endl; return false; }
            streamed = true;
            E.set_prefilter_counting(ctx, P.flt_counting);
            rc = codes(ctx, ptr, len, 0, &kept);
        }
    }
    if (rc == LZANI_OK) { ids.resize(kept); rc = E.prefilter_fetch(ctx, nullptr, row_off.data(), ids.data(), nullptr); }
    if (rc != LZANI_OK) { cerr << "K-mer filter failed: " << E.last_error(ctx) << endl; E.destroy(ctx); return false; }
    lzani_prefilter_info pi;
    lzani_prefilter_stream_info si;
    lzani_prefilter_pass_info ps;
    lzani_prefilter_sparse_info sp;
    string stream_note, sparse_note;
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
             << " ms, sorts " << pi.sort_ms << " ms, counting " << pi.count_ms << " ms, compaction " << pi.compact_ms << " ms" << sparse_note << stream_note << "\n";
    E.destroy(ctx);
    flt.names.clear();
    filter_from_pairs(n, row_off, ids, flt);
    return true;
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
static void print_group_devices(const Engine& E, lzani_group* grp, const vector<int>& devs)
{
    for (int d = 0; d < (int)devs.size(); ++d) {
        lzani_timing t; lzani_residency_info ri; double gather = 0;
        if (E.group_get_timing(grp, (uint32_t)d, &t, &gather) == LZANI_OK) print_gpu_timing(devs[d], t, false, d == 0 && devs.size() > 1 ? &gather : nullptr);
        if (E.group_get_residency(grp, (uint32_t)d, &ri) == LZANI_OK) print_residency(devs[d], ri, ri.tiles, ri.block_uploads, ri.upload_ms);
    }
}

// store_alignment (lz_matcher.cpp:102-169): one BLAST-tab-like row per region; rows of one pair in
// calc_regions order (length desc, seq_start asc), pairs in (reference, query) order.
static bool store_alignment(const vector<Genome>& g, vector<AlnRegion>& regs)
{
    ofstream o(P.out_aln, ios::binary);
    if (!o.is_open()) { cerr << "Cannot open output file: " << P.out_aln << endl; return false; }
    o << "query\treference\tpident\talnlen\tqstart\tqend\trstart\trend\tnt_match\tnt_mismatch\n";
    sort(regs.begin(), regs.end(), [](const AlnRegion& a, const AlnRegion& b) {
        if (a.ref != b.ref) return a.ref < b.ref;
        if (a.qry != b.qry) return a.qry < b.qry;
        int la = a.r.seq_end - a.r.seq_start, lb = b.r.seq_end - b.r.seq_start;
        if (la != lb) return la > lb;
        return a.r.seq_start < b.r.seq_start;
    });
    string line;
    char num[64];
    for (size_t k = 0; k < regs.size();) {
        size_t k1 = k;
        long mat = 0, lit = 0;
        while (k1 < regs.size() && regs[k1].ref == regs[k].ref && regs[k1].qry == regs[k].qry) { mat += regs[k1].r.num_matches; lit += regs[k1].r.num_mismatches; ++k1; }
        const uint32_t r = regs[k].ref, q = regs[k].qry;
        const int len1 = (int)g[r].codes.size(), len2 = (int)g[q].codes.size();
        bool keep = true;
        if (P.flt_mask != 0) {                                  // the part of --out-filter that applies here (124-137)
            double gani = (double)mat / len2, ani = mat + lit != 0 ? (double)mat / (mat + lit) : 0, qcov = (double)(mat + lit) / len2;
            keep = !(gani < P.flt_vals[(int)Comp::gani]) && !(ani < P.flt_vals[(int)Comp::ani]) && !(qcov < P.flt_vals[(int)Comp::qcov]);
        }
        const int rc_corr = 2 * len1 + 2 * P.lz.max_dist_in_ref + 1;
        for (; k < k1; ++k) {
            if (!keep) continue;
            const lzani_region& x = regs[k].r;
            const int length = x.seq_end - x.seq_start;
            line.clear();
            line += g[q].name; line += '\t'; line += g[r].name; line += '\t';
            line.append(num, real_to_chars(100.0 * x.num_matches / length, num, 6)); line += '\t';
            auto put = [&](long v, char sep) { line += to_string(v); line += sep; };
            put(length, '\t'); put(1 + x.seq_start, '\t'); put(x.seq_end, '\t');
            if (x.ref_start < len1) { put(1 + x.ref_start, '\t'); put(x.ref_end, '\t'); }
            else { put(rc_corr - (1 + x.ref_start), '\t'); put(rc_corr - x.ref_end, '\t'); }
            put(x.num_matches, '\t'); put(x.num_mismatches, '\n');
            o.write(line.data(), (streamsize)line.size());
        }
    }
    return true;
}

// --out-filter as the engine takes it, and whether the device applies it: a two-TSV output, no --out-alignment (its own cut
// stays on the host), no --results-in / --results-out (they carry every pair), numbers for minima (a NaN drops nothing on
// the host and is refused by the engine), and LZANI_OUT_FILTER=host not set.
static lzani_out_filter out_filter_minima()
{
    return lzani_out_filter{P.flt_vals[(int)Comp::tani], P.flt_vals[(int)Comp::gani], P.flt_vals[(int)Comp::ani], P.flt_vals[(int)Comp::qcov], P.flt_vals[(int)Comp::rcov]};
}
static bool out_filter_on_device()
{
    const lzani_out_filter f = out_filter_minima();
    const bool nan = f.min_tani != f.min_tani || f.min_gani != f.min_gani || f.min_ani != f.min_ani || f.min_qcov != f.min_qcov || f.min_rcov != f.min_rcov;
    const char* e = getenv("LZANI_OUT_FILTER");
    return P.flt_mask != 0 && !P.single_txt && P.out_aln.empty() && P.results_in.empty() && P.results_out.empty() && !nan && !(e && e == "host"s);
}

// -V 2: the one line of the device's output filter (a tiled all2all: the sums over its blocks)
static void print_kept(const lzani_kept_info& k)
{
    cerr << "out-filter on the device: " << k.kept_pairs << " pairs, " << k.kept_lines << " lines kept of " << k.leading << " pairs, " << k.unpaired
         << " unpaired, " << k.filter_ms << " ms\n";
}

// --cluster-out: one line per genome in the order of the ids file, its id and its cluster number or its representative's id.
static bool write_clusters(const vector<Genome>& g, const vector<uint32_t>& rep_of, const vector<uint32_t>& cluster_of)
{
    ofstream o(P.cluster_out, ios::binary);
    if (!o.is_open()) { cerr << "Cannot open output file: " << P.cluster_out << endl; return false; }
    o << "object\t" << (P.cluster_reps ? "representative" : "cluster") << "\n";
    for (size_t i = 0; i < g.size(); ++i) {
        o << g[i].name << '\t';
        if (P.cluster_reps) o << g[rep_of[i]].name; else o << cluster_of[i];
        o << '\n';
    }
    o.close();
    return !o.fail();
}

// The device path of --cluster: an empty edge set before the kept calls, the edges of each kept call added behind it, and
// at the end the run, the fetch and the file.
static bool cluster_begin(const Engine& E, lzani_group* grp, const vector<uint32_t>& rlen)
{
    if (E.group_cluster_begin(grp, (uint32_t)rlen.size(), rlen.data(), P.cluster_measure) == LZANI_OK) return true;
    cerr << "Clustering failed: " << E.group_last_error(grp) << endl;
    return false;
}
static bool cluster_add_kept(const Engine& E, lzani_group* grp)
{
    if (E.group_cluster_add_kept(grp, nullptr) == LZANI_OK) return true;
    cerr << "Clustering failed: " << E.group_last_error(grp) << endl;
    return false;
}
static bool cluster_finish(const Engine& E, lzani_group* grp, const vector<Genome>& g)
{
    vector<uint32_t> rep_of(g.size()), cluster_of(g.size());
    if (E.group_cluster_run(grp, P.cluster_algo, nullptr) != LZANI_OK || E.group_cluster_fetch(grp, rep_of.data(), cluster_of.data()) != LZANI_OK) {
        cerr << "Clustering failed: " << E.group_last_error(grp) << endl;
        return false;
    }
    lzani_cluster_info ci;
    if (P.verbosity >= 2 && E.group_get_cluster_info(grp, &ci) == LZANI_OK)
        cerr << "clusters on the device: " << ci.clusters << " of " << ci.n << " sequences (" << ci.singletons << " singletons, the largest of " << ci.largest
             << ") from " << ci.edges << " pairs, " << ci.rounds << " round(s), add " << ci.add_ms << " ms, run " << ci.run_ms << " ms\n";
    return write_clusters(g, rep_of, cluster_of);
}

// The host path of --cluster: the pairs of which the emitter lets a line through, by the sequential statement.
static bool cluster_on_host(const vector<Genome>& g, const PairTable& T, const EmitParams& ep)
{
    vector<lzani_cluster_edge> edges;
    cluster_edges_of(report_lengths(g, ep.mrd), T, make_cuts(ep), P.cluster_measure, edges);
    vector<uint32_t> rep_of(g.size()), cluster_of(g.size());
    uint32_t k = 0;
    if (!g.empty() && lzani::cluster_host((uint32_t)g.size(), edges.data(), edges.size(), P.cluster_algo, rep_of.data(), cluster_of.data(), &k) != LZANI_OK) {
        cerr << "Clustering failed" << endl;
        return false;
    }
    if (P.verbosity >= 2) cerr << "clusters on the host: " << k << " of " << g.size() << " sequences from " << edges.size() << " pairs\n";
    return write_clusters(g, rep_of, cluster_of);
}

// The kept records of the group's last kept call, fetched in pieces of a million (36 MB) and written as they come.
static bool emit_kept_result(const Engine& E, lzani_group* grp, const vector<Genome>& g, ResultWriter& W, uint64_t n_kept)
{
    vector<lzani_kept_pair> rec;
    for (uint64_t first = 0; first < n_kept; first += rec.size()) {
        rec.resize((size_t)min<uint64_t>(n_kept - first, 1u << 20));
        if (E.group_kept_fetch(grp, first, rec.size(), rec.data()) != LZANI_OK) { cerr << "LZ matching failed: " << E.group_last_error(grp) << endl; return false; }
        W.emit_kept(g, rec.data(), rec.size());
    }
    return true;
}

// do_matching with the output filter on the device, untiled: the rows in ascending id order (lists ascending), one
// lzani_group_run_rows_kept with the printed lengths, and the kept records -- in the order of the output file -- written
// as they are fetched.  No PairTable.  flt's rows are sorted by the caller (lists_ascend).
static bool do_matching_kept(const Engine& E, const vector<Genome>& g, Filter& flt, const EmitParams& ep)
{
    const uint32_t n = (uint32_t)g.size();
    if (P.verbosity >= 1) cerr << "All2all sparse" << endl;
    const bool dense = flt.empty();
    vector<uint32_t> ref_ids(n), qids;
    vector<uint64_t> row_off((size_t)n + 1, 0);
    for (uint32_t r = 0; r < n; ++r) { ref_ids[r] = r; row_off[r + 1] = row_off[r] + (dense ? (uint64_t)n - 1 : flt.rows[r].size()); }
    if (!dense) {
        qids.reserve(row_off[n] + 1);
        for (auto& row : flt.rows) qids.insert(qids.end(), row.begin(), row.end());
        vector<vector<uint32_t>>().swap(flt.rows);
        qids.push_back(0);                                      // (lists that are all empty are still lists: never null)
    }
    const vector<int> devs = device_list(max(1, min<int>(P.gpus, (int)max<uint32_t>(n, 1))));
    lzani_group* grp = nullptr; double secs[2];
    if (!open_group(E, g, grp, devs, secs)) return false;
    const lzani_out_filter f = out_filter_minima();
    const vector<uint32_t> rlen = report_lengths(g, ep.mrd);   // the lengths the TSV prints
    uint64_t n_kept = 0;
    if (P.cluster && !cluster_begin(E, grp, rlen)) { E.group_destroy(grp); return false; }
    const auto t_c = chrono::steady_clock::now();
    const int rc = E.group_run_rows_kept(grp, n, ref_ids.data(), row_off.data(), dense ? nullptr : qids.data(), &f, rlen.data(), &n_kept);
    if (P.verbosity >= 2)
        cerr << "engine: create " << secs[0] << " s, genomes to the device " << secs[1] << " s, matching " << chrono::duration<double>(chrono::steady_clock::now() - t_c).count() << " s\n";
    if (rc != LZANI_OK) { cerr << "LZ matching failed: " << E.group_last_error(grp) << endl; E.group_destroy(grp); return false; }
    if (P.verbosity >= 2) {
        print_group_devices(E, grp, devs);
        lzani_kept_info ki;
        if (E.group_get_kept_info(grp, &ki) == LZANI_OK) print_kept(ki);
    }
    if (P.cluster && !(cluster_add_kept(E, grp) && cluster_finish(E, grp, g))) { E.group_destroy(grp); return false; }
    if (P.verbosity >= 1) cerr << "Storing results" << endl;
    ResultWriter W;
    const bool ok = W.open(g, ep) && emit_kept_result(E, grp, g, W, n_kept);
    E.group_destroy(grp);
    return ok && W.close();
}

// do_matching (lz_matcher.cpp:172-277).  The reference's workers pull reference rows off an atomic counter and
// run one CParser each; here the whole row table goes to the engine in one call: lzani_group_run_rows deals
// the rows over the GPUs of the group (cyclic for dense rows, LPT for filtered ones), runs them, gathers the
// shards over RCCL on the first GPU and copies the results out once, CSR-aligned with T.
static bool do_matching(const Engine& E, const vector<Genome>& g, Filter& flt, PairTable& T, vector<AlnRegion>* aln)
{
    const uint32_t n = (uint32_t)g.size();
    if (P.verbosity >= 1) cerr << "All2all sparse" << endl;
    if (flt.empty()) T.init_dense(n);
    else { T.init_sparse(flt.rows); vector<vector<uint32_t>>().swap(flt.rows); }   // the reference clears filter rows as it goes (266-267)
    vector<uint32_t> ref_ids(n);
    for (uint32_t i = 0; i < n; ++i) ref_ids[i] = i;
    const uint32_t* qids = T.dense ? nullptr : T.query_ids.data();
    const vector<int> devs = device_list(max(1, min<int>(P.gpus, (int)max<uint32_t>(n, 1))));

    if (!aln) {
        lzani_group* grp = nullptr; double secs[2];
        if (!open_group(E, g, grp, devs, secs)) return false;
        const auto t_c = chrono::steady_clock::now();
        const int rc = E.group_run_rows(grp, n, ref_ids.data(), T.row_off.data(), qids, T.res.data());
        if (P.verbosity >= 2)
            cerr << "engine: create " << secs[0] << " s, genomes to the device " << secs[1] << " s, matching " << chrono::duration<double>(chrono::steady_clock::now() - t_c).count() << " s\n";
        if (rc != LZANI_OK) { cerr << "LZ matching failed: " << E.group_last_error(grp) << endl; E.group_destroy(grp); return false; }
        if (P.verbosity >= 2) print_group_devices(E, grp, devs);
        E.group_destroy(grp);
        return true;
    }

    // --out-alignment: the per-pair region lists are variable-length, so every shard comes back through host memory
    // (lzani_run_rows_regions, a context per entry of the device list); the rows are dealt by the group's partition.
    vector<const uint8_t*> ptr; vector<uint32_t> len;
    genome_views(g, ptr, len);
    vector<uint32_t> part(n);
    vector<uint64_t> cost(T.dense ? 0 : n);
    if (!T.dense) E.row_costs(n, ref_ids.data(), T.row_off.data(), qids, n, len.data(), cost.data());
    E.partition_rows(n, T.dense ? nullptr : cost.data(), (uint32_t)devs.size(), part.data());
    vector<string> errs(devs.size());
    mutex mtx;
    auto shard = [&](int d) {
        lzani_ctx* ctx = nullptr;
        int rc = E.create(&P.lz, devs[d], &ctx);
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
        if (rc != LZANI_OK) errs[d] = E.last_error(ctx);
        else {
            regs.resize(cnt);
            for (size_t k = 0; k < rows.size(); ++k)
                copy(out.begin() + (ptrdiff_t)row_off[k], out.begin() + (ptrdiff_t)row_off[k + 1], T.res.begin() + (ptrdiff_t)T.row_off[rows[k]]);
            lock_guard<mutex> lck(mtx);
            for (const auto& x : regs) {
                size_t k = upper_bound(row_off.begin(), row_off.end(), x.pair) - row_off.begin() - 1;
                aln->push_back(AlnRegion{rows[k], T.id_at(rows[k], x.pair - row_off[k]), x});
            }
            if (P.verbosity >= 2) {
                lzani_timing t; lzani_residency_info ri;
                if (E.get_timing(ctx, &t) == LZANI_OK) print_gpu_timing(devs[d], t, false, nullptr);
                if (E.get_residency(ctx, &ri) == LZANI_OK) print_residency(devs[d], ri, ri.tiles, ri.block_uploads, ri.upload_ms);
            }
        }
        E.destroy(ctx);
    };
    vector<thread> th;
    for (int d = 1; d < (int)devs.size(); ++d) th.emplace_back(shard, d);
    shard(0);
    for (auto& t : th) t.join();
    for (auto& e : errs) if (!e.empty()) { cerr << "LZ matching failed: " << e << endl; return false; }
    return true;
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
    const vector<int> devs = device_list(max(1, min<int>(P.gpus, (int)max<uint32_t>(n, 1))));
    lzani_group* grp = nullptr;
    if (!open_group(E, g, grp, devs)) return false;

    ResultWriter W;
    if (!W.open(g, ep)) { E.group_destroy(grp); return false; }
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
    const lzani_out_filter flt_min = out_filter_minima();
    const bool cluster = kept && P.cluster;                    // every unordered pair lies in exactly one block: its edges are added there
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
    bool ok = !cluster || cluster_begin(E, grp, W.lengths());
    future<void> f_build, f_post;
    build(0);
    for (uint32_t k = 0; k < n_blocks && ok; ++k) {
        Block& B = blk[k % 3];
        if (k + 1 < n_blocks) f_build = async(launch::async, build, k + 1);
        if (!B.rows.empty()) {
            uint64_t n_kept = 0;
            const int rc = kept ? E.group_run_rows_kept(grp, (uint32_t)B.rows.size(), B.rows.data(), B.off.data(), B.q.data(), &flt_min, W.lengths().data(), &n_kept)
                                : E.group_run_rows(grp, (uint32_t)B.rows.size(), B.rows.data(), B.off.data(), B.q.data(), B.out.data());
            if (rc != LZANI_OK) { cerr << "LZ matching failed: " << E.group_last_error(grp) << endl; ok = false; }
            if (cluster && ok) ok = cluster_add_kept(E, grp);       // before the next block's kept call replaces the records
            if (kept && ok) {
                vector<lzani_kept_pair> rec((size_t)n_kept);
                lzani_kept_info ki;
                if (E.group_kept_fetch(grp, 0, n_kept, rec.data()) != LZANI_OK || E.group_get_kept_info(grp, &ki) != LZANI_OK) {
                    cerr << "LZ matching failed: " << E.group_last_error(grp) << endl; ok = false;
                } else {
                    k_sum.entries += ki.entries; k_sum.leading += ki.leading; k_sum.unpaired += ki.unpaired; k_sum.kept_pairs += ki.kept_pairs;
                    k_sum.kept_lines += ki.kept_lines; k_sum.filter_ms += ki.filter_ms;
                    { lock_guard<mutex> lk(mtx); ready_kept.push_back(move(rec)); }
                    cv.notify_one();
                }
            }
            for (size_t d = 0; d < devs.size() && ok; ++d) {
                lzani_timing t; double gather = 0;
                if (E.group_get_timing(grp, (uint32_t)d, &t, &gather) == LZANI_OK) {
                    t_sum[d].index_ms += t.index_ms; t_sum[d].pairs_ms += t.pairs_ms; t_sum[d].cand_ms += t.cand_ms + t.kmers_ms; t_sum[d].pairs += t.pairs;
                    if (d == 0) t_gather += gather;
                }
                lzani_residency_info ri;
                if (E.group_get_residency(grp, (uint32_t)d, &ri) == LZANI_OK) { r_tiles[d] += ri.tiles; r_uploads[d] += ri.block_uploads; r_upload_ms[d] += ri.upload_ms; }
            }
        }
        if (f_build.valid()) f_build.get();
        if (f_post.valid()) f_post.get();                         // (block k - 1 is out of its buffers before block k + 2 is laid out in them)
        if (ok && !kept) f_post = async(launch::async, post, k);
    }
    if (f_post.valid()) f_post.get();
    if (cluster && ok) ok = cluster_finish(E, grp, g);
    { lock_guard<mutex> lk(mtx); done = true; }
    cv.notify_one();
    if (P.verbosity >= 2 && ok) {
        cerr << "LZ matching done (" << (n + tile - 1) / tile << " blocks of " << tile << " rows); the last rows are being written" << endl;
        for (size_t d = 0; d < devs.size(); ++d) print_gpu_timing(devs[d], t_sum[d], true, d == 0 && devs.size() > 1 ? &t_gather : nullptr);
        for (size_t d = 0; d < devs.size(); ++d) {
            lzani_residency_info ri;
            if (E.group_get_residency(grp, (uint32_t)d, &ri) == LZANI_OK) print_residency(devs[d], ri, r_tiles[d], r_uploads[d], r_upload_ms[d]);
        }
        if (kept) print_kept(k_sum);
    }
    emitter.join();
    E.group_destroy(grp);
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

static bool run_all2all(const char* argv0)
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
        if (!E.load(argv0)) return false;
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
    ep.comps = P.comps; ep.filter_mask = P.flt_mask; memcpy(ep.filter_vals, P.flt_vals, sizeof ep.filter_vals);
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
        if (!engine_loaded && !E.load(argv0)) return false;
        // --out-filter on the device where it applies to the TSV, the library has the stage and the filter's lists are sets
        const bool kept = out_filter_on_device() && E.has_kept() && lists_ascend(flt) && (!P.cluster || E.has_cluster());
        clustered = kept && P.cluster;
        if (tiled) {
            if (P.verbosity >= 1) cerr << "Storing results (row blocks, while the matching goes on)" << endl;
            if (!do_matching_tiled(E, g, results, ep, tile, kept)) return false;
        } else if (kept) {
            if (!do_matching_kept(E, g, flt, ep)) return false;
            stored = true;
        } else {
            vector<AlnRegion> aln;
            if (!do_matching(E, g, flt, results, P.out_aln.empty() ? nullptr : &aln)) return false;
            if (!P.out_aln.empty() && !store_alignment(g, aln)) return false;
        }
    }
    stamp(stored ? "LZ matching + storing results" : "LZ matching");
    if (!P.results_out.empty() && !write_raw(P.results_out, results)) return false;

    if (P.cluster && !clustered && !cluster_on_host(g, results, ep)) return false;

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
    if (!run_all2all(argv[0])) { cerr << "Run failed" << endl; exit(1); }
    return 0;
}
