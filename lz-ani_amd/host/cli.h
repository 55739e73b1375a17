// cli.h -- the command line of the `lz-ani` host binary: the parameters (one global, P), the usage text, the flags and
// their checks, and the parameter dump of the single-txt output.  Uses emit.h (the column names) and ingest.h (split,
// parse_fraction); everything behind it reads P.
//
// Drop-in surface: /root/reference/src/lz-ani.cpp:39-355 (modes, flags, defaults, exit codes).
#pragma once
#include <fstream>
#include <iterator>
#include <sstream>

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
    string flt_max_seqs_arg;                                // --flt-kmers-max-seqs as given; checked after the flags are read
    uint32_t flt_max_seqs = 0;                              // 0: no limit
    string cluster_arg, cluster_out, cluster_measure_arg;  // --cluster, --cluster-out, --cluster-measure as given
    bool cluster = false, cluster_reps = false;             // --cluster given; --cluster-representatives
    int cluster_algo = LZANI_CLUSTER_SINGLE, cluster_measure = LZANI_CLUSTER_TANI;
    string leiden_resolution_arg, leiden_iterations_arg;    // --cluster-leiden-resolution, --cluster-leiden-iterations as given
    double leiden_resolution = 0.7;                         // ... and read: Clusty's defaults
    int leiden_iterations = 2;
    // cluster levels: --cluster-cut <par> <value> as given, and --cluster-level <algorithm> <file_name> <cuts> as given
    vector<pair<string, string>> cluster_cut_args;
    struct LevelArg { string algo, out, cuts; };
    vector<LevelArg> cluster_level_args;
    // ... and read: the level of --cluster (its cut on top of --out-filter) first, then those of --cluster-level, in their order
    struct Level { int algo; string out; lzani_cluster_cut cut; };
    vector<Level> levels;
    bool levels_on() const { return !cluster_cut_args.empty() || !cluster_level_args.empty(); }   // either flag was given
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

// One limit of a cut: par is one of tani, gani, ani, qcov, rcov, len_ratio (a minimum, on the scale of --out-filter's values
// as out_filter_minima() hands them on) or num_alns (a maximum, an integer >= 1).  Empty on success, else what is wrong.
static string parse_cut_limit(const string& par, const string& val, lzani_cluster_cut& cut)
{
    const map<string, double*> minima = {{"tani", &cut.min_tani}, {"gani", &cut.min_gani}, {"ani", &cut.min_ani}, {"qcov", &cut.min_qcov},
                                         {"rcov", &cut.min_rcov}, {"len_ratio", &cut.min_len_ratio}};
    char* end = nullptr;
    if (par == "num_alns") {
        const unsigned long long v = strtoull(val.c_str(), &end, 10);
        if (val.empty() || !isdigit((unsigned char)val[0]) || *end || v < 1 || v > UINT32_MAX) return "num_alns takes an integer >= 1, not '" + val + "'";
        cut.max_num_alns = (uint32_t)v;
        return "";
    }
    const auto m = minima.find(par);
    if (m == minima.end()) return "unknown parameter '" + par + "' (tani, gani, ani, qcov, rcov, len_ratio or num_alns)";
    const double v = strtod(val.c_str(), &end);
    if (val.empty() || end == val.c_str() || *end || v != v) return par + " takes a number, not '" + val + "'";
    *m->second = v;
    return "";
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
         << "      --flt-kmers-max-seqs <int> - with --flt-kmers: every sequence (query2ref: every query) keeps only its <int> most similar\n"
         << "                                   sequences by shared k-mers; a pair stays where either sequence keeps it (default: no limit)\n"
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
         << "                                   greedy-first (first representative, as CD-HIT), greedy-best (most similar representative, as UCLUST),\n"
         << "                                   set-cover (the sequence with the most unassigned neighbours first, as MMseqs2's greedy set cover),\n"
         << "                                   complete-linkage (every two members of a cluster are a kept pair; the most similar clusters merge first),\n"
         << "                                   leiden-cpm (deterministic Leiden with the constant Potts model: for genus- and family-level groupings)\n"
         << "      --cluster-out <file_name>  - output file of --cluster: one line per sequence, its id and its cluster number\n"
         << "      --cluster-measure <type>   - the similarity greedy-best and complete-linkage compare and leiden-cpm sums: tani, gani or ani (default: tani); accepted and without\n"
         << "                                   effect for single, greedy-first and set-cover\n"
         << "      --cluster-representatives  - write the representative's id instead of the cluster number\n"
         << "      --cluster-leiden-resolution <float> - leiden-cpm: the resolution, 0 .. 1 (default: 0.7); larger values give smaller clusters\n"
         << "      --cluster-leiden-iterations <int>   - leiden-cpm: the iterations, 1 .. 16 (default: 2)\n"
         << "      --cluster-cut <par> <float> - with --cluster: cluster only the pairs with <par> (can be: tani, gani, ani, qcov, rcov, len_ratio) at least\n"
         << "                                   <float>, or with num_alns at most <int>, among those that --out-filter keeps; the output\n"
         << "                                   files keep every pair of --out-filter; can be used multiple times\n"
         << "      --cluster-level <algorithm> <file_name> <cuts> - with --cluster: one more clustering of the same run, into <file_name>;\n"
         << "                                   <cuts> is none or a comma-separated list par=value as for --cluster-cut, e.g. ani=0.95,qcov=0.85;\n"
         << "                                   up to 16 times; the levels share --cluster-measure, --cluster-representatives and the leiden options\n"
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
        else if (par == "--flt-kmers-max-seqs" && has(1)) { P.flt_max_seqs_arg = argv[i + 1]; i += 2; }
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
        else if (par == "--cluster-cut" && has(2)) { P.cluster_cut_args.emplace_back(argv[i + 1], argv[i + 2]); i += 3; }
        else if (par == "--cluster-level" && has(3)) { P.cluster_level_args.push_back(Params::LevelArg{argv[i + 1], argv[i + 2], argv[i + 3]}); i += 4; }
        else if (par == "--cluster-leiden-resolution" && has(1)) { P.leiden_resolution_arg = argv[i + 1]; i += 2; }
        else if (par == "--cluster-leiden-iterations" && has(1)) { P.leiden_iterations_arg = argv[i + 1]; i += 2; }
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
    if (!P.flt_max_seqs_arg.empty()) {
        if (!P.flt_kmers) { cerr << "--flt-kmers-max-seqs belongs to --flt-kmers" << endl; exit(1); }
        char* end = nullptr;
        const unsigned long long v = strtoull(P.flt_max_seqs_arg.c_str(), &end, 10);
        if (!isdigit((unsigned char)P.flt_max_seqs_arg[0]) || *end || v < 1 || v > UINT32_MAX) {
            cerr << "Invalid value for --flt-kmers-max-seqs: " << P.flt_max_seqs_arg << " (an integer >= 1)" << endl;
            exit(1);
        }
        P.flt_max_seqs = (uint32_t)v;
    }
    // --cluster: refused here, before any input is read
    if (!P.cluster && (!P.cluster_out.empty() || !P.cluster_measure_arg.empty() || P.cluster_reps)) {
        cerr << "--cluster-out, --cluster-measure and --cluster-representatives belong to --cluster" << endl;
        exit(1);
    }
    if (!P.cluster && P.levels_on()) { cerr << "--cluster-cut and --cluster-level belong to --cluster" << endl; exit(1); }
    bool leiden_level = P.cluster_arg == "leiden-cpm";       // a level that takes the Leiden parameters
    for (const auto& l : P.cluster_level_args) leiden_level = leiden_level || l.algo == "leiden-cpm";
    if ((!P.leiden_resolution_arg.empty() || !P.leiden_iterations_arg.empty()) && !leiden_level) {
        cerr << "--cluster-leiden-resolution and --cluster-leiden-iterations belong to --cluster leiden-cpm" << endl;
        exit(1);
    }
    if (!P.leiden_resolution_arg.empty()) {
        char* end = nullptr;
        P.leiden_resolution = strtod(P.leiden_resolution_arg.c_str(), &end);
        if (end == P.leiden_resolution_arg.c_str() || *end || !(P.leiden_resolution >= 0 && P.leiden_resolution <= 1)) {
            cerr << "Unsupported value: --cluster-leiden-resolution " << P.leiden_resolution_arg << " (resolutions 0 .. 1 are supported)" << endl;
            exit(1);
        }
    }
    if (!P.leiden_iterations_arg.empty()) {
        char* end = nullptr;
        const long it = strtol(P.leiden_iterations_arg.c_str(), &end, 10);
        if (end == P.leiden_iterations_arg.c_str() || *end || it < 1 || it > 16) {
            cerr << "Unsupported value: --cluster-leiden-iterations " << P.leiden_iterations_arg << " (1 .. 16 iterations are supported)" << endl;
            exit(1);
        }
        P.leiden_iterations = (int)it;
    }
    if (P.cluster) {
        static const map<string, int> algos = {{"single", LZANI_CLUSTER_SINGLE}, {"greedy-first", LZANI_CLUSTER_GREEDY_FIRST}, {"greedy-best", LZANI_CLUSTER_GREEDY_BEST},
                                               {"set-cover", LZANI_CLUSTER_SET_COVER}, {"complete-linkage", LZANI_CLUSTER_COMPLETE}, {"leiden-cpm", LZANI_CLUSTER_LEIDEN}};
        static const map<string, int> measures = {{"tani", LZANI_CLUSTER_TANI}, {"gani", LZANI_CLUSTER_GANI}, {"ani", LZANI_CLUSTER_ANI}};
        const auto a = algos.find(P.cluster_arg);
        if (a == algos.end()) { cerr << "Unknown value for --cluster: " << P.cluster_arg << " (single, greedy-first, greedy-best, set-cover, complete-linkage or leiden-cpm)" << endl; exit(1); }
        P.cluster_algo = a->second;
        const auto m = measures.find(P.cluster_measure_arg.empty() ? "tani" : P.cluster_measure_arg);
        if (m == measures.end()) { cerr << "Unknown value for --cluster-measure: " << P.cluster_measure_arg << " (tani, gani or ani)" << endl; exit(1); }
        P.cluster_measure = m->second;
        if (P.cluster_out.empty()) { cerr << "--cluster needs --cluster-out <file_name>" << endl; exit(1); }
        if (P.query2ref) { cerr << "--cluster belongs to the mode all2all (query2ref compares two sets)" << endl; exit(1); }
        if (P.single_txt) { cerr << "--cluster cannot be used with --out-type single-txt (it takes no output filter)" << endl; exit(1); }
        if (!P.flt_mask) { cerr << "--cluster needs an --out-filter: the pairs it keeps are the edges of the graph" << endl; exit(1); }
        // the levels: that of --cluster with the cut of --cluster-cut, then those of --cluster-level
        P.levels.assign(1, Params::Level{P.cluster_algo, P.cluster_out, lzani_cluster_cut{}});
        for (const auto& c : P.cluster_cut_args) {
            const string why = parse_cut_limit(c.first, c.second, P.levels[0].cut);
            if (!why.empty()) { cerr << "Invalid value for --cluster-cut: " << why << endl; exit(1); }
        }
        if (P.cluster_level_args.size() > 16) { cerr << "--cluster-level can be used at most 16 times" << endl; exit(1); }
        for (const auto& l : P.cluster_level_args) {
            const auto la = algos.find(l.algo);
            if (la == algos.end()) { cerr << "Unknown value for --cluster-level: " << l.algo << " (single, greedy-first, greedy-best, set-cover, complete-linkage or leiden-cpm)" << endl; exit(1); }
            Params::Level lv{la->second, l.out, lzani_cluster_cut{}};
            if (l.cuts != "none")
                for (const auto& item : split(l.cuts, ',')) {
                    const size_t eq = item.find('=');
                    const string why = eq == string::npos ? "'" + item + "' is not of the form par=value" : parse_cut_limit(item.substr(0, eq), item.substr(eq + 1), lv.cut);
                    if (!why.empty()) { cerr << "Invalid value for --cluster-level: " << why << " (none, or a list par=value)" << endl; exit(1); }
                }
            if (l.cuts.empty()) { cerr << "Invalid value for --cluster-level: empty cuts (none, or a list par=value)" << endl; exit(1); }
            for (const auto& other : P.levels)
                if (other.out == lv.out) { cerr << "--cluster-level: two levels write the same file: " << lv.out << endl; exit(1); }
            P.levels.push_back(lv);
        }
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

// --out-filter as the engine and the emitter take it: the one place that turns the flags into minima (0 where none was named).
static lzani_out_filter out_filter_minima()
{
    return lzani_out_filter{P.flt_vals[(int)Comp::tani], P.flt_vals[(int)Comp::gani], P.flt_vals[(int)Comp::ani], P.flt_vals[(int)Comp::qcov], P.flt_vals[(int)Comp::rcov]};
}
// Whether the device applies it: a two-TSV output, no --results-in / --results-out (they carry every pair), numbers for
// minima (a NaN drops nothing on the host and is refused by the engine), and LZANI_OUT_FILTER=host not set.  With
// --out-alignment the caller asks out_aln_on_device() as well: the kept call is then the aligned call.
static bool out_filter_on_device()
{
    const char* e = getenv("LZANI_OUT_FILTER");
    return P.flt_mask != 0 && !P.single_txt && P.results_in.empty() && P.results_out.empty()
           && !lzani::out_filter_has_nan(out_filter_minima()) && !(e && e == "host"s);
}
// Whether --out-alignment goes through the device's region stage (lzani_run_rows_aligned), as far as the command line says:
// no --results-in / --results-out, numbers for minima, and LZANI_OUT_ALN=host not set.  The caller adds what it alone knows:
// one device, a library with the symbols, filter lists that ascend.
static bool out_aln_on_device()
{
    const char* e = getenv("LZANI_OUT_ALN");
    return !P.out_aln.empty() && P.results_in.empty() && P.results_out.empty() && !lzani::out_filter_has_nan(out_filter_minima()) && !(e && e == "host"s);
}
