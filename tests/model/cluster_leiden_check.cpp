// cluster_leiden_check.cpp -- TEST INFRASTRUCTURE ONLY (a stand-alone host program, tests/test_cluster_leiden.py builds it with
// -fsanitize=address,undefined and runs it).
//
// The sequential form of Leiden (cluster_leiden_host of lz-ani_amd/csrc/lzani_cluster_plan.h) under the sanitizers, on graphs
// read from the file named by the one argument:
//   graph <n> <m> <the resolution's bits, hexadecimal> <iterations>     then m lines  <a> <b> <the weight's bits, hexadecimal>
// For every graph it prints one line: rep <n values> | <quality> <iterations> <levels> <move rounds> <refine rounds> <moves> <merges>.
// The test compares them with tests/cluster_leiden_model.py.  A line that does not parse, or a call that fails, exits non-zero.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan tests/model/cluster_leiden_check.cpp
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../lz-ani_amd/csrc/lzani_cluster_plan.h"

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "cluster_leiden_check: one argument, the graph file\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cluster_leiden_check: cannot read %s\n", argv[1]); return 2; }
    uint32_t n;
    uint64_t m, gbits;
    int iterations, graphs = 0;
    while (fscanf(f, " graph %" SCNu32 " %" SCNu64 " %" SCNx64 " %d", &n, &m, &gbits, &iterations) == 4) {
        double gamma;
        memcpy(&gamma, &gbits, 8);
        std::vector<lzani_cluster_edge> edges((size_t)m);
        for (lzani_cluster_edge& e : edges) {
            uint64_t bits;
            if (fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNx64, &e.a, &e.b, &bits) != 3) { fprintf(stderr, "cluster_leiden_check: a bad edge line\n"); return 2; }
            memcpy(&e.w, &bits, 8);
        }
        std::vector<uint32_t> rep(n);
        lzani_cluster_leiden_info info{};
        const int rc = lzani::cluster_leiden_host(n, edges.data(), edges.size(), gamma, iterations, rep.data(), &info);
        if (rc != LZANI_OK) { fprintf(stderr, "cluster_leiden_check: cluster_leiden_host returned %d on graph %d\n", rc, graphs); return 1; }
        printf("rep");
        for (uint32_t v = 0; v < n; ++v) printf(" %" PRIu32, rep[v]);
        printf(" | %" PRId64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", info.quality, info.iterations, info.levels,
               info.move_rounds, info.refine_rounds, info.moves, info.merges);
        ++graphs;
    }
    fclose(f);
    if (!graphs) { fprintf(stderr, "cluster_leiden_check: no graph\n"); return 2; }
    return 0;
}
