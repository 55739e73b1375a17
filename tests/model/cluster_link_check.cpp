// cluster_link_check.cpp -- TEST INFRASTRUCTURE ONLY (a stand-alone host program, tests/test_cluster_link.py builds it with
// -fsanitize=address,undefined and runs it).
//
// The sequential statement of complete linkage (cluster_host of lz-ani_amd/csrc/lzani_cluster_plan.h, algorithm
// LZANI_CLUSTER_COMPLETE) under the sanitizers, on graphs read from the file named by the one argument:
//   graph <n> <m>          then m lines  <a> <b> <the weight's bits, hexadecimal>
// For every graph it prints one line: rep <n values> | <clusters>.  The test compares them with tests/cluster_link_model.py.
// A line that does not parse, or a call that fails, exits non-zero with a message.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan tests/model/cluster_link_check.cpp
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../lz-ani_amd/csrc/lzani_cluster_plan.h"

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "cluster_link_check: one argument, the graph file\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cluster_link_check: cannot read %s\n", argv[1]); return 2; }
    uint32_t n;
    uint64_t m;
    int graphs = 0;
    while (fscanf(f, " graph %" SCNu32 " %" SCNu64, &n, &m) == 2) {
        std::vector<lzani_cluster_edge> edges((size_t)m);
        for (lzani_cluster_edge& e : edges) {
            uint64_t bits;
            if (fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNx64, &e.a, &e.b, &bits) != 3) { fprintf(stderr, "cluster_link_check: a bad edge line\n"); return 2; }
            memcpy(&e.w, &bits, 8);
        }
        std::vector<uint32_t> rep(n), cl(n);
        uint32_t k = 0;
        const int rc = lzani::cluster_host(n, edges.data(), edges.size(), LZANI_CLUSTER_COMPLETE, rep.data(), cl.data(), &k);
        if (rc != LZANI_OK) { fprintf(stderr, "cluster_link_check: cluster_host returned %d on graph %d\n", rc, graphs); return 1; }
        printf("rep");
        for (uint32_t v = 0; v < n; ++v) printf(" %" PRIu32, rep[v]);
        printf(" | %" PRIu32 "\n", k);
        ++graphs;
    }
    fclose(f);
    if (!graphs) { fprintf(stderr, "cluster_link_check: no graph\n"); return 2; }
    return 0;
}
