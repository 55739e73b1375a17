// engine.h -- the HIP engine as the `lz-ani` host binary binds it: liblzani_hip.so loaded with dlopen (so that the binary
// builds, and its ingest/emit code is testable, without ROCm present), every entry point typed by its declaration in
// include/lzani.h, and the owners of a context and of a group.  Uses nothing of the other host headers.
#pragma once
#include <dlfcn.h>

#include <cstdlib>
#include <filesystem>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/lzani.h"

// Every symbol the binary calls, named once (without its lzani_ prefix).  Required: a library without one is refused.
// Kept (the output filter on the device) and cluster (the cluster stage): bound where the library has them; an older one
// keeps the filter, or the clustering, on the host.  Aligned (the alignment-region stage: --out-alignment on the device): the
// same; an older library keeps the regions' order on the host.  Cover and link (what -V 2 says of a set-cover or a
// complete-linkage run): read where they are there.  Leiden (its parameters and what -V 2 says of a run): a library without
// them leaves --cluster leiden-cpm to the host.  Limit (--flt-kmers-max-seqs): asked for only where the flag is given, and
// a library without them is then refused with the name of the symbol it lacks.  Levels (--cluster-cut, --cluster-level:
// the record store and the levels of the cluster stage): the same, asked for only where either flag is given.
#define LZANI_ENGINE_REQUIRED(X) \
    X(create) X(destroy) X(last_error) X(set_genomes) X(get_timing) X(run_rows_regions) X(row_costs) X(partition_rows) \
    X(group_create) X(group_destroy) X(group_last_error) X(group_set_genomes) X(group_run_rows) X(group_get_timing) \
    X(set_genome_memory) X(get_residency) X(group_set_genome_memory) X(group_get_residency) \
    X(prefilter) X(prefilter_fetch) X(get_prefilter_info) X(prefilter_codes) X(get_prefilter_stream_info) X(get_prefilter_pass_info) \
    X(prefilter_cross) X(prefilter_codes_cross) X(set_prefilter_counting) X(get_prefilter_sparse_info)
#define LZANI_ENGINE_KEPT(X) X(group_run_rows_kept) X(group_kept_fetch) X(group_get_kept_info)
#define LZANI_ENGINE_ALIGNED(X) X(run_rows_aligned) X(regions_fetch) X(get_regions_info) X(regions_host) X(kept_fetch) X(get_kept_info)
#define LZANI_ENGINE_CLUSTER(X) X(group_cluster_begin) X(group_cluster_add_kept) X(group_cluster_run) X(group_cluster_fetch) X(group_get_cluster_info)
#define LZANI_ENGINE_COVER(X) X(group_get_cluster_cover_info) X(group_get_cluster_link_info)
#define LZANI_ENGINE_LEIDEN(X) X(group_set_cluster_leiden) X(group_get_cluster_leiden_info)
#define LZANI_ENGINE_LIMIT(X) X(prefilter_limit) X(get_prefilter_limit_info)
#define LZANI_ENGINE_LEVELS(X) \
    X(group_cluster_store_begin) X(group_cluster_store_add_kept) X(group_cluster_level) X(group_get_cluster_store_info) X(group_get_cluster_level_info)

struct Engine {
    void* so = nullptr;
#define X(f) decltype(&lzani_##f) f = nullptr;             // a signature that drifts from the header does not compile
    LZANI_ENGINE_REQUIRED(X) LZANI_ENGINE_KEPT(X) LZANI_ENGINE_ALIGNED(X) LZANI_ENGINE_CLUSTER(X) LZANI_ENGINE_COVER(X) LZANI_ENGINE_LEIDEN(X) LZANI_ENGINE_LIMIT(X) LZANI_ENGINE_LEVELS(X)
#undef X
#define X(f) && f
    bool has_kept() const { return true LZANI_ENGINE_KEPT(X); }
    bool has_aligned() const { return true LZANI_ENGINE_ALIGNED(X); }
    bool has_cluster() const { return true LZANI_ENGINE_CLUSTER(X); }
    bool has_leiden() const { return true LZANI_ENGINE_CLUSTER(X) LZANI_ENGINE_LEIDEN(X); }
#undef X
    // the first symbol of the limit group that the library lacks, or null
    const char* missing_limit() const
    {
#define X(f) if (!f) return "lzani_" #f;
        LZANI_ENGINE_LIMIT(X)
#undef X
        return nullptr;
    }
    // ... and of the levels group
    const char* missing_levels() const
    {
#define X(f) if (!f) return "lzani_" #f;
        LZANI_ENGINE_LEVELS(X)
#undef X
        return nullptr;
    }
    bool load()
    {
        std::vector<std::string> cand;
        if (const char* e = getenv("LZANI_LIB")) cand.push_back(e);
        std::error_code ec;
        auto self = std::filesystem::canonical("/proc/self/exe", ec);
        if (!ec) { cand.push_back((self.parent_path() / "liblzani_hip.so").string()); cand.push_back((self.parent_path().parent_path() / "liblzani_hip.so").string()); }
        cand.push_back("liblzani_hip.so");
        for (auto& c : cand) if ((so = dlopen(c.c_str(), RTLD_NOW | RTLD_LOCAL))) break;
        if (!so) { std::cerr << "Cannot load liblzani_hip.so (the HIP engine; there is no CPU fallback): " << dlerror() << std::endl; return false; }
#define X(f) f = reinterpret_cast<decltype(f)>(dlsym(so, "lzani_" #f));
        LZANI_ENGINE_REQUIRED(X) LZANI_ENGINE_KEPT(X) LZANI_ENGINE_ALIGNED(X) LZANI_ENGINE_CLUSTER(X) LZANI_ENGINE_COVER(X) LZANI_ENGINE_LEIDEN(X) LZANI_ENGINE_LIMIT(X) LZANI_ENGINE_LEVELS(X)
#undef X
#define X(f) if (!f) { std::cerr << "Missing symbol lzani_" #f << std::endl; return false; }
        LZANI_ENGINE_REQUIRED(X)
#undef X
        return true;
    }
};

// A context and a group, destroyed on every way out of their scope.
struct Context {
    const Engine& E;
    lzani_ctx* p = nullptr;
    explicit Context(const Engine& e) : E(e) {}
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    ~Context() { reset(); }
    void reset() { if (p) E.destroy(p); p = nullptr; }
    operator lzani_ctx*() const { return p; }
};
struct Group {
    const Engine& E;
    lzani_group* p = nullptr;
    std::vector<int> devs;                                  // the devices of the group, in its order
    double secs[2] = {0, 0};                                // the seconds of the create and of the genomes
    explicit Group(const Engine& e) : E(e) {}
    Group(const Group&) = delete;
    Group& operator=(const Group&) = delete;
    ~Group() { if (p) E.group_destroy(p); }
    operator lzani_group*() const { return p; }
};
