// lzani_set_plan.h -- the pure layout decisions of a genome set (lzani_set_genomes, lzani_plan_blocks): the set-level
// switches, the form of the anchor index, the genome-table footprint, the block plan of a set larger than its memory
// limit, the automatic residency decision, the slot count of the index slabs.  No HIP types: it compiles with a plain
// C++ compiler (tests/model/set_plan_check.cpp runs it under the sanitizers), and it is not among the sources a run-time
// compile embeds (lzani_rtc.h).  (The bytes of one slab slot stay in lzani_run_plan.h: the run's batches go by them too.)
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <optional>
#include <string>
#include <vector>

#include "../../include/lzani.h"
#include "lzani_layout.h"

namespace lzani {

// An LZANI_* switch: whether it is set and begins with ch; its number (atoi / strtoull); empty where it is not set.
inline bool env_is(const char* name, char ch) { const char* v = getenv(name); return v && *v == ch; }
inline std::optional<bool> env_flag(const char* name) { const char* v = getenv(name); return v ? std::optional<bool>(*v == '1') : std::nullopt; }
inline std::optional<int> env_int(const char* name) { const char* v = getenv(name); return v ? std::optional<int>(atoi(v)) : std::nullopt; }
inline std::optional<u64> env_u64(const char* name) { const char* v = getenv(name); return v ? std::optional<u64>(strtoull(v, nullptr, 10)) : std::nullopt; }

inline Params params_of(const lzani_params& p)
{
    return Params{p.min_anchor_len, p.min_seed_len, p.max_dist_in_ref, p.max_dist_in_query,
                  p.min_region_len, p.approx_window, p.approx_mismatches, p.approx_run_len};
}

// Per-genome k-mer words exist for mal, msl <= 15 (the fast path).
inline bool kmer_words_of(const Params& P) { return P.mal <= 15 && P.msl <= 15; }

// The set-level switches (experiments and tests), read where a SetKnobs is made: by lzani_set_genomes and by
// lzani_plan_blocks (tests set them before either).
struct SetKnobs {
    int bk_max_dirbits = env_int("LZANI_BK_MAX_DIRBITS").value_or(26);
    bool buckets = !env_is("LZANI_NO_BUCKETS", '1'), tagwords = !env_is("LZANI_NO_TAGWORDS", '1');      // experiments / test_index_forms
    u64 join_min_bytes = env_u64("LZANI_JOIN_MIN_BYTES").value_or(8ull << 20);
    bool join = !env_is("LZANI_NO_JOIN", '1');
    int sort_min_dirbits = env_int("LZANI_SORT_INDEX_MIN_DIRBITS").value_or(20);      // 0, tests: the sort-based build at every size
    bool sort_index = !env_is("LZANI_NO_SORT_INDEX", '1');
    int filter_max_bits = env_int("LZANI_FILTER_MAX_BITS").value_or(18);              // 2^18 bits = 32 KB of LDS per block of 16 waves
    bool filter = !env_is("LZANI_NO_FILTER", '1');
    int max_slots = env_int("LZANI_MAX_SLOTS").value_or(0);                           // > 0, tests: the multi-batch path
    std::optional<u64> free_bytes = env_u64("LZANI_FREE_BYTES");                       // tests: the automatic residency trigger
};

// The form of the anchor index: a property of the genome set and the parameters, decided once per lzani_set_genomes, so
// that the strides of the slabs never change under an allocation.  Strides are 32-bit words per slab slot; 0 = none.
struct SetLayout {
    u64 bk_stride = 0;            // bucket tables
    u64 tw_stride = 0;            // tag words of the bucket tables (tag bits <= 7)
    u64 fl_stride = 0;            // presence filters; 0 = no filter (one all-ones word)
    u32 fmask = 31;
    bool join_mode = false;       // join form of candidate detection (long genomes)
    bool sort_build = false;      // sort-based index build (large directories)
    u32 max_slots = 65535;        // gridDim.y limit; LZANI_MAX_SLOTS lowers it
};

// n genomes, the longest text Tmax, geo = index_geometry(Tmax, P.mal).  (The block plan of an out-of-core set counts
// the join form of the whole set.)
inline SetLayout set_layout_of(const Params& P, const IndexGeom& geo, int Tmax, u32 n, const SetKnobs& k)
{
    SetLayout f;
    int tagbits = 0;
    while (tagbits < 32 && ((geo.tagmask >> tagbits) & 1u)) ++tagbits;
    const bool exact = geo.tagmask == (u32)lowmask(geo.kb - geo.dirbits);
    // bucket table (+ tag words): wherever the sentinels cannot be real entries; 20 B per bucket more per slot
    f.bk_stride = (kmer_words_of(P) && exact && geo.dirbits <= k.bk_max_dirbits && tagbits + geo.posbits <= 30 && k.buckets) ? ((u64)4 << geo.dirbits) : 0;
    f.tw_stride = (f.bk_stride && tagbits <= 7 && k.tagwords) ? ((u64)1 << geo.dirbits) : 0;
    // Join form of candidate detection: where the tag words of one reference exceed what an L2 holds by far, a random
    // probe per query position costs one HBM line each; the query's k-mer list sorted by bucket turns the probes into
    // two streams (DevWave::join).  Needs the anchor queue (tag words, seed window <= 128) and keys of 64 bits.
    const int gbits = ceil_log2((u64)n + 1);                          // the all-ones genome number is the invalid key's
    f.join_mode = f.tw_stride && f.tw_stride * 4 >= k.join_min_bytes && P.mqd + P.mrd <= 128 && gbits + geo.kb + geo.posbits <= 64 && k.join;
    // Sort-based index build where the directory is beyond the LDS-staged build (2^19 buckets): keys of 64 bits with up
    // to 16 bits of slot number
    f.sort_build = kmer_words_of(P) && geo.dirbits >= k.sort_min_dirbits && geo.kb + geo.posbits <= 60 && k.sort_index;
    // Presence filter in front of the tag-word probes (probe form only; k_pairs_blk keeps the reference's in LDS): ~3 bits
    // per text position, at most 2^18 bits (genomes up to ~128 kbp); beyond, one all-ones word passes everything
    const int tbits = ceil_log2((u64)std::max(Tmax, 1024)), fbits = std::min(tbits + 1, k.filter_max_bits);
    if (f.tw_stride && !f.join_mode && tbits <= k.filter_max_bits && k.filter) {
        f.fl_stride = ((u64)1 << fbits) / 32;
        f.fmask = (u32)((1u << fbits) - 1u);
    }
    f.max_slots = k.max_slots > 0 ? (u32)std::min(65535, k.max_slots) : 65535u;
    if (f.sort_build)                                      // the slot number shares the 64-bit key with hash and position
        f.max_slots = (u32)std::min<u64>(f.max_slots, (1ull << std::min(16, 64 - geo.kb - geo.posbits)) - 1);
    return f;
}

// Genome tables of `words` N-mask words (lzani_get_layout's bytes_genomes): packed text 16 B + N mask 8 B per word,
// k-mer words 2 x 4 B per text position.
inline u64 genome_table_bytes(u64 words, bool kmers) { return words * (16 + 8) + (kmers ? words * 64 * 8 : 0); }

// Genome-table footprint of one genome of an out-of-core set: its tables plus its join lists where they apply (8 B per
// forward position for the sorted keys, 20 B of offsets and counts).
inline u64 ooc_genome_bytes(int L, const Params& P, bool kmers, bool join)
{
    return genome_table_bytes(text_wordsN(ref_text_len(L, P.mrd)), kmers) + (join ? (u64)L * 8 + 20 : 0);
}

// The block plan (lzani_plan_blocks): genomes in id order into contiguous blocks of at most limit / 2 bytes each.
// first[b] .. first[b + 1] are block b's genomes, bytes[b] its footprint.  limit 0: one block.  Returns the number of
// blocks, or LZANI_ERR_ARG with the reason in msg.
inline int plan_blocks_impl(u32 n, const u32* len, const Params& P, u64 limit, const SetKnobs& k, std::vector<u32>& first, std::vector<u64>& bytes,
                            std::string& msg)
{
    if (!n || !len) { msg = "lzani_plan_blocks: empty input"; return LZANI_ERR_ARG; }
    int Lmax = 0;
    for (u32 g = 0; g < n; ++g) {
        if (len[g] > 0x3FFFFFFFu - 3u * (u32)P.mrd) { msg = "sequence too long for 32-bit text positions"; return LZANI_ERR_ARG; }
        Lmax = std::max(Lmax, (int)len[g]);
    }
    const int Tmax = ref_text_len(Lmax, P.mrd);
    const bool kmers = kmer_words_of(P), join = set_layout_of(P, index_geometry(Tmax, P.mal), Tmax, n, k).join_mode;
    u64 fmax = 0, total = 0;
    for (u32 g = 0; g < n; ++g) {
        const u64 b = ooc_genome_bytes((int)len[g], P, kmers, join);
        fmax = std::max(fmax, b);
        total += b;
    }
    first.assign(1, 0);
    bytes.clear();
    if (limit == 0) { first.push_back(n); bytes.push_back(total); return 1; }
    if (fmax > limit / 2) {
        msg = "genome-memory limit of " + std::to_string(limit) + " bytes is below the minimum of " + std::to_string(2 * fmax) +
              " bytes (each of the two resident halves must hold the largest genome's tables, " + std::to_string(fmax) + " bytes)";
        return LZANI_ERR_ARG;
    }
    u64 cur = 0;
    for (u32 g = 0; g < n; ++g) {
        const u64 b = ooc_genome_bytes((int)len[g], P, kmers, join);
        if (g > first.back() && cur + b > limit / 2) { first.push_back(g); bytes.push_back(cur); cur = 0; }
        cur += b;
    }
    first.push_back(n);
    bytes.push_back(cur);
    return (int)bytes.size();
}

// Residency in automatic mode (no limit asked for): a set stays in-core where its tables fit the free memory beside the
// staging copy of its codes, and beside one index slab slot; else it gets half of what is free (half for the genomes,
// half for slabs and bitmaps).  Returns the limit; 0 = in-core.
inline u64 auto_genome_limit(u64 tables, u64 codes, u64 per_slot, u64 free_b)
{
    return (tables + codes > free_b || tables + per_slot > free_b) ? free_b / 2 : 0;
}

// The slots the index slabs have after ensure_slabs: 60 % of the memory that is free or theirs already, at most
// want_rows and max_slots, at least 1 -- and never fewer than they hold (slabs only grow).
inline u32 slab_slot_count(u64 free_b, u32 held, u64 per_slot, u32 want_rows, u32 max_slots)
{
    const size_t budget = (size_t)((free_b + held * per_slot) * 0.6);
    const u32 slots = (u32)std::min<size_t>(std::min<u32>(want_rows, max_slots), std::max<size_t>(1, budget / per_slot));
    return std::max(slots, held);
}

}  // namespace lzani
