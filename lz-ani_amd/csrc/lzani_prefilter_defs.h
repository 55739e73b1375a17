// lzani_prefilter_defs.h -- the two definitions of the k-mer prefilter that host and device share: the canonical k-mer
// and the sampling rule (include/lzani.h: lzani_prefilter).  Plain integer arithmetic mod 2^64; the kernels of
// lzani_kernels_prefilter.h and a host test shim compile the same text.
#pragma once
#include "lzani_core.h"

namespace lzani {

// splitmix64's output function on x
LZ_HD u64 pf_splitmix64(u64 x)
{
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

// canonical k-mer of a window: the smaller of its packed value (first symbol least significant) and that of its
// reverse complement
LZ_HD u64 pf_canon(u64 fwd, u64 rc) { return fwd < rc ? fwd : rc; }

// sampling: a canonical k-mer is kept iff its hash does not exceed sample_max (all ones keeps everything)
LZ_HD bool pf_keep(u64 canon, u64 sample_max) { return pf_splitmix64(canon) <= sample_max; }

}  // namespace lzani
