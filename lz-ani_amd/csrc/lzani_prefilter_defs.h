// lzani_prefilter_defs.h -- the definitions of the k-mer prefilter that host and device share: the canonical k-mer and
// the sampling rule (include/lzani.h: lzani_prefilter), the bin that assigns a k-mer to a pass, and how the streamed form
// makes a window's two values from raw symbol codes.  Plain integer arithmetic mod 2^64; the kernels of
// lzani_kernels_prefilter.h and the host test shims compile the same text.
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

// k-mer passes: the bin of a canonical k-mer, one of PF_BINS; a pass works on the k-mers of a contiguous range of bins.
// Bits of the hash's low half: sampling by the hash's value (its high bits decide) does not skew them.
enum { PF_BINS = 4096 };
LZ_HD u32 pf_bin(u64 canon) { return (u32)(pf_splitmix64(canon) >> 20) & (u32)(PF_BINS - 1); }

// The limit stage's score of a kept pair (include/lzani.h: lzani_prefilter_limit): floor(shared * (2^32 - 1) / min(|K(a)|,
// |K(b)|)) in unsigned 64-bit arithmetic; 1 <= shared <= min, so the product fits and the score is 1 .. 2^32 - 1.
LZ_HD u32 pf_limit_score(u32 shared, u32 ka, u32 kb)
{
    const u64 m = ka < kb ? ka : kb;
    return m ? (u32)((u64)shared * 0xFFFFFFFFull / m) : 0u;
}

// ---- windows from raw symbol codes (the streamed prefilter, lzani_prefilter_codes): no packed text, no second strand

// The packed value of a window's reverse complement from the window's own packed value (k <= 32): every 2-bit group
// complemented, the groups reversed, and the k of them that belong to the window moved down.
LZ_HD u64 pf_rc_of(u64 fwd, int k)
{
    const u64 y = brev64(~fwd);                                   // groups reversed, the two bits of a group too
    const u64 x = ((y >> 1) & 0x5555555555555555ULL) | ((y & 0x5555555555555555ULL) << 1);
    return x >> (64 - 2 * k);
}

// 16 symbol codes (A0 C1 G2 T3, >= 4 is N) as one group of a packed text: sym = 2 bits a symbol, the first lowest, 0 for
// an N; nbits = bit j set iff symbol j is an N.  Only c[0 .. n) is read (n <= 16): the rest of the group is N.
LZ_HD void pf_pack16(const unsigned char* c, int n, u32& sym, u32& nbits)
{
    sym = 0; nbits = 0;
    for (int j = 0; j < 16; ++j) {
        const u32 v = j < n ? (u32)c[j] : 4u;
        sym |= (v < 4u ? v : 0u) << (2 * j);
        nbits |= (u32)(v >= 4u) << j;
    }
}

// v(q): the window of k <= 31 symbols from symbol q on, in a text of pf_pack16 groups (group j = symbols 16 j .. 16 j + 15
// in t2[j], nm[j]); false where the window holds an N.  Reads the groups q / 16 .. q / 16 + 2.
LZ_HD bool pf_window(const u32* t2, const unsigned short* nm, int q, int k, u64& v)
{
    const int w = q >> 4, s = q & 15;
    const u64 nb = ((u64)nm[w] | ((u64)nm[w + 1] << 16) | ((u64)nm[w + 2] << 32)) >> s;
    if (nb & lowmask(k)) return false;
    const u64 lo = (u64)t2[w] | ((u64)t2[w + 1] << 32);
    const u64 x = s ? (lo >> (2 * s)) | ((u64)t2[w + 2] << (64 - 2 * s)) : lo;
    v = x & lowmask(2 * k);
    return true;
}

}  // namespace lzani
