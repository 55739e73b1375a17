"""The k-mer passes of the prefilter (include/lzani.h: "K-mer passes") as Python statements, beside the definitions of
tests/prefilter_model.py: the bin of a canonical k-mer, the pass plan, the windows of a pass, the number of key sweeps --
and the small genome set the pass tests share."""
import numpy as np

import prefilter_model as PM
import synth_genomes as SG

BINS = 4096
U64 = np.uint64


def bin_of(x):
    """bin(x) = (splitmix64(x) >> 20) & 4095 of canonical k-mer value(s)."""
    return ((PM.splitmix64(x) >> U64(20)) & U64(BINS - 1)).astype(np.int64)


def forced_plan(P):
    return [BINS * p // P for p in range(P + 1)]


def plan(hist, cap, forced=0):
    """bin_lo[P + 1]; None for LZANI_ERR_ARG (a bin above cap, or a forced P outside 1 .. 4096)."""
    if forced:
        return forced_plan(forced) if forced <= BINS else None
    lo, total = [0], 0
    for b, h in enumerate(int(x) for x in hist):
        if h > cap:
            return None
        if total + h > cap:                    # the pass is full: bin b opens the next one
            lo.append(b)
            total = 0
        total += h
    return lo + [BINS]


def kept_bins(seqs, k, sample_max=PM.SAMPLE_ALL):
    """The bin of every kept canonical window of the set (one entry per window, not per distinct k-mer)."""
    out = []
    for s in seqs:
        x = PM.canon_windows(s, k)
        out.append(bin_of(x[PM.keep(x, sample_max)]))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def histogram(seqs, k, sample_max=PM.SAMPLE_ALL):
    return np.bincount(kept_bins(seqs, k, sample_max), minlength=BINS).astype(np.uint64)


def pass_windows(hist, bin_lo):
    """Kept windows of every pass of a plan."""
    c = np.concatenate(([0], np.cumsum(np.asarray(hist, dtype=np.int64))))
    return [int(c[b] - c[a]) for a, b in zip(bin_lo[:-1], bin_lo[1:])]


def key_sweeps(tiles, windows_of_pass):
    """W of include/lzani.h: 1 where no window is kept; 3 with one pass; 2 + 3 * T * P' with several, P' the passes that
    hold a window."""
    if sum(windows_of_pass) == 0:
        return 1
    if len(windows_of_pass) == 1:
        return 3
    return 2 + 3 * tiles * sum(1 for w in windows_of_pass if w)


def _rand(seed, n):
    return (SG.splitmix64(seed, np.arange(n, dtype=np.uint64)) % np.uint64(4)).astype(np.uint8)


def pass_set():
    """24 genomes of 2-6 kbp (about 90 k windows): three families of 5 at 3-10 % divergence, one genome with a run of N,
    one shorter than any k, one of length 0, the reverse complement of a family member, the rest random."""
    _, fam = SG.make_set(15, 29, lmin=2000, lmax=6000, fam=5, dmin=0.03, dmax=0.10)
    seqs = [np.array(s, dtype=np.uint8) for s in fam]
    g = _rand(701, 4500)
    g[1800:2100] = 4
    seqs.append(g)                                             # 15: a run of N
    seqs.append(_rand(702, 7))                                 # 16: shorter than k
    seqs.append(_rand(703, 0))                                 # 17: empty
    seqs.append((3 - seqs[6][::-1]).astype(np.uint8))          # 18: reverse complement of a family member
    for i, n in enumerate((2000, 3111, 4097, 5000, 6000)):
        seqs.append(_rand(710 + i, n))
    assert len(seqs) == 24
    return seqs
