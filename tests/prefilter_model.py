"""The k-mer prefilter's definitions (include/lzani.h: lzani_prefilter) as numpy statements: what the device stage is
compared with, entry by entry.  Sequences are reservoir symbol codes (A0 C1 G2 T3, >= 4 is N), one uint8 array each."""
import numpy as np

U64 = np.uint64
SAMPLE_ALL = 0xFFFFFFFFFFFFFFFF


def splitmix64(x):
    """The output function of splitmix64 on uint64 value(s), mod 2^64."""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=U64) + U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
        return x ^ (x >> U64(31))


def keep(x, sample_max=SAMPLE_ALL):
    return splitmix64(x) <= U64(sample_max)


def window_values(codes, k):
    """(v, rc, valid) of every window 0 <= p <= L - k: packed value (first symbol least significant), that of the
    reverse complement, and whether the window holds no N."""
    c = np.asarray(codes, dtype=np.uint8)
    w = len(c) - k + 1
    if w <= 0:
        z = np.zeros(0, dtype=U64)
        return z, z, np.zeros(0, dtype=bool)
    isn = np.concatenate(([0], np.cumsum(c >= 4)))
    valid = (isn[k:] - isn[:-k]) == 0
    s = np.where(c >= 4, 0, c).astype(U64)
    v = np.zeros(w, dtype=U64)
    rc = np.zeros(w, dtype=U64)
    for j in range(k):
        v |= s[j:j + w] << U64(2 * j)
        rc |= (U64(3) - s[k - 1 - j:k - 1 - j + w]) << U64(2 * j)
    return v, rc, valid


def canon_windows(codes, k):
    """canon(p) of the valid windows, in position order."""
    v, rc, valid = window_values(codes, k)
    return np.minimum(v, rc)[valid]


def kmer_set(codes, k, sample_max=SAMPLE_ALL):
    """K(g): the distinct kept canonical k-mers, ascending."""
    x = canon_windows(codes, k)
    return np.unique(x[keep(x, sample_max)])


def shared_matrix(seqs, k, sample_max=SAMPLE_ALL):
    """(kmers_of[n], shared[n, n]): |K(g)| and, above the diagonal, |K(a) & K(b)| (zero elsewhere)."""
    n = len(seqs)
    sets = [kmer_set(s, k, sample_max) for s in seqs]
    kmers_of = np.array([len(x) for x in sets], dtype=np.int64)
    km = np.concatenate(sets) if n else np.zeros(0, dtype=U64)
    gid = np.repeat(np.arange(n, dtype=np.int64), kmers_of)
    order = np.argsort(km, kind="stable")                   # (k-mer, genome) ascending: unique pairs already
    km, gid = km[order], gid[order]
    shared = np.zeros(n * n, dtype=np.int64)
    d = 1
    while d < len(km):                                      # pairs d apart inside a run of equal k-mers
        same = km[d:] == km[:-d]
        if not same.any():
            break
        shared += np.bincount(gid[:-d][same] * n + gid[d:][same], minlength=n * n)
        d += 1
    return kmers_of, shared.reshape(n, n)


def kept_pairs(kmers_of, shared, min_shared=1, min_ratio=0.0):
    """CSR of the kept pairs a < b: (row_off[n + 1], ids, shared values), ids ascending inside a row."""
    n = len(kmers_of)
    a, b = np.triu_indices(n, 1)
    s = shared[a, b]
    mn = np.minimum(kmers_of[a], kmers_of[b])
    ok = s >= max(int(min_shared), 1)
    ratio = np.zeros(len(s), dtype=np.float64)
    ratio[ok] = s[ok].astype(np.float64) / mn[ok].astype(np.float64)
    ok &= ratio >= np.float64(min_ratio)
    row_off = np.zeros(n + 1, dtype=np.uint64)
    row_off[1:] = np.cumsum(np.bincount(a[ok], minlength=n))
    return row_off, b[ok].astype(np.uint32), s[ok].astype(np.uint32)


def prefilter(seqs, k, sample_max=SAMPLE_ALL, min_shared=1, min_ratio=0.0):
    """What lzani_prefilter + lzani_prefilter_fetch return: kmers_of, row_off, ids, shared."""
    kmers_of, shared = shared_matrix(seqs, k, sample_max)
    row_off, ids, sh = kept_pairs(kmers_of, shared, min_shared, min_ratio)
    return kmers_of.astype(np.uint32), row_off, ids, sh
