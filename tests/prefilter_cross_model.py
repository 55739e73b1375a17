"""The cross form of the k-mer prefilter (include/lzani.h: lzani_prefilter_cross) as a numpy statement: the kept pairs of
tests/prefilter_model.py restricted to a < n_ref <= b -- references 0 .. n_ref - 1 against queries n_ref .. n - 1 -- in the
same CSR shape, the rows from n_ref on empty."""
import numpy as np

import prefilter_model as PM


def restrict(row_off, ids, shared, n_ref):
    """The CSR (row_off[n + 1], ids, shared) of kept pairs a < b cut down to the pairs a < n_ref <= b."""
    n = len(row_off) - 1
    a = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_off.astype(np.int64)))
    ok = (a < n_ref) & (ids.astype(np.int64) >= n_ref)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.bincount(a[ok], minlength=n))
    return off, ids[ok], shared[ok]


def kept_pairs(kmers_of, shared, n_ref, min_shared=1, min_ratio=0.0):
    """PM.kept_pairs restricted to the cross pairs: (row_off[n + 1], ids, shared values)."""
    return restrict(*PM.kept_pairs(kmers_of, shared, min_shared, min_ratio), n_ref)


def prefilter_cross(seqs, k, n_ref, sample_max=PM.SAMPLE_ALL, min_shared=1, min_ratio=0.0):
    """What lzani_prefilter_cross + lzani_prefilter_fetch return: kmers_of, row_off, ids, shared."""
    kmers_of, shared = PM.shared_matrix(seqs, k, sample_max)
    return (kmers_of.astype(np.uint32),) + kept_pairs(kmers_of, shared, n_ref, min_shared, min_ratio)
