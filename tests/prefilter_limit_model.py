"""The prefilter's limit stage (include/lzani.h: lzani_prefilter_limit) in Python integers, straight from its definition:
every limiting genome's list of partners sorted by (-q, partner), the first N of every list marked.  No device trick."""
import numpy as np

Q_ONE = (1 << 32) - 1


def score(shared, ka, kb):
    """q = floor(shared * (2^32 - 1) / min(|K(a)|, |K(b)|)) in Python integers."""
    return int(shared) * Q_ONE // min(int(ka), int(kb))


def pairs_of(row_off, ids):
    """(a, b) of every CSR entry."""
    a = np.repeat(np.arange(len(row_off) - 1, dtype=np.int64), np.diff(np.asarray(row_off).astype(np.int64)))
    return a, np.asarray(ids).astype(np.int64)


def lists(n, n_ref, kmers_of, row_off, ids, shared):
    """Per limiting genome its list: (-q, partner, entry), sorted.  n_ref 0: every genome limits; else the queries only."""
    a, b = pairs_of(row_off, ids)
    out = {g: [] for g in range(n) if not n_ref or g >= n_ref}
    for e, (x, y, s) in enumerate(zip(a.tolist(), b.tolist(), np.asarray(shared).tolist())):
        q = score(s, kmers_of[x], kmers_of[y])
        if x in out:
            out[x].append((-q, y, e))
        if y in out:
            out[y].append((-q, x, e))
    for lst in out.values():
        lst.sort()
    return out


def limit(n, n_ref, kmers_of, row_off, ids, shared, N):
    """keep uint8[e]: 1 where the entry's pair is among the N best of one of its limiting endpoints."""
    keep = np.zeros(len(ids), dtype=np.uint8)
    for lst in lists(n, n_ref, kmers_of, row_off, ids, shared).values():
        for _, _, e in lst[:N]:
            keep[e] = 1
    return keep


def counts(n, n_ref, kmers_of, row_off, ids, shared, N):
    """(limiting genomes, genomes whose list is longer than N)."""
    ls = lists(n, n_ref, kmers_of, row_off, ids, shared)
    return len(ls), sum(len(lst) > N for lst in ls.values())


def apply(row_off, ids, shared, keep):
    """The CSR restricted to keep: (row_off, ids, shared)."""
    a, _ = pairs_of(row_off, ids)
    k = keep.astype(bool)
    cnt = np.bincount(a[k], minlength=len(row_off) - 1)
    off = np.concatenate(([0], np.cumsum(cnt))).astype(np.uint64)
    return off, np.asarray(ids, dtype=np.uint32)[k], np.asarray(shared, dtype=np.uint32)[k]


def csr_of(n, edges):
    """CSR (row_off, ids, shared) of a dict {(a, b): shared} with a < b."""
    items = sorted(edges.items())
    a = np.array([x[0][0] for x in items], dtype=np.int64)
    off = np.concatenate(([0], np.cumsum(np.bincount(a, minlength=n) if len(a) else np.zeros(n, dtype=np.int64)))).astype(np.uint64)
    return off, np.array([x[0][1] for x in items], dtype=np.uint32), np.array([x[1] for x in items], dtype=np.uint32)


def random_result(seed, n, p, n_ref=0, values=(250, 500, 1000), k_of=1000):
    """A made-up prefilter result: every pair a < b (cross form: a < n_ref <= b) is kept with probability p, |K| = k_of for
    every genome and shared drawn from `values`, so that q takes len(values) values and ties dominate."""
    rng = np.random.default_rng(seed)
    a, b = np.triu_indices(n, 1)
    if n_ref:
        cross = (a < n_ref) & (b >= n_ref)
        a, b = a[cross], b[cross]
    pick = rng.random(len(a)) < p
    a, b = a[pick], b[pick]
    shared = rng.choice(np.asarray(values, dtype=np.uint32), size=len(a)).astype(np.uint32)
    off = np.concatenate(([0], np.cumsum(np.bincount(a, minlength=n)))).astype(np.uint64)
    return np.full(n, k_of, dtype=np.uint32), off, b.astype(np.uint32), shared
