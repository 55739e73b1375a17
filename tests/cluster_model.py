"""The cluster stage in plain Python / numpy, written from the definitions and not from the product's code.
Graph: nodes 0 .. n - 1; the edge {a, b} exists iff it was added, once or several times, in either order.
Weight of the pair a < b with X = result of (ref a, query b), Y = result of (ref b, query a), la / lb the reported lengths
and `lines` of the output filter (bit 0: line 0, bit 1: line 1), float64 divisions of exact integers, sums in 32 bits:
    tani   (X.m + Y.m) / (la + lb) for both lines
    gani   line 0: X.m / lb; line 1: Y.m / la
    ani    line 0: X.m / (X.m + X.l), or 0 where X.m + X.l == 0; line 1: the same with Y
w = the largest value over the lines that `lines` names; NaN reads as 0 (as does anything not above 0); inf stays.
rep_of: single = the smallest id of the connected component; greedy-first = ids ascending, v is a representative iff no
earlier representative is its neighbour, else the smallest neighbouring representative; greedy-best = the same
representatives, else the neighbouring representative below v with the largest w, ties to the smallest.
cluster_of[v] = the number of representatives below rep_of[v]."""
import numpy as np

ALGOS = ("single", "greedy-first", "greedy-best")
MEASURES = ("tani", "gani", "ani")


def _i32(v):
    return np.asarray(v, dtype=np.int64).astype(np.int32)


def values(measure, x, y, la, lb):
    """float64[..., 2]: the measure's value of line 0 and of line 1.  x, y: int[..., 3]."""
    x, y = _i32(x), _i32(y)
    la, lb = np.asarray(la, dtype=np.uint32), np.asarray(lb, dtype=np.uint32)
    with np.errstate(all="ignore"):
        if measure == "tani":
            t = (x[..., 0] + y[..., 0]).astype(np.float64) / (la + lb).astype(np.float64)
            return np.stack((t, t), axis=-1)
        if measure == "gani":
            return np.stack((x[..., 0].astype(np.float64) / lb.astype(np.float64), y[..., 0].astype(np.float64) / la.astype(np.float64)), axis=-1)
        assert measure == "ani"
        out = []
        for r in (x, y):
            al = r[..., 0] + r[..., 1]                                            # int32 sum
            out.append(np.where(al != 0, r[..., 0].astype(np.float64) / np.where(al != 0, al, 1).astype(np.float64), 0.0))
        return np.stack(out, axis=-1)


def weight(measure, x, y, lines, la, lb):
    v = values(measure, x, y, la, lb)
    with np.errstate(invalid="ignore"):
        v = np.where(v > 0, v, 0.0)                                               # NaN -> 0
    lines = np.asarray(lines, dtype=np.uint32)
    named = np.stack(((lines & 1) != 0, (lines & 2) != 0), axis=-1)
    return np.where(named, v, 0.0).max(axis=-1)


def edge_set(a, b, w=None):
    """{(lo, hi): w}: an edge added twice is there once."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    w = np.ones(len(a)) if w is None else np.asarray(w, dtype=np.float64)
    return {(int(min(p, q)), int(max(p, q))): float(x) for p, q, x in zip(a, b, w)}


def single(n, es):
    """components by repeated label minimum"""
    lab = np.arange(n, dtype=np.int64)
    if not es:
        return lab
    a = np.array([e[0] for e in es], dtype=np.int64)
    b = np.array([e[1] for e in es], dtype=np.int64)
    while True:
        m = np.minimum(lab[a], lab[b])
        new = lab.copy()
        np.minimum.at(new, a, m)
        np.minimum.at(new, b, m)
        if np.array_equal(new, lab):
            return lab
        lab = new


def greedy(n, es, best):
    below = [[] for _ in range(n)]                                                # the neighbours below each node
    for (lo, hi), w in es.items():
        below[hi].append((lo, w))
    rep = np.zeros(n, dtype=np.int64)
    is_rep = [False] * n
    for v in range(n):
        reps = [(r, w) for r, w in below[v] if is_rep[r]]
        if not reps:
            is_rep[v] = True
            rep[v] = v
        elif best:
            top = max(w for _, w in reps)
            rep[v] = min(r for r, w in reps if w == top)
        else:
            rep[v] = min(r for r, _ in reps)
    return rep


def number(rep_of):
    n = len(rep_of)
    is_rep = rep_of == np.arange(n)
    before = np.concatenate(([0], np.cumsum(is_rep)))
    return before[rep_of], int(is_rep.sum())


def cluster(n, es, algo):
    """(rep_of, cluster_of, stats) with stats = dict(clusters, singletons, largest)."""
    rep = single(n, es) if algo == "single" else greedy(n, es, algo == "greedy-best")
    cl, k = number(rep)
    sizes = np.bincount(rep, minlength=n)
    return rep.astype(np.uint32), cl.astype(np.uint32), dict(clusters=k, singletons=int((sizes == 1).sum()), largest=int(sizes.max()))
