"""The made-up graphs of the cluster tests (tests/test_cluster.py on the host statement, tests/test_gpu_cluster.py on the
device stage): name -> (n, a, b, w), the edges as they are passed in -- either orientation, any order."""
import numpy as np

RANDOM = ("random_4000", "random_15000")            # must show 1 < clusters < n, a cluster of three or more, a singleton


def _arr(n, edges):
    a = np.array([e[0] for e in edges], dtype=np.uint32)
    b = np.array([e[1] for e in edges], dtype=np.uint32)
    w = np.array([e[2] for e in edges], dtype=np.float64)
    return n, a, b, w


def _levels(rng, m):
    """weights from a few levels, so that ties occur"""
    return rng.choice([0.0, 0.25, 0.5, 0.75, 0.9, 0.95, 1.0], m)


def _random(n, m, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n, m)
    b = (a + rng.integers(1, n, m)) % n              # never a == b; some pairs twice, in either orientation
    w = {}
    for p, q, x in zip(a, b, _levels(rng, m)):       # an edge given twice carries one weight
        w.setdefault((min(p, q), max(p, q)), x)
    return n, a.astype(np.uint32), b.astype(np.uint32), np.array([w[(min(p, q), max(p, q))] for p, q in zip(a, b)])


def _families(fams, size, seed):
    rng = np.random.default_rng(seed)
    n = fams * size
    ids = rng.permutation(n)
    iu = np.triu_indices(size, 1)
    a = np.concatenate([ids[f * size + iu[0]] for f in range(fams)])
    b = np.concatenate([ids[f * size + iu[1]] for f in range(fams)])
    return n, a.astype(np.uint32), b.astype(np.uint32), _levels(rng, len(a)), ids.reshape(fams, size)


def path(n, order):
    rng = np.random.default_rng(7)
    if order == "asc":
        return _arr(n, [(i, i + 1, 0.5) for i in range(n - 1)])
    if order == "desc":                              # from the far end, the higher id first
        return _arr(n, [(i + 1, i, 0.5) for i in range(n - 2, -1, -1)])
    ids = rng.permutation(n)
    return _arr(n, [(int(ids[i]), int(ids[i + 1]), 0.5) for i in range(n - 1)])


def cliques_with_bridge():
    e = [(i, j, 0.8) for c in (0, 6) for i in range(c, c + 6) for j in range(i + 1, c + 6)]
    return _arr(12, e + [(5, 6, 0.3)])


def graphs():
    g = {
        "empty_1": _arr(1, []),
        "empty_5": _arr(5, []),
        "one_edge": _arr(4, [(3, 1, 0.7)]),
        "path_asc": path(300, "asc"),
        "path_desc": path(300, "desc"),
        "path_shuffled": path(300, "shuffled"),
        "star_0": _arr(50, [(0, i, i / 50) for i in range(1, 50)]),
        "star_last": _arr(50, [(i, 49, i / 50) for i in range(49)]),
        "cliques_bridge": cliques_with_bridge(),
        # node 2 with the representatives 0 and 1 below it
        "best_not_first": _arr(4, [(0, 2, 0.5), (1, 2, 0.9)]),
        "tie": _arr(4, [(1, 2, 0.9), (0, 2, 0.9)]),
        # node 1 between the representatives 0 and 2: the one above has the largest weight and does not count
        "rep_above": _arr(3, [(0, 1, 0.3), (1, 2, 0.9)]),
        "inf_weight": _arr(3, [(0, 2, 5.0), (1, 2, float("inf"))]),
        "random_4000": _random(10000, 4000, 11),
        "random_15000": _random(10000, 15000, 12),
        "small_random": _random(500, 700, 13),
    }
    return g


_FAM = None


def families():
    """200 planted families of 50 with shuffled ids, each a clique: (n, a, b, w, members[200, 50])"""
    global _FAM
    if _FAM is None:
        _FAM = _families(200, 50, 14)
    return _FAM
