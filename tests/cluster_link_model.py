"""Complete linkage of the cluster stage in plain Python / numpy, written from the definition and not from the product's code.
Graph: nodes 0 .. n - 1 and the distinct pairs of the edge records (a, b, w), either orientation; the weight of an edge is the
smallest w over its records (a value that is not above 0 reads as 0; an edge of weight 0 is an edge).  Every node starts as a
cluster; id(C) = its smallest member.  Two clusters A, B are linked iff every pair {a, b}, a in A, b in B, is an edge; the
link's value s is the smallest weight among those |A| * |B| edges.
linkage (i): while a link exists, the link with the largest s, ties to the smallest lower id, then to the smallest other id,
is taken and its clusters merge.  Every step recomputes every link from the edges; nothing is carried over but the partition.
linkage_rounds (ii): the round form.  From a cluster's own point of view its best link is the one with the largest s, ties
to the smallest neighbouring id; in a round every pair of clusters that are each other's best link merges.
links: the links of a partition, from the definition: what the property checks and the random schedules read."""
import functools

import numpy as np


def edge_min(a, b, w=None):
    """{(lo, hi): w}: the distinct edges, each with the smallest weight of its records."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    w = np.ones(len(a)) if w is None else np.asarray(w, dtype=np.float64)
    es = {}
    for p, q, x in zip(a.tolist(), b.tolist(), w.tolist()):
        assert p != q
        k = (min(p, q), max(p, q))
        x = x if x > 0 else 0.0
        es[k] = min(es.get(k, x), x)
    return es


def links(es, rep):
    """{(A, B): s}, A < B: the links of the partition that rep (node -> id of its cluster) describes."""
    size = np.bincount(np.asarray(rep, dtype=np.int64))
    got = {}
    for (lo, hi), w in es.items():
        A, B = int(rep[lo]), int(rep[hi])
        if A == B:
            continue
        k = (min(A, B), max(A, B))
        c, s = got.get(k, (0, w))
        got[k] = (c + 1, min(s, w))
    return {k: s for k, (c, s) in got.items() if c == int(size[k[0]]) * int(size[k[1]])}


def _components(n, es):
    lab = list(range(n))

    def root(v):
        while lab[v] != v:
            lab[v] = lab[lab[v]]
            v = lab[v]
        return v
    for lo, hi in es:
        ra, rb = root(lo), root(hi)
        if ra != rb:
            lab[max(ra, rb)] = min(ra, rb)
    parts = {}
    for (lo, hi), w in es.items():
        parts.setdefault(root(lo), []).append((lo, hi, w))
    return parts.values()


def linkage(n, es):
    """rep_of by the sequential statement (i).  A link lies inside one connected component and a merge changes no link of
    another, so the global order restricted to a component is that component's own order: the components are taken one by
    one, and inside one every step recomputes all its links (count and smallest weight per pair of clusters, over all
    edges) with numpy."""
    rep = np.arange(n, dtype=np.int64)
    size = np.ones(n, dtype=np.int64)
    for part in _components(n, es):
        la = np.array([e[0] for e in part], dtype=np.int64)                       # the cluster of the lower end, of the other end
        lb = np.array([e[1] for e in part], dtype=np.int64)
        w = np.array([e[2] for e in part], dtype=np.float64)
        while True:
            lo, hi = np.minimum(la, lb), np.maximum(la, lb)
            m = lo != hi
            if not m.any():
                break
            key = lo[m] * n + hi[m]
            order = np.argsort(key, kind="stable")
            ks, ws = key[order], w[m][order]
            start = np.flatnonzero(np.concatenate(([True], ks[1:] != ks[:-1])))
            cnt = np.diff(np.concatenate((start, [len(ks)])))
            s = np.minimum.reduceat(ws, start)
            A, B = ks[start] // n, ks[start] % n
            full = cnt == size[A] * size[B]
            if not full.any():
                break
            A, B, s = A[full], B[full], s[full]
            top = s == s.max()
            A, B = A[top], B[top]
            i = np.lexsort((B, A))[0]                                             # the smallest lower id, then the smallest other id
            x, y = int(A[i]), int(B[i])
            la[la == y] = x
            lb[lb == y] = x
            rep[rep == y] = x
            size[x] += size[y]
    return rep.astype(np.uint32)


def linkage_rounds(n, es):
    """(rep_of, merges of every round, rounds) by the round form (ii); rounds = the number of the first round that merged
    nothing, 1 for an edgeless graph.  The entries of a round are the last round's links relabelled (a pair that is no link
    is never one again: no superset of an incomplete pair is complete), at first the edges."""
    label, size, rep = list(range(n)), [1] * n, list(range(n))
    entries = {k: (1, w) for k, w in es.items()}
    merges = []
    while True:
        table = {}
        for (ca, cb), (c, w) in entries.items():
            ca, cb = label[ca], label[cb]
            if ca == cb:
                continue
            k = (min(ca, cb), max(ca, cb))
            c0, w0 = table.get(k, (0, w))
            table[k] = (c0 + c, min(w0, w))
        entries = {k: v for k, v in table.items() if v[0] == size[k[0]] * size[k[1]]}
        best = {}                                                                 # cluster -> (-s, id) of its best link, the smallest wins
        for (ca, cb), (c, w) in entries.items():
            best[ca] = min(best.get(ca, (-w, cb)), (-w, cb))
            best[cb] = min(best.get(cb, (-w, ca)), (-w, ca))
        pairs = [(x, y) for x, (_, y) in best.items() if x < y and best[y][1] == x]
        merges.append(len(pairs))
        if not pairs:
            return np.array(rep, dtype=np.uint32), merges, len(merges)
        for x, y in pairs:
            label[y] = x
            size[x] += size[y]
        rep = [label[r] for r in rep]


def number(rep_of):
    """cluster_of and the number of clusters: clusters in ascending order of their representative."""
    rep_of = np.asarray(rep_of, dtype=np.int64)
    is_rep = rep_of == np.arange(len(rep_of))
    before = np.concatenate(([0], np.cumsum(is_rep)))
    return before[rep_of].astype(np.uint32), int(is_rep.sum())


def complete_graph(n):
    """the complete graph with w(i, j) = 1 - max(i, j) / n: by (ii) exactly one merge a round"""
    iu = np.triu_indices(n, 1)
    return n, iu[0].astype(np.uint32), iu[1].astype(np.uint32), 1.0 - iu[1] / n


@functools.lru_cache(maxsize=None)
def reference(name):
    """(n, a, b, w, rep_of by (i)) of a graph of tests/cluster_graphs.py or of "families", computed once per process and
    left unchanged."""
    import cluster_graphs as G
    n, a, b, w = G.families()[:4] if name == "families" else G.graphs()[name]
    rep = linkage(n, edge_min(a, b, w))
    rep.setflags(write=False)
    return n, a, b, w, rep


def names():
    import cluster_graphs as G
    return tuple(G.graphs()) + ("families",)
