"""Greedy set cover of the cluster stage in plain Python / numpy, written from the definition and not from the product's code.
Graph: nodes 0 .. n - 1 and the distinct edges of an edge set ({(lo, hi): w} of cluster_model.edge_set, or any iterable of
pairs); weights play no part.
cover: all nodes start unassigned.  While a node is unassigned: c(v) = the number of unassigned neighbours of the unassigned
node v; the unassigned v with the largest c(v), ties to the smallest id, becomes a representative, and every unassigned
neighbour of v gets v as its representative.
cover_rounds: the round form.  key(v) = c(v) << 32 | (0xFFFFFFFF - v) for an unassigned v.  A round looks at the unassigned
nodes as they are at its start, selects every one whose key is the largest among the unassigned nodes within two hops
(itself, its unassigned neighbours, theirs), and every selected node covers its unassigned neighbours as of the start."""
import numpy as np


def neighbours(n, edge_set):
    nb = [set() for _ in range(n)]
    for a, b in edge_set:
        a, b = int(a), int(b)
        assert a != b
        nb[a].add(b)
        nb[b].add(a)
    return nb


def cover(n, edge_set):
    """rep_of by the sequential statement: a naive arg-max per step over (c, -id) of the unassigned nodes, with c kept as
    the count of unassigned neighbours (one less for every neighbour that is assigned)."""
    nb = neighbours(n, edge_set)
    rep = np.full(n, -1, dtype=np.int64)
    c = np.array([len(s) for s in nb], dtype=np.int64)
    ids = np.arange(n, dtype=np.int64)
    left = n
    while left:
        order = np.where(rep == -1, c * n + (n - 1 - ids), -1)                    # largest c, then smallest id; assigned: out
        v = int(np.argmax(order))
        members = [v] + [u for u in nb[v] if rep[u] == -1]
        for u in members:
            rep[u] = v
        for u in members:
            for y in nb[u]:
                c[y] -= 1                                                         # (of an assigned y it is no longer read)
        left -= len(members)
    return rep.astype(np.uint32)


def cover_rounds(n, edge_set):
    """(rep_of, rounds) by the rounds; rounds = the number of the first round that left no node unassigned (1 for n == 0
    is never asked: n >= 1)."""
    nb = neighbours(n, edge_set)
    rep = np.full(n, -1, dtype=np.int64)
    free = set(range(n))
    rounds = 0
    while free:
        rounds += 1
        live = {v: nb[v] & free for v in free}                                    # the snapshot
        key = {v: (len(live[v]) << 32) | (0xFFFFFFFF - v) for v in free}
        m1 = {v: max([key[v]] + [key[u] for u in live[v]]) for v in free}
        m2 = {v: max([m1[v]] + [m1[u] for u in live[v]]) for v in free}
        selected = [v for v in free if m2[v] == key[v]]
        for v in selected:
            rep[v] = v
            for u in live[v]:
                assert rep[u] == -1 and u not in selected                         # two selected nodes are more than two hops apart
                rep[u] = v
        free = {v for v in free if rep[v] == -1}
    return rep.astype(np.uint32), rounds


def number(rep_of):
    """cluster_of and the number of clusters: clusters in ascending order of their representative."""
    rep_of = np.asarray(rep_of, dtype=np.int64)
    is_rep = rep_of == np.arange(len(rep_of))
    before = np.concatenate(([0], np.cumsum(is_rep)))
    return before[rep_of].astype(np.uint32), int(is_rep.sum())


SIX = (6, [(0, 1), (1, 2), (2, 3), (3, 4), (3, 5)])       # where a one-hop maximum goes wrong: rep_of = 0 0 3 3 3 3
