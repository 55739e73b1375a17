"""A literal statement of LZANI_CLUSTER_LEIDEN (include/lzani.h, "clustering the kept pairs"): dicts and loops.

leiden(n, edges, gamma, iterations) -> dict with rep_of, cluster_of, clusters, the counts that lzani_cluster_leiden_info
reports, and `trace`: the integer quality Q of the level after every moving round.  The model asserts that Q rises
strictly, by exactly the sum of the movers' D, in every moving round that moves something.
"""
import math

ONE = 1 << 20
ALONE = "alone"


class RoundCap(Exception):
    """A phase has run cap_mul * n_level + cap_add rounds (LZANI_ERR_DEVICE on the host and the device)."""


def quantise(w):
    return ONE if w >= 1.0 else min(int(math.floor(w * ONE)), ONE)


def resolution_q(gamma):
    return int(math.floor(gamma * ONE + 0.5))


def distinct_entries(edges):
    """{(lo, hi): q} with q of the smallest w over the records of a pair."""
    ent = {}
    for a, b, w in edges:
        key = (min(int(a), int(b)), max(int(a), int(b)))
        q = quantise(float(w))
        ent[key] = min(ent.get(key, q), q)
    return ent


class Level:
    def __init__(self, m, s, ent, P):
        self.m, self.s, self.ent, self.P = m, list(s), dict(ent), list(P)
        self.adj = [dict() for _ in range(m)]
        for (a, b), q in self.ent.items():
            self.adj[a][b] = q
            self.adj[b][a] = q

    def sizes(self, part):
        S = {}
        for v in range(self.m):
            S[part[v]] = S.get(part[v], 0) + self.s[v]
        return S

    def quality(self, g):
        inside = sum(q for (a, b), q in self.ent.items() if self.P[a] == self.P[b])
        S, sq = self.sizes(self.P), {}
        for v in range(self.m):
            sq[self.P[v]] = sq.get(self.P[v], 0) + self.s[v] * self.s[v]
        return inside - g * sum((S[c] * S[c] - sq[c]) // 2 for c in S)


def smallest_member(labels):
    low = {}
    for v, lab in enumerate(labels):
        low[lab] = min(low.get(lab, v), v)
    return [low[lab] for lab in labels]


def exclusive_movers(cand, touched):
    """cand: v -> (D, target).  The candidates that hold the largest key (largest D, then smallest v) in every community
    they touch."""
    best = {}
    for v in cand:
        key = (cand[v][0], -v)
        for c in touched(v):
            if c not in best or key > best[c]:
                best[c] = key
    return [v for v in sorted(cand) if all(best[c] == (cand[v][0], -v) for c in touched(v))]


def move_round(lv, g):
    """One moving round on lv.P; returns the number of movers and the sum of their D."""
    P, s = lv.P, lv.s
    S = lv.sizes(P)
    cand = {}
    for v in range(lv.m):
        own = P[v]
        W = {}
        for u, q in lv.adj[v].items():
            W[P[u]] = W.get(P[u], 0) + q
        val_own = W.get(own, 0) - g * s[v] * (S[own] - s[v])
        best, target = val_own, own                       # staying first
        for c in sorted(W):                               # then the smallest community id
            if c == own:
                continue
            val = W[c] - g * s[v] * S[c]
            if val > best:
                best, target = val, c
        if S[own] != s[v] and 0 > best:                   # alone last, and only for a node that is not alone
            best, target = 0, ALONE
        if best - val_own > 0:
            cand[v] = (best - val_own, target)
    movers = exclusive_movers(cand, lambda v: {P[v]} | ({cand[v][1]} if cand[v][1] != ALONE else set()))
    labels = [("c", P[v]) for v in range(lv.m)]
    for v in movers:
        labels[v] = ("a", v) if cand[v][1] == ALONE else ("c", cand[v][1])
    lv.P = smallest_member(labels)
    return len(movers), sum(cand[v][0] for v in movers)


def refine_round(lv, g, R, well):
    """One refinement round on R inside lv.P; returns the number of movers."""
    P, s = lv.P, lv.s
    SP, SR = lv.sizes(P), lv.sizes(R)
    count = {}
    for v in range(lv.m):
        count[R[v]] = count.get(R[v], 0) + 1
    ext = {}
    for (a, b), q in lv.ent.items():
        if P[a] == P[b] and R[a] != R[b]:
            ext[R[a]] = ext.get(R[a], 0) + q
            ext[R[b]] = ext.get(R[b], 0) + q
    cand = {}
    for v in range(lv.m):
        if count[R[v]] != 1 or not well[v]:
            continue
        W = {}
        for u, q in lv.adj[v].items():
            if P[u] == P[v] and R[u] != R[v]:
                W[R[u]] = W.get(R[u], 0) + q
        best = None
        for c in sorted(W):
            if W[c] <= 0 or ext.get(c, 0) < g * SR[c] * (SP[P[v]] - SR[c]):
                continue
            D = W[c] - g * s[v] * SR[c]
            if D >= 0 and (best is None or D > best[0]):
                best = (D, c)
        if best is not None:
            cand[v] = best
    movers = exclusive_movers(cand, lambda v: {R[v], cand[v][1]})
    labels = list(R)
    for v in movers:
        labels[v] = cand[v][1]
    R[:] = smallest_member(labels)
    return len(movers)


def leiden(n, edges, gamma=0.7, iterations=2, cap_mul=64, cap_add=64, start=None):
    g = resolution_q(gamma)
    ent0 = distinct_entries(edges)
    st = dict(iterations=0, levels=0, move_rounds=0, refine_rounds=0, moves=0, merges=0, resolution_q=g, distinct_edges=len(ent0))
    trace = []
    rep = list(range(n)) if start is None else smallest_member(list(start))
    for _ in range(iterations):
        st["iterations"] += 1
        lv = Level(n, [1] * n, ent0, rep)
        node_of = list(range(n))
        moved_in_iteration = 0
        while True:
            st["levels"] += 1
            cap = cap_mul * lv.m + cap_add
            moved, rounds = 0, 0
            while True:
                if rounds >= cap:
                    raise RoundCap("moving phase")
                rounds += 1
                before = lv.quality(g)
                k, gain = move_round(lv, g)
                after = lv.quality(g)
                trace.append(after)
                assert after == before + gain and (k == 0 or after > before), (before, after, gain, k)
                moved += k
                if k == 0:
                    break
            st["move_rounds"] += rounds
            st["moves"] += moved
            moved_in_iteration += moved
            if all(lv.P[v] == v for v in range(lv.m)):
                break
            SP = lv.sizes(lv.P)
            well = [sum(q for u, q in lv.adj[v].items() if lv.P[u] == lv.P[v]) >= g * lv.s[v] * (SP[lv.P[v]] - lv.s[v]) for v in range(lv.m)]
            R = list(range(lv.m))
            merged, rounds = 0, 0
            while True:
                if rounds >= cap:
                    raise RoundCap("refinement")
                rounds += 1
                k = refine_round(lv, g, R, well)
                merged += k
                if k == 0:
                    break
            st["refine_rounds"] += rounds
            st["merges"] += merged
            if moved == 0 and merged == 0:
                break
            # aggregation: the R-communities in ascending order of their smallest member
            reps = [v for v in range(lv.m) if R[v] == v]
            index = {r: i for i, r in enumerate(reps)}
            sizes = lv.sizes(R)
            ent = {}
            for (a, b), q in lv.ent.items():
                x, y = index[R[a]], index[R[b]]
                if x != y:
                    key = (min(x, y), max(x, y))
                    ent[key] = ent.get(key, 0) + q
            lv = Level(len(reps), [sizes[r] for r in reps], ent, smallest_member([lv.P[r] for r in reps]))
            node_of = [index[R[x]] for x in node_of]
        rep = smallest_member([lv.P[node_of[v]] for v in range(n)])
        if moved_in_iteration == 0:
            break
    below, k = [], 0
    for v in range(n):
        below.append(k)
        k += rep[v] == v
    final = Level(n, [1] * n, ent0, rep)
    out = dict(st)
    out.update(rep_of=rep, cluster_of=[below[rep[v]] for v in range(n)], clusters=k, quality=final.quality(g), trace=trace)
    return out
