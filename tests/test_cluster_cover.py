"""CPU: greedy set cover of the cluster stage.  The sequential statement of lz-ani_amd/csrc/lzani_cluster_plan.h (through the
pure export lzani_cluster_host, algorithm 4) against tests/cluster_cover_model.py on the graphs of tests/cluster_graphs.py;
the model's round form against its sequential form, which is the test of the argument that the device's rounds are exact
(include/lzani.h); the named cases; the argument errors.  No GPU."""
import numpy as np
import pytest

import cluster_cover_model as CC
import cluster_graphs as G
import cluster_model as CM
import lzani_ctypes as L

ALGO = "set-cover"


@pytest.fixture(scope="module", autouse=True)
def lib():
    L.build_library()
    return L.load_library()


@pytest.fixture(scope="module")
def cases():
    """name -> (n, a, b, w, the model's rep_of): the made-up graphs, the planted families and the six-node graph; the
    model's answer computed once and left unchanged"""
    out = dict(G.graphs())
    out["families"] = G.families()[:4]
    n, e = CC.SIX
    out["six"] = (n, np.array([p[0] for p in e], dtype=np.uint32), np.array([p[1] for p in e], dtype=np.uint32), np.ones(len(e)))
    for name, (n, a, b, w) in list(out.items()):
        rep = CC.cover(n, CM.edge_set(a, b, w))
        rep.setflags(write=False)
        out[name] = (n, a, b, w, rep)
    return out


def host(n, a, b, w, algo=ALGO):
    return L.cluster_host(n, L.cluster_edges(a, b, w), algo)


def test_the_id_is_four():
    assert L.CLUSTER_ALGOS[ALGO] == 4 and 3 not in L.CLUSTER_ALGOS.values()


def test_host_statement_against_the_model(cases):
    for name, (n, a, b, w, rep) in cases.items():
        got_rep, got_cl, k = host(n, a, b, w)
        assert np.array_equal(got_rep, rep), name
        cl, clusters = CC.number(rep)
        assert np.array_equal(got_cl, cl) and k == clusters, name
        assert (got_rep[got_rep] == got_rep).all(), name              # a representative represents itself
        if name in G.RANDOM:                                          # the model alone shows what the random cases must show
            sizes = np.bincount(rep, minlength=n)
            assert 1 < clusters < n and sizes.max() >= 3 and (sizes == 1).any(), name
            assert (rep > np.arange(n)).any(), name                   # unlike the greedy forms: a representative above a member


def test_rounds_equal_the_sequential_statement(cases):
    rounds = {}
    for name, (n, a, b, w, rep) in cases.items():
        got, rounds[name] = CC.cover_rounds(n, CM.edge_set(a, b, w))
        assert np.array_equal(got, rep), name
        assert 1 <= rounds[name] <= n, name
    # a path with ascending ids: three nodes a round; a clique per family: its smallest id wins the tie at once
    assert rounds["path_asc"] == 100 and rounds["families"] == 1 and rounds["six"] == 2
    # some hundred random graphs of up to 40 nodes, from near-empty to dense: ties throughout (small counts, many nodes)
    rng = np.random.default_rng(2024)
    several = 0
    for i in range(300):
        n = int(rng.integers(1, 41))
        m = int(rng.integers(0, 3 * n + 1)) if n > 1 else 0
        a = rng.integers(0, n, m)
        b = (a + rng.integers(1, max(n, 2), m)) % n if n > 1 else a
        es = CM.edge_set(a, b)
        want = CC.cover(n, es)
        got, r = CC.cover_rounds(n, es)
        assert np.array_equal(got, want), (i, n, sorted(es))
        assert np.array_equal(host(n, a, b, np.ones(m))[0], want), (i, n, sorted(es))     # ... and the host statement on them
        several += r > 1
    assert several > 100                                              # the rounds were not all trivial


def test_named_cases(cases):
    # where a one-hop maximum goes wrong: first 3 with c = 3, then the tie of 0 and 1 at c = 1 goes to 0
    n, a, b, w, rep = cases["six"]
    assert rep.tolist() == [0, 0, 3, 3, 3, 3] and host(n, a, b, w)[0].tolist() == [0, 0, 3, 3, 3, 3]
    # the centre of a star is the representative wherever its id lies; greedy-first takes the first id
    n, a, b, w, rep = cases["star_last"]
    got = host(n, a, b, w)
    assert got[0].tolist() == [49] * 50 and got[2] == 1 and got[1].tolist() == [0] * 50
    assert host(n, a, b, w, "greedy-first")[0][0] == 0 and host(n, a, b, w, "greedy-first")[2] > 1
    n, a, b, w, rep = cases["star_0"]
    assert host(n, a, b, w)[0].tolist() == [0] * 50
    # two cliques of six and the bridge (5, 6): by the model, two clusters -- node 5 has the largest c, 6, and takes its
    # clique and node 6 with it; 7 .. 11 are left with c = 4 each, and the tie goes to 7
    n, a, b, w, rep = cases["cliques_bridge"]
    got = host(n, a, b, w)
    assert np.array_equal(got[0], rep) and got[2] == len(set(rep.tolist())) == 2
    assert rep.tolist() == [5] * 7 + [7] * 5
    # weights play no part
    n, a, b, w, rep = cases["best_not_first"]
    assert np.array_equal(host(n, a, b, w)[0], host(n, a, b, np.ones(len(a)))[0])
    # no edge: every node its own representative
    assert host(5, [], [], [])[0].tolist() == [0, 1, 2, 3, 4] and host(1, [], [], [])[2] == 1


def test_order_repetition_and_orientation(cases):
    n, a, b, w, rep = cases["small_random"]
    p = np.random.default_rng(3).permutation(len(a))
    want = host(n, a, b, w)
    assert np.array_equal(want[0], rep)
    for aa, bb, ww in ((a[p], b[p], w[p]), (b, a, w), (np.tile(a, 2), np.tile(b, 2), np.tile(w, 2)),
                       (np.concatenate((a, b)), np.concatenate((b, a)), np.tile(w, 2)), (np.tile(a[p], 3), np.tile(b[p], 3), np.tile(w[p], 3))):
        got = host(n, aa, bb, ww)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def test_argument_errors():
    ok = L.cluster_edges([0], [1], [0.5])
    assert L.cluster_host(3, ok, 4)[0].tolist() == [0, 0, 2]
    for algo in (3, 5, -1):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            L.cluster_host(3, ok, algo)
    for bad in (L.cluster_edges([1], [1], [0.5]),            # a == b
                L.cluster_edges([0], [3], [0.5]),            # an id >= n
                L.cluster_edges([3], [0], [0.5]),
                L.cluster_edges([0], [1], [float("nan")]),
                L.cluster_edges([0], [1], [-0.25])):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            L.cluster_host(3, bad, ALGO)
