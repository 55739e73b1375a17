"""CPU: the rule and the sequential statement of the cluster stage (lz-ani_amd/csrc/lzani_cluster_plan.h through the pure
exports lzani_cluster_weight and lzani_cluster_host) against tests/cluster_model.py: the weights on made-up records, the
three algorithms on the graphs of tests/cluster_graphs.py, the argument errors.  No GPU."""
import numpy as np
import pytest

import cluster_graphs as G
import cluster_model as CM
import lzani_ctypes as L


@pytest.fixture(scope="module", autouse=True)
def lib():
    L.build_library()
    return L.load_library()


def bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


def test_weight_against_the_model():
    rng = np.random.default_rng(1)
    k = 400
    la, lb = rng.integers(1000, 5000, k).astype(np.uint32), rng.integers(1000, 5000, k).astype(np.uint32)
    x = np.stack((rng.integers(0, 3000, k), rng.integers(0, 900, k), rng.integers(0, 30, k)), axis=1).astype(np.int32)
    y = np.stack((rng.integers(0, 3000, k), rng.integers(0, 900, k), rng.integers(0, 30, k)), axis=1).astype(np.int32)
    # a printed length of 0: inf where matches are there, NaN -> 0 where none are; no aligned symbols at all
    la[:6] = 0
    lb[3:9] = 0
    x[:12:2, 0] = 0
    y[1:12:3, 0] = 0
    x[20:24, :2] = 0
    y[22:26, :2] = 0
    seen_inf = seen_zero_from_nan = False
    for measure in CM.MEASURES:
        for lines in (1, 2, 3):
            want = CM.weight(measure, x, y, np.full(k, lines), la, lb)
            got = np.array([L.cluster_weight(measure, x[i], y[i], lines, la[i], lb[i]) for i in range(k)])
            assert np.array_equal(bits(got), bits(want)), (measure, lines)
            assert not np.isnan(got).any() and (got >= 0).all()
            seen_inf |= bool(np.isinf(got).any())
            v = CM.values(measure, x, y, la, lb)
            seen_zero_from_nan |= bool((np.isnan(v[:, 0]) & (got == 0)).any()) if lines == 1 else False
    assert seen_inf and seen_zero_from_nan
    # the largest of the two lines; one line alone
    assert L.cluster_weight("gani", (100, 0, 1), (300, 0, 1), 3, 1000, 1000) == 300 / 1000
    assert L.cluster_weight("gani", (100, 0, 1), (300, 0, 1), 1, 1000, 1000) == 100 / 1000
    assert L.cluster_weight("gani", (100, 0, 1), (300, 0, 1), 2, 1000, 1000) == 300 / 1000
    assert L.cluster_weight("ani", (0, 0, 0), (0, 0, 0), 3, 10, 10) == 0.0
    assert L.cluster_weight("tani", (5, 0, 1), (0, 0, 1), 3, 0, 0) == float("inf")
    assert L.cluster_weight("tani", (0, 0, 1), (0, 0, 1), 3, 0, 0) == 0.0          # 0 / 0
    assert np.isnan(L.cluster_weight(3, (1, 1, 1), (1, 1, 1), 3, 10, 10)) and np.isnan(L.cluster_weight(-1, (1, 1, 1), (1, 1, 1), 3, 10, 10))


@pytest.fixture(scope="module")
def graphs():
    return G.graphs()


@pytest.mark.parametrize("algo", CM.ALGOS)
def test_host_statement_against_the_model(graphs, algo):
    for name, (n, a, b, w) in graphs.items():
        rep, cl, st = CM.cluster(n, CM.edge_set(a, b, w), algo)
        got_rep, got_cl, k = L.cluster_host(n, L.cluster_edges(a, b, w), algo)
        assert np.array_equal(got_rep, rep), name
        assert np.array_equal(got_cl, cl) and k == st["clusters"], name
        if name in G.RANDOM:                                # the model alone shows what the random cases must show
            assert 1 < st["clusters"] < n and st["largest"] >= 3 and st["singletons"] >= 1, (name, st)


def test_families_and_what_the_graphs_must_show(graphs):
    n, a, b, w, members = G.families()
    assert len(a) == 245000
    rep, _, k = L.cluster_host(n, L.cluster_edges(a, b, w), "single")
    assert k == 200
    for fam in members:
        assert (rep[fam] == fam.min()).all()
    for algo in CM.ALGOS[1:]:
        assert np.array_equal(L.cluster_host(n, L.cluster_edges(a, b, w), algo)[0], CM.cluster(n, CM.edge_set(a, b, w), algo)[0])
    # single joins the two cliques, greedy does not
    n, a, b, w = graphs["cliques_bridge"]
    e = L.cluster_edges(a, b, w)
    assert L.cluster_host(n, e, "single")[2] == 1
    for algo in CM.ALGOS[1:]:
        rep = L.cluster_host(n, e, algo)[0]
        assert rep.tolist() == [0] * 6 + [6] * 6
    # first and best part where the weights say so, and only there
    first = lambda name: L.cluster_host(graphs[name][0], L.cluster_edges(*graphs[name][1:]), "greedy-first")[0].tolist()
    best = lambda name: L.cluster_host(graphs[name][0], L.cluster_edges(*graphs[name][1:]), "greedy-best")[0].tolist()
    assert first("best_not_first") == [0, 1, 0, 3] and best("best_not_first") == [0, 1, 1, 3]
    assert first("tie") == best("tie") == [0, 1, 0, 3]
    assert first("rep_above") == best("rep_above") == [0, 0, 2]
    assert first("inf_weight") == [0, 1, 0] and best("inf_weight") == [0, 1, 1]


def test_order_repetition_and_orientation(graphs):
    n, a, b, w = graphs["small_random"]
    rng = np.random.default_rng(3)
    p = rng.permutation(len(a))
    for algo in CM.ALGOS:
        want = L.cluster_host(n, L.cluster_edges(a, b, w), algo)
        for aa, bb, ww in ((a[p], b[p], w[p]), (b, a, w), (np.tile(a, 2), np.tile(b, 2), np.tile(w, 2)),
                           (np.concatenate((a, b)), np.concatenate((b, a)), np.tile(w, 2))):
            got = L.cluster_host(n, L.cluster_edges(aa, bb, ww), algo)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def test_argument_errors():
    ok = L.cluster_edges([0], [1], [0.5])
    assert L.cluster_host(3, ok, "single")[2] == 2
    for bad in (L.cluster_edges([1], [1], [0.5]),            # a == b
                L.cluster_edges([0], [3], [0.5]),            # an id >= n
                L.cluster_edges([3], [0], [0.5]),
                L.cluster_edges([0], [1], [float("nan")]),
                L.cluster_edges([0], [1], [-0.25])):
        for algo in CM.ALGOS:
            with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
                L.cluster_host(3, bad, algo)
    for algo in (3, -1):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            L.cluster_host(3, ok, algo)
