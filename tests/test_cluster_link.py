"""CPU: complete linkage of the cluster stage.  The sequential statement of lz-ani_amd/csrc/lzani_cluster_plan.h (through the
pure export lzani_cluster_host, algorithm 6) against the literal statement of tests/cluster_link_model.py on the graphs of
tests/cluster_graphs.py; the properties that need no model (every cluster a clique, no two final clusters linked); the named
cases; the argument that the device's rounds are exact (include/lzani.h), as three schedules that must agree; the counters
of the round form; the argument errors; and the host statement in a stand-alone program under the sanitizers.  No GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cluster_graphs as G
import cluster_link_model as LM
import lzani_ctypes as L
import util as U

ALGO = "complete-linkage"


@pytest.fixture(scope="module", autouse=True)
def lib():
    L.build_library()
    return L.load_library()


def host(n, a, b, w, algo=ALGO):
    return L.cluster_host(n, L.cluster_edges(a, b, w), algo)


def edges_of(*e):
    return [p[0] for p in e], [p[1] for p in e], [p[2] for p in e]


def test_the_id_is_six():
    assert L.CLUSTER_ALGOS[ALGO] == 6 and not {3, 5} & set(L.CLUSTER_ALGOS.values()) and "complete" not in L.CLUSTER_ALGOS


def test_host_statement_against_the_model():
    for name in LM.names():
        n, a, b, w, rep = LM.reference(name)
        got_rep, got_cl, k = host(n, a, b, w)
        assert np.array_equal(got_rep, rep), name
        cl, clusters = LM.number(rep)
        assert np.array_equal(got_cl, cl) and k == clusters, name
        assert (got_rep <= np.arange(n)).all() and (got_rep[got_rep] == got_rep).all(), name      # the id is the smallest member
        if name in G.RANDOM:                                          # the model alone shows what the random cases must show
            sizes = np.bincount(rep, minlength=n)
            assert 1 < clusters < n and sizes.max() >= 2 and (sizes == 1).any(), name       # (sparse: pairs; the families and cliques show more)
    n, a, b, w, members = G.families()
    rep = LM.reference("families")[4]
    for fam in members:                                               # each planted family is a clique: one cluster
        assert (rep[fam] == fam.min()).all()


def test_every_cluster_is_a_clique_and_no_two_are_linked():
    """of the host function's answer, by the definition alone"""
    for name in LM.names():
        n, a, b, w, _ = LM.reference(name)
        rep = host(n, a, b, w)[0]
        es = LM.edge_min(a, b, w)
        inside = np.zeros(n, dtype=np.int64)
        for lo, hi in es:
            if rep[lo] == rep[hi]:
                inside[rep[lo]] += 1
        size = np.bincount(rep, minlength=n).astype(np.int64)
        assert np.array_equal(inside, size * (size - 1) // 2), name
        assert LM.links(es, rep) == {}, name


def test_named_cases():
    # the path 0-1-2 with equal weights: the tie goes to the smallest lower id, and 0-2 is no edge
    assert host(3, *edges_of((0, 1, 0.5), (1, 2, 0.5)))[0].tolist() == [0, 0, 2]
    # a 4-clique without the edge 0-3, under two weightings.  1-2 first: {1, 2} is linked with 0 and with 3 at 0.5, the
    # tie goes to the lower id 0, and 3 stays alone
    five = ((0, 1), (0, 2), (1, 2), (1, 3), (2, 3))
    w1 = {(1, 2): 0.9}
    assert host(4, *edges_of(*[(p, q, w1.get((p, q), 0.5)) for p, q in five]))[0].tolist() == [0, 0, 0, 3]
    # 2-3 first, then 0-1 at 0.8 before {2, 3}-1 at 0.5; {0, 1} and {2, 3} are not linked
    w2 = {(2, 3): 0.9, (0, 1): 0.8}
    assert host(4, *edges_of(*[(p, q, w2.get((p, q), 0.5)) for p, q in five]))[0].tolist() == [0, 0, 2, 2]
    # two cliques of six and the bridge (5, 6): single linkage chains them, complete linkage does not
    n, a, b, w = G.graphs()["cliques_bridge"]
    got = host(n, a, b, w)
    assert got[0].tolist() == [0] * 6 + [6] * 6 and got[2] == 2 and got[1].tolist() == [0] * 6 + [1] * 6
    assert host(n, a, b, w, "single")[2] == 1
    # a pair given with two weights: the smaller one decides -- 1-2 at 0.5 goes before 0-1 at 0.2, not behind 0-1 at 0.9
    assert host(3, *edges_of((0, 1, 0.9), (1, 2, 0.5), (1, 0, 0.2)))[0].tolist() == [0, 1, 1]
    assert host(3, *edges_of((0, 1, 0.9), (1, 2, 0.5)))[0].tolist() == [0, 0, 2]
    # an edge of weight 0 is an edge: it links, and it completes a clique
    assert host(2, *edges_of((1, 0, 0.0)))[0].tolist() == [0, 0]
    assert host(4, *edges_of((0, 1, 0.7), (0, 2, 0.0), (1, 2, 0.3)))[0].tolist() == [0, 0, 0, 3]
    # +inf is the largest weight
    n, a, b, w = G.graphs()["inf_weight"]
    assert host(n, a, b, w)[0].tolist() == [0, 1, 1]
    # no edge: every node its own cluster
    assert host(5, [], [], [])[0].tolist() == [0, 1, 2, 3, 4] and host(1, [], [], [])[2] == 1


def test_order_repetition_and_orientation():
    n, a, b, w, rep = LM.reference("small_random")
    p = np.random.default_rng(3).permutation(len(a))
    want = host(n, a, b, w)
    assert np.array_equal(want[0], rep)
    for aa, bb, ww in ((a[p], b[p], w[p]), (b, a, w), (np.tile(a, 2), np.tile(b, 2), np.tile(w, 2)),
                       (np.concatenate((a, b)), np.concatenate((b, a)), np.tile(w, 2)), (np.tile(a[p], 3), np.tile(b[p], 3), np.tile(w[p], 3))):
        got = host(n, aa, bb, ww)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def _random_schedule(n, es, rng):
    """one valid merge at a time, chosen at random: a pair of clusters that are each other's best link"""
    rep = np.arange(n)
    while True:
        lk = LM.links(es, rep)
        best = {}
        for (A, B), s in lk.items():
            best[A] = min(best.get(A, (-s, B)), (-s, B))
            best[B] = min(best.get(B, (-s, A)), (-s, A))
        valid = sorted((A, B) for A, (_, B) in best.items() if A < B and best[B][1] == A)
        if not valid:
            assert not lk                                             # while a link exists, the global best one is valid
            return rep.astype(np.uint32)
        A, B = valid[int(rng.integers(len(valid)))]
        rep[rep == B] = A


def test_the_three_schedules_agree():
    """the sequential statement, the rounds, and random single valid merges: one partition (the header's argument)"""
    rng = np.random.default_rng(2025)
    several = ties = 0
    for i in range(300):
        n = int(rng.integers(8, 15))
        m = int(rng.integers(n, 3 * n + 1))
        a = rng.integers(0, n, m)
        b = (a + rng.integers(1, n, m)) % n
        w = rng.choice([0.25, 0.5, 0.75], m)
        es = LM.edge_min(a, b, w)
        want = LM.linkage(n, es)
        got, merges, rounds = LM.linkage_rounds(n, es)
        assert np.array_equal(got, want), (i, n, sorted(es.items()))
        assert np.array_equal(_random_schedule(n, es, rng), want), (i, n, sorted(es.items()))
        assert np.array_equal(host(n, a, b, w)[0], want), (i, n, sorted(es.items()))
        assert rounds == len(merges) and merges[-1] == 0 and all(merges[:-1]) and sum(merges) == n - len(set(want.tolist()))
        several += rounds > 2
        ties += len(es) > 3 * len(set(es.values()))
    assert several > 100 and ties > 200                               # the rounds were not all trivial, and weights tied throughout


def test_counters_of_the_round_form():
    n, a, b, w, rep = LM.reference("path_asc")
    got, merges, rounds = LM.linkage_rounds(n, LM.edge_min(a, b, w))
    assert np.array_equal(got, rep) and rep.tolist() == [v - v % 2 for v in range(300)]
    assert rounds == 151 and sum(merges) == 150 and merges == [1] * 150 + [0]     # one reciprocal pair a round: all point downwards
    r, merges, rounds = LM.linkage_rounds(5, {})
    assert r.tolist() == [0, 1, 2, 3, 4] and merges == [0] and rounds == 1         # an edgeless graph: round 1 merges nothing
    n, a, b, w = LM.complete_graph(40)
    r, merges, rounds = LM.linkage_rounds(n, LM.edge_min(a, b, w))
    assert not r.any() and merges == [1] * 39 + [0] and np.array_equal(r, LM.linkage(n, LM.edge_min(a, b, w)))
    for name in ("families", "small_random", "cliques_bridge"):
        n, a, b, w, rep = LM.reference(name)
        got, merges, rounds = LM.linkage_rounds(n, LM.edge_min(a, b, w))
        assert np.array_equal(got, rep) and sum(merges) == n - len(set(rep.tolist())) and 1 <= rounds <= n, name


def test_argument_errors():
    ok = L.cluster_edges([0], [1], [0.5])
    assert L.cluster_host(3, ok, 6)[0].tolist() == [0, 0, 2]
    for algo in (3, 5, -1, 7):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            L.cluster_host(3, ok, algo)
    for bad in (L.cluster_edges([1], [1], [0.5]),            # a == b
                L.cluster_edges([0], [3], [0.5]),            # an id >= n
                L.cluster_edges([3], [0], [0.5]),
                L.cluster_edges([0], [1], [float("nan")]),
                L.cluster_edges([0], [1], [-0.25])):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            L.cluster_host(3, bad, ALGO)


def test_the_host_statement_under_the_sanitizers(tmp_path):
    """tests/model/cluster_link_check.cpp: cluster_host in a program of its own, built with the address and
    undefined-behaviour sanitizers, on a handful of the graphs"""
    picked = ("empty_1", "one_edge", "path_asc", "path_shuffled", "cliques_bridge", "tie", "inf_weight", "small_random", "random_4000")
    n, a, b, w = G.graphs()["small_random"]
    extra = (n, np.concatenate((a, b)), np.concatenate((b, a)), np.concatenate((w, w * 0.5)))     # every pair twice, two weights
    cases = [LM.reference(name)[:4] for name in picked] + [extra]
    text = []
    for n, a, b, w in cases:
        text.append(f"graph {n} {len(a)}")
        text += [f"{int(p)} {int(q)} {struct.unpack('<Q', struct.pack('<d', float(x)))[0]:x}" for p, q, x in zip(a, b, w)]
    (tmp_path / "graphs.txt").write_text("\n".join(text) + "\n")
    exe = str(tmp_path / "cluster_link_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(U.ROOT, "tests", "model", "cluster_link_check.cpp"), "-o", exe])
    r = subprocess.run([exe, str(tmp_path / "graphs.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for line, (n, a, b, w) in zip(lines, cases):
        rep = LM.linkage(n, LM.edge_min(a, b, w))
        got, k = line[4:].split(" | ")
        assert line.startswith("rep ") and [int(x) for x in got.split()] == rep.tolist() and int(k) == LM.number(rep)[1]
