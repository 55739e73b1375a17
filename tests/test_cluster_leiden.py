"""CPU: deterministic Leiden (CPM) of the cluster stage, LZANI_CLUSTER_LEIDEN.  The sequential form of
lz-ani_amd/csrc/lzani_cluster_plan.h (through the pure exports lzani_cluster_leiden_host and lzani_cluster_host, algorithm 8)
against the literal statement of tests/cluster_leiden_model.py -- rep_of, cluster_of, the quality and the counts of rounds --
on seeded random graphs whose weights tie throughout and on the graphs of tests/cluster_graphs.py; what the model alone must
show (the quality rises strictly in every round that moves something: asserted inside the model; every community is connected; a
second run on the result of a run that ended by itself changes nothing); the named cases; the cap of rounds with a lowered cap; the argument errors; and the host form in a stand-alone program under the sanitizers.  No GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cluster_graphs as G
import cluster_leiden_model as LD
import lzani_ctypes as L
import util as U

ALGO = "leiden-cpm"
GAMMAS = (0, 0.3, 0.7, 1)
COUNTS = ("iterations", "levels", "move_rounds", "refine_rounds", "moves", "merges", "quality", "resolution_q", "distinct_edges")


@pytest.fixture(scope="module", autouse=True)
def lib():
    L.build_library()
    return L.load_library()


def random_graph(i):
    """graph i of the seeded family: 8 to 40 nodes, three weight levels, gamma and the iterations in turn"""
    rng = np.random.default_rng(1000 + i)
    n = int(rng.integers(8, 41))
    m = int(rng.integers(n, 4 * n + 1))
    a = rng.integers(0, n, m)
    b = (a + rng.integers(1, n, m)) % n
    return n, a.astype(np.uint32), b.astype(np.uint32), rng.choice([0.25, 0.5, 0.9], m), GAMMAS[i % 4], 1 + (i // 4) % 2


def model(n, a, b, w, gamma=0.7, iterations=2, **kw):
    return LD.leiden(n, zip(np.asarray(a).tolist(), np.asarray(b).tolist(), np.asarray(w, dtype=np.float64).tolist()), gamma, iterations, **kw)


def host(n, a, b, w, gamma=0.7, iterations=2, cap=None):
    return L.cluster_leiden_host(n, L.cluster_edges(a, b, w), gamma, iterations, cap)


def same(got, want, tag):
    rep, cl, info = got
    assert rep.tolist() == want["rep_of"], tag
    assert cl.tolist() == want["cluster_of"], tag
    assert {k: info[k] for k in COUNTS} == {k: want[k] for k in COUNTS}, tag
    assert info["duplicate_edges"] >= 0 and info["table_slots"] == 0 and info["rounds_ms"] == 0, tag      # the device's fields


def connected(n, a, b, rep):
    """every community is connected by the edges inside it"""
    root = list(range(n))

    def find(v):
        while root[v] != v:
            root[v] = root[root[v]]
            v = root[v]
        return v
    for p, q in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        if rep[p] == rep[q]:
            root[find(p)] = find(q)
    return all(find(v) == find(rep[v]) for v in range(n))


def test_the_id_is_eight():
    assert L.CLUSTER_ALGOS[ALGO] == 8 and not {3, 5, 7} & set(L.CLUSTER_ALGOS.values()) and "leiden" not in L.CLUSTER_ALGOS


def test_host_form_against_the_model_on_random_graphs():
    levels = moved = several = unsettled = 0
    partitions = set()
    for i in range(300):
        n, a, b, w, gamma, it = random_graph(i)
        want = model(n, a, b, w, gamma, it)
        same(host(n, a, b, w, gamma, it), want, i)
        assert connected(n, a, b, want["rep_of"]), i                                      # by the model alone
        # a second run with the result as input changes nothing -- of a run that was left to end by itself.  (After one or two
        # iterations a node may still gain by a move that the aggregated level could not make, which is why Leiden is iterated;
        # graph 41 of this family is such a case.)
        ended = want if want["iterations"] < it else model(n, a, b, w, gamma, 16)
        assert ended["iterations"] < 16, i
        again = model(n, a, b, w, gamma, it, start=ended["rep_of"])
        assert again["rep_of"] == ended["rep_of"] and (again["moves"], again["iterations"]) == (0, 1), i
        unsettled += ended["rep_of"] != want["rep_of"]
        assert len(want["trace"]) == want["move_rounds"], i
        levels += want["levels"] > want["iterations"]
        moved += want["moves"] > 0
        several += 1 < want["clusters"] < n
        partitions.add((gamma, want["clusters"] == n))
    assert levels > 150 and moved > 200 and several > 150                                 # the runs were not trivial
    assert 0 < unsettled < 150                                                            # more iterations do change some results
    assert (1, True) in partitions and (0, False) in partitions


def test_host_form_against_the_model_on_the_made_up_graphs():
    for key, (n, a, b, w) in G.graphs().items():
        want = model(n, a, b, w)
        same(host(n, a, b, w), want, key)
        rep, cl, k = L.cluster_host(n, L.cluster_edges(a, b, w), ALGO)                    # algorithm 8 of lzani_cluster_host: the defaults
        assert rep.tolist() == want["rep_of"] and cl.tolist() == want["cluster_of"] and k == want["clusters"], key
        assert np.array_equal(L.cluster_host(n, L.cluster_edges(a, b, w), 8)[0], rep), key
        assert connected(n, a, b, want["rep_of"]), key


def test_order_repetition_and_orientation():
    n, a, b, w = G.graphs()["small_random"]
    want = model(n, a, b, w)
    p = np.random.default_rng(3).permutation(len(a))
    for aa, bb, ww in ((a[p], b[p], w[p]), (b, a, w), (np.tile(a, 2), np.tile(b, 2), np.tile(w, 2)),
                       (np.concatenate((a, b)), np.concatenate((b, a)), np.tile(w, 2))):
        rep, cl, info = host(n, aa, bb, ww)
        assert rep.tolist() == want["rep_of"] and cl.tolist() == want["cluster_of"] and info["quality"] == want["quality"]
        assert info["distinct_edges"] == want["distinct_edges"] and info["duplicate_edges"] == len(aa) - want["distinct_edges"]
    # a pair given with two weights: the smaller one is the edge's
    light = model(3, [0, 1, 1], [1, 2, 0], [0.9, 0.9, 0.2])
    assert light["rep_of"] == model(3, [0, 1], [1, 2], [0.2, 0.9])["rep_of"] == [0, 1, 1]
    same(host(3, [0, 1, 1], [1, 2, 0], [0.9, 0.9, 0.2]), light, "two weights")


def clique(ids, w):
    return [(p, q, w) for i, p in enumerate(ids) for q in ids[i + 1:]]


def test_named_cases():
    # disjoint cliques of weight 0.9 at gamma 0.7: one cluster each, the smallest id its representative
    ids = np.random.default_rng(4).permutation(40).tolist()
    e = [x for c in range(5) for x in clique(ids[8 * c:8 * c + 8], 0.9)]
    a, b, w = zip(*e)
    rep = host(40, a, b, w)[0].tolist()
    for c in range(5):
        assert {rep[v] for v in ids[8 * c:8 * c + 8]} == {min(ids[8 * c:8 * c + 8])}
    same(host(40, a, b, w), model(40, a, b, w), "cliques")
    # a 6-clique of weight 0.6: six singletons at gamma 0.7, one cluster at gamma 0.5 -- the parameter arrives
    a, b, w = zip(*clique(list(range(6)), 0.6))
    assert host(6, a, b, w, 0.7)[0].tolist() == [0, 1, 2, 3, 4, 5] == model(6, a, b, w, 0.7)["rep_of"]
    assert host(6, a, b, w, 0.5)[0].tolist() == [0] * 6 == model(6, a, b, w, 0.5)["rep_of"]
    # two 6-cliques joined by a bridge: two clusters, where single linkage gives one
    n, a, b, w = G.graphs()["cliques_bridge"]
    rep, cl, info = host(n, a, b, w)
    assert rep.tolist() == [0] * 6 + [6] * 6 and cl.tolist() == [0] * 6 + [1] * 6
    assert L.cluster_host(n, L.cluster_edges(a, b, w), "single")[2] == 1
    # no edge: every node its own cluster, one moving round that moves nothing
    rep, cl, info = host(5, [], [], [])
    assert rep.tolist() == [0, 1, 2, 3, 4] and (info["iterations"], info["levels"], info["move_rounds"], info["refine_rounds"]) == (1, 1, 1, 0)
    # +inf clamps to 1
    n, a, b, w = G.graphs()["inf_weight"]
    assert host(n, a, b, w)[2]["quality"] == model(n, a, b, [1.0, 1.0])["quality"]
    assert LD.quantise(float("inf")) == LD.quantise(5.0) == 1 << 20 and LD.quantise(0.7) == 734003 and LD.resolution_q(0.7) == 734003


def test_the_cap_of_rounds():
    """a lowered cap: the model and the host form stop at the same graphs, and nowhere else"""
    stopped = 0
    for i in range(60):
        n, a, b, w, gamma, it = random_graph(i)
        full = model(n, a, b, w, gamma, it)
        for cap in ((0, 2), (0, 4)):
            try:
                want = model(n, a, b, w, gamma, it, cap_mul=cap[0], cap_add=cap[1])
            except LD.RoundCap:
                stopped += 1
                with pytest.raises(L.LzaniError, match="LZANI_ERR_DEVICE"):
                    host(n, a, b, w, gamma, it, cap)
                continue
            assert want["rep_of"] == full["rep_of"]
            same(host(n, a, b, w, gamma, it, cap), want, (i, cap))
    assert 20 < stopped < 120
    n, a, b, w = G.graphs()["path_asc"]
    same(host(n, a, b, w, cap=(64, 64)), model(n, a, b, w), "the cap of the statement")


def test_argument_errors():
    ok = L.cluster_edges([0], [1], [0.9])
    assert L.cluster_host(3, ok, 8)[0].tolist() == [0, 0, 2]
    for algo in (3, 5, 7, -1):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            L.cluster_host(3, ok, algo)
    for bad in (L.cluster_edges([1], [1], [0.5]),            # a == b
                L.cluster_edges([0], [3], [0.5]),            # an id >= n
                L.cluster_edges([3], [0], [0.5]),
                L.cluster_edges([0], [1], [float("nan")]),
                L.cluster_edges([0], [1], [-0.25])):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            L.cluster_host(3, bad, ALGO)
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            L.cluster_leiden_host(3, bad)
    for gamma, it in ((-0.01, 2), (1.01, 2), (float("nan"), 2), (0.7, 0), (0.7, 17), (0.7, -1)):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            L.cluster_leiden_host(3, ok, gamma, it)
    for gamma, it in ((0, 1), (1, 16)):
        L.cluster_leiden_host(3, ok, gamma, it)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        L.cluster_leiden_host((1 << 21) + 1, ok)             # n > 2^21


def test_the_host_form_under_the_sanitizers(tmp_path):
    """tests/model/cluster_leiden_check.cpp: cluster_leiden_host in a program of its own, built with the address and
    undefined-behaviour sanitizers, on a handful of the graphs"""
    def bits(x):
        return f"{struct.unpack('<Q', struct.pack('<d', float(x)))[0]:x}"
    cases = [G.graphs()[name] + (0.7, 2) for name in ("empty_1", "one_edge", "path_asc", "cliques_bridge", "tie", "inf_weight", "small_random", "random_4000")]
    cases += [G.graphs()["path_shuffled"] + (0.3, 3), G.graphs()["star_0"] + (0.0, 1), G.graphs()["small_random"] + (1.0, 16)]
    cases += [random_graph(i) for i in range(0, 120, 3)]
    text = []
    for n, a, b, w, gamma, it in cases:
        text.append(f"graph {n} {len(a)} {bits(gamma)} {it}")
        text += [f"{int(p)} {int(q)} {bits(x)}" for p, q, x in zip(a, b, w)]
    (tmp_path / "graphs.txt").write_text("\n".join(text) + "\n")
    exe = str(tmp_path / "cluster_leiden_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(U.ROOT, "tests", "model", "cluster_leiden_check.cpp"), "-o", exe])
    r = subprocess.run([exe, str(tmp_path / "graphs.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for line, (n, a, b, w, gamma, it) in zip(lines, cases):
        want = model(n, a, b, w, gamma, it)
        rep, counts = line[4:].split(" | ")
        assert line.startswith("rep ") and [int(x) for x in rep.split()] == want["rep_of"]
        assert [int(x) for x in counts.split()] == [want[k] for k in ("quality", "iterations", "levels", "move_rounds", "refine_rounds", "moves", "merges")]
