"""GPU: deterministic Leiden (CPM) of the cluster stage (LZANI_CLUSTER_LEIDEN).  The device run on made-up edges
(lzani_debug_cluster_add_edges) against the literal statement of tests/cluster_leiden_model.py -- rep_of, cluster_of and the
counts of lzani_cluster_leiden_info: levels, rounds, moves, merges, quality, distinct edges -- on the graphs of
tests/cluster_graphs.py (on the small ones the tables have 1 to 16 slots, so probes collide and wrap), on 40 of the seeded
random graphs of tests/test_cluster_leiden.py (four resolutions, one and two iterations), on 400 near-cliques of 50 (the
workload's shape), and on duplicate records of different weights; the other algorithms before and behind a Leiden run on one
edge buffer; the setter; then kept results -> add_kept -> run on a genome set, on a context and on the group with one device
twice.  The table-full error path and the cap of rounds are not provoked here: tests/test_cluster_leiden.py covers the cap
on the model and the host form."""
import numpy as np
import pytest

import cluster_graphs as G
import cluster_model as CM
import lzani_ctypes as L
import out_filter_model as M
import synth_genomes as SG
from test_cluster_leiden import COUNTS, model, random_graph
from test_gpu_cluster import minima_of
from test_gpu_out_filter import rows_of

pytestmark = pytest.mark.gpu

ALGO = "leiden-cpm"


@pytest.fixture(scope="module")
def eng():
    e = L.Engine()
    e.set_genomes([np.zeros(100, np.uint8), np.ones(120, np.uint8)])          # the stage needs a genome set, made-up edges not its size
    yield e
    e.close()


def begin(eng, n, a, b, w, pieces=1):
    eng.cluster_begin(n, np.ones(n, np.uint32))
    for part in np.array_split(L.cluster_edges(a, b, w), pieces):
        eng.debug_cluster_add_edges(part)


def slots(insertions):
    s = 1
    while s < 2 * insertions:
        s *= 2
    return s


def check_run(eng, n, want, tag, gamma=0.7, iterations=2):
    """a Leiden run on the edges there are against the model's result `want`; returns rep_of and the two infos"""
    eng.set_cluster_leiden(gamma, iterations)
    k = eng.cluster_run(ALGO)
    rep, cl = eng.cluster_fetch()
    assert rep.tolist() == want["rep_of"], tag
    assert cl.tolist() == want["cluster_of"] and k == want["clusters"], tag
    info, ld = eng.cluster_info(), eng.cluster_leiden_info()
    sizes = np.bincount(rep, minlength=n)
    assert (info["n"], info["algo"], info["clusters"], info["singletons"], info["largest"]) == (n, 8, k, int((sizes == 1).sum()), int(sizes.max())), (tag, info)
    assert {c: ld[c] for c in COUNTS} == {c: want[c] for c in COUNTS}, tag
    assert info["rounds"] == want["move_rounds"] + want["refine_rounds"] and info["run_ms"] > 0, (tag, info)
    assert ld["duplicate_edges"] == info["edges"] - want["distinct_edges"], (tag, ld)
    assert ld["table_slots"] == slots(2 * info["edges"]) and ld["workspace_bytes"] >= 16 * ld["table_slots"] + 32 * info["edges"] + 80 * n, (tag, ld)
    assert ld["rounds_ms"] > 0 and ld["dedup_ms"] >= 0, (tag, ld)
    return rep, info, ld


def test_made_up_graphs(eng):
    seen = set()
    for key, (n, a, b, w) in G.graphs().items():
        begin(eng, n, a, b, w)
        for gamma in (0.7, 0.3):                            # (at 0.7 the paths, of weight 0.5, stay singletons)
            want = model(n, a, b, w, gamma)
            rep, info, ld = check_run(eng, n, want, (key, gamma), gamma)
            assert info["edges"] == len(a)
            seen.add(ld["table_slots"])
            if key == "cliques_bridge":
                assert rep.tolist() == [0] * 6 + [6] * 6
            if key == "empty_5":                            # an edgeless graph: one moving round that moves nothing
                assert rep.tolist() == [0, 1, 2, 3, 4] and (ld["levels"], ld["move_rounds"], ld["refine_rounds"], ld["table_slots"]) == (1, 1, 0, 1)
            if key == "path_asc":                           # the ascending path of 300 nodes
                assert (ld["moves"] == 0 and info["clusters"] == 300) if gamma == 0.7 else (ld["levels"] > 2 and ld["moves"] > 100 and 1 < info["clusters"] <= 150)
    assert {1, 4, 8} <= seen and max(seen) >= 65536         # the small tables, where probes collide and wrap, and large ones


def test_random_graphs(eng):
    several = 0
    for i in range(40):
        n, a, b, w, gamma, it = random_graph(i)
        want = model(n, a, b, w, gamma, it)
        begin(eng, n, a, b, w, pieces=1 + i % 3)
        check_run(eng, n, want, i, gamma, it)
        several += want["levels"] > want["iterations"]
    assert several > 20


@pytest.mark.parametrize("n, move_rounds, refine_rounds", [(3, 6, 6), (4, 7, 8), (5, 8, 10), (8, 11, 16), (9, 12, 18)])
def test_batch_seams_of_the_rounds(eng, n, move_rounds, refine_rounds):
    """a clique of equal weights: one mover a round, so a phase of about n rounds -- below, at and above one batch of four
    rounds and two"""
    iu = np.triu_indices(n, 1)
    a, b, w = iu[0], iu[1], np.full(len(iu[0]), 0.9)
    want = model(n, a, b, w)
    assert (want["move_rounds"], want["refine_rounds"], want["clusters"]) == (move_rounds, refine_rounds, 1)
    begin(eng, n, a, b, w)
    _, _, ld = check_run(eng, n, want, f"clique of {n}")
    for count in ("levels", "move_rounds", "refine_rounds", "moves", "merges"):           # (check_run holds them all; by name here)
        assert ld[count] == want[count], (n, count)


# table_slots and workspace_bytes of lzani_cluster_leiden_info of the commit before the workspaces summed their own
# allocations, read from its build on an MI355X: graph -> (slots, bytes).  Sizes, not timings: any difference is a defect.
WORKSPACE = {"small_random": (4096, 144008), "one_edge": (4, 616), "empty_1": (1, 232)}


@pytest.mark.parametrize("key", list(WORKSPACE))
def test_workspace_bytes_are_those_of_the_hand_written_sum(eng, key):
    n, a, b, w = G.graphs()[key]
    begin(eng, n, a, b, w)
    eng.set_cluster_leiden()
    eng.cluster_run(ALGO)
    ld = eng.cluster_leiden_info()
    assert (ld["table_slots"], ld["workspace_bytes"]) == WORKSPACE[key]


def near_cliques(fams=400, size=50, seed=50):
    """`fams` cliques of `size` with shuffled ids and 1 % of their edges removed; weights of three levels"""
    rng = np.random.default_rng(seed)
    n = fams * size
    ids = rng.permutation(n)
    iu = np.triu_indices(size, 1)
    a = np.concatenate([ids[f * size + iu[0]] for f in range(fams)])
    b = np.concatenate([ids[f * size + iu[1]] for f in range(fams)])
    keep = rng.random(len(a)) >= 0.01
    return n, a[keep].astype(np.uint32), b[keep].astype(np.uint32), rng.choice([0.85, 0.9, 0.95], int(keep.sum())), ids.reshape(fams, size)


# What the model gives on near_cliques(): it takes a minute at this size, so it was run once and the test holds the host form
# (three seconds) to these counts, and the device to the host form.  near_cliques(16) goes through the model itself.
WORKLOAD = dict(clusters=400, iterations=2, levels=8, move_rounds=59, refine_rounds=116, moves=29530, merges=39200, quality=98161612226,
                distinct_edges=485117)


def test_the_workloads_shape(eng):
    n, a, b, w, members = near_cliques(16)
    want = model(n, a, b, w)
    assert want["clusters"] == 16 and want["move_rounds"] >= 50
    begin(eng, n, a, b, w)
    check_run(eng, n, want, "16 near-cliques")
    n, a, b, w, members = near_cliques()
    rep, cl, info = L.cluster_leiden_host(n, L.cluster_edges(a, b, w))
    for fam in members:                                     # every near-clique is one cluster
        assert (rep[fam] == fam.min()).all()
    want = dict(info, rep_of=rep.tolist(), cluster_of=cl.tolist(), clusters=int(cl.max()) + 1)
    assert {k: want[k] for k in WORKLOAD} == WORKLOAD
    begin(eng, n, a, b, w, pieces=3)
    rep, info, ld = check_run(eng, n, want, "400 near-cliques")
    assert info["clusters"] == 400 and ld["table_slots"] == 1 << 21


def test_duplicate_records_of_different_weights(eng):
    # 3,000 distinct edges of 600 nodes, each given three times in either orientation, the third time with half the weight
    rng = np.random.default_rng(21)
    a = rng.integers(0, 600, 3000)
    b = (a + rng.integers(1, 600, 3000)) % 600
    w = rng.choice([0.5, 0.8, 0.95], 3000)
    p = rng.permutation(9000)
    aa, bb, ww = np.concatenate((a, b, a))[p], np.concatenate((b, a, b))[p], np.concatenate((w, w, w * 0.5))[p]
    want = model(600, aa, bb, ww, 0.3)
    assert want["rep_of"] == model(600, a, b, w * 0.5, 0.3)["rep_of"] != model(600, a, b, w, 0.3)["rep_of"]     # the smallest weight is the edge's
    assert 1 < want["clusters"] < 600
    begin(eng, 600, aa, bb, ww, pieces=3)
    _, info, ld = check_run(eng, 600, want, "9,000 records", 0.3)
    assert info["edges"] == 9000 and ld["duplicate_edges"] == 9000 - want["distinct_edges"] and ld["table_slots"] == 65536
    # one node; and 5,000 records of one pair
    begin(eng, 1, [], [], [])
    check_run(eng, 1, model(1, [], [], []), "n = 1")
    i = np.arange(5000)
    a, b, w = np.where(i % 2, 7, 3), np.where(i % 2, 3, 7), np.where(i % 3, 0.9, 0.2)
    begin(eng, 9, a, b, w)
    rep, info, ld = check_run(eng, 9, model(9, a, b, w), "one pair")
    assert rep.tolist() == list(range(9)) and ld["distinct_edges"] == 1         # 0.2 is below the resolution: no cluster
    rep, info, ld = check_run(eng, 9, model(9, a, b, w, 0.1), "one pair, gamma 0.1", 0.1)
    assert rep.tolist() == [0, 1, 2, 3, 4, 5, 6, 3, 8]


def test_the_other_algorithms_and_the_parameters(eng):
    n, a, b, w = G.graphs()["small_random"]
    begin(eng, n, a, b, w, pieces=2)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        eng.cluster_leiden_info()                           # before any run
    others = CM.ALGOS + ("set-cover", "complete-linkage")
    before = {}
    for algo in others:
        eng.cluster_run(algo)
        before[algo] = eng.cluster_fetch()
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            eng.cluster_leiden_info()                       # the last run was none of Leiden
    edges = eng.cluster_info()["edges"]
    # two resolutions on one edge set: the model's two partitions, and they differ
    low, high = model(n, a, b, w, 0.2), model(n, a, b, w, 0.9)
    assert low["rep_of"] != high["rep_of"] and low["clusters"] < high["clusters"]
    check_run(eng, n, low, "gamma 0.2", 0.2)
    check_run(eng, n, high, "gamma 0.9", 0.9)
    check_run(eng, n, model(n, a, b, w, 0.9, 1), "one iteration", 0.9, 1)
    for algo in ("set-cover", "complete-linkage"):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            getattr(eng, "cluster_cover_info" if algo == "set-cover" else "cluster_link_info")()
    assert eng.cluster_info()["edges"] == edges == len(a)
    for algo in others:                                     # the run only read the edge buffer: it is as it was
        want = L.cluster_host(n, L.cluster_edges(a, b, w), algo)
        assert eng.cluster_run(algo) == want[2]
        got = eng.cluster_fetch()
        assert np.array_equal(got[0], before[algo][0]) and np.array_equal(got[1], before[algo][1])
        assert np.array_equal(got[0], want[0]) and eng.cluster_info()["edges"] == edges
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            eng.cluster_leiden_info()
    # the setter: a refused value leaves the parameters as they were, and they hold over a new begin
    eng.set_cluster_leiden(0.2, 2)
    for gamma, it in ((-0.01, 2), (1.01, 2), (float("nan"), 2), (0.7, 0), (0.7, 17)):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            eng.set_cluster_leiden(gamma, it)
    begin(eng, n, a, b, w)
    assert eng.cluster_run(ALGO) == low["clusters"] and eng.cluster_fetch()[0].tolist() == low["rep_of"]
    assert eng.cluster_leiden_info()["resolution_q"] == low["resolution_q"]
    for bad in (7, 3, 5, -1):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            eng.cluster_run(bad)
    assert eng.cluster_fetch()[0].tolist() == low["rep_of"]          # a refused run leaves the last result
    eng.set_cluster_leiden()
    check_run(eng, n, model(n, a, b, w), "the defaults again")


def test_kept_pairs_of_a_genome_set_and_the_group():
    seqs = SG.make_set(60, 815, lmin=2000, lmax=4000, fam=10, dmin=0.01, dmax=0.3)[1]      # the family set of tests/test_gpu_cluster.py
    n, lens = len(seqs), np.array([len(s) for s in seqs], dtype=np.uint32)
    e = L.Engine()
    e.set_genomes(seqs)
    ref, off = L.dense_rows(n)
    res = rows_of(e.all2all(), ref, off, None)
    flt = minima_of(n, lens, ref, off, None, res)
    grp = L.Group(None, (0, 0))                             # the group with one device twice
    grp.set_genomes(seqs)
    reps = {}
    for measure in CM.MEASURES:
        rec = M.kept(flt, n, lens, ref, off, None, res)[0]                                  # the edges by host code
        w = CM.weight(measure, rec["x"], rec["y"], rec["lines"], lens[rec["a"]], lens[rec["b"]])
        want = model(n, rec["a"], rec["b"], w)
        assert 1 < want["clusters"] < n and max(np.bincount(want["rep_of"])) >= 3            # by the model alone
        e.cluster_begin(measure=measure)
        e.run_rows_kept(ref, off, None, flt, fetch=False)
        assert e.cluster_add_kept() == len(rec)
        reps[measure] = check_run(e, n, want, measure)[0]
        if measure == "ani":
            grp.cluster_begin(measure=measure)
            assert len(grp.run_rows_kept(ref, off, None, flt)) == len(rec)
            assert grp.cluster_add_kept() == len(rec)
            with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
                grp.cluster_leiden_info()                   # before a run
            sharp = model(n, rec["a"], rec["b"], w, 0.95, 3)
            check_run(grp, n, sharp, "group", 0.95, 3)
            check_run(grp, n, want, "group, defaults")
            grp.cluster_run("single")
            with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
                grp.cluster_leiden_info()                   # the last run was one of single linkage
    grp.close()
    e.close()
