"""GPU: complete linkage of the cluster stage (LZANI_CLUSTER_COMPLETE).  The device run on made-up edges
(lzani_debug_cluster_add_edges) entry by entry against lzani_cluster_host and the literal statement of
tests/cluster_link_model.py on the graphs of tests/cluster_graphs.py -- on the small ones the table has 2 to 16 slots, so
probes collide and wrap --; rounds and merges against the model's round form; what the run says of the distinct edges and
the table; the other algorithms before and behind a complete-linkage run on one edge buffer; then kept results -> add_kept ->
run under measures that order the weights differently, on a context and on the group.
Not tested: the 64-bit product of two cluster sizes.  It passes 2^32 only for clusters of more than 65,536 members each,
whose link needs 2^32 edges; no test of a few seconds reaches that, and none pretends to."""
import numpy as np
import pytest

import cluster_graphs as G
import cluster_link_model as LM
import cluster_model as CM
import lzani_ctypes as L
import out_filter_model as M
import synth_genomes as SG
from test_gpu_cluster import minima_of
from test_gpu_out_filter import rows_of

pytestmark = pytest.mark.gpu

ALGO = "complete-linkage"


@pytest.fixture(scope="module")
def eng():
    e = L.Engine()
    e.set_genomes([np.zeros(100, np.uint8), np.ones(120, np.uint8)])          # the stage needs a genome set, made-up edges not its size
    yield e
    e.close()


def begin(eng, n, a, b, w=None, pieces=1):
    eng.cluster_begin(n, np.ones(n, np.uint32))
    e = L.cluster_edges(a, b, np.ones(len(a)) if w is None else w)
    for part in np.array_split(e, pieces):
        eng.debug_cluster_add_edges(part)
    return e


def distinct(a, b):
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return len(np.unique((np.minimum(a, b) << np.uint64(32)) | np.maximum(a, b)))


def slots(records):
    s = 1
    while s < 2 * records:
        s *= 2
    return s


def check_run(eng, n, a, b, w=None, tag="", model=None):
    """a complete-linkage run on the edges there are against the host statement of (a, b, w) and, where given, the model's
    rep_of; returns rep_of, info and link info"""
    e = L.cluster_edges(a, b, np.ones(len(a)) if w is None else w)
    want_rep, want_cl, want_k = L.cluster_host(n, e, ALGO)
    k = eng.cluster_run(ALGO)
    rep, cl = eng.cluster_fetch()
    assert np.array_equal(rep, want_rep), tag
    assert np.array_equal(cl, want_cl) and k == want_k, tag
    assert model is None or np.array_equal(rep, model), tag
    info, lk = eng.cluster_info(), eng.cluster_link_info()
    sizes = np.bincount(want_rep, minlength=n)
    assert (info["n"], info["algo"], info["clusters"], info["singletons"], info["largest"]) == (n, 6, want_k, int((sizes == 1).sum()), int(sizes.max())), (tag, info)
    assert 1 <= info["rounds"] <= n + 1 and info["run_ms"] > 0, (tag, info)
    d = distinct(a, b)
    assert (lk["distinct_edges"], lk["duplicate_edges"], lk["merges"]) == (d, info["edges"] - d, n - want_k), (tag, lk, info)
    assert lk["table_slots"] == slots(info["edges"]) and lk["table_slots"] & (lk["table_slots"] - 1) == 0, (tag, lk)
    assert lk["workspace_bytes"] >= 24 * lk["table_slots"] + 24 * info["edges"] + 20 * n and lk["rounds_ms"] > 0 and lk["dedup_ms"] >= 0, (tag, lk)
    return rep, info, lk


def test_made_up_graphs(eng):
    seen = set()
    for key, (n, a, b, w) in G.graphs().items():
        model = LM.reference(key)[4]
        begin(eng, n, a, b, w)
        rep, info, lk = check_run(eng, n, a, b, w, key, model)
        assert info["edges"] == len(a)
        seen.add(lk["table_slots"])
        if key.startswith("path") or key.startswith("empty") or key in ("one_edge", "small_random", "cliques_bridge", "star_0", "tie", "inf_weight"):
            want, merges, rounds = LM.linkage_rounds(n, LM.edge_min(a, b, w))     # the round form, and its counters
            assert np.array_equal(rep, want) and (info["rounds"], lk["merges"]) == (rounds, sum(merges)), (key, info["rounds"], rounds)
            if key == "path_asc":
                assert (rounds, sum(merges)) == (151, 150)
        if key == "cliques_bridge":
            assert rep.tolist() == [0] * 6 + [6] * 6
        if key == "inf_weight":
            assert rep.tolist() == [0, 1, 1]
    assert {1, 2, 4} <= seen and min(s for s in seen if s > 4) <= 256             # the small tables, where probes collide and wrap


def test_planted_families(eng):
    n, a, b, w, members = G.families()
    assert len(a) == 245000                                 # a table of 2^19 slots: 128 blocks of the compaction
    begin(eng, n, a, b, w)
    rep, info, lk = check_run(eng, n, a, b, w, "families", LM.reference("families")[4])
    want, merges, rounds = LM.linkage_rounds(n, LM.edge_min(a, b, w))
    assert (info["rounds"], lk["merges"], lk["duplicate_edges"]) == (rounds, sum(merges), 0) and lk["merges"] == n - 200
    for fam in members:                                     # each family is a clique: one cluster
        assert (rep[fam] == fam.min()).all()


def test_one_merge_a_round(eng):
    n, a, b, w = LM.complete_graph(200)
    want, merges, rounds = LM.linkage_rounds(n, LM.edge_min(a, b, w))
    assert merges == [1] * 199 + [0] and not want.any()     # by the model: exactly one merge a round, one cluster
    begin(eng, n, a, b, w)
    rep, info, lk = check_run(eng, n, a, b, w, "complete graph")
    assert not rep.any() and (info["rounds"], lk["merges"], info["clusters"]) == (200, 199, 1)


# table_slots and workspace_bytes of lzani_cluster_link_info of the commit before the workspaces summed their own allocations,
# read from its build on an MI355X: graph -> (slots, bytes).  Sizes, not timings: any difference is a defect.
WORKSPACE = {"small_random": (2048, 75980), "one_edge": (2, 180), "empty_1": (1, 96)}


@pytest.mark.parametrize("key", list(WORKSPACE))
def test_workspace_bytes_are_those_of_the_hand_written_sum(eng, key):
    n, a, b, w = G.graphs()[key]
    begin(eng, n, a, b, w)
    eng.cluster_run(ALGO)
    lk = eng.cluster_link_info()
    assert (lk["table_slots"], lk["workspace_bytes"]) == WORKSPACE[key]


def test_small_cases_and_seams(eng):
    # one node, no edge: round 1 merges nothing
    begin(eng, 1, [], [])
    rep, info, lk = check_run(eng, 1, [], [], tag="n = 1")
    assert rep.tolist() == [0] and info["rounds"] == 1 and (lk["distinct_edges"], lk["merges"], lk["table_slots"]) == (0, 0, 1)
    # the named cases of the host test, on the device
    for n, e, want in ((3, ((0, 1, 0.5), (1, 2, 0.5)), [0, 0, 2]),
                       (4, ((0, 1, 0.5), (0, 2, 0.5), (1, 2, 0.9), (1, 3, 0.5), (2, 3, 0.5)), [0, 0, 0, 3]),
                       (4, ((0, 1, 0.8), (0, 2, 0.5), (1, 2, 0.5), (1, 3, 0.5), (2, 3, 0.9)), [0, 0, 2, 2]),
                       (3, ((0, 1, 0.9), (1, 2, 0.5), (1, 0, 0.2)), [0, 1, 1]),           # the smaller weight of a pair decides
                       (2, ((1, 0, 0.0),), [0, 0]),                                        # an edge of weight 0 links
                       (4, ((0, 1, 0.7), (0, 2, 0.0), (1, 2, 0.3)), [0, 0, 0, 3])):
        a, b, w = [p[0] for p in e], [p[1] for p in e], [p[2] for p in e]
        begin(eng, n, a, b, w)
        rep, info, lk = check_run(eng, n, a, b, w, str(e), LM.linkage(n, LM.edge_min(a, b, w)))
        assert rep.tolist() == want, e
    # n = 257: a second block of one node, which closes a triangle with 0 and 1; 256 records, then 255
    for m in (256, 255):
        a, b, w = np.arange(m) % 2, np.full(m, 256), np.full(m, 0.5)
        a, b, w = np.append(a, 0), np.append(b, 1), np.append(w, 0.25)
        begin(eng, 257, a[1:], b[1:], w[1:])
        rep, info, lk = check_run(eng, 257, a[1:], b[1:], w[1:], f"n = 257, {m} records")
        assert rep[256] == 0 and rep[1] == 0 and lk["distinct_edges"] == 3 and info["clusters"] == 255
    # 5,000 records of one pair, in both orientations, with two weights: one edge, of the smaller weight.  With 0.9 the
    # pair (3, 7) would go before (7, 8) at 0.5
    i = np.arange(5000)
    a, b, w = np.where(i % 2, 7, 3), np.where(i % 2, 3, 7), np.where(i % 3, 0.9, 0.2)
    a, b, w = np.append(a, 8), np.append(b, 7), np.append(w, 0.5)
    begin(eng, 9, a, b, w)
    rep, info, lk = check_run(eng, 9, a, b, w, "one pair")
    assert rep.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 7] and (lk["distinct_edges"], lk["duplicate_edges"], lk["table_slots"]) == (2, 4999, 16384)
    # 3,000 distinct edges of 600 nodes, each given three times in either orientation, shuffled, over three add calls
    rng = np.random.default_rng(21)
    a = rng.integers(0, 600, 3000)
    b = (a + rng.integers(1, 600, 3000)) % 600
    w = rng.choice([0.25, 0.5, 0.75], 3000)
    p = rng.permutation(9000)
    aa, bb, ww = np.concatenate((a, b, a))[p], np.concatenate((b, a, b))[p], np.concatenate((w, w, w * 0.5))[p]
    begin(eng, 600, aa, bb, ww, pieces=3)
    _, info, lk = check_run(eng, 600, aa, bb, ww, "9,000 records", LM.linkage(600, LM.edge_min(aa, bb, ww)))
    assert info["edges"] == 9000 and lk["distinct_edges"] == distinct(a, b) and lk["table_slots"] == 32768


def test_add_calls(eng):
    """the edges over three add calls with an overlap, and once more in full: the result of the edges given once"""
    n, a, b, w, model = LM.reference("small_random")
    eng.cluster_begin(n, np.ones(n, np.uint32))
    eng.debug_cluster_add_edges(L.cluster_edges(a[:300], b[:300], w[:300]))
    eng.debug_cluster_add_edges(L.cluster_edges(b[200:500], a[200:500], w[200:500]))      # 100 records again, turned
    eng.debug_cluster_add_edges(L.cluster_edges(a[500:], b[500:], w[500:]))
    aa, bb, ww = np.concatenate((a[:300], b[200:500], a[500:])), np.concatenate((b[:300], a[200:500], b[500:])), np.concatenate((w[:300], w[200:500], w[500:]))
    rep, info, lk = check_run(eng, n, aa, bb, ww, "three calls", model)
    assert info["edges"] == len(a) + 100 and lk["distinct_edges"] == distinct(a, b)
    eng.debug_cluster_add_edges(L.cluster_edges(a, b, w))
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        eng.cluster_fetch()                                 # edges were added: a fetch wants a run behind them
    rep2, info, lk = check_run(eng, n, np.concatenate((aa, a)), np.concatenate((bb, b)), np.concatenate((ww, w)), "and in full", model)
    assert info["edges"] == 2 * len(a) + 100 and lk["duplicate_edges"] == info["edges"] - distinct(a, b) and np.array_equal(rep, rep2)


def test_the_other_algorithms_on_the_same_edges(eng):
    n, a, b, w, model = LM.reference("small_random")
    begin(eng, n, a, b, w, pieces=2)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        eng.cluster_fetch()                                 # before any run
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        eng.cluster_link_info()
    others = CM.ALGOS + ("set-cover",)
    before = {}
    for algo in others:
        eng.cluster_run(algo)
        before[algo] = eng.cluster_fetch()
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            eng.cluster_link_info()                         # the last run was none of complete linkage
    edges = eng.cluster_info()["edges"]
    check_run(eng, n, a, b, w, "between", model)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        eng.cluster_cover_info()
    assert eng.cluster_info()["edges"] == edges == len(a)
    for algo in others:                                     # the run only read the edge buffer: it is as it was
        want = L.cluster_host(n, L.cluster_edges(a, b, w), algo)
        assert eng.cluster_run(algo) == want[2]
        got = eng.cluster_fetch()
        assert np.array_equal(got[0], before[algo][0]) and np.array_equal(got[1], before[algo][1])
        assert np.array_equal(got[0], want[0]) and eng.cluster_info()["edges"] == edges
        if algo in CM.ALGOS:
            assert np.array_equal(got[0], CM.cluster(n, CM.edge_set(a, b, w), algo)[0])
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            eng.cluster_link_info()
    check_run(eng, n, a, b, w, "again", model)
    for bad in (3, 5, -1, 7):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            eng.cluster_run(bad)


def made_up_results(n=24, seed=1):
    """dense rows of n genomes with made-up integers: matches 300 .. 999, literals 0 .. 699, lengths 1,000 .. 2,999"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1000, 3000, n).astype(np.uint32)
    ref, off = L.dense_rows(n)
    m, lit = rng.integers(300, 1000, (n * (n - 1), 1)), rng.integers(0, 700, (n * (n - 1), 1))
    return n, lens, ref, off, np.concatenate((m, lit, np.ones_like(m)), axis=1).astype(np.int32)


def test_kept_results_under_three_measures(eng):
    n, lens, ref, off, res = made_up_results()
    flt = {"ani": 0.7}
    reps = {}
    for measure in CM.MEASURES:
        eng.cluster_begin(n, lens, measure)
        rec = eng.filter_results(n, lens, ref, off, None, res, flt)
        assert len(rec) == len(M.kept(flt, n, lens, ref, off, None, res)[0]) and 100 < len(rec) < n * (n - 1) // 2
        assert eng.cluster_add_kept() == len(rec)
        w = np.array([L.cluster_weight(measure, r["x"], r["y"], r["lines"], lens[r["a"]], lens[r["b"]]) for r in rec])
        assert np.array_equal(w, CM.weight(measure, rec["x"], rec["y"], rec["lines"], lens[rec["a"]], lens[rec["b"]]))
        want_rep, want_cl, want_k = L.cluster_host(n, L.cluster_edges(rec["a"], rec["b"], w), ALGO)
        assert np.array_equal(want_rep, LM.linkage(n, LM.edge_min(rec["a"], rec["b"], w)))
        assert eng.cluster_run(ALGO) == want_k and 1 < want_k < n and np.bincount(want_rep).max() >= 4
        rep, cl = eng.cluster_fetch()
        assert np.array_equal(rep, want_rep) and np.array_equal(cl, want_cl), measure
        lk = eng.cluster_link_info()
        assert (lk["distinct_edges"], lk["duplicate_edges"], lk["merges"]) == (len(rec), 0, n - want_k)
        assert eng.cluster_info()["measure"] == L.CLUSTER_MEASURES[measure]
        reps[measure] = rep
    # the measures order the weights differently: three partitions of one graph
    assert not np.array_equal(reps["tani"], reps["ani"]) and not np.array_equal(reps["tani"], reps["gani"]) and not np.array_equal(reps["ani"], reps["gani"])


def test_kept_pairs_of_a_genome_set_and_the_group():
    seqs = SG.make_set(40, 815, lmin=2000, lmax=3000, fam=8, dmin=0.01, dmax=0.3)[1]
    n, lens = len(seqs), np.array([len(s) for s in seqs], dtype=np.uint32)
    e = L.Engine()
    e.set_genomes(seqs)
    ref, off = L.dense_rows(n)
    flt = minima_of(n, lens, ref, off, None, rows_of(e.all2all(), ref, off, None))
    grp = L.Group(None, (0,))                               # the group of one device
    grp.set_genomes(seqs)
    for measure in ("gani", "ani"):
        e.cluster_begin(measure=measure)
        rec = e.run_rows_kept(ref, off, None, flt)
        assert e.cluster_add_kept() == len(rec) > 0
        w = np.array([L.cluster_weight(measure, r["x"], r["y"], r["lines"], lens[r["a"]], lens[r["b"]]) for r in rec])
        want_rep, want_cl, want_k = L.cluster_host(n, L.cluster_edges(rec["a"], rec["b"], w), ALGO)
        model = LM.linkage(n, LM.edge_min(rec["a"], rec["b"], w))
        assert np.array_equal(want_rep, model) and 1 < want_k < n and np.bincount(model).max() >= 2     # by the model alone
        assert e.cluster_run(ALGO) == want_k
        rep, cl = e.cluster_fetch()
        assert np.array_equal(rep, want_rep) and np.array_equal(cl, want_cl)
        assert e.cluster_link_info()["distinct_edges"] == len(rec)
        grp.cluster_begin(measure=measure)
        assert len(grp.run_rows_kept(ref, off, None, flt)) == len(rec)
        assert grp.cluster_add_kept() == len(rec)
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            grp.cluster_fetch()                             # before a run
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            grp.cluster_link_info()
        assert grp.cluster_run(ALGO) == want_k
        rep, cl = grp.cluster_fetch()
        assert np.array_equal(rep, want_rep) and np.array_equal(cl, want_cl)
        lk = grp.cluster_link_info()
        assert (lk["distinct_edges"], lk["duplicate_edges"], lk["merges"]) == (len(rec), 0, n - want_k) and grp.cluster_info()["algo"] == 6
        grp.cluster_run("single")
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            grp.cluster_link_info()                         # the last run was one of single linkage
    grp.close()
    e.close()
