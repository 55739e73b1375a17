"""GPU: the cluster stage.  The stage on made-up edges (lzani_debug_cluster_add_edges) -- all three algorithms entry by
entry against tests/cluster_model.py and against lzani_cluster_host, on the graphs of tests/cluster_graphs.py; the order and
repetition of additions; the call order; then lzani_run_rows_kept -> add_kept -> run on a small genome set -- dense rows,
lists, the group, an out-of-core context, the tiled block pattern -- against lzani_run_rows put through the models."""
import numpy as np
import pytest

import cluster_graphs as G
import cluster_model as CM
import lzani_ctypes as L
import ooc_model as OM
import out_filter_model as M
import synth_genomes as SG
from test_gpu_out_filter import lists, median_minimum, rows_of, symmetric_lists

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = L.Engine()
    e.set_genomes([np.zeros(100, np.uint8), np.ones(120, np.uint8)])          # the stage needs a genome set, made-up edges not its size
    yield e
    e.close()


@pytest.fixture(scope="module")
def graphs():
    return G.graphs()


_want = {}


def wanted(key, n, a, b, w, algo):
    """the model's answer, computed once per graph and algorithm"""
    if (key, algo) not in _want:
        _want[(key, algo)] = CM.cluster(n, CM.edge_set(a, b, w), algo)
    return _want[(key, algo)]


def begin(eng, n, a, b, w, pieces=1):
    eng.cluster_begin(n, np.ones(n, np.uint32))
    e = L.cluster_edges(a, b, w)
    for part in np.array_split(e, pieces):
        eng.debug_cluster_add_edges(part)
    return e


def check_run(eng, key, n, a, b, w, algo, added):
    rep, cl, st = wanted(key, n, a, b, w, algo)
    k = eng.cluster_run(algo)
    got_rep, got_cl = eng.cluster_fetch()
    assert np.array_equal(got_rep, rep), (key, algo)
    assert np.array_equal(got_cl, cl), (key, algo)
    host = L.cluster_host(n, L.cluster_edges(a, b, w), algo)
    assert np.array_equal(got_rep, host[0]) and np.array_equal(got_cl, host[1]) and k == host[2] == st["clusters"]
    info = eng.cluster_info()
    assert (info["n"], info["edges"], info["algo"], info["measure"]) == (n, added, L.CLUSTER_ALGOS[algo], 0), info
    assert (info["clusters"], info["singletons"], info["largest"]) == (st["clusters"], st["singletons"], st["largest"]), (info, st)
    assert info["edge_bytes"] >= 16 * added and info["run_ms"] > 0
    assert info["rounds"] == 1 if algo == "single" else 1 <= info["rounds"] <= n + 1
    return got_rep, info


def test_made_up_graphs(eng, graphs):
    reps = {}
    for key, (n, a, b, w) in graphs.items():
        begin(eng, n, a, b, w)
        for algo in CM.ALGOS + ("single",):                   # several algorithms one after another on one edge set
            reps[(key, algo)], info = check_run(eng, key, n, a, b, w, algo, len(a))
            if key == "path_asc" and algo != "single":
                assert info["rounds"] > 1                   # the worst case of the rounds: a path with ascending ids
        if key in G.RANDOM:
            st = wanted(key, n, a, b, w, "greedy-first")[2]
            assert 1 < st["clusters"] < n and st["largest"] >= 3 and st["singletons"] >= 1
    assert len(set(reps[("cliques_bridge", "single")].tolist())) == 1
    for algo in CM.ALGOS[1:]:                               # single joins the cliques over the bridge, greedy does not
        assert reps[("cliques_bridge", algo)].tolist() == [0] * 6 + [6] * 6
    assert reps[("best_not_first", "greedy-first")].tolist() == [0, 1, 0, 3] and reps[("best_not_first", "greedy-best")].tolist() == [0, 1, 1, 3]
    assert reps[("tie", "greedy-first")].tolist() == reps[("tie", "greedy-best")].tolist() == [0, 1, 0, 3]
    assert reps[("rep_above", "greedy-best")].tolist() == [0, 0, 2]
    assert reps[("inf_weight", "greedy-first")].tolist() == [0, 1, 0] and reps[("inf_weight", "greedy-best")].tolist() == [0, 1, 1]


@pytest.mark.parametrize("algo", CM.ALGOS[1:])
@pytest.mark.parametrize("key, rounds", [("empty_1", 1), ("empty_5", 1), ("star_0", 2)])
def test_greedy_rounds_where_the_schedule_cannot_change_them(eng, graphs, key, rounds, algo):
    """elsewhere a stale read may delay a decision by a round; without an edge every node is a representative in round 1, and
    in the star with the centre lowest the centre is decided in round 1 and, a kernel boundary later, its leaves in round 2"""
    n, a, b, w = graphs[key]
    begin(eng, n, a, b, w)
    _, info = check_run(eng, key, n, a, b, w, algo, len(a))
    assert info["rounds"] == rounds, (key, algo, info)


def test_planted_families(eng):
    n, a, b, w, members = G.families()
    assert len(a) == 245000                                 # 958 blocks of edges
    begin(eng, n, a, b, w)
    for algo in CM.ALGOS:
        rep, _ = check_run(eng, "families", n, a, b, w, algo, len(a))
        for fam in members:                                 # a clique has one representative, its smallest id
            assert (rep[fam] == fam.min()).all()


def test_order_and_repetition(eng, graphs):
    n, a, b, w = graphs["small_random"]
    p = np.random.default_rng(5).permutation(len(a))
    forms = {"one call": (a, b, w, 1), "three calls": (a, b, w, 3), "shuffled": (a[p], b[p], w[p], 2), "turned": (b, a, w, 1),
             "doubled": (np.tile(a, 2), np.tile(b, 2), np.tile(w, 2), 1),
             "both ways": (np.concatenate((a, b)), np.concatenate((b, a)), np.tile(w, 2), 3)}
    for name, (aa, bb, ww, pieces) in forms.items():
        begin(eng, n, aa, bb, ww, pieces)
        for algo in CM.ALGOS:
            check_run(eng, "small_random", n, a, b, w, algo, len(aa))
    # one edge given as (a, b) and as (b, a) counts as one edge
    eng.cluster_begin(3, np.ones(3, np.uint32))
    eng.debug_cluster_add_edges(L.cluster_edges([0, 2], [2, 0], [0.5, 0.5]))
    assert eng.cluster_run("single") == 2 and eng.cluster_fetch()[0].tolist() == [0, 1, 0]
    assert eng.cluster_info()["largest"] == 2 and eng.cluster_info()["singletons"] == 1


def test_call_order_and_refusals(graphs):
    e = L.Engine()
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        e.cluster_begin(3, np.ones(3, np.uint32))           # no genome set
    e.set_genomes([np.zeros(100, np.uint8), np.ones(120, np.uint8), np.zeros(90, np.uint8)])
    e._cluster_n = 3
    for call in (lambda: e.cluster_run("single"), e.cluster_fetch, e.cluster_info, e.cluster_add_kept,
                 lambda: e.debug_cluster_add_edges(L.cluster_edges([0], [1], [1.0]))):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            call()                                          # before a begin
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        e.cluster_begin(3, None, measure=7)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        e.cluster_begin(5)                                  # the set's own lengths are those of its 3 genomes
    e.cluster_begin()
    assert e.cluster_info()["n"] == 3 and e.cluster_info()["algo"] == -1 and e.cluster_info()["edges"] == 0
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        e.cluster_fetch()                                   # before a run
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        e.cluster_add_kept()                                # without a kept result
    for bad in (L.cluster_edges([1], [1], [0.5]), L.cluster_edges([0], [3], [0.5]), L.cluster_edges([0], [1], [float("nan")]),
                L.cluster_edges([0], [1], [-1.0])):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            e.debug_cluster_add_edges(bad)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        e.cluster_run(3)
    assert e.cluster_info()["edges"] == 0 and e.cluster_run("greedy-best") == 3
    # a kept result of another n
    ref, off = L.dense_rows(4)
    e.filter_results(4, np.full(4, 1000, np.uint32), ref, off, None, np.full((12, 3), 500, np.int32), {})
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        e.cluster_add_kept()
    # ... and one of this n: every pair an edge; a fetch wants a run behind the add
    ref, off = L.dense_rows(3)
    e.filter_results(3, np.full(3, 1000, np.uint32), ref, off, None, np.full((6, 3), 500, np.int32), {})
    assert e.cluster_add_kept() == 3
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        e.cluster_fetch()
    assert e.cluster_run("single") == 1 and e.cluster_info()["add_ms"] > 0
    # lzani_set_genomes drops the state
    e.set_genomes([np.zeros(100, np.uint8)])
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        e.cluster_info()
    e.close()


# ---- lzani_run_rows_kept -> add_kept -> run on genomes ---------------------------------------------------------------

@pytest.fixture(scope="module")
def genomes():
    seqs = SG.make_set(60, 815, lmin=2000, lmax=4000, fam=10, dmin=0.01, dmax=0.3)[1]
    e = L.Engine()
    e.set_genomes(seqs)
    full = e.all2all()                                      # the reference of every case below: computed once, left unchanged
    full.setflags(write=False)
    yield seqs, e, full
    e.close()


def minima_of(n, lens, ref, off, q, res):
    """minima among the lines of related pairs, taken from the data itself: the medians of their values"""
    return dict(median_minimum(n, lens, ref, off, q, res, "ani", 0.5, above=0.5), **median_minimum(n, lens, ref, off, q, res, "qcov", 0.5, above=0.2))


def expected(flt, n, lens, ref, off, q, res, measure, algo):
    rec = M.kept(flt, n, lens, ref, off, q, res)[0]
    w = CM.weight(measure, rec["x"], rec["y"], rec["lines"], lens[rec["a"]], lens[rec["b"]])
    return CM.cluster(n, CM.edge_set(rec["a"], rec["b"], w), algo), len(rec)


def same(e, want):
    (rep, cl, st), edges = want
    got_rep, got_cl = e.cluster_fetch()
    assert np.array_equal(got_rep, rep) and np.array_equal(got_cl, cl)
    info = e.cluster_info()
    assert (info["edges"], info["clusters"], info["singletons"], info["largest"]) == (edges, st["clusters"], st["singletons"], st["largest"]), (info, st)


def tiled_blocks(n, tile):
    """The blocks of a tiled dense all2all: block A = the rows of A against the queries from A on, and the rows behind A
    against the queries of A; every unordered pair lies in exactly one block, in both directions."""
    for a0 in range(0, n, tile):
        a1 = min(n, a0 + tile)
        rows = [(r, [x for x in range(a0, n) if x != r] if r < a1 else list(range(a0, a1))) for r in range(a0, n)]
        yield lists([(r, qs) for r, qs in rows if qs])


def test_end_to_end(genomes):
    seqs, eng, full = genomes
    n, lens = len(seqs), np.array([len(s) for s in seqs], dtype=np.uint32)
    dense = L.dense_rows(n) + (None,)
    flt = minima_of(n, lens, *dense, rows_of(full, *dense))
    sym = lists(symmetric_lists(n, 41, 0.5))
    grp = L.Group(None, (0, 0))
    grp.set_genomes(seqs)
    ooc = L.Engine()
    ooc.set_genome_memory(OM.limit_for_blocks([int(x) for x in lens], None, 3))
    ooc.set_genomes(seqs)
    assert ooc.residency()["blocks"] == 3
    for measure in CM.MEASURES:
        for form, (ref, off, q) in (("dense", dense), ("lists", sym)):
            res = rows_of(full, ref, off, q)
            eng.cluster_begin(measure=measure)
            eng.run_rows_kept(ref, off, q, flt, fetch=False)
            edges = eng.cluster_add_kept()
            assert edges == eng.kept_info()["kept_pairs"]
            for algo in CM.ALGOS:
                want = expected(flt, n, lens, ref, off, q, res, measure, algo)
                st = want[0][2]
                assert 1 < st["clusters"] < n and st["largest"] >= 3 and st["singletons"] >= 1, (form, st)      # by the model alone
                assert eng.cluster_run(algo) == st["clusters"]
                same(eng, want)
                if measure != "tani":
                    continue
                for other in (grp, ooc):                    # the group with one device twice; an out-of-core context
                    other.cluster_begin(measure=measure)
                    if other is grp:
                        other.run_rows_kept(ref, off, q, flt)
                    else:
                        other.run_rows_kept(ref, off, q, flt, fetch=False)
                    assert other.cluster_add_kept() == edges
                    assert other.cluster_run(algo) == st["clusters"]
                    same(other, want)
    assert ooc.residency()["tiles"] > 1
    # the tiled block pattern accumulated over several kept calls: the one-call result; reported lengths of the caller's
    rl = lens + np.uint32(40)
    res = rows_of(full, *dense)
    eng.cluster_begin(n, rl, "gani")
    total = 0
    for ref, off, q in tiled_blocks(n, 16):
        total += eng.run_rows_kept(ref, off, q, flt, report_len=rl, fetch=False)
        assert eng.cluster_add_kept() == total
    assert total > 0 and eng.cluster_info()["edge_bytes"] >= 16 * total
    for algo in CM.ALGOS:
        want = expected(flt, n, rl, *dense, res, "gani", algo)
        assert want[1] == total
        eng.cluster_run(algo)
        same(eng, want)
    grp.close()
    ooc.close()
