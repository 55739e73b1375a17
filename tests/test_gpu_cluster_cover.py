"""GPU: greedy set cover of the cluster stage (LZANI_CLUSTER_SET_COVER).  The device run on made-up edges
(lzani_debug_cluster_add_edges) entry by entry against lzani_cluster_host and tests/cluster_cover_model.py on the graphs of
tests/cluster_graphs.py; the number of rounds against the model's round form; the shapes at the kernels' seams; what the
run says of the distinct edges; the other algorithms before and behind a set-cover run on one edge buffer; then
lzani_run_rows_kept -> add_kept -> run on a small genome set, on a context and on the group."""
import numpy as np
import pytest

import cluster_cover_model as CC
import cluster_graphs as G
import cluster_model as CM
import lzani_ctypes as L
import synth_genomes as SG
from test_gpu_cluster import minima_of
from test_gpu_out_filter import rows_of

pytestmark = pytest.mark.gpu

ALGO = "set-cover"


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


def check_run(eng, n, a, b, w=None, tag=""):
    """a set-cover run on the edges there are against the host statement of (a, b); returns rep_of, info and cover info"""
    e = L.cluster_edges(a, b, np.ones(len(a)) if w is None else w)
    want_rep, want_cl, want_k = L.cluster_host(n, e, ALGO)
    k = eng.cluster_run(ALGO)
    rep, cl = eng.cluster_fetch()
    assert np.array_equal(rep, want_rep), tag
    assert np.array_equal(cl, want_cl) and k == want_k, tag
    info, cov = eng.cluster_info(), eng.cluster_cover_info()
    sizes = np.bincount(want_rep, minlength=n)
    assert (info["n"], info["algo"], info["clusters"], info["singletons"], info["largest"]) == (n, 4, want_k, int((sizes == 1).sum()), int(sizes.max())), (tag, info)
    assert 1 <= info["rounds"] <= n and info["run_ms"] > 0, (tag, info)
    d = distinct(a, b)
    assert (cov["distinct_edges"], cov["duplicate_edges"]) == (d, info["edges"] - d), (tag, cov, info)
    assert cov["workspace_bytes"] >= 16 * info["edges"] + 28 * n and cov["rounds_ms"] > 0 and cov["dedup_ms"] >= 0, (tag, cov)
    return rep, info, cov


def test_made_up_graphs(eng):
    n6, e6 = CC.SIX
    graphs = dict(G.graphs(), six=(n6, [p[0] for p in e6], [p[1] for p in e6], None))
    for key, (n, a, b, w) in graphs.items():
        begin(eng, n, a, b, w)
        rep, info, _ = check_run(eng, n, a, b, w, key)
        assert info["edges"] == len(a)
        if key.startswith("path") or key in ("six", "small_random", "cliques_bridge", "star_last"):
            want, rounds = CC.cover_rounds(n, CM.edge_set(a, b))               # the model itself, and its rounds
            assert np.array_equal(rep, want) and info["rounds"] == rounds, (key, info["rounds"], rounds)
            if key == "path_asc":
                assert rounds == 100
        if key == "six":
            assert rep.tolist() == [0, 0, 3, 3, 3, 3]
        if key == "star_last":
            assert rep.tolist() == [49] * 50
        if key == "cliques_bridge":
            assert rep.tolist() == [5] * 7 + [7] * 5


def test_planted_families(eng):
    n, a, b, w, members = G.families()
    assert len(a) == 245000                                 # 958 blocks of edges, 60 blocks of the compaction
    begin(eng, n, a, b, w)
    rep, info, cov = check_run(eng, n, a, b, w, "families")
    assert info["rounds"] == 1 and cov["duplicate_edges"] == 0
    for fam in members:                                     # a clique: every c the same, the smallest id wins the tie
        assert (rep[fam] == fam.min()).all()


def test_seams_of_the_kernels(eng):
    # one node, no edge
    begin(eng, 1, [], [])
    rep, info, cov = check_run(eng, 1, [], [], tag="n = 1")
    assert rep.tolist() == [0] and info["rounds"] == 1 and cov["distinct_edges"] == 0
    # n = 257: a second block of one node, and it is the centre of a star -- 256 edges, then 255 (no multiple of 256)
    for m in (256, 255):
        a, b = np.arange(m), np.full(m, 256)
        begin(eng, 257, a, b)
        rep, info, _ = check_run(eng, 257, a, b, tag=f"n = 257, {m} edges")
        assert (rep[:m] == 256).all() and rep[256] == 256 and info["rounds"] == 1
    # more than one compaction block of 4,096 keys, with repetitions that straddle the blocks: 3,000 distinct edges of
    # 600 nodes, each given three times in either orientation, shuffled -- 9,000 records
    rng = np.random.default_rng(21)
    a = rng.integers(0, 600, 3000)
    b = (a + rng.integers(1, 600, 3000)) % 600
    p = rng.permutation(9000)
    aa, bb = np.concatenate((a, b, a))[p], np.concatenate((b, a, b))[p]
    begin(eng, 600, aa, bb, pieces=3)
    _, info, cov = check_run(eng, 600, aa, bb, tag="9,000 records")
    assert info["edges"] == 9000 and cov["distinct_edges"] == distinct(a, b) and cov["duplicate_edges"] == 9000 - distinct(a, b)
    # distinct edges beyond one compaction block: a path of 5,000 nodes with shuffled ids
    ids = rng.permutation(5000)
    begin(eng, 5000, ids[:-1], ids[1:])
    _, info, cov = check_run(eng, 5000, ids[:-1], ids[1:], tag="4,999 distinct edges")
    assert cov["distinct_edges"] == 4999 and cov["duplicate_edges"] == 0
    # one pair 5,000 times, in both orientations
    a, b = np.where(np.arange(5000) % 2, 7, 3), np.where(np.arange(5000) % 2, 3, 7)
    begin(eng, 9, a, b)
    rep, info, cov = check_run(eng, 9, a, b, tag="one pair")
    assert rep.tolist() == [0, 1, 2, 3, 4, 5, 6, 3, 8] and cov["distinct_edges"] == 1 and cov["duplicate_edges"] == 4999


@pytest.mark.parametrize("n, rounds", [(21, 7), (24, 8), (27, 9), (48, 16), (51, 17)])
def test_batch_seams_of_the_rounds(eng, n, rounds):
    """the ascending path takes n / 3 rounds: one below, at and one above a batch of eight rounds, then the same at two batches"""
    _, a, b, w = G.path(n, "asc")
    want, model_rounds = CC.cover_rounds(n, CM.edge_set(a, b))
    assert model_rounds == rounds
    begin(eng, n, a, b, w)
    rep, info, _ = check_run(eng, n, a, b, w, f"path of {n}")
    assert np.array_equal(rep, want) and info["rounds"] == rounds, (n, info["rounds"], rounds)


# lzani_cluster_cover_info.workspace_bytes of the commit before the workspaces summed their own allocations, read from its build
# on an MI355X: graph -> bytes.  A size, not a timing: any difference is a defect.
WORKSPACE = {"small_random": 32900, "one_edge": 2196, "empty_1": 1080}


@pytest.mark.parametrize("key", list(WORKSPACE))
def test_workspace_bytes_are_those_of_the_hand_written_sum(eng, key):
    n, a, b, w = G.graphs()[key]
    begin(eng, n, a, b, w)
    eng.cluster_run(ALGO)
    assert eng.cluster_cover_info()["workspace_bytes"] == WORKSPACE[key]


def test_two_add_calls_with_an_overlap(eng):
    n, a, b, w = G.graphs()["small_random"]
    eng.cluster_begin(n, np.ones(n, np.uint32))
    eng.debug_cluster_add_edges(L.cluster_edges(a[:450], b[:450], w[:450]))
    eng.debug_cluster_add_edges(L.cluster_edges(b[250:], a[250:], w[250:]))     # 200 records again, turned
    aa, bb = np.concatenate((a[:450], b[250:])), np.concatenate((b[:450], a[250:]))
    _, info, cov = check_run(eng, n, aa, bb, tag="overlap")
    assert info["edges"] == len(a) + 200 and cov["distinct_edges"] == distinct(a, b) and cov["duplicate_edges"] == info["edges"] - distinct(a, b)
    assert np.array_equal(eng.cluster_fetch()[0], L.cluster_host(n, L.cluster_edges(a, b, w), ALGO)[0])


def test_the_other_algorithms_on_the_same_edges(eng):
    n, a, b, w = G.graphs()["small_random"]
    begin(eng, n, a, b, w, pieces=2)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        eng.cluster_cover_info()                            # before any run
    before = {}
    for algo in CM.ALGOS:
        eng.cluster_run(algo)
        before[algo] = eng.cluster_fetch()
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            eng.cluster_cover_info()                        # the last run was none of set cover
    edges = eng.cluster_info()["edges"]
    check_run(eng, n, a, b, w, "between")
    assert eng.cluster_info()["edges"] == edges == len(a)
    for algo in CM.ALGOS:                                   # the run made its distinct edges elsewhere: the buffer is as it was
        want = CM.cluster(n, CM.edge_set(a, b, w), algo)
        assert eng.cluster_run(algo) == want[2]["clusters"]
        got = eng.cluster_fetch()
        assert np.array_equal(got[0], before[algo][0]) and np.array_equal(got[1], before[algo][1])
        assert np.array_equal(got[0], want[0]) and eng.cluster_info()["edges"] == edges
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            eng.cluster_cover_info()
    check_run(eng, n, a, b, w, "again")
    for bad in (3, 5, -1):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            eng.cluster_run(bad)


def test_kept_pairs_of_a_genome_set():
    seqs = SG.make_set(40, 815, lmin=2000, lmax=3000, fam=8, dmin=0.01, dmax=0.3)[1]
    n, lens = len(seqs), np.array([len(s) for s in seqs], dtype=np.uint32)
    e = L.Engine()
    e.set_genomes(seqs)
    ref, off = L.dense_rows(n)
    flt = minima_of(n, lens, ref, off, None, rows_of(e.all2all(), ref, off, None))
    e.cluster_begin(measure="gani")                         # the measure plays no part
    rec = e.run_rows_kept(ref, off, None, flt)
    assert e.cluster_add_kept() == len(rec) > 0
    want_rep, want_cl, want_k = L.cluster_host(n, L.cluster_edges(rec["a"], rec["b"], np.ones(len(rec))), ALGO)
    model = CC.cover(n, CM.edge_set(rec["a"], rec["b"]))
    sizes = np.bincount(model, minlength=n)
    assert np.array_equal(want_rep, model) and 1 < want_k < n and sizes.max() >= 3, sizes     # by the model alone
    assert e.cluster_run(ALGO) == want_k
    rep, cl = e.cluster_fetch()
    assert np.array_equal(rep, want_rep) and np.array_equal(cl, want_cl)
    cov = e.cluster_cover_info()
    assert (cov["distinct_edges"], cov["duplicate_edges"]) == (len(rec), 0)
    # the group, one device twice
    grp = L.Group(None, (0, 0))
    grp.set_genomes(seqs)
    grp.cluster_begin()
    assert len(grp.run_rows_kept(ref, off, None, flt)) == len(rec)
    assert grp.cluster_add_kept() == len(rec)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        grp.cluster_cover_info()
    assert grp.cluster_run(ALGO) == want_k
    rep, cl = grp.cluster_fetch()
    assert np.array_equal(rep, want_rep) and np.array_equal(cl, want_cl)
    assert grp.cluster_cover_info()["distinct_edges"] == len(rec) and grp.cluster_info()["algo"] == 4
    grp.close()
    e.close()
