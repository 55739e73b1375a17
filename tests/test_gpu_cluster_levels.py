"""GPU: cluster levels -- the record store, the cut and the level's edges (lzani_cluster_store_*, lzani_cluster_level).
Made-up records around one block of 4,096 and over several (lzani_debug_cluster_store_add), edge by edge against
tests/cluster_cut_model.py through lzani_debug_cluster_edges; the all-zero cut against lzani_cluster_add_kept; a level under
stricter minima against the stricter output filter; growth of the store and independence of the levels; all six algorithms on
a level; call order and refusals; every out-of-memory promise; then genomes: two kept calls into the store and two levels,
against lzani_run_rows put through the models, on a context and on the group."""
import numpy as np
import pytest

import cluster_cover_model as CC
import cluster_cut_model as CUT
import cluster_graphs as G
import cluster_link_model as KM
import cluster_model as CM
import lzani_ctypes as L
import out_filter_model as M
import synth_genomes as SG
from test_cluster_leiden import model as leiden_model
from test_gpu_cluster import tiled_blocks
from test_gpu_out_filter import made_up, median_minimum, rows_of

pytestmark = pytest.mark.gpu

CHUNK = 4096                                            # PF_CHUNK: the records of one block of the level's passes
SIZES = (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5)
N = 300                                                 # nodes of the made-up records
CUT_A = dict(ani=0.6, qcov=0.3, len_ratio=0.5, num_alns=6)
CUT_B = dict(tani=0.2, gani=0.35, rcov=0.25)


@pytest.fixture(scope="module")
def eng():
    e = L.Engine()
    e.set_genomes([np.zeros(100, np.uint8), np.ones(120, np.uint8)])          # the stage needs a genome set, made-up records not its size
    yield e
    e.close()


def node_lengths():
    """the nodes 0 .. 9 share a length (len_ratio 1 among them), two nodes have none"""
    lens = np.random.default_rng(1).integers(1500, 4000, N).astype(np.uint32)
    lens[:10] = 1000
    lens[[50, 51]] = 0
    return lens


def records(count, seed, lens=None):
    """made-up KEPT_DTYPE records, a < b < N: plausible values mixed with negative ones, m + l == 0 and every `lines`; from
    3 * CHUNK + 5 on, the second block of 4,096 fails CUT_A whole and the third passes it whole"""
    rng = np.random.default_rng(seed)
    lens = node_lengths() if lens is None else lens
    rec = np.zeros(count, dtype=L.KEPT_DTYPE)
    a = rng.integers(0, N - 1, count)
    b = a + 1 + rng.integers(0, N, count) % (N - 1 - a)
    rec["a"], rec["b"] = a, b
    for side, other in (("x", "a"), ("y", "b")):
        al = (rng.random(count) * np.maximum(lens[rec[other]], 1)).astype(np.int64)
        m = (al * (0.4 + 0.6 * rng.random(count))).astype(np.int64)
        rec[side] = np.stack((m, al - m, rng.integers(0, 10, count)), axis=1)
    odd = rng.random(count)
    rec["x"][odd < 0.05] = 0
    rec["y"][(odd > 0.05) & (odd < 0.10), 0] *= -1
    rec["lines"] = rng.integers(1, 4, count)
    if count >= 3 * CHUNK:
        rec["x"][CHUNK:2 * CHUNK, 2] = 100                                  # more alignments than CUT_A takes, on both lines
        rec["y"][CHUNK:2 * CHUNK, 2] = 100
        mid = slice(2 * CHUNK, 3 * CHUNK)
        rec["a"][mid] = rng.integers(0, 5, CHUNK)
        rec["b"][mid] = rng.integers(5, 10, CHUNK)
        rec["x"][mid] = rec["y"][mid] = (900, 50, 1)
    return rec


def bits(w):
    return np.ascontiguousarray(w, dtype=np.float64).view(np.uint64)


def check_level(eng, rec, lens, measure, cut):
    """a level of the store against the model: the edges in record order, a, b and the weight's 64 bits; the info"""
    a, b, w, lines_in, lines_out = CUT.level(cut, measure, rec, lens)
    assert eng.cluster_level(measure, cut) == len(a)
    got = eng.debug_cluster_edges()
    assert np.array_equal(got["a"], a) and np.array_equal(got["b"], b), (measure, cut)
    assert np.array_equal(bits(got["w"]), bits(w)), (measure, cut, np.flatnonzero(bits(got["w"]) != bits(w))[:5])
    info = eng.cluster_level_info()
    assert (info["records_in"], info["edges_out"], info["lines_in"], info["lines_out"]) == (len(rec), len(a), lines_in, lines_out), info
    assert info["level_ms"] > 0
    ci = eng.cluster_info()
    assert (ci["n"], ci["edges"], ci["algo"], ci["measure"]) == (len(lens), len(a), -1, L.CLUSTER_MEASURES[measure]), ci
    return got


@pytest.mark.parametrize("size", SIZES)
def test_made_up_records(eng, size):
    lens, rec = node_lengths(), records(size, 20 + size % 7)
    eng.cluster_store_begin(N, lens)
    eng.debug_cluster_store_add(rec)
    si = eng.cluster_store_info()
    assert (si["n"], si["records"]) == (N, size) and si["record_bytes"] >= 36 * size, si
    if size > 3 * CHUNK:                                # by the model alone: a block without an edge, a block of edges only
        stay = CUT.cut_lines(CUT_A, rec["x"], rec["y"], rec["lines"], lens[rec["a"]], lens[rec["b"]])
        assert not stay[CHUNK:2 * CHUNK].any() and stay[2 * CHUNK:3 * CHUNK].all() and 0 < (stay[:CHUNK] != 0).sum() < CHUNK
    for measure in CM.MEASURES:
        for cut in (CUT_A, CUT_B):
            check_level(eng, rec, lens, measure, cut)


@pytest.fixture(scope="module")
def forty():
    """40 genomes, dense rows, made-up results that are not negative: 780 pairs"""
    n = 40
    ref, off = L.dense_rows(n)
    lens, res = made_up(n, ref, off, None, 31)
    return n, ref, off, lens, res


def edges_of_add_kept(eng, n, lens, ref, off, res, flt, measure):
    eng.filter_results(n, lens, ref, off, None, res, flt, fetch=False)
    eng.cluster_begin(n, lens, measure)
    eng.cluster_add_kept()
    return eng.debug_cluster_edges()


def test_all_zero_cut_is_add_kept(eng, forty):
    n, ref, off, lens, res = forty
    for flt in ({}, median_minimum(n, lens, ref, off, None, res, "ani")):
        for measure in CM.MEASURES:
            want = edges_of_add_kept(eng, n, lens, ref, off, res, flt, measure)
            assert len(want) == 780 if not flt else 0 < len(want) < 780
            eng.cluster_store_begin(n, lens)
            assert eng.cluster_store_add_kept() == len(want)
            assert eng.cluster_level(measure, {}) == len(want)
            assert eng.debug_cluster_edges().tobytes() == want.tobytes()       # the same edges, bit for bit, in the same order


def test_level_under_stricter_minima_is_the_stricter_filter(eng, forty):
    n, ref, off, lens, res = forty
    q = lambda field, quant: median_minimum(n, lens, ref, off, None, res, field, quant)
    pairs = ((q("ani", 0.2), dict(q("ani", 0.6), **q("qcov", 0.3))),
             (dict(q("tani", 0.3), **q("gani", 0.1)), dict(q("tani", 0.5), **q("gani", 0.4), **q("rcov", 0.3))))
    for loose, strict in pairs:
        assert all(strict.get(k, 0.0) >= loose.get(k, 0.0) for k in M.FIELDS)
        for measure in CM.MEASURES:
            want = edges_of_add_kept(eng, n, lens, ref, off, res, strict, measure)
            records_in = eng.filter_results(n, lens, ref, off, None, res, loose, fetch=False)
            eng.cluster_store_begin(n, lens)
            eng.cluster_store_add_kept()
            assert 0 < eng.cluster_level(measure, strict) == len(want) < records_in
            got = eng.debug_cluster_edges()
            assert np.sort(got, order=("a", "b")).tobytes() == np.sort(want, order=("a", "b")).tobytes()


def test_growth_and_independence(eng):
    lens = node_lengths()
    parts = [records(1, 41), records(5000, 42), records(3, 43)]
    eng.cluster_store_begin(N, lens)
    for p in parts:
        eng.debug_cluster_store_add(p)
    rec = np.concatenate(parts)
    si = eng.cluster_store_info()
    assert si["records"] == 5004 and si["record_bytes"] >= 36 * 5004 and si["add_ms"] > 0, si
    first = check_level(eng, rec, lens, "ani", CUT_A)
    second = check_level(eng, rec, lens, "gani", CUT_B)
    third = check_level(eng, rec, lens, "ani", CUT_A)
    assert len(first) != len(second) and third.tobytes() == first.tobytes()
    assert eng.cluster_store_info()["records"] == 5004


def graph_records():
    """the pairs of a graph of tests/cluster_graphs.py as records: a pair given twice carries one record's values"""
    n, a, b, _ = G.graphs()["small_random"]
    lens = np.random.default_rng(2).integers(1500, 4000, n).astype(np.uint32)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    _, first, inverse = np.unique(lo.astype(np.int64) * n + hi, return_index=True, return_inverse=True)
    rng = np.random.default_rng(3)
    rec = np.zeros(len(first), dtype=L.KEPT_DTYPE)
    rec["a"], rec["b"] = lo[first], hi[first]
    for side, other in (("x", "a"), ("y", "b")):
        al = (rng.random(len(rec)) * lens[rec[other]]).astype(np.int64)
        m = (al * (0.4 + 0.6 * rng.random(len(rec)))).astype(np.int64)
        rec[side] = np.stack((m, al - m, rng.integers(1, 10, len(rec))), axis=1)
    rec["lines"] = rng.integers(1, 4, len(rec))
    return n, lens, rec[inverse.ravel()]


def model_clusters(n, a, b, w, algo):
    """rep_of and cluster_of of the models, each written from its algorithm's definition"""
    if algo in CM.ALGOS:
        rep = CM.cluster(n, CM.edge_set(a, b, w), algo)[0]
    elif algo == "set-cover":
        rep = CC.cover(n, CM.edge_set(a, b))
    elif algo == "complete-linkage":
        rep = KM.linkage(n, KM.edge_min(a, b, w))
    else:
        rep = leiden_model(n, a, b, w)["rep_of"]
    rep = np.asarray(rep, dtype=np.int64)
    return rep.astype(np.uint32), CM.number(rep)[0].astype(np.uint32)


def test_every_algorithm_on_a_level(eng):
    n, lens, rec = graph_records()
    eng.cluster_store_begin(n, lens)
    eng.debug_cluster_store_add(rec)
    sizes = []
    for measure, cut in (("ani", {}), ("gani", dict(qcov=0.4)), ("tani", dict(ani=0.7, num_alns=7))):
        a, b, w, _, _ = CUT.level(cut, measure, rec, lens)
        sizes.append(len(a))
        for algo in L.CLUSTER_ALGOS:
            assert eng.cluster_level(measure, cut) == len(a)       # a level for every run: a run leaves the edges as they are, and so does a level
            rep, cl = model_clusters(n, a, b, w, algo)
            assert eng.cluster_run(algo) == len(set(rep.tolist())), (measure, cut, algo)
            got_rep, got_cl = eng.cluster_fetch()
            assert np.array_equal(got_rep, rep) and np.array_equal(got_cl, cl), (measure, cut, algo)
    assert sizes[0] == len(rec) > sizes[1] > 0 and len(rec) > sizes[2] > 0


def test_call_order_and_refusals(forty):
    n, ref, off, lens, res = forty
    e = L.Engine()
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        e.cluster_store_begin(3, np.ones(3, np.uint32))     # no genome set
    e.set_genomes([np.zeros(100, np.uint8), np.ones(120, np.uint8), np.zeros(90, np.uint8)])
    for call in (lambda: e.cluster_level("tani", {}), e.cluster_store_add_kept, e.cluster_store_info,
                 lambda: e.debug_cluster_store_add(records(2, 1))):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            call()                                          # before a store begin
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        e.cluster_store_begin(5)                            # the set's own lengths are those of its 3 genomes
    e.cluster_store_begin()
    assert e.cluster_store_info() == dict(n=3, records=0, record_bytes=0, add_ms=0.0)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        e.cluster_store_add_kept()                          # without a kept result
    e.filter_results(n, lens, ref, off, None, res, {}, fetch=False)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        e.cluster_store_add_kept()                          # a kept result of another n
    one = np.zeros(1, dtype=L.KEPT_DTYPE)
    for a, b, lines in ((1, 1, 3), (2, 1, 3), (0, 3, 3), (0, 1, 0), (0, 1, 4)):
        one["a"], one["b"], one["lines"] = a, b, lines
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            e.debug_cluster_store_add(one)                  # a < b < n, lines in 1..3
    assert e.cluster_store_info()["records"] == 0
    for bad in (L.cluster_cut(ani=float("nan")), L.cluster_cut(len_ratio=float("nan")), L.cluster_cut({}, reserved=1)):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            e.cluster_level("tani", bad)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        e.cluster_level(7, {})
    # a level of an empty store is a begun cluster state without an edge
    assert e.cluster_level("gani", {}) == 0 and e.cluster_run("single") == 3 and e.cluster_level_info()["records_in"] == 0
    one["a"], one["b"], one["lines"], one["x"], one["y"] = 0, 2, 3, (50, 5, 1), (60, 5, 1)
    e.debug_cluster_store_add(one)
    assert e.cluster_level("gani", {}) == 1 and e.cluster_run("single") == 2 and e.cluster_fetch()[0].tolist() == [0, 1, 0]
    assert len(e.debug_cluster_edges(1, 0)) == 0
    for first, count in ((0, 2), (2, 0), (1, 1)):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            e.debug_cluster_edges(first, count)             # past the end
    # an ordinary begun state: more edges may be added; a plain begin has no level info
    e.debug_cluster_add_edges(L.cluster_edges([1], [2], [0.5]))
    assert e.cluster_run("single") == 1 and e.cluster_level_info()["edges_out"] == 1 and e.cluster_info()["edges"] == 2
    e.cluster_begin()
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        e.cluster_level_info()
    assert e.cluster_store_info()["records"] == 1           # the store is independent of the cluster state
    # lzani_set_genomes drops the store
    e.set_genomes([np.zeros(100, np.uint8)])
    for call in (e.cluster_store_info, lambda: e.cluster_level("tani", {}), e.debug_cluster_edges):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            call()
    e.close()


def test_out_of_memory(eng):
    lens, rec, more = node_lengths(), records(10, 51), records(5000, 52)
    eng.cluster_store_begin(N, lens)
    eng.debug_cluster_store_add(rec)
    before = check_level(eng, rec, lens, "ani", CUT_A)
    si = eng.cluster_store_info()
    # a growth that is refused -- at twice the size and at the exact size, its two attempts -- leaves the store
    for count in (2, L.ALLOC_FAULT_ALL):
        fault = L.AllocFault(1, count)
        with pytest.raises(L.LzaniError, match="LZANI_ERR_NOMEM"), fault:
            eng.debug_cluster_store_add(more)
        assert fault.seen >= 1 and eng.cluster_store_info() == si
        assert check_level(eng, rec, lens, "ani", CUT_A).tobytes() == before.tobytes()
    # a level refused at each of its allocation attempts in turn: no cluster state, the store intact, and the call again succeeds
    L.alloc_fault(0)
    eng.cluster_level("ani", CUT_A)
    attempts = L.alloc_fault(0)
    assert attempts >= 5, attempts                          # the lengths, the block counts and offsets, the counters, the edges
    for k in range(1, attempts + 1):
        for count in (1, L.ALLOC_FAULT_ALL):
            fault = L.AllocFault(k, count)
            with pytest.raises(L.LzaniError, match="LZANI_ERR_NOMEM"), fault:
                eng.cluster_level("ani", CUT_A)
            assert fault.seen >= k, (k, fault.seen)
            for call in (eng.cluster_info, eng.cluster_level_info, eng.debug_cluster_edges, lambda: eng.cluster_run("single")):
                with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
                    call()
            assert eng.cluster_store_info() == si
            assert check_level(eng, rec, lens, "ani", CUT_A).tobytes() == before.tobytes()
    # the store grows after all
    eng.debug_cluster_store_add(more)
    check_level(eng, np.concatenate((rec, more)), lens, "tani", CUT_B)


# ---- lzani_run_rows_kept -> store_add_kept -> levels on genomes ---------------------------------------------------------

@pytest.fixture(scope="module")
def genomes():
    seqs = SG.make_set(60, 815, lmin=2000, lmax=4000, fam=10, dmin=0.01, dmax=0.3)[1]
    e = L.Engine()
    e.set_genomes(seqs)
    full = e.all2all()                                      # the raw integers of a plain lzani_run_rows: computed once, left unchanged
    full.setflags(write=False)
    yield seqs, e, full
    e.close()


def test_end_to_end(genomes):
    seqs, eng, full = genomes
    n, lens = len(seqs), np.array([len(s) for s in seqs], dtype=np.uint32)
    dense = L.dense_rows(n) + (None,)
    res = rows_of(full, *dense)
    q = lambda field, quant, above: median_minimum(n, lens, *dense, res, field, quant, above=above)
    loose = q("ani", 0.1, 0.5)
    levels = (("tani", dict(q("ani", 0.6, 0.5), **q("qcov", 0.5, 0.2)), "complete-linkage"), ("ani", dict(len_ratio=0.8, num_alns=40), "single"))
    blocks = list(tiled_blocks(n, 32))
    assert len(blocks) == 2
    # the model: the records of the two kept calls one behind the other
    rec = np.concatenate([M.kept(loose, n, lens, ref, off, qq, rows_of(full, ref, off, qq))[0] for ref, off, qq in blocks])
    want = []
    for measure, cut, algo in levels:
        a, b, w, lines_in, lines_out = CUT.level(cut, measure, rec, lens)
        rep, cl = model_clusters(n, a, b, w, algo)
        k = len(set(rep.tolist()))
        assert 0 < len(a) < len(rec) and 1 < k < n, (cut, len(a), len(rec), k)          # by the model alone
        want.append((len(a), lines_in, lines_out, rep, cl, k))
    assert want[0][0] != want[1][0]
    grp1, grp2 = L.Group(None, (0,)), L.Group(None, (0, 0))
    for other in (eng, grp1, grp2):
        if other is not eng:
            other.set_genomes(seqs)
        other.cluster_store_begin()
        total = 0
        for ref, off, qq in blocks:
            kept = other.run_rows_kept(ref, off, qq, loose)
            total += len(kept)
            assert other.cluster_store_add_kept() == total
        assert total == len(rec) and other.cluster_store_info()["records"] == total and other.cluster_store_info()["add_ms"] > 0
        for (measure, cut, algo), (edges, lines_in, lines_out, rep, cl, k) in zip(levels, want):
            assert other.cluster_level(measure, cut) == edges
            info = other.cluster_level_info()
            assert (info["records_in"], info["edges_out"], info["lines_in"], info["lines_out"]) == (total, edges, lines_in, lines_out), info
            if other is eng:
                check_level(eng, rec, lens, measure, cut)
            assert other.cluster_run(algo) == k
            got_rep, got_cl = other.cluster_fetch()
            assert np.array_equal(got_rep, rep) and np.array_equal(got_cl, cl), (measure, cut, algo)
    grp1.close()
    grp2.close()
