"""GPU: the prefilter's limit stage (lzani_prefilter_limit) against the definition in Python integers
(tests/prefilter_limit_model.py) applied to the unlimited fetch.  Every comparison is total and exact: kmers_of, row_off,
ids and shared of the whole result."""
import numpy as np
import pytest

import lzani_ctypes as L
import prefilter_limit_model as LM
import synth_genomes as SG

pytestmark = pytest.mark.gpu


def _rc(s):
    return (3 - s[::-1]).astype(np.uint8)


def _rand(seed, n):
    return (SG.splitmix64(seed, np.arange(n, dtype=np.uint64)) % np.uint64(4)).astype(np.uint8)


def small_set():
    """The 102 genomes of tests/test_gpu_prefilter.py: 96 of 3-6 kbp in families of 8, an all-N genome, one shorter than
    every k, an exact reverse-complement copy, one with N runs, and a pair that shares half of the smaller k-mer set."""
    _, seqs = SG.make_set(96, 11, lmin=3000, lmax=6000, fam=8)
    seqs = [np.array(s) for s in seqs]
    seqs.append(np.full(200, 5, dtype=np.uint8))
    seqs.append(_rand(71, 6))
    seqs.append(_rc(seqs[3]))
    g = seqs[9].copy()
    g[100:140] = 5
    g[1000:1003] = 4
    g[-5:] = 5
    seqs.append(g)
    x = _rand(72, 1000)
    seqs.append(x)
    seqs.append(np.concatenate((x[:510], np.full(1, 5, dtype=np.uint8), _rand(73, 600))))
    return seqs


@pytest.fixture(scope="module")
def small():
    seqs = small_set()
    eng = L.Engine()
    eng.set_genomes(seqs)
    yield seqs, eng
    eng.close()


@pytest.fixture()
def eng():
    e = L.Engine()
    yield e
    e.close()


def _same(got, want, what):
    for name, g, w in zip(("kmers_of", "row_off", "ids", "shared"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name, g[:8], w[:8])


def _want(unl, n_ref, N):
    """The limited result by the model, from the unlimited fetch."""
    k_of, row_off, ids, shared = unl
    keep = LM.limit(len(k_of), n_ref, k_of, row_off, ids, shared, N)
    return (k_of,) + LM.apply(row_off, ids, shared, keep)


def _limit_and_compare(eng, make, n_ref, Ns, what):
    """make() runs a prefilter; for every N: the result made anew, limited, fetched and compared; returns the infos."""
    make()
    unl = eng.prefilter_fetch()
    infos = []
    for i, N in enumerate(Ns):
        if i:
            make()
        before = eng.prefilter_info()
        want = _want(unl, n_ref, N)
        cnt = eng.prefilter_limit(N)
        _same(eng.prefilter_fetch(), want, (what, N))
        info, after = eng.prefilter_limit_info(), eng.prefilter_info()
        n = len(unl[0])
        limiting, cut = LM.counts(n, n_ref, *unl, N)
        assert cnt == len(want[2]) == info["entries_out"] == after["entries"], (what, N, info)
        assert (info["max_per_genome"], info["limiting"], info["entries_in"], info["genomes_cut"]) == (N, limiting, len(unl[2]), cut), (what, N, info)
        E = len(unl[2])                                     # (keys: 8 B the score key, 16 B or, cross, 8 B the two directed keys, twice)
        assert (info["limit_ms"] > 0 and info["workspace_bytes"] >= 29 * E) if E else (info["limit_ms"], info["workspace_bytes"]) == (0, 0)
        assert {k: v for k, v in after.items() if k != "entries"} == {k: v for k, v in before.items() if k != "entries"}
        infos.append(info)
    return unl, infos


@pytest.mark.parametrize("k", [16, 21])
def test_small_set_against_the_model(small, k):
    seqs, eng = small
    unl, infos = _limit_and_compare(eng, lambda: eng.prefilter(k), 0, (1, 3, 8), ("small", k))
    assert len(unl[0]) == 102 and infos[0]["entries_out"] < infos[0]["entries_in"] and infos[0]["genomes_cut"] > 0
    assert infos[0]["entries_out"] <= infos[1]["entries_out"] <= infos[2]["entries_out"]


def test_a_result_of_several_tiles_and_a_sparse_one(small, monkeypatch):
    seqs, eng = small
    monkeypatch.delenv("LZANI_PREFILTER_TILE_ROWS", raising=False)
    eng.prefilter(16)
    whole = eng.prefilter_fetch()
    monkeypatch.setenv("LZANI_PREFILTER_TILE_ROWS", "7")

    def tiled():
        eng.prefilter(16)
        assert eng.prefilter_info()["tiles"] == (len(seqs) + 6) // 7 > 1

    unl, infos = _limit_and_compare(eng, tiled, 0, (3, 8), "tiled")
    _same(unl, whole, "tiled against whole")
    assert infos[0]["genomes_cut"] > 0
    monkeypatch.delenv("LZANI_PREFILTER_TILE_ROWS")
    eng.set_prefilter_counting("sparse")
    try:
        def sparse():
            eng.prefilter(16)
            assert eng.prefilter_sparse_info()["sparse"] == 1

        unl, _ = _limit_and_compare(eng, sparse, 0, (3,), "sparse")
        _same(unl, whole, "sparse against whole")
    finally:
        eng.set_prefilter_counting("auto")


def test_cross_results(small):
    seqs, eng = small
    n_ref = 40
    unl, infos = _limit_and_compare(eng, lambda: eng.prefilter_cross(16, n_ref), n_ref, (1, 3), "cross")
    assert infos[0]["limiting"] == len(seqs) - n_ref and 0 < infos[0]["entries_out"] < infos[0]["entries_in"]
    unl2, _ = _limit_and_compare(eng, lambda: eng.prefilter_codes_cross(seqs, 16, n_ref), n_ref, (1, 3), "codes cross")
    _same(unl2, unl, "streamed against resident")


def _hub_result(seed, n, n_ref=0):
    """About 40,000 entries over n = 600 (cross form: fewer): most pairs with probability 0.2, the pairs of every 97th genome
    with 0.6, so that the degrees go up to a few hundred; |K| = 1,000 everywhere and three values of shared."""
    rng = np.random.default_rng(seed)
    a, b = np.triu_indices(n, 1)
    if n_ref:
        cross = (a < n_ref) & (b >= n_ref)
        a, b = a[cross], b[cross]
    pick = rng.random(len(a)) < np.where((a % 97 == 0) | (b % 97 == 5), 0.6, 0.2)
    a, b = a[pick], b[pick]
    shared = rng.choice(np.array([250, 500, 1000], dtype=np.uint32), size=len(a)).astype(np.uint32)
    off = np.concatenate(([0], np.cumsum(np.bincount(a, minlength=n)))).astype(np.uint64)
    return np.full(n, 1000, dtype=np.uint32), off, b.astype(np.uint32), shared


@pytest.mark.parametrize("n_ref", [0, 200])
def test_a_made_up_result_across_the_kernels_boundaries(eng, n_ref):
    n, N = 600, 16
    res = _hub_result(5, n, n_ref)
    deg = np.bincount(np.concatenate(LM.pairs_of(res[1], res[2])), minlength=n)
    if not n_ref:
        assert 35_000 < len(res[2]) < 45_000 and deg.max() > 300
    assert 2 * len(res[2]) > 4 * 8192 or n_ref
    unl, infos = _limit_and_compare(eng, lambda: eng.debug_prefilter_set(n, n_ref, *res), n_ref, (N,), ("made up", n_ref))
    _same(unl, res, "the installed result")
    assert infos[0]["genomes_cut"] > 0.9 * infos[0]["limiting"] and infos[0]["entries_out"] <= infos[0]["limiting"] * N


def test_made_up_edge_cases(eng):
    one = (np.array([9], dtype=np.uint32), np.zeros(2, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32))
    _limit_and_compare(eng, lambda: eng.debug_prefilter_set(1, 0, *one), 0, (1, 5), "n = 1")
    none = (np.full(5, 9, dtype=np.uint32), np.zeros(6, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32))
    _, infos = _limit_and_compare(eng, lambda: eng.debug_prefilter_set(5, 0, *none), 0, (2,), "no entry")
    assert (infos[0]["entries_in"], infos[0]["entries_out"], infos[0]["genomes_cut"]) == (0, 0, 0)
    n = 300                                                 # row 0 holds every entry; equal scores in blocks of 50
    row = (np.full(n, 600, dtype=np.uint32),) + LM.csr_of(n, {(0, b): 600 - b // 50 for b in range(1, n)})
    assert int(row[1][1]) == n - 1 == int(row[1][-1])
    _, infos = _limit_and_compare(eng, lambda: eng.debug_prefilter_set(n, 0, *row), 0, (4, 299), "one row")
    assert infos[0]["entries_out"] == n - 1 and infos[0]["genomes_cut"] == 1      # every leaf keeps its only pair
    # the same star as a cross result with one query, the centre, whose rank alone counts
    m = 200
    star = (np.full(m, 600, dtype=np.uint32),) + LM.csr_of(m, {(a, m - 1): 600 - (a % 7) for a in range(m - 1)})
    _, infos = _limit_and_compare(eng, lambda: eng.debug_prefilter_set(m, m - 1, *star), m - 1, (4, 70), "one query")
    assert [i["entries_out"] for i in infos] == [4, 70]


def test_idempotence_on_the_device(small):
    seqs, eng = small
    eng.prefilter(16)
    eng.prefilter_limit(3)
    once = eng.prefilter_fetch()
    cnt = eng.prefilter_limit(3)
    info = eng.prefilter_limit_info()
    _same(eng.prefilter_fetch(), once, "twice")
    assert cnt == len(once[2]) == info["entries_in"] == info["entries_out"]
    # a larger N after a smaller one cannot bring pairs back; a smaller one cuts further, as the model does from there
    eng.prefilter_limit(8)
    _same(eng.prefilter_fetch(), once, "8 after 3")
    eng.prefilter_limit(1)
    _same(eng.prefilter_fetch(), _want(once, 0, 1), "1 after 3")


def test_states_and_refusals(small):
    seqs, eng = small
    fresh = L.Engine()
    try:
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            fresh.prefilter_limit(3)
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            fresh.prefilter_limit_info()
    finally:
        fresh.close()
    eng.prefilter(16)
    unl = eng.prefilter_fetch()
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        eng.prefilter_limit_info()                          # the current result was never limited
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        eng.prefilter_limit(0)
    _same(eng.prefilter_fetch(), unl, "after a refused call")
    assert eng.prefilter_info()["entries"] == len(unl[2])
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        eng.prefilter_limit_info()
    eng.prefilter_limit(2)
    assert eng.prefilter_limit_info()["max_per_genome"] == 2
    eng.prefilter(16)                                       # a new result: not limited
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        eng.prefilter_limit_info()


def test_the_hook_checks_its_arrays(eng):
    k_of = np.full(4, 10, dtype=np.uint32)
    good = ([0, 2, 3, 3, 3], [1, 3, 2], [5, 5, 5])
    eng.debug_prefilter_set(4, 0, k_of, *good)
    for n_ref, off, ids, shared in ((0, [0, 2, 3, 3, 3], [3, 1, 2], [5, 5, 5]), (0, [0, 2, 3, 3, 3], [1, 3, 1], [5, 5, 5]),
                                    (0, [0, 2, 3, 3, 3], [1, 4, 2], [5, 5, 5]), (0, good[0], good[1], [5, 0, 5]),
                                    (0, good[0], good[1], [5, 11, 5]), (4, *good), (2, *good)):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            eng.debug_prefilter_set(4, n_ref, k_of, off, ids, shared)
    _same(eng.prefilter_fetch(), (k_of, np.array(good[0], dtype=np.uint64), np.array(good[1], dtype=np.uint32), np.array(good[2], dtype=np.uint32)),
          "a refused hook call leaves the result")
