"""CPU: the limit rule of the prefilter as a pure host function (lzani_prefilter_limit_host) against the definition in
Python integers (tests/prefilter_limit_model.py), the properties the definition gives, and the refused inputs."""
import ctypes as C

import numpy as np
import pytest

import lzani_ctypes as L
import prefilter_limit_model as LM


@pytest.fixture(scope="module")
def lib():
    L.build_library()
    return L.load_library()


def _host(n, n_ref, res, N):
    return L.prefilter_limit_host(n, n_ref, *res, N)


def _check(lib, n, n_ref, res, N):
    got = _host(n, n_ref, res, N)
    want = LM.limit(n, n_ref, *res, N)
    assert got.dtype == np.uint8 and np.array_equal(got, want), (n, n_ref, N, np.flatnonzero(got != want)[:8])
    return got


def _degrees(n, row_off, ids):
    a, b = LM.pairs_of(row_off, ids)
    return np.bincount(a, minlength=n) + np.bincount(b, minlength=n)


@pytest.mark.parametrize("seed,n,p", [(1, 200, 0.2), (2, 150, 0.6), (3, 37, 1.0), (4, 64, 0.05), (5, 2, 1.0)])
def test_random_graphs_with_ties(lib, seed, n, p):
    res = LM.random_result(seed, n, p)
    for N in (1, 2, 5, 17):
        keep = _check(lib, n, 0, res, N)
        assert n < 10 or 0 < keep.sum()
    if n >= 64 and p >= 0.2:
        assert _host(n, 0, res, 2).sum() < len(res[2])              # the limit cuts something


@pytest.mark.parametrize("seed,n,n_ref,p", [(11, 120, 40, 0.5), (12, 90, 1, 1.0), (13, 90, 89, 0.7)])
def test_random_cross_results(lib, seed, n, n_ref, p):
    res = LM.random_result(seed, n, p, n_ref=n_ref)
    for N in (1, 3, 8):
        _check(lib, n, n_ref, res, N)


def test_star(lib):
    """Genome 0 with 30 partners of descending score: the centre ranks N of them, every leaf ranks the centre first."""
    n = 31
    k_of = np.full(n, 100, dtype=np.uint32)
    res = (k_of,) + LM.csr_of(n, {(0, b): 100 - b for b in range(1, n)})
    for N in (1, 4, 30, 31):
        assert _check(lib, n, 0, res, N).all()                          # the union: every leaf keeps its only pair


def test_clique(lib):
    n = 12                                                              # every degree is 11
    k_of = np.full(n, 50, dtype=np.uint32)
    res = (k_of,) + LM.csr_of(n, {(a, b): 25 for a in range(n) for b in range(a + 1, n)})
    for N in (3, 10, 11, 12):
        keep = _check(lib, n, 0, res, N)
        assert keep.all() == (N >= 11)
    # all scores equal: a genome's list is its partners ascending, so with N = 1 genome g > 0 names 0 and genome 0 names 1
    keep = _host(n, 0, res, 1)
    a, b = LM.pairs_of(res[1], res[2])
    assert sorted(zip(a[keep == 1].tolist(), b[keep == 1].tolist())) == [(0, b) for b in range(1, n)]


def test_empty_graph_and_one_genome(lib):
    for n in (1, 5):
        res = (np.full(n, 7, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32))
        assert len(_check(lib, n, 0, res, 3)) == 0


def test_cross_form_with_one_reference_that_is_every_query_s_best_hit(lib):
    """The references do not limit: reference 0 is the best hit of all 20 queries and keeps all 20 pairs at N = 1; only the
    queries' ranks count.  The same entries read as an all-pairs result give another answer."""
    n_ref, n = 3, 23
    k_of = np.full(n, 1000, dtype=np.uint32)
    edges = {}
    for q in range(n_ref, n):
        edges[(0, q)] = 900
        edges[(1, q)] = 500
        edges[(2, q)] = 100 + q
    res = (k_of,) + LM.csr_of(n, edges)
    keep = _check(lib, n, n_ref, res, 1)
    a, b = LM.pairs_of(res[1], res[2])
    assert keep.sum() == n - n_ref and (a[keep == 1] == 0).all()
    keep2 = _check(lib, n, n_ref, res, 2)
    assert keep2.sum() == 2 * (n - n_ref) and (a[keep2 == 1] <= 1).all()
    # the same entries read as an all-pairs result: the references limit too, and reference 2 keeps its best query
    both = _check(lib, n, 0, res, 1)
    assert both.sum() > keep.sum() and not np.array_equal(both, keep)


def test_the_union_keeps_a_pair_that_only_one_endpoint_ranks(lib):
    """Genome 0 has three strong partners and the weak partner 4, whose only pair it is: at N = 1 genome 0 does not rank 4,
    4 ranks 0, and the pair stays."""
    n = 5
    k_of = np.full(n, 100, dtype=np.uint32)
    res = (k_of,) + LM.csr_of(n, {(0, 1): 90, (0, 2): 80, (0, 3): 70, (0, 4): 10})
    ls = LM.lists(n, 0, *res)
    e = 3                                                               # the entry (0, 4)
    assert [x[2] for x in ls[0]].index(e) == 3 and [x[2] for x in ls[4]].index(e) == 0
    assert _check(lib, n, 0, res, 1).tolist() == [1, 1, 1, 1]           # every leaf names the centre
    # with a second, stronger pair of genome 4 the pair (0, 4) goes: neither endpoint ranks it
    res = (k_of,) + LM.csr_of(n, {(0, 1): 90, (0, 2): 80, (0, 3): 70, (0, 4): 10, (3, 4): 50})
    assert _check(lib, n, 0, res, 1).tolist() == [1, 1, 1, 0, 1]


@pytest.mark.parametrize("n_ref", [0, 25])
def test_properties_of_the_definition(lib, n_ref):
    n = 80
    res = LM.random_result(21 + n_ref, n, 0.4, n_ref=n_ref, values=(100, 300, 301, 900))
    k_of, row_off, ids, shared = res
    deg = _degrees(n, row_off, ids)
    limiting = np.arange(n) >= n_ref
    for N in (1, 3, 9):
        keep = _check(lib, n, n_ref, res, N)
        off2, ids2, sh2 = LM.apply(row_off, ids, shared, keep)
        # idempotence
        assert _host(n, n_ref, (k_of, off2, ids2, sh2), N).all()
        # every limiting genome keeps at least min(d, N) pairs
        deg2 = _degrees(n, off2, ids2)
        assert (deg2[limiting] >= np.minimum(deg, N)[limiting]).all()
        assert keep.sum() <= int(limiting.sum()) * N
    # N >= the largest degree changes nothing; one below cuts the genome that has it (all-pairs: unless its partners keep it)
    top = int(deg[limiting].max())
    assert _host(n, n_ref, res, top).all() and _host(n, n_ref, res, 0xFFFFFFFF).all()
    if n_ref:
        assert not _host(n, n_ref, res, top - 1).all()


def test_the_score_at_its_ends(lib):
    assert LM.score(7, 7, 9) == 0xFFFFFFFF and LM.score(1, 0xFFFFFFFF, 0xFFFFFFFF) == 1
    # shared == min scores 2^32 - 1, above any other ratio; shared = 1 of min = 2^32 - 1 scores 1, below any other
    top = 0xFFFFFFFF
    k_of = np.array([top, top, 5, top, top - 1], dtype=np.uint32)
    edges = {(0, 1): top - 1, (0, 2): 5, (0, 3): 1, (0, 4): 2}
    res = (k_of,) + LM.csr_of(5, edges)
    assert [x[1] for x in LM.lists(5, 0, *res)[0]] == [2, 1, 4, 3]
    assert [-x[0] for x in LM.lists(5, 0, *res)[0]] == [top, top - 1, 2, 1]
    # all-pairs with N = 1: genome 0 keeps (0, 2); the others keep their only pair
    assert _check(lib, 5, 0, res, 1).all()
    # the cross form with the four as references of the one query: the query ranks them by q
    k2 = np.array([top, 5, top, top - 1, top], dtype=np.uint32)
    res = (k2,) + LM.csr_of(5, {(0, 4): top - 1, (1, 4): 5, (2, 4): 1, (3, 4): 2})
    for N, want in ((1, [0, 1, 0, 0]), (2, [1, 1, 0, 0]), (3, [1, 1, 0, 1]), (4, [1, 1, 1, 1])):
        assert _check(lib, 5, 4, res, N).tolist() == want


def _raw(lib, n, n_ref, k_of, row_off, ids, shared, N, keep=True):
    k_of, row_off, ids, shared = (np.ascontiguousarray(x, dtype=t) for x, t in
                                  zip((k_of, row_off, ids, shared), (np.uint32, np.uint64, np.uint32, np.uint32)))
    out = np.zeros(max(len(ids), 1), dtype=np.uint8)
    return lib.lzani_prefilter_limit_host(n, n_ref, L._ptr(k_of), L._ptr(row_off), L._ptr(ids), L._ptr(shared), C.c_uint32(N), L._ptr(out) if keep else None)


def test_refused_inputs(lib):
    ARG = -1
    k_of = [10, 10, 10, 10]
    good = ([0, 2, 3, 3, 3], [1, 3, 2], [5, 5, 5])
    assert _raw(lib, 4, 0, k_of, *good, 1) == 0
    assert _raw(lib, 4, 0, k_of, *good, 0) == ARG                                        # N == 0
    assert _raw(lib, 0, 0, k_of, *good, 1) == ARG                                        # no genomes
    assert _raw(lib, 4, 4, k_of, *good, 1) == ARG and _raw(lib, 4, 9, k_of, *good, 1) == ARG     # n_ref >= n
    assert _raw(lib, 4, 0, k_of, *good, 1, keep=False) == ARG                            # nowhere to write
    assert _raw(lib, 4, 0, k_of, [0, 2, 3, 3, 3], [3, 1, 2], [5, 5, 5], 1) == ARG        # ids descend in a row
    assert _raw(lib, 4, 0, k_of, [0, 2, 3, 3, 3], [1, 1, 2], [5, 5, 5], 1) == ARG        # an id twice
    assert _raw(lib, 4, 0, k_of, [0, 2, 3, 3, 3], [1, 3, 1], [5, 5, 5], 1) == ARG        # an id equal to its row
    assert _raw(lib, 4, 0, k_of, [0, 2, 3, 3, 3], [1, 3, 0], [5, 5, 5], 1) == ARG        # an id below its row
    assert _raw(lib, 4, 0, k_of, [0, 2, 3, 3, 3], [1, 4, 2], [5, 5, 5], 1) == ARG        # an id >= n
    assert _raw(lib, 4, 0, k_of, *good[:2], [5, 0, 5], 1) == ARG                          # shared == 0
    assert _raw(lib, 4, 0, k_of, *good[:2], [5, 11, 5], 1) == ARG                         # shared > min(|K|)
    assert _raw(lib, 4, 0, [10, 10, 10, 4], *good[:2], [5, 5, 5], 1) == ARG               # ... of the smaller set
    assert _raw(lib, 4, 0, k_of, *good[:2], [5, 10, 5], 1) == 0                           # shared == min is the top score
    assert _raw(lib, 4, 0, k_of, [1, 2, 3, 3, 3], *good[1:], 1) == ARG                    # offsets that do not start at 0
    assert _raw(lib, 4, 0, k_of, [0, 2, 1, 3, 3], *good[1:], 1) == ARG                    # offsets that descend
    assert _raw(lib, 4, 0, k_of, [0, 0, 0, 0, (1 << 31) - 8], [], [], 1) == ARG           # more than 2^31 - 9 entries
    # the cross form holds pairs a < n_ref <= b only
    assert _raw(lib, 4, 2, k_of, [0, 2, 3, 3, 3], [2, 3, 2], [5, 5, 5], 1) == 0
    assert _raw(lib, 4, 2, k_of, *good, 1) == ARG                                        # (0, 1): two references
    assert _raw(lib, 4, 1, k_of, [0, 1, 2, 2, 2], [1, 2], [5, 5], 1) == ARG              # (1, 2): two queries


def test_the_binding_raises(lib):
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        L.prefilter_limit_host(2, 0, [5, 5], [0, 1, 1], [1], [5], 0)
