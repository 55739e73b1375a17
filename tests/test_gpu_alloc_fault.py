"""GPU: every out-of-memory promise of include/lzani.h, and every fallback form that only memory pressure selects, reached
with the allocation fault of lzani_devmem.h (lzani_debug_alloc_fault; no memory is exhausted).

One helper, sweep(): a call is run once unarmed -- its result equals the reference, and `A`, the allocation attempts it
makes, is read from the hook -- then once for every k in 1 .. A with attempt k refused (count = 1) or attempt k and every
one behind it (count = 2^63), from a fresh state each time.  A refused attempt may end in two ways only:
  LZANI_ERR_NOMEM with a message, and the state the header promises (after_failure);
  success with the reference's result and, in the call's own report, the trace of a fallback form (fallback_seen).
Then the same call again in the same context gives the reference's result, and so does a call of another stage (two dense
rows against the oracle: "otherwise unchanged").  References: oracle_all2all, prefilter_model, prefilter_cross_model,
prefilter_limit_model, out_filter_model and the cluster models; run_rows_regions' region records against an unarmed run of
the same rows (the records' own parity is tests/test_gpu_parity.py's).  Every comparison is total and exact."""
import numpy as np
import pytest

import cluster_cover_model as CC
import cluster_graphs as G
import cluster_link_model as KM
import cluster_model as CM
import lzani_ctypes as L
import ooc_model as OM
import oracle as O
import out_filter_model as M
import prefilter_cross_model as XM
import prefilter_limit_model as LM
import prefilter_model as PM
import synth_genomes as SG

pytestmark = pytest.mark.gpu

ALL = L.ALLOC_FAULT_ALL
COUNTS = [pytest.param(1, id="one"), pytest.param(ALL, id="from_k_on")]
K = 16                                                  # the prefilter's k


# ---- the shapes: the smallest at which every allocation site of a call is reached ------------------------------------
_cache = {}


def genomes():
    """8 genomes of 2-4 kbp in families of 4, an empty one and an all-N one; their oracle all2all, made once."""
    if "set" not in _cache:
        seqs = SG.make_set(8, 77, lmin=2000, lmax=4000, fam=4)[1] + [np.zeros(0, np.uint8), np.full(300, 5, np.uint8)]
        full = O.oracle_all2all(seqs, None, threads=4)
        full.setflags(write=False)
        _cache["set"] = (seqs, full)
    return _cache["set"]


def long_genomes():
    """4 genomes of 8.5-9.5 kbp (tag words at mal 11, which the join form needs) and their oracle all2all."""
    if "long" not in _cache:
        seqs = SG.make_set(4, 78, lmin=8500, lmax=9500, fam=2)[1]
        full = O.oracle_all2all(seqs, None, threads=4)
        full.setflags(write=False)
        _cache["long"] = (seqs, full)
    return _cache["long"]


def rows_of(full, ref, off, q):
    r, x = M.entries_of(full.shape[0], ref, off, q)
    return full[r, x]


def sym_lists(n, seed, p=0.6):
    """ref_ids, row_off, query_ids of symmetric lists: distinct references, ascending lists, every pair in both directions"""
    rng = np.random.default_rng(seed)
    adj = np.triu(rng.random((n, n)) < p, 1)
    adj = adj | adj.T
    rows = [(r, np.flatnonzero(adj[r]).tolist()) for r in range(n)]
    ref = np.array([r for r, _ in rows], dtype=np.uint32)
    off = np.cumsum([0] + [len(x) for _, x in rows]).astype(np.uint64)
    return ref, off, np.array([x for _, xs in rows for x in xs], dtype=np.uint32)


def same(got, want):
    """total and exact: arrays by dtype-free value and shape, records by their bytes, tuples and dicts member by member"""
    if isinstance(want, dict):
        return isinstance(got, dict) and got.keys() == want.keys() and all(same(got[k], want[k]) for k in want)
    if isinstance(want, (tuple, list)):
        return len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    if isinstance(want, np.ndarray):
        got = np.asarray(got)
        if want.dtype.names:
            return got.dtype == want.dtype and got.tobytes() == want.tobytes()
        return got.shape == want.shape and np.array_equal(got, want)
    return got == want


def code_of(err):
    """the LZANI_ERR_* name and the message behind it, of an LzaniError of the binding"""
    text = str(err)
    for name in L.ERRORS.values():
        if name in text:
            return name, text.split(name, 1)[1].lstrip(": ").strip()
    return None, text


def is_state(fn):
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        fn()
    return True


def sweep(fresh, call, reference, after_failure, fallback_seen, *, min_attempts, count=1, read=None, other=None, message=True, appends=False):
    """fresh(): the state the call starts from (unarmed).  call(): the call under the fault; read(): its result, fetched
    unarmed (default: what call() returned).  after_failure(): the header's postcondition of LZANI_ERR_NOMEM.
    fallback_seen(): whether the call's own report shows a fallback form (None: the call has none).  other(): a call of
    another stage checked against its own reference.  appends: the call adds to what is there, so that after a success
    it is not made a second time.  Returns (A, the k that ended in NOMEM, the k that were absorbed)."""
    result = (lambda r: r) if read is None else (lambda r: read())
    fresh()
    L.alloc_fault(0)
    r = call()
    A = L.alloc_fault(0)                                    # the attempts of the call alone
    assert same(result(r), reference), "unarmed"
    assert A >= min_attempts, (A, min_attempts)             # a hook that has come unplugged fails here
    nomem, absorbed = [], []
    for k in range(1, A + 1):
        fresh()
        fault = L.AllocFault(k, count)
        try:
            with fault:
                r = call()
            failed = None
        except L.LzaniError as e:
            failed = e
        assert fault.seen >= k, (k, fault.seen)             # the armed attempt was reached
        if failed is not None:
            name, msg = code_of(failed)
            if name == "LZANI_ERR_DEVICE":                  # the device itself objected: nothing more is started on it in this session
                pytest.exit(f"alloc-fault sweep, attempt {k} refused: {failed}", returncode=3)
            assert name == "LZANI_ERR_NOMEM" and (msg or not message), (k, str(failed))
            after_failure()
            nomem.append(k)
        else:
            assert same(result(r), reference), ("absorbed", k)
            assert fallback_seen is not None and fallback_seen(), ("a success that leaves no trace of a fallback", k)
            absorbed.append(k)
        if failed is not None or not appends:
            assert same(result(call()), reference), ("the same call again", k)
        if other is not None:
            other()
    print(f"alloc-fault sweep: A={A} count={'1' if count == 1 else 'all'} nomem={nomem} absorbed={absorbed}")
    return A, nomem, absorbed


@pytest.fixture()
def eng():
    e = L.Engine()
    yield e
    L.alloc_fault(0)
    e.close()


LAUNCHES = ("bitmap_launches", "lpt_launches", "split_launches")


def faster_form_gone(e, base):
    """the fallback's trace in lzani_get_layout: a faster form's launches, there in the unarmed run (`base`), are 0 in the last run"""
    def seen():
        lay = e.layout()
        return any(base[x] > 0 and lay[x] == 0 for x in LAUNCHES)
    return seen


def two_rows(e, full):
    """the other stage: two dense rows against the oracle"""
    ref, off = L.dense_rows(full.shape[0], [1, 2])

    def other():
        assert np.array_equal(e.run_rows(ref, off), rows_of(full, ref, off, None))
    return other


# ---- Engine() and lzani_set_genomes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
def test_create(count):
    seqs, full = genomes()
    made = []

    def call():
        made.append(L.Engine())
        return True

    def fresh():
        while made:
            made.pop().close()

    def other():                                            # a context made after the refusal is a whole one
        e = L.Engine()
        e.set_genomes(seqs)
        two_rows(e, full)()
        e.close()

    sweep(fresh, call, True, lambda: None, None, min_attempts=1, count=count, other=other, message=False)
    fresh()


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("form", ["in_core", "out_of_core"])
def test_set_genomes(eng, form, count):
    seqs, full = genomes()
    lens = [len(s) for s in seqs]
    eng.set_genome_memory(OM.limit_for_blocks(lens, None, 3) if form == "out_of_core" else 0)
    ref, off = L.dense_rows(len(seqs))

    def no_set():                                           # the header: without a genome set until a set_genomes succeeds
        assert is_state(lambda: eng.run_rows(ref, off))
        assert is_state(lambda: eng.prefilter(K))
        assert is_state(lambda: eng.cluster_begin(len(seqs)))
        assert eng.residency()["blocks"] == 0

    def read():
        assert eng.residency()["blocks"] == (3 if form == "out_of_core" else 1)
        return eng.run_rows(ref, off)

    # in-core: codes, offsets, five tables, two k-mer arrays, two pinned buffers; out-of-core: seven tables, staging, two upload tables
    sweep(lambda: None, lambda: eng.set_genomes(seqs), rows_of(full, ref, off, None), no_set, None,
          min_attempts=11 if form == "in_core" else 10, count=count, read=read, other=two_rows(eng, full))


# ---- lzani_run_rows: one configuration per allocation-distinct path -----------------------------------------------------
BITMAPS = {"LZANI_PM_MIN_ROWS": "1", "LZANI_SPLIT": "0", "LZANI_LPT": "0"}
RUN_CONFIGS = {
    # name: (environment, genome set, rows, unconditional attempts, a check of the unarmed run's layout)
    "dense": ({}, "set", "dense", 4, None),
    "bitmaps": (dict(BITMAPS, LZANI_PM_FROM_INDEX="0"), "set", "dense", 6, lambda lay: lay["bitmap_launches"] > 0 and lay["matrix_from_index"] == 0),
    "bitmaps_from_index": (dict(BITMAPS, LZANI_PM_FROM_INDEX="1"), "set", "dense", 6, lambda lay: lay["bitmap_launches"] > 0 and lay["matrix_from_index"] > 0),
    "lists": (dict(BITMAPS, LZANI_PM_MIN_SHARE="1"), "set", "lists", 8, lambda lay: lay["bitmap_launches"] > 0),
    "probe_lists": ({"LZANI_PM": "0"}, "set", "lists", 5, lambda lay: lay["bitmap_launches"] == 0),
    "split": ({"LZANI_PM_MIN_ROWS": "1", "LZANI_SPLIT": "1", "LZANI_SPLIT_SEGLEN": "512", "LZANI_SPLIT_ALL": "1"}, "set", "dense", 15,
              lambda lay: lay["split_launches"] > 0),
    "lpt": ({"LZANI_PM_MIN_ROWS": "1", "LZANI_SPLIT": "0", "LZANI_LPT": "1"}, "set", "dense", 8, lambda lay: lay["lpt_launches"] > 0),
    "join": ({"LZANI_JOIN_MIN_BYTES": "1", "LZANI_PM": "0"}, "long", "dense", 10, lambda lay: lay["join_lists"] == 1),
    "sort_index": ({"LZANI_SORT_INDEX_MIN_DIRBITS": "0", "LZANI_PM": "0"}, "set", "dense", 9, None),
}
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("config", list(RUN_CONFIGS))
def test_run_rows(eng, monkeypatch, config, count):
    env, which, rows, least, layout_ok = RUN_CONFIGS[config]
    monkeypatch.setenv("LZANI_RTC", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    seqs, full = genomes() if which == "set" else long_genomes()
    n = len(seqs)
    ref, off, q = (L.dense_rows(n) + (None,)) if rows == "dense" else sym_lists(n, 5)
    eng.set_genomes(seqs)
    eng.run_rows(ref, off, q)
    base = eng.layout()
    assert layout_ok is None or layout_ok(base), base
    if config == "sort_index":
        assert eng.debug_index_slab([0])["build"] == "sort"

    sweep(lambda: eng.set_genomes(seqs), lambda: eng.run_rows(ref, off, q), rows_of(full, ref, off, q), lambda: None, faster_form_gone(eng, base),
          min_attempts=least, count=count, other=two_rows(eng, full))


@pytest.mark.parametrize("count", COUNTS)
def test_run_rows_regions_with_its_grow_and_retry(eng, monkeypatch, count):
    monkeypatch.setenv("LZANI_RTC", "0")
    seqs, full = genomes()
    ref, off = L.dense_rows(len(seqs))
    eng.set_genomes(seqs)
    res, regs = eng.run_rows_regions(ref, off)
    assert np.array_equal(res, rows_of(full, ref, off, None)) and len(regs) > 64          # (capacity 64 below: a second call)
    # two calls of two region buffers, the result buffer and the run's four
    sweep(lambda: eng.set_genomes(seqs), lambda: eng.run_rows_regions(ref, off, capacity=64), (rows_of(full, ref, off, None), regs),
          lambda: None, None, min_attempts=14, count=count, other=two_rows(eng, full))


@pytest.mark.parametrize("count", COUNTS)
def test_run_rows_out_of_core(eng, monkeypatch, count):
    monkeypatch.setenv("LZANI_RTC", "0")
    seqs, full = genomes()
    eng.set_genome_memory(OM.limit_for_blocks([len(s) for s in seqs], None, 3))
    ref, off = L.dense_rows(len(seqs))
    eng.set_genomes(seqs)
    eng.run_rows(ref, off)
    base = eng.layout()

    def call():
        out = eng.run_rows(ref, off)
        assert eng.residency()["tiles"] == 9
        return out

    # per tile: the result buffer (grown), and the run's four
    sweep(lambda: eng.set_genomes(seqs), call, rows_of(full, ref, off, None), lambda: None, faster_form_gone(eng, base), min_attempts=5, count=count,
          other=two_rows(eng, full))


# ---- the prefilter family ----------------------------------------------------------------------------------------------
def _pf_model(seqs):
    if "pf" not in _cache:
        _cache["pf"] = PM.shared_matrix(seqs, K, PM.SAMPLE_ALL)
    return _cache["pf"]


PF_FORMS = ("one_pass", "three_passes", "tiles_of_7", "sparse", "cross", "codes_two_slices")


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("form", PF_FORMS)
def test_prefilter(eng, monkeypatch, form, count):
    seqs, full = genomes()
    n, n_ref = len(seqs), 2
    kmers_of, shared = _pf_model(seqs)
    want = (kmers_of.astype(np.uint32),) + (XM.kept_pairs(kmers_of, shared, n_ref) if form == "cross" else PM.kept_pairs(kmers_of, shared))
    assert len(want[2]) >= 3
    if form == "three_passes":
        monkeypatch.setenv("LZANI_PREFILTER_PASSES", "3")
    if form == "tiles_of_7":
        monkeypatch.setenv("LZANI_PREFILTER_TILE_ROWS", "7")
    if form == "sparse":
        eng.set_prefilter_counting("sparse")
    slice_bytes = sum(len(s) for s in seqs[:5])
    if form == "codes_two_slices":
        assert L.plan_slices([len(s) for s in seqs], slice_bytes)[0] == 2
    eng.set_genomes(seqs)

    def call():
        if form == "cross":
            return eng.prefilter_cross(K, n_ref)
        if form == "codes_two_slices":
            return eng.prefilter_codes(seqs, K, slice_bytes=slice_bytes)
        return eng.prefilter(K)

    def read():
        if form == "three_passes":
            assert eng.prefilter_pass_info()["passes"] == 3
        if form == "tiles_of_7":
            assert eng.prefilter_info()["tiles"] == 2
        if form == "sparse":
            assert eng.prefilter_sparse_info()["sparse"] == 1
        if form == "codes_two_slices":
            assert eng.prefilter_stream_info()["slices"] == 2
        return eng.prefilter_fetch()

    def no_result():                                        # "holds no prefilter result and is otherwise unchanged"
        assert is_state(eng.prefilter_fetch) and is_state(eng.prefilter_info) and is_state(eng.prefilter_limit_info)

    def fresh():                                            # an earlier result, of another k: never served in place of the failed call's
        eng.set_genomes(seqs)
        eng.prefilter(K + 1)

    # cbase, blkcnt, blkoff, kmers_of; ka, kb, ucnt, uoff, tmp; runoff; the tile's or the table's three or five; a tile's ids and shared
    sweep(fresh, call, want, no_result, None, min_attempts=14 if form != "codes_two_slices" else 17, count=count, read=read, other=two_rows(eng, full))


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("source", ["resident_tiles", "debug_set"])
def test_prefilter_limit(eng, monkeypatch, source, count):
    seqs, full = genomes()
    n, N = len(seqs), 2
    eng.set_genomes(seqs)
    if source == "resident_tiles":
        monkeypatch.setenv("LZANI_PREFILTER_TILE_ROWS", "7")
        unl = PM.prefilter(seqs, K)
    else:
        unl = tuple(np.ascontiguousarray(x) for x in LM.random_result(9, 40, 0.3))

    def fresh():
        if source == "resident_tiles":
            eng.prefilter(K)
            assert eng.prefilter_info()["tiles"] == 2     # the stage gathers the tiles into buffers of its own
        else:
            eng.debug_prefilter_set(len(unl[0]), 0, *unl)
        state["fetch"], state["info"] = eng.prefilter_fetch(), eng.prefilter_info()
        assert same(state["fetch"], unl)

    state = {}
    keep = LM.limit(len(unl[0]), 0, *unl, N)
    want = (unl[0].astype(np.uint32),) + LM.apply(unl[1], unl[2], unl[3], keep)
    assert 0 < len(want[2]) < len(unl[2])

    def read():
        info = eng.prefilter_limit_info()
        assert (info["max_per_genome"], info["entries_in"], info["entries_out"]) == (N, len(unl[2]), len(want[2]))
        return eng.prefilter_fetch()

    def unlimited_in_place():                               # "leaves the unlimited result in place and readable"
        got = eng.prefilter_fetch()
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, state["fetch"]))
        assert is_state(eng.prefilter_limit_info)
        assert eng.prefilter_info() == state["info"]

    # rowoff, row_of, ka, kb, kq, scratch, survive, deg, rowcnt, cut, start, outoff, the result's ids and shared (+ the gathered ids and shared)
    sweep(fresh, lambda: eng.prefilter_limit(N), want, unlimited_in_place, None, min_attempts=14, count=count, read=read, other=two_rows(eng, full))


# ---- the output filter ------------------------------------------------------------------------------------------------
def _filter_of(seqs, full, ref, off, q):
    lens = np.array([len(s) for s in seqs], dtype=np.uint32)
    res = rows_of(full, ref, off, q)
    rec = M.kept({}, len(seqs), lens, ref, off, q, res)[0]
    v = np.sort(M.ratios(rec["x"], rec["y"], lens[rec["a"]], lens[rec["b"]])["ani"].ravel())
    v = v[v > 0.5]                                          # (the lines of related pairs: unrelated genomes align next to nothing)
    flt = {"ani": float(v[len(v) // 2])}                    # a minimum of the data itself: some pairs kept, some not
    want = M.kept(flt, len(seqs), lens, ref, off, q, res)[0]
    assert 0 < len(want) < len(rec)
    return lens, res, flt, want


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("form", ["dense", "lists", "filter_results"])
def test_kept(eng, monkeypatch, form, count):
    monkeypatch.setenv("LZANI_RTC", "0")
    seqs, full = genomes()
    n = len(seqs)
    ref, off, q = sym_lists(n, 6) if form == "lists" else L.dense_rows(n) + (None,)
    lens, res, flt, want = _filter_of(seqs, full, ref, off, q)
    eref, eoff = L.dense_rows(n, [0, 1, 2, 3])
    eng.set_genomes(seqs)
    eng.run_rows(ref, off, q)
    base = eng.layout()

    def fresh():                                            # an earlier kept result, of other rows
        eng.set_genomes(seqs)
        assert len(eng.run_rows_kept(eref, eoff)) > 0

    def call():
        if form == "filter_results":
            return eng.filter_results(n, lens, ref, off, q, res, flt)
        return eng.run_rows_kept(ref, off, q, flt)

    def no_result():                                        # "without a kept result": the earlier call's is not served either
        assert is_state(lambda: eng.kept_fetch(0, 0)) and is_state(eng.kept_info)

    # the result buffer; (the run's four;) the stage's seven, the lists, the records
    sweep(fresh, call, want, no_result, None if form == "filter_results" else faster_form_gone(eng, base), min_attempts=9 if form == "filter_results" else 8 + 5, count=count, other=two_rows(eng, full))


# ---- the cluster stage -----------------------------------------------------------------------------------------------
def cluster_want(algo, n, a, b, w):
    """(rep_of, cluster_of) of the algorithm's model"""
    key = ("cl", algo, len(a))
    if key not in _cache:
        if algo in CM.ALGOS:
            rep = CM.cluster(n, CM.edge_set(a, b, w), algo)[0]
        elif algo == "set-cover":
            rep = CC.cover(n, CM.edge_set(a, b))
        elif algo == "complete-linkage":
            rep = KM.linkage(n, KM.edge_min(a, b, w))
        else:
            from test_cluster_leiden import model
            rep = np.array(model(n, a, b, w)["rep_of"], dtype=np.uint32)
        _cache[key] = (np.asarray(rep, dtype=np.uint32), KM.number(rep)[0])
    return _cache[key]


def small_random():
    n, a, b, w = G.graphs()["small_random"]
    return n, a, b, w, L.cluster_edges(a, b, w)


CL_STAMPS = ("add_ms", "run_ms")


@pytest.mark.parametrize("count", COUNTS)
def test_cluster_begin(eng, count):
    seqs, full = genomes()
    n, a, b, w, edges = small_random()
    eng.set_genomes(seqs)

    def fresh():                                            # a state there was: the begin drops it first
        eng.cluster_begin(n, np.ones(n, np.uint32))
        eng.debug_cluster_add_edges(edges)

    def read():
        info = eng.cluster_info()
        return (info["n"], info["edges"], info["algo"], info["edge_bytes"])

    def no_state():                                         # the header: no cluster state until a begin succeeds
        assert is_state(eng.cluster_info) and is_state(lambda: eng.cluster_run("single")) and is_state(lambda: eng.debug_cluster_add_edges(edges))

    sweep(fresh, lambda: eng.cluster_begin(n, np.full(n, 7, np.uint32), "ani"), (n, 0, -1, 0), no_state, None, min_attempts=1, count=count, read=read,
          other=two_rows(eng, full))


@pytest.mark.parametrize("count", COUNTS)
def test_cluster_add_edges_in_two_pieces(eng, count):
    seqs, full = genomes()
    n, a, b, w, edges = small_random()
    first, second = edges[:450], edges[450:]                # 2 * 450 > 700: "twice the size" and "the exact size" differ
    eng.set_genomes(seqs)
    want_all, want_first = cluster_want("single", n, a, b, w), cluster_want("single", n, a[:450], b[:450], w[:450])

    def fresh():
        eng.cluster_begin(n, np.ones(n, np.uint32))
        eng.debug_cluster_add_edges(first)
        eng.cluster_run("greedy-first")
        state["last"] = eng.cluster_fetch()

    state = {}

    def read():
        assert eng.cluster_info()["edges"] == len(edges)
        eng.cluster_run("single")
        return eng.cluster_fetch()

    def edges_as_they_were():                               # the header: the edges that were there, and the last run's result with them
        assert eng.cluster_info()["edges"] == len(first) and eng.cluster_info()["edge_bytes"] == 16 * len(first)
        assert same(eng.cluster_fetch(), state["last"])
        eng.cluster_run("single")
        assert same(eng.cluster_fetch(), want_first)

    def fallback_seen():                                    # cluster_reserve's second try: the exact size, not twice the buffer
        info = eng.cluster_info()
        return info["edge_bytes"] == 16 * info["edges"]

    A, nomem, absorbed = sweep(fresh, lambda: eng.debug_cluster_add_edges(second), want_all, edges_as_they_were, fallback_seen, min_attempts=1, count=count, read=read, other=two_rows(eng, full),
                                appends=True)
    assert A == 1 and (absorbed == [1]) == (count == 1)


@pytest.mark.parametrize("count", COUNTS)
def test_cluster_add_kept(eng, monkeypatch, count):
    monkeypatch.setenv("LZANI_RTC", "0")
    seqs, full = genomes()
    n = len(seqs)
    ref, off = L.dense_rows(n)
    lens, res, flt, kept = _filter_of(seqs, full, ref, off, None)
    wt = CM.weight("tani", kept["x"], kept["y"], kept["lines"], lens[kept["a"]], lens[kept["b"]])
    want = CM.cluster(n, CM.edge_set(kept["a"], kept["b"], wt), "greedy-best")[:2]
    eng.set_genomes(seqs)
    assert same(eng.run_rows_kept(ref, off, None, flt), kept)

    def fresh():
        eng.cluster_begin()
        assert eng.cluster_add_kept() == len(kept)

    def read():
        assert eng.cluster_info()["edges"] == 2 * len(kept)
        eng.cluster_run("greedy-best")
        return eng.cluster_fetch()

    def edges_as_they_were():                               # "leaves the edges that were there": a run gives the model's clusters of exactly those
        assert eng.cluster_info()["edges"] == len(kept)
        eng.cluster_run("greedy-best")
        assert same(eng.cluster_fetch(), want)

    def fallback_seen():
        info = eng.cluster_info()
        return info["edge_bytes"] == 16 * info["edges"]

    sweep(fresh, lambda: eng.cluster_add_kept(), want, edges_as_they_were, fallback_seen, min_attempts=1, count=count, read=read, other=two_rows(eng, full),
          appends=True)


# unconditional attempts of a run: the stage's own (flag, size, below, counters, undecided, rep_of, cluster_of; parent, state, blocked, best)
# and the algorithm's workspace
CLUSTER_ALGOS = {"single": 11, "greedy-first": 11, "greedy-best": 11, "set-cover": 7 + 9, "complete-linkage": 7 + 13, "leiden-cpm": 7 + 30}


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("algo", list(CLUSTER_ALGOS))
def test_cluster_run(eng, algo, count):
    seqs, full = genomes()
    n, a, b, w, edges = small_random()
    eng.set_genomes(seqs)
    earlier = "greedy-first" if algo == "single" else "single"
    want = cluster_want(algo, n, a, b, w)
    assert not same(want, cluster_want(earlier, n, a, b, w))

    def fresh():                                            # an earlier successful run, of another algorithm
        eng.cluster_begin(n, np.ones(n, np.uint32))
        eng.debug_cluster_add_edges(edges)
        eng.cluster_run(earlier)
        state["fetch"], state["info"] = eng.cluster_fetch(), eng.cluster_info()
        assert same(state["fetch"], cluster_want(earlier, n, a, b, w))

    state = {}

    def read():
        info = eng.cluster_info()
        assert info["algo"] == L.CLUSTER_ALGOS[algo] and info["edges"] == len(edges)
        return eng.cluster_fetch()

    def as_before_the_run():                                # the header, every algorithm: the earlier run's result and figures
        assert same(eng.cluster_fetch(), state["fetch"])
        assert eng.cluster_info() == state["info"]
        for other_info in (eng.cluster_cover_info, eng.cluster_link_info, eng.cluster_leiden_info):
            assert is_state(other_info)

    sweep(fresh, lambda: eng.cluster_run(algo), want, as_before_the_run, None, min_attempts=CLUSTER_ALGOS[algo], count=count, read=read,
          other=two_rows(eng, full))


# ---- the group: two contexts on one device, their threads share the counter ------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("form", ["run_rows", "run_rows_kept"])
def test_group(monkeypatch, form, count):
    monkeypatch.setenv("LZANI_RTC", "0")
    seqs, full = genomes()
    n = len(seqs)
    ref, off = L.dense_rows(n)
    lens, res, flt, kept = _filter_of(seqs, full, ref, off, None)
    single = L.Engine()
    single.set_genomes(seqs)
    want = single.run_rows(ref, off) if form == "run_rows" else single.run_rows_kept(ref, off, None, flt)
    single.close()
    assert same(want, rows_of(full, ref, off, None) if form == "run_rows" else kept)
    grp = []

    def fresh():                                            # a new group: buffers an earlier iteration grew would hide the later sites
        while grp:
            grp.pop().close()
        grp.append(L.Group(None, (0, 0)))
        grp[0].set_genomes(seqs)

    def call():
        return grp[0].run_rows(ref, off) if form == "run_rows" else grp[0].run_rows_kept(ref, off, None, flt)

    def after_failure():
        if form == "run_rows_kept":
            assert is_state(lambda: grp[0].kept_fetch(0, 0)) and is_state(grp[0].kept_info)

    try:
        # the gathered and the ordered buffer, a shard buffer, the scatter table, (two pinned buffers | the stage), each context's run
        # (five rows a context: below the rows candidate bitmaps take, so no refusal can be absorbed and every k ends in NOMEM)
        sweep(fresh, call, want, after_failure, None, min_attempts=12, count=count)
    finally:
        L.alloc_fault(0)
        while grp:
            grp.pop().close()
