"""GPU: the alignment-region stage on the device.  The stage alone (lzani_debug_order_regions) on made-up regions, byte for
byte against tests/aln_regions_model.py, at the shapes at which it can go wrong; then lzani_run_rows_aligned on the example
set and on small genome sets -- dense rows, lists, an out-of-core context -- against lzani_run_rows_regions put through the
model and against the oracle's regions; the state rules; and every allocation of both calls refused in turn."""
import numpy as np
import pytest

import aln_regions_model as M
import lzani_ctypes as L
import ooc_model as OM
import oracle as O
import out_filter_model as FM
import synth_genomes as SG
import util as U

pytestmark = pytest.mark.gpu

CHUNK, TILE = 4096, 8192                                # raw regions a block of the compaction takes; keys a tile of the sort takes
COUNTS = ("entries", "found", "kept", "entries_with_regions", "entries_dropped")


def same(got, want):
    assert got.dtype == L.REGION_DTYPE == M.REGION_DTYPE and got.dtype.itemsize == 32
    assert len(got) == len(want)
    for k in M.REGION_DTYPE.names:
        assert np.array_equal(got[k], want[k]), k
    assert got.tobytes() == want.tobytes()


def check(eng, call, flt):
    """one order_regions call against the model: the bytes, the counts, the passes, the bytes that came to the host"""
    n, aln_len, ref, off, q, regs = call
    want, info, stays, _ = M.order(n, aln_len, ref, off, q, regs, flt)
    got = eng.order_regions(n, aln_len, ref, off, q, regs, flt)
    same(got, want)
    gi = eng.regions_info()
    assert {k: gi[k] for k in COUNTS} == info, (gi, info)
    assert gi["sort_passes"] == M.sort_passes(info["entries"], want), gi
    assert gi["bytes_to_host"] == 32 * len(got) and gi["capacity"] == len(regs) and gi["runs"] == 0
    return want, info, stays


@pytest.fixture(scope="module")
def eng():
    e = L.Engine()                                      # the stage alone needs no genome set
    yield e
    e.close()


def symmetric_lists(n, seed, p=0.5):
    rng = np.random.default_rng(seed)
    adj = np.triu(rng.random((n, n)) < p, 1)
    adj = adj | adj.T
    return [(r, np.flatnonzero(adj[r]).tolist()) for r in range(n)]


def list_call(seed, count, maxv, n=12):
    """a made-up call on symmetric lists of n genomes: between 8 and 255 entries, 70 % of them own regions"""
    rng = np.random.default_rng(seed)
    ref, off, q = M.lists(symmetric_lists(n, seed))
    assert 8 < int(off[-1]) < 256
    return n, rng.integers(1, 6 * maxv, n).astype(np.uint32), ref, off, q, M.random_regions(rng, int(off[-1]), count, maxv)


def median_of(call, field="qcov"):
    flt = M.median_filters(*call)[field]
    assert flt is not None
    return flt


@pytest.mark.parametrize("count", [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, TILE - 1, TILE, TILE + 1])
def test_chunk_and_tile_edges(eng, count):
    """`count` raw regions with a NULL filter (as many keys: the sort's tile, and every block of the compaction full) and with
    a median (regions that stay and regions that go just before the edge)"""
    call = list_call(700 + count, count, 60000)
    want, info, _ = check(eng, call, None)
    assert len(want) == count
    if count >= 4:
        flt = median_of(call)
        want, info, stays = check(eng, call, flt)
        assert 0 < len(want) < count
        keep = stays[call[5]["pair"].astype(np.int64)]
        for edge in (CHUNK, TILE):
            if count >= edge - 1:                       # (behind the edge there is at most one region here: the NULL filter keeps it)
                assert keep[edge - 65:edge - 1].any() and not keep[edge - 65:edge - 1].all()


def test_all_regions_in_one_entry_and_in_the_first_and_last_only(eng):
    rng = np.random.default_rng(31)
    n = 9
    ref, off, q = M.lists(symmetric_lists(n, 31))
    E = int(off[-1])
    assert E > 8
    al = rng.integers(1000, 90000, n).astype(np.uint32)
    for owners in ([E // 2], [0], [E - 1], [0, E - 1]):
        regs = M.random_regions(rng, E, 5000, 60000, owners=owners)
        want, info, _ = check(eng, (n, al, ref, off, q, regs), None)
        assert info["entries_with_regions"] == len(owners) and len(want) == 5000
        assert sorted(set(want["pair"].tolist())) == owners
        check(eng, (n, al, ref, off, q, regs), {"ani": 2.0})                  # ... and the filter drops it (them)


def test_the_filter_drops_the_first_the_last_every_and_no_entry(eng):
    # genome 0 is a query in the first entry only, genome 6 in the last entry only
    ref, off, q = M.lists([(1, [0]), (2, [3, 4, 5]), (3, [2, 4, 5]), (4, [2, 3]), (5, [6])])
    E = int(off[-1])
    rng = np.random.default_rng(32)
    regs = M.random_regions(rng, E, 600, 400, owners=np.arange(E), ties=0)
    regs["num_matches"], regs["num_mismatches"] = regs["seq_end"] - regs["seq_start"], 0
    base = np.full(7, 20000, dtype=np.uint32)           # 60 regions of 200 on average in 20,000: qcov around 0.6
    flt = {"qcov": 0.2}
    for long_ones, gone in (((0,), [0]), ((6,), [E - 1]), ((0, 6), [0, E - 1]), ((), [])):
        al = base.copy()
        al[list(long_ones)] = 4_000_000
        want, info, stays = check(eng, (7, al, ref, off, q, regs), flt)
        assert np.flatnonzero(~stays).tolist() == gone and info["entries_dropped"] == len(gone)
    want, info, stays = check(eng, (7, base, ref, off, q, regs), {"ani": 2.0})
    assert len(want) == 0 and info["entries_dropped"] == E
    assert len(eng.regions_fetch(0, 0)) == 0
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        eng.regions_fetch(0, 1)


@pytest.mark.parametrize("maxv,passes", [(200, 1), (60000, 2), (1 << 23, 3)])
def test_fields_of_one_two_and_three_radix_passes(eng, maxv, passes):
    call = list_call(40 + passes, 3000, maxv)           # (the entry takes one pass)
    want, _, _ = check(eng, call, None)
    assert eng.regions_info()["sort_passes"] == 2 * passes + 1
    check(eng, call, median_of(call, "gani"))


def test_fields_of_zero_bits(eng):
    """A call of one entry (the entry's sort covers no bit: the sort is a copy), every start 0, every length the same."""
    ref, off, q = M.lists([(1, [0])])
    al = np.array([5000, 7], dtype=np.uint32)
    rng = np.random.default_rng(44)
    regs = M.random_regions(rng, 1, 300, 900, owners=[0], ties=0)
    want, _, _ = check(eng, (2, al, ref, off, q, regs), None)
    assert eng.regions_info()["sort_passes"] == 2 + 2 + 0 and len(want) == 300
    zero = regs.copy()
    zero["seq_end"] -= zero["seq_start"]
    zero["seq_start"] = 0
    check(eng, (2, al, ref, off, q, zero), {"qcov": 0.0})
    assert eng.regions_info()["sort_passes"] == 0 + 2 + 0
    flat = zero.copy()
    flat["seq_end"] = 1                                  # one start, one length, one entry: three copies, the input order stays
    want, _, _ = check(eng, (2, al, ref, off, q, flat), None)
    assert eng.regions_info()["sort_passes"] == 0 + 1 + 0 and want.tobytes() == flat.tobytes()
    check(eng, (2, al, ref, off, q, flat), {"ani": 2.0})


@pytest.mark.parametrize("n,passes", [(300, 3), (4200, 4)])
def test_entry_numbers_beyond_two_to_the_16_and_24(eng, n, passes):
    rng = np.random.default_rng(n)
    ref, off, q = M.dense(n)
    E = int(off[-1])
    assert E > (1 << (8 * (passes - 1))) and E == n * (n - 1)
    owners = np.unique(np.concatenate((rng.integers(0, E, 60), [0, (1 << (8 * (passes - 1))) + 3, E - 1])))
    regs = M.random_regions(rng, E, 400, 200, owners=owners)
    al = rng.integers(100, 3000, n).astype(np.uint32)
    call = (n, al, ref, off, q, regs)
    want, info, _ = check(eng, call, None)
    assert eng.regions_info()["sort_passes"] == 2 + passes and int(want["pair"].max()) == E - 1
    want, info, _ = check(eng, call, median_of(call, "ani"))
    assert 0 < info["entries_dropped"] < info["entries_with_regions"]


def test_ties_empty_rows_and_a_fetch_in_pieces(eng):
    rng = np.random.default_rng(33)
    ref, off, q = M.lists([(5, [0, 1, 2, 3, 4, 6, 7]), (7, []), (0, [4, 5, 7]), (2, []), (4, [0, 1, 2])])
    E = int(off[-1])
    regs = M.random_regions(rng, E, 6000, 60000, owners=np.arange(E), ties=0.5)
    key = np.stack((regs["pair"].astype(np.int64), regs["seq_start"], regs["seq_end"]), axis=1)
    assert len(np.unique(key, axis=0)) < 0.8 * len(key)
    al = rng.integers(1000, 90000, 8).astype(np.uint32)
    call = (8, al, ref, off, q, regs)
    check(eng, call, None)
    want, _, _ = check(eng, call, median_of(call))
    K = len(want)
    a, b = K // 3, K - 5
    same(np.concatenate((eng.regions_fetch(0, a), eng.regions_fetch(a, b - a), eng.regions_fetch(b, K - b))), want)
    assert eng.regions_info()["bytes_to_host"] == 32 * 2 * K
    same(eng.regions_fetch(K, 0), want[:0])
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        eng.regions_fetch(1, K)
    # the rows out of id order: the order is the call's entries', not the ids'
    r_of, _ = FM.entries_of(8, ref, off, q)
    assert r_of[want["pair"].astype(np.int64)].tolist() != sorted(r_of[want["pair"].astype(np.int64)].tolist())


def test_refusals_on_the_host_leave_the_last_result(eng):
    ref, off, q = M.lists([(0, [1, 2]), (1, [0, 2]), (2, [0, 1])])
    al = np.array([100, 100, 100], dtype=np.uint32)
    good = M.random_regions(np.random.default_rng(1), 6, 10, 50)
    want, _, _ = check(eng, (3, al, ref, off, q, good), None)
    bad = good.copy()
    bad["pair"][3] = 6
    empty = good.copy()
    empty["seq_end"][2] = empty["seq_start"][2]
    neg = good.copy()
    neg["num_matches"][0] = -1
    for args in ((3, al, ref, off, q, bad, None), (3, al, ref, off, q, empty, None), (3, al, ref, off, q, neg, None),
                 (3, al, ref, off, q, good, {"qcov": float("nan")}),
                 (3, al, *M.lists([(0, [2, 1]), (1, [0, 2]), (2, [0, 1])]), good, None),
                 (3, al, *M.lists([(0, [1, 2]), (1, [0, 2]), (0, [1])]), good[good["pair"] < 5], None)):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            eng.order_regions(*args)
    same(eng.regions_fetch(0, len(want)), want)
    assert len(eng.order_regions(3, al, ref, off, q, good, {"tani": float("nan"), "rcov": float("nan")})) == 10      # (not read)


# ---- lzani_run_rows_aligned on the example set -------------------------------------------------------------------------
COLS = ("ref_start", "ref_end", "seq_start", "seq_end", "num_matches", "num_mismatches")


def oracle_regions(seqs, ref, off, q):
    r_of, q_of = FM.entries_of(len(seqs), ref, off, q)
    parts = []
    for e, (r, x) in enumerate(zip(r_of, q_of)):
        w = O.oracle_pair(seqs[r], seqs[x], None, want_regions=True)[1]
        p = np.zeros(len(w), dtype=M.REGION_DTYPE)
        p["pair"] = e
        for k, c in enumerate(COLS):
            p[c] = w[:, k]
        parts.append(p)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=M.REGION_DTYPE)


@pytest.fixture(scope="module")
def example():
    """the example set in the file's order, an engine that holds it, and the references of every case below, computed once
    and left unchanged: lzani_run_rows, lzani_run_rows_regions and the oracle's regions of the dense rows"""
    names, seqs = U.reorder(*U.load_example())
    e = L.Engine()
    e.set_genomes(seqs)
    ref, off = L.dense_rows(len(seqs))
    plain = e.run_rows(ref, off)
    res, raw = e.run_rows_regions(ref, off)
    assert np.array_equal(res, plain)
    orc = oracle_regions(seqs, ref, off, None)
    for a in (plain, raw, orc):
        a.setflags(write=False)
    yield seqs, e, plain, raw, orc
    e.close()


def aligned(eng, ref, off, q, **kw):
    out, nk, nr = eng.run_rows_aligned(ref, off, q, **kw)
    return out, nk, eng.regions_fetch(0, nr)


def test_example_set_dense_rows_capacity_and_the_one_repeat(example):
    seqs, eng, plain, raw, orc = example
    n, lens = len(seqs), np.array([len(s) for s in seqs], dtype=np.uint32)
    ref, off = L.dense_rows(n)
    want, winfo, _, _ = M.order(n, lens, ref, off, None, raw)
    assert len(raw) == 5693 and CHUNK < len(raw) < TILE
    same(want, M.order(n, lens, ref, off, None, orc)[0])                     # the oracle's regions, through the model
    out, nk, got = aligned(eng, ref, off, None)
    assert np.array_equal(out, plain) and nk == 0
    same(got, want)
    info = eng.regions_info()
    assert {k: info[k] for k in COUNTS} == winfo
    assert info["runs"] == 1 and info["capacity"] >= 5693 and info["bytes_to_host"] == 32 * 5693
    assert info["sort_passes"] == M.sort_passes(132, want)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):              # no kept filter: no kept result
        eng.kept_info()
    eng.set_region_capacity(1024)
    try:
        out, nk, got = aligned(eng, ref, off, None)
    finally:
        eng.set_region_capacity(0)
    info = eng.regions_info()
    assert info["runs"] == 2 and info["capacity"] == 5693
    assert np.array_equal(out, plain)
    same(got, want)
    assert np.array_equal(eng.run_rows(ref, off), plain)


def test_example_set_with_a_kept_filter_and_an_alignment_filter(example):
    seqs, eng, plain, raw, orc = example
    n, lens = len(seqs), np.array([len(s) for s in seqs], dtype=np.uint32)
    ref, off = L.dense_rows(n)
    rec = FM.kept({}, n, lens, ref, off, None, plain)[0]
    v = np.sort(FM.ratios(rec["x"], rec["y"], lens[rec["a"]], lens[rec["b"]])["ani"].ravel())
    kflt = {"ani": float(v[len(v) // 2])}
    records = eng.run_rows_kept(ref, off, None, kflt)
    assert 0 < len(records) < len(rec)
    kinfo = eng.kept_info()
    aflt = {}
    for f in M.median_filters(n, lens, ref, off, None, raw).values():
        aflt.update(f)
    want, winfo, _, _ = M.order(n, lens, ref, off, None, raw, aflt)
    assert 0 < winfo["entries_dropped"] < 132
    rl = lens + np.uint32(40)
    for report_len, aln_len in ((None, None), (rl, lens), (None, rl)):
        out, nk, got = aligned(eng, ref, off, None, kept_flt=kflt, report_len=report_len, aln_flt=aflt, aln_len=aln_len)
        assert np.array_equal(out, plain)
        krec = eng.kept_fetch(0, nk)
        if report_len is None:
            assert krec.tobytes() == records.tobytes()
            ki = eng.kept_info()
            assert {k: ki[k] for k in ki if k != "filter_ms"} == {k: kinfo[k] for k in kinfo if k != "filter_ms"}
        else:
            assert krec.tobytes() == FM.kept(kflt, n, rl, ref, off, None, plain)[0].tobytes()
        same(got, want if aln_len is None or aln_len is lens else M.order(n, rl, ref, off, None, raw, aflt)[0])
    assert {k: eng.regions_info()[k] for k in COUNTS} == M.order(n, rl, ref, off, None, raw, aflt)[1]
    _, _, got = aligned(eng, ref, off, None, results=False)                   # no results asked for: the regions alone
    same(got, M.order(n, lens, ref, off, None, raw)[0])


def through_the_model(eng, seqs, ref, off, q, flt=None):
    """run_rows_aligned against run_rows_regions put through the model; returns the regions info"""
    n, lens = len(seqs), np.array([len(s) for s in seqs], dtype=np.uint32)
    res, raw = eng.run_rows_regions(ref, off, q)
    want, winfo, _, _ = M.order(n, lens, ref, off, q, raw, flt)
    out, nk, got = aligned(eng, ref, off, q, aln_flt=flt)
    assert np.array_equal(out, res)
    same(got, want)
    info = eng.regions_info()
    assert {k: info[k] for k in COUNTS} == winfo
    return info


def test_example_set_lists_and_out_of_core(example):
    seqs, eng, plain, raw, orc = example
    n, lens = len(seqs), np.array([len(s) for s in seqs], dtype=np.uint32)
    sym = M.lists(symmetric_lists(n, 51))
    rng = np.random.default_rng(52)
    one_way = M.lists([(int(r), [x for x in range(n) if x > r and rng.random() < 0.6]) for r in rng.permutation(n)])       # a pair in one direction only
    assert int(one_way[1][-1]) > 10
    for ref, off, q in (sym, one_way):
        info = through_the_model(eng, seqs, ref, off, q)
        assert info["runs"] == 1 and info["found"] > 0
        same(eng.regions_fetch(0, info["kept"]), M.order(n, lens, ref, off, q, oracle_regions(seqs, ref, off, q))[0])
    ooc = L.Engine()
    ooc.set_genome_memory(OM.limit_for_blocks([int(x) for x in lens], None, 3))
    ooc.set_genomes(seqs)
    assert ooc.residency()["blocks"] == 3
    ref, off = L.dense_rows(n)
    want = M.order(n, lens, ref, off, None, raw)[0]
    out, nk, got = aligned(ooc, ref, off, None)
    assert ooc.residency()["tiles"] > 1 and np.array_equal(out, plain)
    same(got, want)
    ooc.set_region_capacity(1024)
    out, nk, got = aligned(ooc, *sym)
    assert ooc.regions_info()["runs"] == 2
    same(got, M.order(n, lens, *sym, eng.run_rows_regions(*sym)[1])[0])
    ooc.close()


def test_a_small_set_with_n_runs():
    seqs = U.instantiation_set("small N")
    eng = L.Engine()
    eng.set_genomes(seqs)
    ref, off = L.dense_rows(len(seqs))
    info = through_the_model(eng, seqs, ref, off, None)
    assert info["found"] > 20 and info["runs"] == 1
    raw = eng.run_rows_regions(ref, off)[1]
    flt = M.median_filters(len(seqs), [len(s) for s in seqs], ref, off, None, raw)["ani"]
    info = through_the_model(eng, seqs, ref, off, None, flt)
    assert 0 < info["entries_dropped"] < info["entries_with_regions"]
    eng.close()


# ---- state ------------------------------------------------------------------------------------------------------------
def test_state_rules():
    seqs = SG.make_set(6, 91, lmin=2000, lmax=3000, fam=3)[1]
    n = len(seqs)
    eng = L.Engine()
    for fn in (lambda: eng.regions_fetch(0, 0), eng.regions_info):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            fn()
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        eng.run_rows_aligned(*L.dense_rows(n))                                # no genome set
    eng.set_genomes(seqs)
    ref, off = L.dense_rows(n)
    # a prefilter result and cluster state survive a regions call
    pairs = eng.prefilter(16)
    pf = eng.prefilter_fetch()
    kept = eng.run_rows_kept(ref, off, None, {})
    eng.cluster_begin()
    eng.cluster_add_kept()
    clusters = eng.cluster_run("single")
    reps = eng.cluster_fetch()
    out, nk, nr = eng.run_rows_aligned(ref, off)
    assert nr > 0 and eng.regions_info()["kept"] == nr
    assert eng.prefilter_info()["entries"] == pairs and all(a.tobytes() == b.tobytes() for a, b in zip(eng.prefilter_fetch(), pf))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(eng.cluster_fetch(), reps)) and eng.cluster_info()["clusters"] == clusters
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):              # the aligned call is a kept call: the last kept result went
        eng.kept_info()
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        eng.regions_fetch(nr, 1)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        eng.regions_fetch(nr + 1, 0)
    # refused on the host: the result stays
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        eng.run_rows_aligned(*M.lists([(0, [2, 1])]))
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        eng.run_rows_aligned(ref, off, aln_flt={"ani": float("nan")})
    assert eng.regions_info()["kept"] == nr
    # a kept call leaves the regions; lzani_set_genomes drops them
    assert len(eng.run_rows_kept(ref, off, None, {})) == len(kept)
    assert len(eng.regions_fetch(0, nr)) == nr
    eng.set_genomes(seqs)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        eng.regions_fetch(0, 0)
    assert eng.run_rows_aligned(*L.dense_rows(n, []))[2] == 0 and eng.regions_info()["entries"] == 0       # no rows at all
    eng.close()


# ---- out of memory ----------------------------------------------------------------------------------------------------
FAULT_COUNTS = [pytest.param(1, id="one"), pytest.param(L.ALLOC_FAULT_ALL, id="from_k_on")]


@pytest.fixture()
def fault_eng():
    e = L.Engine()
    yield e
    L.alloc_fault(0)
    e.close()


def no_results(eng):
    def check_it():
        for fn in (lambda: eng.regions_fetch(0, 0), eng.regions_info, lambda: eng.kept_fetch(0, 0), eng.kept_info):
            with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
                fn()
    return check_it


@pytest.mark.parametrize("count", FAULT_COUNTS)
@pytest.mark.parametrize("form", ["lists_filtered", "dense_filtered", "no_filter"])
def test_every_allocation_of_order_regions_refused_in_turn(fault_eng, form, count):
    from test_gpu_alloc_fault import sweep
    eng = fault_eng
    call = list_call(61, 5000, 60000, n=9)
    if form == "dense_filtered":
        call = (9, call[1]) + M.dense(9) + (M.random_regions(np.random.default_rng(62), 72, 5000, 60000),)
    flt = None if form == "no_filter" else median_of(call)
    want = M.order(*call, flt)[0]
    assert 0 < len(want)
    ref, off, q = M.lists([(0, [1, 2]), (1, [0, 2]), (2, [0, 1])])
    lens3, res3 = np.array([900, 900, 900], dtype=np.uint32), np.full((6, 3), 5, dtype=np.int32)

    def fresh():                                            # an earlier regions result and an earlier kept result
        eng.order_regions(*call[:5], call[5][:100], None)
        assert len(eng.filter_results(3, lens3, ref, off, q, res3, {})) == 3

    # the upload; sums, has, keep, counters, blkcnt, blkoff; (the rule's two or three tables;) the result, two key buffers, the scratch
    sweep(fresh, lambda: eng.order_regions(*call, flt), want, no_results(eng), None, min_attempts=11 if flt is None else 13, count=count)


@pytest.mark.parametrize("count", FAULT_COUNTS)
def test_every_allocation_of_run_rows_aligned_refused_in_turn(fault_eng, monkeypatch, count):
    from test_gpu_alloc_fault import genomes, rows_of, sweep, two_rows
    monkeypatch.setenv("LZANI_RTC", "0")
    eng = fault_eng
    seqs, full = genomes()
    n, lens = len(seqs), np.array([len(s) for s in seqs], dtype=np.uint32)
    ref, off = L.dense_rows(n)
    eng.set_genomes(seqs)
    raw = eng.run_rows_regions(ref, off)[1]
    assert len(raw) > 64
    kflt = {"ani": 0.8}
    aflt = M.median_filters(n, lens, ref, off, None, raw)["ani"]
    want_regs = M.order(n, lens, ref, off, None, raw, aflt)[0]
    want_kept = FM.kept(kflt, n, lens, ref, off, None, rows_of(full, ref, off, None))[0]
    assert 0 < len(want_regs) < len(raw) and 0 < len(want_kept)
    eng.set_region_capacity(64)                              # a second run: its buffers are attempts too

    def fresh():
        eng.set_genomes(seqs)
        eng.run_rows_aligned(*L.dense_rows(n, [0, 1, 2, 3]), kept_flt={})

    def call():
        out, nk, nr = eng.run_rows_aligned(ref, off, None, kept_flt=kflt, aln_flt=aflt)
        assert eng.regions_info()["runs"] == 2
        return out, eng.kept_fetch(0, nk), eng.regions_fetch(0, nr)

    # the result buffer, the counter, two raw buffers, two runs' four, the kept stage's eight, the region stage's thirteen
    sweep(fresh, call, (rows_of(full, ref, off, None), want_kept, want_regs), no_results(eng), None, min_attempts=30, count=count, other=two_rows(eng, full))
