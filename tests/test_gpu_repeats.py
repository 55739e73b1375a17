"""GPU: the pair path, the index and the k-mer prefilter on repeat-structured genomes (tests/repeat_genomes.py).

The random genomes of the other GPU tests hold a k-mer once, so which occurrence the device's index hands out -- tag words,
bucket table, LDS index build, refill resolve, LDS filter, null and stretch chains, candidate bitmaps, presence matrix, join,
split -- is never put to the question there.  Every expected value here is made on the CPU and pinned by
tests/test_repeats.py: the oracle (equal to the reference build and the host model on these inputs), the host model's index
and split counts, and the numpy statement of the prefilter."""
import ctypes as C
import time

import numpy as np
import pytest

import lzani_ctypes as L
import oracle as O
import path_cover as PC
import prefilter_cross_model as XM
import prefilter_model as PM
import repeat_genomes as RG
import repeat_ties as RT
import synth_genomes as SG
import util as U
from inst_cell import FORM_ENV, diff, regions_of, run_cell
from test_gpu_parity import _bucketwise_sorted

pytestmark = pytest.mark.gpu

INDEX_FORMS = {"tagwords": {}, "buckets": {"LZANI_NO_TAGWORDS": "1"}, "directory": {"LZANI_NO_BUCKETS": "1"}}
INDEX_BUILDS = {"lds-build": {}, "global-atomics": {"LZANI_NO_LDS_INDEX": "1"}, "sort-build": {"LZANI_SORT_INDEX_MIN_DIRBITS": "0"}}
SLAB_BUILD = {"lds-build": "lds", "global-atomics": "atomics", "sort-build": "sort"}      # what debug_index_slab calls them
BUILD_ENV = ("LZANI_NO_LDS_INDEX", "LZANI_SORT_INDEX_MIN_DIRBITS")
PF_ENV = ("LZANI_PREFILTER_PASSES", "LZANI_PREFILTER_MAX_WINDOWS", "LZANI_PREFILTER_TILE_ROWS", "LZANI_PREFILTER_SLICE_BYTES",
          "LZANI_PREFILTER_TABLE_SLOTS")
_ORACLE = {}


@pytest.fixture(scope="module")
def rtc_cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("rtc_cache"))


def _oracle(setname, prm_name):
    key = (setname, prm_name)
    if key not in _ORACLE:
        _ORACLE[key] = O.oracle_all2all(RG.repeat_set(setname), U.INST_PARAMS[prm_name], threads=16)
    return _ORACLE[key]


def _env(monkeypatch, env):
    for k in FORM_ENV + BUILD_ENV + PF_ENV + ("LZANI_PM_FROM_INDEX",):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _gpu_all2all(seqs, prm=None):
    eng = L.Engine(prm)
    try:
        eng.set_genomes(seqs)
        return eng.all2all()
    finally:
        eng.close()


# ---- every instantiation cell on its repeat set ------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", U.INST_CELLS, ids=[c["id"] for c in U.INST_CELLS])
def test_instantiation_matches_the_oracle_on_repeats(monkeypatch, rtc_cache, cell):
    run_cell(monkeypatch, rtc_cache, cell, RG.repeat_set(cell["set"]), _oracle(cell["set"], cell["prm"]))


# ---- the exit sets: pairs laid out for single exits of the hand-written loops, on the shipped library -------------------------
EXIT_CELLS = [c for c in PC.cells() if c["set"] in RG.EXIT_SET_NAMES]


@pytest.mark.parametrize("cell", EXIT_CELLS, ids=[c["id"].replace(" | ", "-").replace(" ", "_") for c in EXIT_CELLS])
def test_exit_sets_match_the_oracle(monkeypatch, rtc_cache, cell):
    """Every chain class of tests/path_cover.py that runs an exit set (repeat_genomes.exit_set), on the shipped library: the
    class's kernel in the launch record, every pair bit-equal to the oracle."""
    key = ("exit", cell["set"], cell["prm"])
    if key not in _ORACLE:
        _ORACLE[key] = O.oracle_all2all(RG.exit_set(cell["set"]), U.INST_PARAMS[cell["prm"]], threads=16)
    run_cell(monkeypatch, rtc_cache, cell, RG.exit_set(cell["set"]), _ORACLE[key])


# ---- differential fuzz ---------------------------------------------------------------------------------------------------------
def _fuzz(monkeypatch, make, seeds):
    _env(monkeypatch, {})
    t0 = time.time()
    for seed in seeds:
        prm, seqs = make(SG.Stream(seed))
        got = _gpu_all2all(seqs, prm)
        want = O.oracle_all2all(seqs, prm, threads=16)
        bad = np.argwhere((got != want).any(axis=2))
        assert len(bad) == 0, (seed, prm, [len(s) for s in seqs], bad[:3].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    print(f"{len(seeds)} cases, {time.time() - t0:.2f} s")


@pytest.mark.parametrize("chunk", range(8))
def test_fuzz_medium_structured(monkeypatch, chunk):
    """40 cases of five structured genomes of 8-40 kbp under fuzz_case_medium's parameters, five a test."""
    _fuzz(monkeypatch, RG.fuzz_medium, [810000 + s for s in range(5 * chunk, 5 * chunk + 5)])


@pytest.mark.parametrize("chunk", range(4))
def test_fuzz_short_structured(monkeypatch, chunk):
    """60 cases of five structured genomes of 50-1,500 bp under fuzz_case's parameters (the wide tuples among them)."""
    _fuzz(monkeypatch, RG.fuzz_short, [820000 + s for s in range(15 * chunk, 15 * chunk + 15)])


# ---- the tie cases -------------------------------------------------------------------------------------------------------------
TIES = RT.tie_cases()
_TIE_SET = [x for c in TIES for x in (c["ref"], c["qry"])]                  # genome 2 i the reference of case i, 2 i + 1 its query
_TIE_ORACLE = {}


def _tie_oracle():
    if not _TIE_ORACLE:
        for i, c in enumerate(TIES):
            for r, q in ((2 * i, 2 * i + 1), (2 * i + 1, 2 * i)):
                _TIE_ORACLE[(r, q)] = O.oracle_pair(_TIE_SET[r], _TIE_SET[q], None, want_regions=True)
    return _TIE_ORACLE


@pytest.mark.parametrize("build", INDEX_BUILDS, ids=list(INDEX_BUILDS))
@pytest.mark.parametrize("form", INDEX_FORMS, ids=list(INDEX_FORMS))
def test_tie_cases_take_the_stated_occurrence(monkeypatch, form, build):
    """Every tie case, both directions, through run_rows_regions under each form of the index and each of its builds: every
    region equal to the oracle's, and the stated occurrence taken."""
    env = dict(INDEX_FORMS[form], **INDEX_BUILDS[build])
    _env(monkeypatch, env)
    want = _tie_oracle()
    n = len(_TIE_SET)
    ref_ids = np.arange(n, dtype=np.uint32)
    off = np.arange(n + 1, dtype=np.uint64)
    q = (ref_ids ^ 1).astype(np.uint32)
    eng = L.Engine()
    try:
        eng.set_genomes(_TIE_SET)
        out, regs = eng.run_rows_regions(ref_ids, off, q)
        rec = eng.kernel_launches()
        slab = eng.debug_index_slab(ref_ids[:4])
    finally:
        eng.close()
    assert slab["build"] == SLAB_BUILD[build], (build, slab["build"])           # the switches chose the build the case names
    assert set(rec) == U.predict_kernels(_TIE_SET, None, env, "regions"), rec
    for e in range(n):
        res, oregs = want[(e, e ^ 1)]
        got = regions_of(regs, e)
        assert tuple(out[e]) == res and np.array_equal(got, oregs), (TIES[e // 2]["name"], e, got[:3].tolist(), oregs[:3].tolist())
        if e % 2 == 0:
            c = TIES[e // 2]
            assert RT.occurrence(c, got) == c["want"] != c["other"], c["name"]


@pytest.mark.parametrize("form", ["block", "bitmaps", "join", "probe"])
def test_tie_cases_through_the_other_forms(monkeypatch, form):
    """The tie cases' result triples through the block kernel with its LDS filter (every query 128 times in its row), the
    candidate bitmaps of the presence matrix, the join form and the probe form: bit-equal to the oracle, by the kernel the form
    names.  These runs check agreement, not the choice: where both copies give equally long matches (a, c, g) the triple
    mostly cannot tell which one was taken.  The choice is pinned on the regions path alone (the test above)."""
    env = dict(U._INST_FORM_ENV[form], LZANI_RTC="0")
    _env(monkeypatch, env)
    want = _tie_oracle()
    n = len(_TIE_SET)
    ref_ids = np.arange(n, dtype=np.uint32)
    per_row = 128 if form == "block" else 1
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(per_row)
    q = np.repeat(ref_ids ^ 1, per_row).astype(np.uint32)
    eng = L.Engine()
    try:
        eng.set_genomes(_TIE_SET)
        if form == "bitmaps":
            dense = eng.all2all()
            out = np.stack([dense[e, e ^ 1] for e in range(n)])
            per_row = n - 1
        else:
            full = eng.run_rows(ref_ids, off, q)
            out = full[::per_row]
            assert np.array_equal(full.reshape(n, per_row, 3), np.repeat(out[:, None, :], per_row, axis=1))
        rec = eng.kernel_launches()
    finally:
        eng.close()
    kform = "all2all" if form == "bitmaps" else "dup_lists" if form == "block" else "lists"
    assert set(rec) == U.predict_kernels(_TIE_SET, None, env, kform, pairs_per_row=per_row, n_rows=n), (form, rec)
    assert len(rec) == 1 and {"block": "pairs_blk", "bitmaps": "cand=2", "join": "cand=1", "probe": "cand=0"}[form] in next(iter(rec)), rec
    exp = np.array([want[(e, e ^ 1)][0] for e in range(n)], dtype=np.int32)
    assert np.array_equal(out, exp), (form, diff(out, exp))


# ---- the index of repeat genomes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", INDEX_BUILDS, ids=list(INDEX_BUILDS))
@pytest.mark.parametrize("name", ["small", "split", "split N"])
def test_index_of_repeat_genomes(monkeypatch, name, build):
    """debug_index of every genome against the host model's directory and entries, for the three builds.  Buckets of
    repeated k-mers hold up to a few hundred entries here (the random sets: two).  The LDS build falls back where a range of
    16,384 buckets holds more than 24,576 entries or a bucket more than 65,535: by the model's directory no genome within the
    generator's caps does, and the slots' status must say the same."""
    _env(monkeypatch, INDEX_BUILDS[build])
    seqs = RG.repeat_set(name)
    lib = U.model_lib()
    maxlen = max(len(s) for s in seqs)
    eng = L.Engine()
    try:
        eng.set_genomes(seqs)
        big_buckets = 0
        falls = []
        for gid, s in enumerate(seqs):
            d = eng.debug_index(gid)
            T = 2 * len(s) + 3 * eng.params["mrd"]
            wn = (T + 63) // 64 + 2
            t2, nm = np.zeros(2 * wn, np.uint64), np.zeros(wn, np.uint64)
            dirz, ent = np.zeros(len(d["dirz"]), np.uint32), np.zeros(T + 1, np.uint32)
            n_ent = C.c_uint32(0)
            s = np.ascontiguousarray(s)
            assert lib.model_index(O._ptr(s), len(s), maxlen, O.params_array(None), O._ptr(t2), O._ptr(nm), O._ptr(dirz), O._ptr(ent),
                                   C.byref(n_ent)) == 0
            assert np.array_equal(d["dirz"], dirz), (name, gid)
            assert n_ent.value == len(d["ent"]) and np.array_equal(_bucketwise_sorted(d["dirz"], d["ent"]), ent[:n_ent.value]), (name, gid)
            cnt = np.diff(dirz.astype(np.int64))
            for b in np.nonzero((cnt > 1) & (cnt <= 32))[0][:2000]:                # small buckets come sorted from the device
                seg = d["ent"][dirz[b]:dirz[b + 1]]
                assert np.all(seg[:-1] <= seg[1:]), (name, gid, int(b))
            big_buckets += int((cnt > 32).sum())
            rb = min(len(cnt), 16384)
            falls.append(int(cnt.max() > 65535 or max(int(cnt[r:r + rb].sum()) for r in range(0, len(cnt), rb)) > 24576))
        assert big_buckets > 0, name                                                 # (fill-order buckets exist at all)
        slab = eng.debug_index_slab(np.arange(len(seqs), dtype=np.uint32))
        print(name, build, "slab build:", slab["build"], "status:", slab["status"].tolist(), "model:", falls)
        assert slab["build"] == SLAB_BUILD[build], (build, slab["build"])
        if slab["build"] == "lds":
            assert [int(x != 0) for x in slab["status"]] == falls, (name, slab["status"].tolist(), falls)
    finally:
        eng.close()


# ---- the split ---------------------------------------------------------------------------------------------------------------
SPLIT_CASES = [(name, pn) for name in ("split", "split N") for pn in ("defaults", "long", "generic")] + \
    [("fuzz 8", "long"), ("fuzz 20", "long"), ("fuzz 20", "generic"), ("fuzz 16", "defaults")]


@pytest.mark.parametrize("name,pn", SPLIT_CASES, ids=["%s-%s" % c for c in SPLIT_CASES])
def test_split_of_repeat_sets(monkeypatch, name, pn):
    """The 'split' repeat sets, and the four seeded sets of tests/test_repeats.py with the most void segments on the model
    (up to ten resumes of one pair and eleven rounds, voids of two classes), cut every 512 query positions (util.SPLIT_REPAIR_ENV): results
    equal to the oracle, and the repair loop's counts -- these sets get void segments by themselves -- equal to the model's."""
    _env(monkeypatch, U.SPLIT_REPAIR_ENV)
    prm = U.INST_PARAMS[pn]
    if name.startswith("fuzz "):
        seqs = RG.fuzz_set(int(name.split(" ")[1]))
        want = O.oracle_all2all(seqs, prm, threads=16)
    else:
        seqs, want = RG.repeat_set(name), _oracle(name, pn)
    mres, model = U.model_split_rounds(seqs, prm, seglen=512)
    assert np.array_equal(mres, want)
    eng = L.Engine(prm)
    try:
        eng.set_genomes(seqs)
        got = eng.all2all()
        st, rec = eng.split_stats(), eng.kernel_launches()
    finally:
        eng.close()
    counts = ("pairs_cut", "rounds", "resumed", "given_up", "voids")
    print(name, pn, "device", {k: st[k] for k in counts}, "model", {k: model[k] for k in counts})
    assert set(rec) == U.predict_kernels(seqs, prm, U.SPLIT_REPAIR_ENV) and all(k.startswith("split ") for k in rec), rec
    assert np.array_equal(got, want), (name, pn, diff(got, want))
    assert {k: st[k] for k in counts} == {k: model[k] for k in counts}, (name, pn)
    assert st["resumed"] + st["given_up"] == sum(st["voids"]) and (st["resumed"] >= 4 or not name.startswith("fuzz ")), st


# ---- the prefilter -----------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    for field, g, w in zip(("kmers_of", "row_off", "ids", "shared"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (what, field, g[:8], w[:8])


@pytest.mark.parametrize("k", [16, 21, 25])
@pytest.mark.parametrize("name", ["small", "split", "split N"])
def test_prefilter_of_repeat_sets(monkeypatch, name, k):
    """kmers_of, row_off, ids and shared against the numpy statement, whole and sampled: counted in the matrix and in the
    sparse table, in three passes, streamed with every genome a slice of its own (a genome, its exact copy and its reverse
    complement never share a slice), and in the cross form with the relatives as queries.  A k-mer repeated inside a
    genome, or present on both its strands, counts once (tests/test_repeats.py: the sets hold both)."""
    _env(monkeypatch, {})
    seqs = RG.repeat_set(name)
    n = len(seqs)
    lens = [len(s) for s in seqs]
    queries = [1, 2, 5, 7]                                                           # the relatives of the two families
    order = [g for g in range(n) if g not in queries] + queries
    cross, n_ref = [seqs[g] for g in order], n - len(queries)
    ns, _ = L.plan_slices(lens, max(lens))
    assert ns >= n - 2
    eng, xeng, streamer = L.Engine(), L.Engine(), L.Engine()
    try:
        eng.set_genomes(seqs)
        xeng.set_genomes(cross)
        for smax in (PM.SAMPLE_ALL, 1 << 62):
            kmers_of, shared = PM.shared_matrix(seqs, k, smax)
            xk, xs = PM.shared_matrix(cross, k, smax)
            assert int(np.triu(shared, 1).max()) > 0
            for min_shared, min_ratio in ((1, 0.0), (3, 0.05)):
                what = (name, k, smax, min_shared, min_ratio)
                want = (kmers_of.astype(np.uint32),) + PM.kept_pairs(kmers_of, shared, min_shared, min_ratio)
                for mode in ("dense", "sparse"):
                    eng.set_prefilter_counting(mode)
                    cnt = eng.prefilter(k, smax, min_shared, min_ratio)
                    _same(eng.prefilter_fetch(), want, what + (mode,))
                    assert cnt == len(want[2]) > 0 and eng.prefilter_sparse_info()["sparse"] == int(mode == "sparse")
                    assert eng.prefilter_info()["postings"] == int(kmers_of.sum())
                    monkeypatch.setenv("LZANI_PREFILTER_PASSES", "3")
                    eng.prefilter(k, smax, min_shared, min_ratio)
                    monkeypatch.delenv("LZANI_PREFILTER_PASSES")
                    _same(eng.prefilter_fetch(), want, what + (mode, "3 passes"))
                    assert eng.prefilter_pass_info()["passes"] == 3
                eng.set_prefilter_counting("auto")
                streamer.prefilter_codes(seqs, k, smax, min_shared, min_ratio, slice_bytes=max(lens))
                _same(streamer.prefilter_fetch(), want, what + ("streamed",))
                assert streamer.prefilter_stream_info()["slices"] == ns
                xwant = (xk.astype(np.uint32),) + XM.kept_pairs(xk, xs, n_ref, min_shared, min_ratio)
                cnt = xeng.prefilter_cross(k, n_ref, smax, min_shared, min_ratio)
                _same(xeng.prefilter_fetch(), xwant, what + ("cross",))
                assert cnt == len(xwant[2]) > 0
    finally:
        for e in (eng, xeng, streamer):
            e.close()
