"""GPU: the structures that decide which query positions the pair kernel looks up at all -- the anchor index of every
reference slot (directory, entries, bucket table, tag words), its presence filter, and the candidate bitmaps and counts
of the candidate stage -- against host statements made from the raw sequences (tests/index_model.py).  Every case also
checks the run's triples against the oracle, so the structures checked are those of a correct run; and every case asserts
from the engine's own report that the planned form really ran (build path, matrix from the index, hashed rows, group size,
batches).  Out of scope: the join form's per-wave bitmaps and the split path's segments (the split's buffers, which the
candidate scratch keeps between batches and runs, have one test at the end)."""
import numpy as np
import pytest

import index_model as IM
import lzani_ctypes as L
import oracle as O
import synth_genomes as SG
import util as U

pytestmark = pytest.mark.gpu

_SETS = {}


def _rand(st, n, alphabet=4):
    return (st.u64(n) % np.uint64(alphabet)).astype(np.uint8)


def _set(name):
    """Genome sets, made once per session."""
    if name in _SETS:
        return _SETS[name]
    st = SG.Stream(9090)
    if name == "viral":          # viral sizes with N runs, a genome shorter than mal, bitmap tile edges (L + 40 + 320 = 3072 +- 1)
        seqs = U._put_n_runs(SG.make_set(12, 611, lmin=3000, lmax=9000, fam=4)[1])
        seqs += [_rand(st, 7), _rand(st, 2711), _rand(st, 2712), _rand(st, 2713), np.full(500, 4, np.uint8)]
    elif name == "mixed":        # + a 66 kbp poly-A (one k-mer 65,990 times), a tandem repeat, a 30 kbp low-complexity stretch
        seqs = U._put_n_runs(SG.make_set(10, 612, lmin=20000, lmax=60000, fam=5)[1])
        unit = _rand(st, 97)
        lowc = _rand(st, 40000)
        lowc[5000:35000] = _rand(st, 30000, 2) * 3            # A/T only
        seqs += [np.zeros(66000, np.uint8), np.tile(unit, 320), lowc, _rand(st, 9)]
    elif name == "small":        # edge tuples: short genomes with N runs
        seqs = U._put_n_runs(SG.make_set(9, 613, lmin=2300, lmax=3000, fam=3)[1]) + [_rand(st, 3)]
    elif name == "hashed":       # mal 15 on 20-70 kbp: a matrix of fewer rows than k-mers
        seqs = SG.make_set(10, 614, lmin=20000, lmax=70000, fam=5)[1]
    elif name == "three":        # the index hooks, the timing and the event tests: random, no N
        seqs = [_rand(st, 300), _rand(st, 2000), _rand(st, 9000)]
    elif name == "tiny530":      # 530 genomes of 250-600 bp (mal 9: exact matrix made from the index, groups of 512)
        base = SG.make_set(530, 615, lmin=250, lmax=600, fam=10)[1]
        seqs = [s.copy() for s in base]
        for k in range(0, 530, 37):
            seqs[k][len(seqs[k]) // 3:len(seqs[k]) // 3 + 5] = 4
    else:
        raise KeyError(name)
    _SETS[name] = [np.ascontiguousarray(s) for s in seqs]
    return _SETS[name]


_ORACLE = {}


def _oracle(name, prm):
    key = (name, tuple(sorted((prm or {}).items())))
    if key not in _ORACLE:
        _ORACLE[key] = O.oracle_all2all(_set(name), prm, threads=16)
    return _ORACLE[key]


def _engine(monkeypatch, env, prm, seqs):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = L.Engine(prm)
    eng.set_genomes(seqs)
    return eng


# ---- index slabs -----------------------------------------------------------------------------------------------------

def _check_slabs(eng, seqs, prm, ref_ids, with_filter=True, with_tw=True):
    s = eng.debug_index_slab(ref_ids, with_filter, with_tw)
    geo = dict(key_bits=s["key_bits"], dir_bits=s["dir_bits"], pos_bits=s["pos_bits"], tag_mask=s["tag_mask"])
    for slot, g in enumerate(ref_ids):
        IM.check_index_slot(seqs[g], prm["mrd"], prm["mal"], geo, s["dirz"][slot], s["ent"][slot],
                            None if s["bk"] is None else s["bk"][slot], None if s["tw"] is None else s["tw"][slot],
                            None if s["fl"] is None else s["fl"][slot], s["filter_mask"], what=f"slot {slot} (genome {g}, {s['build']})")
    return s


INDEX_CASES = {
    # name: (set, params, environment, build expected, forms expected (bk, tw, fl))
    "lds_viral": ("viral", None, {}, "lds", (True, True, True)),
    "lds_fallback": ("mixed", None, {}, "lds", (True, True, True)),
    "atomics": ("mixed", None, {"LZANI_NO_LDS_INDEX": "1"}, "atomics", (True, True, True)),
    "sort": ("mixed", None, {"LZANI_SORT_INDEX_MIN_DIRBITS": "0"}, "sort", (True, True, True)),
    "sort_viral": ("viral", None, {"LZANI_SORT_INDEX_MIN_DIRBITS": "0"}, "sort", (True, True, True)),
    "buckets_only": ("viral", None, {"LZANI_NO_TAGWORDS": "1"}, "lds", (True, False, False)),
    "directory_only": ("viral", None, {"LZANI_NO_BUCKETS": "1"}, "lds", (False, False, False)),
    "atomics_directory_only": ("small", None, {"LZANI_NO_BUCKETS": "1", "LZANI_NO_LDS_INDEX": "1"}, "atomics", (False, False, False)),
    # k-mer words from the edge tuples (forms None: whatever the geometry gives, util.index_form)
    "mal1_msl1": ("small", "mal1_msl1", {}, "lds", None),
    "mal9_msl9": ("small", "mal9_msl9", {}, "lds", None),
    "mal15_msl8": ("small", "mal15_msl8", {}, "lds", None),
    "mal16_msl16": ("small", "mal16_msl16", {}, "atomics", (False, False, False)),       # no k-mer words beyond 15
    "mal32_msl11": ("small", "mal32_msl11", {}, "atomics", (False, False, False)),
    "mqd0_mrd0": ("small", "mqd0_mrd0", {}, "lds", None),
}


@pytest.mark.parametrize("case", list(INDEX_CASES))
def test_index_slabs_match_statement(monkeypatch, case):
    name, tup, env, build, forms = INDEX_CASES[case]
    seqs = _set(name)
    prm = U.full_params(None if tup is None else U.EDGE_TUPLES[tup])
    eng = _engine(monkeypatch, env, prm, seqs)
    n = len(seqs)
    # several slots a batch, references repeated, in no particular order
    ref_ids = np.array(list(range(n - 1, -1, -1)) + [0, n - 1, n // 2], np.uint32)
    s = _check_slabs(eng, seqs, prm, ref_ids)
    assert s["build"] == build, s["build"]
    if forms is None:
        f = U.index_form(seqs, prm)
        forms = (f["bucket_table"], f["tag_words"], f["tag_words"])
    assert (s["bk"] is not None, s["tw"] is not None, s["fl"] is not None) == forms
    if build == "lds":
        polya = [k for k, g in enumerate(ref_ids) if len(seqs[g]) >= 65536 and not seqs[g].any()]
        assert set(np.nonzero(s["status"])[0].tolist()) == set(polya), s["status"]
        if name == "mixed":
            assert polya, "the poly-A slot must fall back"
    if build == "sort":
        assert s["ent_stride"] % 8192 != 0
        t = _check_slabs(eng, seqs, prm, ref_ids[:4], with_filter=False, with_tw=False)
        assert t["tw"] is None and t["fl"] is None and t["bk"] is not None
    got = eng.all2all()
    eng.close()
    assert np.array_equal(got, _oracle(name, None if tup is None else U.EDGE_TUPLES[tup]))


def _buckets_equal(dirz, ent_a, ent_b, what):
    """Two entry arrays of one directory, bucket by bucket: exactly where a bucket has at most 32 entries (the builds sort
    those), as sorted arrays beyond (fill order).  Returns the share of buckets beyond 32."""
    cnt = np.diff(dirz.astype(np.int64))
    bucket = np.repeat(np.arange(len(cnt)), cnt)
    small = cnt[bucket] <= 32
    assert np.array_equal(ent_a[small], ent_b[small]), f"{what}: entries of sorted buckets differ"
    assert np.array_equal(ent_a[np.lexsort((ent_a, bucket))], ent_b[np.lexsort((ent_b, bucket))]), f"{what}: large buckets differ"
    return float((cnt > 32).mean())


@pytest.mark.parametrize("build, env", [("lds", {}), ("atomics", {"LZANI_NO_LDS_INDEX": "1"}), ("sort", {"LZANI_SORT_INDEX_MIN_DIRBITS": "0"})])
def test_the_two_index_hooks_agree(monkeypatch, build, env):
    """lzani_debug_get_index is the one-row case of lzani_debug_index_slab: for every genome, geometry, directory, entry
    count and entries equal slot 0 of the slab of that one reference, on each of the three index builds."""
    seqs = _set("three")
    eng = _engine(monkeypatch, env, None, seqs)          # (the sort switch is read by set_genomes)
    for g in range(len(seqs)):
        a = eng.debug_index(g)
        s = eng.debug_index_slab([g])
        assert s["build"] == build, s["build"]
        assert a["geom"].tolist() == [s["key_bits"], s["dir_bits"], s["pos_bits"], s["tag_mask"]]
        assert np.array_equal(a["dirz"], s["dirz"][0])
        n_ent = int(a["dirz"][-1])
        assert n_ent == len(a["ent"]) == int(s["dirz"][0][-1]) and n_ent > 0
        large = _buckets_equal(a["dirz"], a["ent"], s["ent"][0][:n_ent], f"genome {g}, {build}")
        assert large < 0.01, large                       # (the exact comparison is what runs)
    eng.close()


def test_kmer_words_are_timed_once_per_genome_set(monkeypatch):
    """kmers_ms: the first run after set_genomes makes the k-mer words and reports their time, the second finds them; a
    new set_genomes starts over.  (tests/test_gpu_parity.py prints kmers_ms and asserts nothing about it.)"""
    seqs = _set("three")
    eng = _engine(monkeypatch, {}, None, seqs)
    first = eng.all2all()
    assert eng.timing()["kmers_ms"] > 0
    second = eng.all2all()
    assert eng.timing()["kmers_ms"] == 0
    assert np.array_equal(first, second) and np.array_equal(first, _oracle("three", None))
    eng.set_genomes(seqs)
    third = eng.all2all()
    assert eng.timing()["kmers_ms"] > 0
    assert np.array_equal(third, first)
    eng.close()


def test_batch_events_grow_and_are_used_again(monkeypatch):
    """The context's per-batch events: a run of three batches (LZANI_MAX_SLOTS=1: a slab slot, so a row a batch) makes them,
    a run of one batch on the same context uses the first of them again, close() releases them."""
    seqs = _set("three")
    eng = _engine(monkeypatch, {"LZANI_MAX_SLOTS": "1"}, None, seqs)
    got = eng.all2all()
    assert eng.layout()["batches_last_run"] == len(seqs) and eng.layout()["slots"] == 1
    assert np.array_equal(got, _oracle("three", None))
    monkeypatch.delenv("LZANI_MAX_SLOTS")
    eng.set_genomes(seqs)
    got = eng.all2all()
    assert eng.layout()["batches_last_run"] == 1 and eng.layout()["slots"] == len(seqs)
    assert np.array_equal(got, _oracle("three", None))
    eng.close()


# ---- candidate bitmaps -----------------------------------------------------------------------------------------------

def _pairs(n, ref_ids, row_off, query_ids):
    pair_ref = np.repeat(np.asarray(ref_ids, np.int64), np.diff(np.asarray(row_off, np.int64)))
    if query_ids is None:
        pair_qry = np.concatenate([np.delete(np.arange(n), r) for r in ref_ids]) if len(ref_ids) else np.zeros(0, np.int64)
    else:
        pair_qry = np.asarray(query_ids, np.int64)
    return pair_ref, pair_qry


def _check_candidates(eng, seqs, prm, ref_ids, row_off, query_ids, want, plain_pairs=48):
    """Run the rows with the candidate capture; triples against `want` (oracle [n, n, 3]); every pair's bitmap over the
    words k_pm_cand writes against the statement; counts against the bitmaps' popcounts.  Returns the plan."""
    n = len(seqs)
    got, cb, pc, plan = eng.debug_run_candidates(ref_ids, row_off, query_ids)
    pair_ref, pair_qry = _pairs(n, ref_ids, row_off, query_ids)
    assert np.array_equal(got, want[pair_ref, pair_qry]), "triples differ from the oracle"
    if not plan["pm"]:
        return plan
    words = cb.shape[1]
    assert plan["cb_words"] <= words
    exp = IM.expected_bitmaps(seqs, prm["mrd"], prm["mal"], plan["rshift"], plan["pm_bits"], pair_ref, pair_qry, words)
    lens = np.array([len(s) for s in seqs])
    nw = (lens[pair_qry] + prm["mrd"] + 320 + 1023) // 1024 * 32
    mask = np.arange(words)[None, :] < nw[:, None]
    bad = np.argwhere((cb != exp) & mask)
    if len(bad):
        e, w = bad[0]
        raise AssertionError(f"{len(bad)} bitmap words differ; first: pair {e} (ref {pair_ref[e]}, query {pair_qry[e]}, "
                             f"L_q {lens[pair_qry[e]]}) word {w}: {cb[e, w]:#010x} != {exp[e, w]:#010x}; plan {plan}")
    if plan["rshift"] == 0:           # the exact matrix, restated without the hash
        for e in np.linspace(0, len(pair_ref) - 1, min(plain_pairs, len(pair_ref))).astype(int):
            r, q = pair_ref[e], pair_qry[e]
            assert np.array_equal(IM.plain_bitmap(seqs[r], seqs[q], prm["mrd"], prm["mal"], words)[:nw[e]], cb[e, :nw[e]]), (e, r, q)
    counted = pc != 0xFFFFFFFF
    if counted.any():
        assert np.array_equal(pc[counted], IM.popcounts(exp[counted])), "candidate counts differ from the bitmaps"
    return plan


def _dense(ref_ids, n):
    ref_ids = np.asarray(ref_ids, np.uint32)
    return ref_ids, np.arange(len(ref_ids) + 1, dtype=np.uint64) * np.uint64(n - 1)


def test_dense_exact_matrix_tile_edges_and_batches(monkeypatch):
    """Exact matrix (rshift 0) by k_pm_build on viral sizes with N runs; queries whose L + mrd + 320 is one below, at and
    one above a tile edge; then the same rows in batches of 8 (e0 != 0) with counted candidates."""
    seqs = _set("viral")
    prm = U.full_params(None)
    n = len(seqs)
    eng = _engine(monkeypatch, {"LZANI_PM_MIN_ROWS": "1"}, prm, seqs)
    want = _oracle("viral", None)
    plan = _check_candidates(eng, seqs, prm, *_dense(np.arange(n)[::-1], n), None, want)
    assert plan["pm"] and plan["rshift"] == 0 and plan["from_index_launches"] == 0 and plan["batches"] == 1, plan
    eng.close()
    eng = _engine(monkeypatch, {"LZANI_PM_MIN_ROWS": "1", "LZANI_MAX_SLOTS": "8", "LZANI_LPT": "1", "LZANI_SPLIT": "0"}, prm, seqs)
    plan = _check_candidates(eng, seqs, prm, *_dense(np.arange(n), n), None, want)
    assert plan["pm"] and plan["batches"] >= 3 and plan["counted_batches"] == plan["batches"], plan
    eng.close()


def test_dense_hashed_matrix(monkeypatch):
    """mal 15 on 20-70 kbp: 2^27 matrix rows for 2^30 k-mers (rshift 3), k_pm_build."""
    seqs = _set("hashed")
    prm = U.full_params(dict(mal=15, msl=9, reg=60))
    eng = _engine(monkeypatch, {"LZANI_PM_MIN_ROWS": "1", "LZANI_LPT": "1"}, prm, seqs)
    plan = _check_candidates(eng, seqs, prm, *_dense(np.arange(len(seqs)), len(seqs)), None, _oracle("hashed", dict(mal=15, msl=9, reg=60)))
    assert plan["pm"] and plan["rshift"] > 0 and plan["pm_group"] == 512 and plan["from_index_launches"] == 0, plan
    assert plan["counted_batches"] >= 1, plan
    eng.close()


@pytest.mark.parametrize("rows", [128, 129, 257, 385, 530])
def test_matrix_from_index_every_width(monkeypatch, rows):
    """k_pm_from_index<4|8|12|16> (1-128, 129-256, 257-384, 385-512 slots a group) and two groups (530 rows: 512 + 18),
    every slot at the word edges 31/32 and 127/128 included; exact matrix, mal 9."""
    seqs = _set("tiny530")
    prm = U.full_params(dict(mal=9))
    n = len(seqs)
    eng = _engine(monkeypatch, {"LZANI_PM_MIN_ROWS": "1", "LZANI_PM_FROM_INDEX": "1"}, prm, seqs)
    ref_ids = (np.arange(rows) * 7 + 3) % n if rows < n else np.arange(rows)
    plan = _check_candidates(eng, seqs, prm, *_dense(ref_ids, n), None, _oracle("tiny530", dict(mal=9)), plain_pairs=16)
    groups = (rows + 511) // 512
    assert plan["pm"] and plan["rshift"] == 0 and plan["pm_group"] == 512 and plan["batches"] == 1, plan
    assert plan["from_index_launches"] == groups and plan["cand_launches"] == groups, plan
    eng.close()


def test_query_lists_several_groups(monkeypatch):
    """Rows with query lists over two groups: unsorted lists, empty rows, queries in both groups (k_pm_pairs, qlist)."""
    seqs = _set("tiny530")
    prm = U.full_params(dict(mal=9))
    n = len(seqs)
    st = SG.Stream(777)
    ref_ids, lists = [], []
    for k in range(560):
        r = k % n
        cnt = 0 if k % 9 == 4 else st.randint(1, 40)
        q = np.unique((st.u64(cnt) % np.uint64(n)).astype(np.int64))
        q = q[q != r]
        q = q[np.argsort(st.u64(len(q)))]               # unsorted
        ref_ids.append(r)
        lists.append(q)
    row_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    qids = np.concatenate(lists).astype(np.uint32)
    in0, in1 = set(np.concatenate(lists[:512]).tolist()), set(np.concatenate(lists[512:]).tolist())
    assert in0 & in1
    eng = _engine(monkeypatch, {"LZANI_PM_MIN_ROWS": "1", "LZANI_PM_MIN_SHARE": "1"}, prm, seqs)
    plan = _check_candidates(eng, seqs, prm, np.array(ref_ids, np.uint32), row_off, qids, _oracle("tiny530", dict(mal=9)), plain_pairs=16)
    assert plan["pm"] and plan["cand_launches"] == 2, plan
    eng.close()


def test_pm_group_128(monkeypatch):
    """pm_bits 28 > 27: groups of 128 slots (16-byte matrix rows); mal 15 on 200 kbp (texts of 2^18 .. 2^19 positions:
    a bucket table still fits tag and position in 30 bits); counted candidates."""
    st = SG.Stream(31337)
    a = _rand(st, 200000)
    seqs = [a, SG.mutate(a, 0.03, st), _rand(st, 198000), _rand(st, 20000)]
    seqs = [np.ascontiguousarray(s) for s in seqs]
    prm = U.full_params(dict(mal=15, msl=9, reg=60))
    want = O.oracle_all2all(seqs, dict(mal=15, msl=9, reg=60), threads=16)
    eng = _engine(monkeypatch, {"LZANI_PM_MIN_ROWS": "1", "LZANI_LPT": "1", "LZANI_SPLIT": "0"}, prm, seqs)
    plan = _check_candidates(eng, seqs, prm, *_dense(np.arange(4), 4), None, want)
    assert plan["pm"] and plan["pm_bits"] == 28 and plan["pm_group"] == 128 and plan["rshift"] == 2, plan
    assert plan["counted_batches"] == plan["batches"], plan
    eng.close()


def test_fail_cbits_falls_back(monkeypatch):
    """LZANI_PM_FAIL_CBITS=1: the bitmaps cannot be had; the run reports pm off and computes the same triples."""
    seqs = _set("viral")
    prm = U.full_params(None)
    eng = _engine(monkeypatch, {"LZANI_PM_MIN_ROWS": "1", "LZANI_PM_FAIL_CBITS": "1"}, prm, seqs)
    plan = _check_candidates(eng, seqs, prm, *_dense(np.arange(len(seqs)), len(seqs)), None, _oracle("viral", None))
    assert not plan["pm"] and plan["cand_launches"] == 0, plan
    eng.close()


def test_more_than_32768_queries_in_one_group(monkeypatch):
    """One group whose queries do not fit one launch (gridDim.y): 33,000 genomes of 40-70 bp, two dense rows."""
    st = SG.Stream(2024)
    n = 33000
    lens = 40 + (st.u64(n) % np.uint64(31)).astype(np.int64)
    flat = _rand(st, int(lens.sum()))
    seqs = [np.ascontiguousarray(x) for x in np.split(flat, np.cumsum(lens)[:-1])]
    seqs[5] = seqs[1].copy()                                    # a related pair or two
    seqs[32900] = seqs[0].copy()
    prm = U.full_params(None)
    eng = _engine(monkeypatch, {"LZANI_PM_MIN_ROWS": "1"}, prm, seqs)
    ref_ids = np.array([1, 0], np.uint32)
    pair_ref, pair_qry = _pairs(n, ref_ids, _dense(ref_ids, n)[1], None)
    got, cb, pc, plan = eng.debug_run_candidates(*_dense(ref_ids, n))
    eng.close()
    assert plan["pm"] and plan["cand_launches"] == 2, plan
    oracle = np.array([O.oracle_pair(seqs[r], seqs[q], None) for r, q in zip(pair_ref, pair_qry)], np.int32).reshape(-1, 3)
    assert np.array_equal(got, oracle)
    exp = IM.expected_bitmaps(seqs, prm["mrd"], prm["mal"], plan["rshift"], plan["pm_bits"], pair_ref, pair_qry, cb.shape[1])
    assert np.array_equal(cb, exp)                              # every query's bitmap is one tile: all words written


# ---- the split's buffers in the candidate scratch --------------------------------------------------------------------

def test_split_buffers_survive_batches_and_runs(monkeypatch):
    """The split path's buffers live in the context's candidate scratch: two batches of one run share them, a batch of
    more segments and a larger batch grow them, a smaller batch reuses them -- every run equal to the same rows without
    the split and to the oracle.  16 related genomes of 4-6 kbp, N runs in four; 8 index slots (the fewest the bitmap plan
    takes for 16 rows) make two batches of 8 rows = 120 pairs, every pair cut into 3-5 segments of 1,500 positions.
    LZANI_MAX_SLOTS is read when the genomes are set, so run (b) sets them again on the same engine: the scratch goes with
    the set and is made anew, larger; the growth in place is the run with segments of 700 positions before it."""
    seqs = [np.ascontiguousarray(s) for s in U._put_n_runs(SG.make_set(16, 616, lmin=4000, lmax=6000, fam=4)[1])]
    n = len(seqs)
    env = {"LZANI_PM_MIN_ROWS": "1", "LZANI_MAX_SLOTS": "8", "LZANI_SPLIT": "1", "LZANI_SPLIT_SEGLEN": "1500", "LZANI_SPLIT_ALL": "1",
           "LZANI_RTC": "0"}
    # the shape, before the GPU is asked: candidate bitmaps and the split for a batch of 8 rows, two such batches
    names = {"split nfree=0 defp=1 mode=0", "split nfree=0 defp=1 mode=1"}
    assert U.predict_kernels(seqs, None, env, n_rows=8) == names and U.predict_kernels(seqs, None, env, n_rows=4) == names
    assert n == 16 and -(-n // int(env["LZANI_MAX_SLOTS"])) == 2
    assert all(3 <= -(-(len(s) + 40) // 1500) <= 5 for s in seqs)
    want = O.oracle_all2all(seqs, None, threads=16)
    eng = _engine(monkeypatch, env, None, seqs)

    def check(got, batches, min_segments):
        lay = eng.layout()
        assert lay["batches_last_run"] == batches and lay["split_launches"] == batches and lay["bitmap_launches"] == batches, lay
        assert lay["split_segments"] >= min_segments, lay
        assert set(eng.kernel_launches()) == names
        assert np.array_equal(got, base) and np.array_equal(got, want)

    monkeypatch.setenv("LZANI_SPLIT", "0")
    base = eng.all2all()
    lay = eng.layout()
    assert lay["batches_last_run"] == 2 and lay["split_launches"] == 0 and lay["bitmap_launches"] == 2, lay
    monkeypatch.setenv("LZANI_SPLIT", "1")
    check(eng.all2all(), 2, 2 * 240)                        # (a) two batches: the second finds the first one's buffers
    monkeypatch.setenv("LZANI_SPLIT_SEGLEN", "700")
    check(eng.all2all(), 2, 2 * 120 * 6)                    # more segments a pair: the segment buffers grow in place
    monkeypatch.setenv("LZANI_SPLIT_SEGLEN", "1500")
    monkeypatch.delenv("LZANI_MAX_SLOTS")
    eng.set_genomes(seqs)
    check(eng.all2all(), 1, 240 * 3)                        # (b) one batch of 240 pairs
    ref_ids, row_off = _dense(np.arange(4), n)
    pair_ref, pair_qry = _pairs(n, ref_ids, row_off, None)
    base, want = base[pair_ref, pair_qry], want[pair_ref, pair_qry]
    check(eng.run_rows(ref_ids, row_off), 1, 60 * 3)        # (c) rows 0 .. 3: a smaller batch in the same buffers
    eng.close()
