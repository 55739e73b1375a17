"""GPU: every tuple of the edge table (U.EDGE_TUPLES) through every form of the device path it can reach, bit for bit
equal to the oracle (itself pinned to the reference build at these tuples by tests/test_envelope.py and
tests/golden/ref_envelope_vectors.json), each form checked through eng.layout() / eng.rtc_info() to have really run.

Forms: the default dispatch (ahead-of-time kernels: LZANI_RTC=0, what a cold run of a few pairs gets), dense rows by
candidate bitmaps, filtered rows by query lists, the block kernel, the split into segments, the alignment instantiation
(regions), and -- for tuples with k-mer words other than the two folded in ahead of time -- the run-time compiled
kernel, all of its code objects in one module-scoped cache directory.  Genomes with N (the edge set, the family set)
for every tuple, the N-free family set (the NFREE instantiations) for a subset."""
import json
import os

import numpy as np
import pytest

import lzani_ctypes as L
import oracle as O
import util as U

pytestmark = pytest.mark.gpu

# tuples that also run on the N-free family set: the chain's window bounds, the ChainP clamps, the hashed seed bitmap,
# mal < msl, the FAST limit, 32-symbol k-mers, a region length of zero
NFREE_ROWS = ("mqd0_mrd0", "mqd63_mrd65", "aw2_am1_ar0", "aw15_am20_ar0", "mal7_msl9", "mal15_msl8", "mal16_msl16",
              "mal32_msl7", "mal32_msl32", "reg0")
ROWS = dict(U.EDGE_TUPLES, **{"aot_" + k: v for k, v in U.AOT_SETS.items()})
SPLIT_SEGLEN = 1500
FORM_ENV = ("LZANI_RTC", "LZANI_RTC_MIN_PAIRS", "LZANI_PM_MIN_ROWS", "LZANI_BLOCK_KERNEL", "LZANI_SPLIT", "LZANI_SPLIT_SEGLEN",
            "LZANI_SPLIT_ALL", "LZANI_SPLIT_GIVE_UP", "LZANI_PM")


@pytest.fixture(scope="module")
def rtc_cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("rtc_cache"))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(U.GOLD, "ref_envelope_vectors.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def sets():
    return {"edge": U.edge_set(), "family": U.envelope_family_set(), "family N-free": U.envelope_family_set(with_n=False)}


def _diff(got, want):
    bad = np.argwhere((got != want).reshape(-1, 3).any(axis=1))
    return f"{len(bad)} pairs differ, first {bad[:3].ravel().tolist()}"


def _forms(eng, monkeypatch, seqs, prm, want, what):
    """Every form other than the run-time compiled kernel, on one context (eng), each against want = the oracle."""
    n = len(seqs)
    fast = U.is_fast(prm)
    form = U.index_form(seqs, prm)
    window_ok = prm["mqd"] + prm["mrd"] <= 128
    bitmaps_ok = fast and form["bucket_table"] and window_ok
    monkeypatch.setenv("LZANI_RTC", "0")
    # 1. the default dispatch
    got = eng.all2all()
    lay = eng.layout()
    assert np.array_equal(got, want), (what, "default", _diff(got, want))
    assert lay["kmer_words"] == fast and lay["bucket_table"] == form["bucket_table"] and lay["tag_words"] == form["tag_words"], (what, lay)
    assert lay["n_free"] == all((s < 4).all() for s in seqs) and lay["rtc_launches"] == 0, (what, lay)
    assert set(eng.kernel_launches()) == U.predict_kernels(seqs, prm, {"LZANI_RTC": "0"}), (what, "default", eng.kernel_launches())
    # 2. dense rows by candidate bitmaps (k-mer words, a bucket table and a seed window of up to 128 positions)
    monkeypatch.setenv("LZANI_PM_MIN_ROWS", "1")
    got = eng.all2all()
    lay = eng.layout()
    rec = eng.kernel_launches()
    monkeypatch.delenv("LZANI_PM_MIN_ROWS")
    assert set(rec) == U.predict_kernels(seqs, prm, {"LZANI_RTC": "0", "LZANI_PM_MIN_ROWS": "1"}), (what, "bitmaps", rec)
    assert np.array_equal(got, want), (what, "bitmaps", _diff(got, want))
    assert (lay["bitmap_launches"] >= 1) == bitmaps_ok, (what, "bitmaps", lay)
    # 3. filtered rows: a few queries per reference
    lists = [[(r + d) % n for d in (1, 2, 5) if (r + d) % n != r] for r in range(n)]
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    out = eng.run_rows(np.arange(n, dtype=np.uint32), off, np.array([q for x in lists for q in x], np.uint32))
    exp = np.concatenate([want[r, lists[r]] for r in range(n)])
    assert np.array_equal(out, exp), (what, "query lists", _diff(out, exp))
    # 4. the block kernel: rows of >= 128 pairs (every query many times), where the index has tag words
    lists = [[q for q in range(n) if q != r] * (128 // max(n - 1, 1) + 1) for r in range(n)]
    off[1:] = np.cumsum([len(x) for x in lists])
    monkeypatch.setenv("LZANI_BLOCK_KERNEL", "1")
    out = eng.run_rows(np.arange(n, dtype=np.uint32), off, np.array([q for x in lists for q in x], np.uint32))
    lay = eng.layout()
    rec = eng.kernel_launches()
    monkeypatch.delenv("LZANI_BLOCK_KERNEL")
    assert set(rec) == U.predict_kernels(seqs, prm, {"LZANI_RTC": "0", "LZANI_BLOCK_KERNEL": "1"}, "dup_lists", len(lists[0])), (what, "block kernel", rec)
    exp = np.concatenate([want[r, lists[r]] for r in range(n)])
    assert np.array_equal(out, exp), (what, "block kernel", _diff(out, exp))
    assert (lay["block_launches"] >= 1) == form["tag_words"], (what, "block kernel", lay)
    # 5. the split: every pair by segments of SPLIT_SEGLEN query positions (candidate bitmaps needed)
    if bitmaps_ok:
        for k, v in (("LZANI_PM_MIN_ROWS", "1"), ("LZANI_SPLIT", "1"), ("LZANI_SPLIT_SEGLEN", str(SPLIT_SEGLEN)), ("LZANI_SPLIT_ALL", "1")):
            monkeypatch.setenv(k, v)
        got = eng.all2all()
        lay = eng.layout()
        assert set(eng.kernel_launches()) == U.predict_kernels(seqs, prm, {"LZANI_RTC": "0", "LZANI_PM_MIN_ROWS": "1", "LZANI_SPLIT": "1", "LZANI_SPLIT_SEGLEN": str(SPLIT_SEGLEN)}), (what, "split")
        for k in ("LZANI_PM_MIN_ROWS", "LZANI_SPLIT", "LZANI_SPLIT_SEGLEN", "LZANI_SPLIT_ALL"):
            monkeypatch.delenv(k)
        assert np.array_equal(got, want), (what, "split", _diff(got, want))
        assert lay["split_launches"] >= 1 and lay["split_segments"] >= 2 * n * (n - 1), (what, "split", lay)
    # 6. the alignment instantiation: every region of every pair
    ref_ids, row_off = L.dense_rows(n)
    out, regs = eng.run_rows_regions(ref_ids, row_off, None)
    assert set(eng.kernel_launches()) == U.predict_kernels(seqs, prm, form="regions"), (what, "regions", eng.kernel_launches())
    assert np.array_equal(out.reshape(-1, 3), want[~np.eye(n, dtype=bool)]), (what, "regions: results")
    cols = ("ref_start", "ref_end", "seq_start", "seq_end", "num_matches", "num_mismatches")
    e = total = 0
    for r in range(n):
        for q in range(n):
            if q == r:
                continue
            mine = regs[regs["pair"] == e]
            got = np.stack([mine[c] for c in cols], axis=1) if len(mine) else np.zeros((0, 6), np.int32)
            _, oregs = O.oracle_pair(seqs[r], seqs[q], prm, want_regions=True)
            assert np.array_equal(got, oregs), (what, "regions", r, q, got[:3].tolist(), oregs[:3].tolist())
            total += len(oregs)
            e += 1
    assert total == len(regs), (what, "regions", total, len(regs))
    monkeypatch.delenv("LZANI_RTC")


def _rtc(monkeypatch, rtc_cache, seqs, prm, want, what):
    """The kernel compiled at run time for this tuple (dense rows; candidate bitmaps where the window allows them)."""
    monkeypatch.setenv("LZANI_RTC_MIN_PAIRS", "0")
    monkeypatch.setenv("LZANI_RTC_CACHE", rtc_cache)
    monkeypatch.setenv("LZANI_PM_MIN_ROWS", "1")
    eng = L.Engine(prm)
    try:
        eng.set_genomes(seqs)
        got = eng.all2all()
        lay, info, rec = eng.layout(), eng.rtc_info(), eng.kernel_launches()
    finally:
        eng.close()
        for k in ("LZANI_RTC_MIN_PAIRS", "LZANI_PM_MIN_ROWS"):
            monkeypatch.delenv(k)
    assert np.array_equal(got, want), (what, "run-time compiled", _diff(got, want))
    assert lay["rtc_launches"] >= 1 and info["kernels_failed"] == 0 and info["kernels_built"] >= 1, (what, lay, info)
    assert info["folded_ahead_of_time"] == 0 and info["null_chain"] == U.chain_params_ok(prm), (what, info)
    assert set(rec) == U.predict_kernels(seqs, prm, {"LZANI_PM_MIN_ROWS": "1"}, rtc_ready=True), (what, "run-time compiled", rec)


@pytest.mark.parametrize("name", list(ROWS))
def test_edge_tuple_every_form(monkeypatch, rtc_cache, golden, sets, name):
    for k in FORM_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LZANI_RTC_CACHE", rtc_cache)
    prm = ROWS[name]
    for setname, seqs in sets.items():
        if setname == "family N-free" and name not in NFREE_ROWS:
            continue
        what = (name, setname)
        want = O.oracle_all2all(seqs, prm, threads=16)
        ref = golden["res"].get(setname, {}).get(name)
        if ref is not None:                                # the reference build's own answer where one is stored
            assert np.array_equal(want, np.array(ref, dtype=np.int32)), what
        eng = L.Engine(prm)
        try:
            eng.set_genomes(seqs)
            _forms(eng, monkeypatch, seqs, prm, want, what)
            info = eng.rtc_info()
        finally:
            eng.close()
        assert info["folded_ahead_of_time"] == U.is_aot(prm) and info["kernels_built"] == 0, (what, info)
        if U.is_fast(prm) and not U.is_aot(prm) and setname != "edge":
            _rtc(monkeypatch, rtc_cache, seqs, prm, want, what)


def test_nfree_rows_cover_both_instantiations():
    assert set(NFREE_ROWS) <= set(U.EDGE_TUPLES)
    assert any(U.is_fast(U.EDGE_TUPLES[k]) for k in NFREE_ROWS) and any(not U.is_fast(U.EDGE_TUPLES[k]) for k in NFREE_ROWS)
    assert any(U.chain_params_ok(U.EDGE_TUPLES[k]) for k in NFREE_ROWS)


def test_params_refusal_edge_through_the_engine():
    """One step inside every bound of params_supported the engine runs (equal to the oracle), one step outside
    lzani_create refuses with LZANI_ERR_PARAMS."""
    seqs = [U.edge_set()[0][:300], U.edge_set()[2][:200], U.edge_set()[3][1450:1650]]
    for knob, ok, bad in U.ENVELOPE_BOUNDS:
        inside, outside = U.bound_pair(knob, ok, bad)
        eng = L.Engine(inside)
        try:
            eng.set_genomes(seqs)
            got = eng.all2all()
        finally:
            eng.close()
        assert np.array_equal(got, O.oracle_all2all(seqs, inside, threads=4)), (knob, ok)
        with pytest.raises(L.LzaniError, match="LZANI_ERR_PARAMS"):
            L.Engine(outside)
