"""GPU: every change of run form and genome set on one warm context (tests/context_walk.py; tests/test_context_walk.py checks
the walk on the CPU).

The cells of tests/test_gpu_instantiations.py each start from a cold context; the product does not run cold.  Here a context
goes through a segment of its tuple's circuit -- every ordered pair of the tuple's nodes (the cells, the run-time compiled
cells' ahead-of-time twins, two out-of-core runs) is crossed exactly once over the segments -- with a lzani_set_genomes only
where the node's set, set-level switches or genome-memory limit differ from the step before.  Every step asserts what the
cell asserts cold (tests/inst_cell.py: call_and_check): the launch record, results bit-equal to the oracle, the regions, the
run-time compile's info, and the blocks of lzani_get_residency; a form that read what the form before it left behind, or that
the context's earlier life led elsewhere, fails at its step, and the message names the edge.

The second test takes the stage results -- prefilter, kept pairs, clusters -- through runs of three forms and a
lzani_set_genomes: they outlive the runs unchanged and are dropped with the genome set."""
import time

import numpy as np
import pytest

import context_walk as W
import lzani_ctypes as L
import out_filter_model as FM
import prefilter_limit_model as LM
import prefilter_model as PM
import util as U
from inst_cell import apply_env, call_and_check, diff, oracle_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rtc_cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("rtc_cache"))


@pytest.mark.parametrize("prm,s", W.segment_ids(), ids=["%s-%d" % x for x in W.segment_ids()])
def test_walk_segment(monkeypatch, rtc_cache, prm, s):
    """One segment on one context; a step that fails ends it."""
    seg = W.segments(prm)[s]
    t0 = time.time()
    for setname in sorted({x["set"] for x in seg}):
        oracle_of(setname, prm)                               # (made once for all tests of the process: not the segment's time)
    t1 = time.time()
    uploads, pairs, prev = 0, 0, None
    eng = L.Engine(U.INST_PARAMS[prm])
    try:
        for step, node in enumerate(seg):
            fresh = prev is None or W.set_key(prev) != W.set_key(node)
            where = "%s segment %d step %d: %s -> %s, %s" % (prm, s, step, prev["id"] if prev else "(new context)", node["id"],
                                                           "lzani_set_genomes between" if fresh else "on the same upload")
            apply_env(monkeypatch, rtc_cache, node)
            seqs = U.instantiation_set(node["set"])
            try:
                if fresh:
                    eng.set_genome_memory(node["limit"])
                    eng.set_genomes(seqs)
                    uploads += 1
                pairs += call_and_check(eng, node, seqs, oracle_of(node["set"], prm), where)
            except L.LzaniError as e:
                raise AssertionError((where, str(e))) from e
            prev = node
    finally:
        eng.close()
    print(f"walk {prm} segment {s}: {len(seg)} steps ({len(seg) - 1} edges), {uploads} uploads, {pairs} pairs, "
          f"{time.time() - t1:.2f} s (oracles {t1 - t0:.2f} s)")


def _same_csr(got, want, what):
    for name, g, w in zip(("kmers_of", "row_off", "ids", "shared"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name, g[:8], w[:8])


def _dense(eng, form_env, monkeypatch, rtc_cache, seqs, prm, want, what):
    """A dense run under the switches form_env: bit-equal to the oracle, by the kernels util.predict_kernels names."""
    env = dict(form_env, LZANI_RTC="0")
    apply_env(monkeypatch, rtc_cache, dict(env=env))
    got = eng.all2all()
    rec = eng.kernel_launches()
    assert set(rec) == U.predict_kernels(seqs, prm, env, "all2all"), (what, rec)
    assert np.array_equal(got, want), (what, diff(got, want))
    return rec


def test_stage_results_between_runs_and_across_a_set(monkeypatch, rtc_cache):
    """Defaults, the set 'small': the prefilter's result, the kept pairs and the clusters stay what they were while runs in
    the bitmap, probe and split forms go by, and lzani_set_genomes drops all three."""
    prm = U.INST_PARAMS["defaults"]
    seqs, want = U.instantiation_set("small"), oracle_of("small", "defaults")
    n, lens = len(seqs), np.array([len(s) for s in seqs], dtype=np.uint32)
    k = 16
    kmers_of, shared = PM.shared_matrix(seqs, k)
    f_want = (kmers_of.astype(np.uint32),) + PM.kept_pairs(kmers_of, shared, 1, 0.0)
    apply_env(monkeypatch, rtc_cache, dict(env={"LZANI_RTC": "0"}))
    eng = L.Engine(prm)
    try:
        eng.set_genomes(seqs)
        # 1. the prefilter
        assert eng.prefilter(k) == len(f_want[2]) >= 6
        f0 = eng.prefilter_fetch()
        _same_csr(f0, f_want, "step 1: prefilter")
        # 2. a dense run by candidate bitmaps
        rec = _dense(eng, U._INST_FORM_ENV["bitmaps"], monkeypatch, rtc_cache, seqs, prm, want, "step 2: bitmap form")
        assert all("cand=2" in x for x in rec), rec
        _same_csr(eng.prefilter_fetch(), f0, "step 2: the prefilter's result after a bitmap run")
        # 3. the kept pairs of the prefilter's lists, both directions of every pair; an empty edge set takes them
        ref, off, q = L.cross_rows(n, 0, f0[1], f0[2])
        flt = dict(ani=0.8)
        k_want = FM.kept(flt, n, lens, ref, off, q, want[FM.entries_of(n, ref, off, q)])[0]
        assert 0 < len(k_want) < len(f0[2])                                         # (by the model alone: the filter keeps and drops)
        k0 = eng.run_rows_kept(ref, off, q, flt)
        assert k0.dtype == L.KEPT_DTYPE and k0.tobytes() == k_want.astype(L.KEPT_DTYPE).tobytes(), ("step 3: kept pairs", k0[:3], k_want[:3])
        eng.cluster_begin()
        assert eng.cluster_add_kept() == len(k0)
        # 4. query lists in the probe form; then the three results
        node = next(c for c in U.INST_CELLS if c["prm"] == "defaults" and c["set"] == "small" and c["form"] == "lists" and
                    c["env"].get("LZANI_PM") == "0" and len(c["env"]) == 2)
        assert node["name"] == U.PAIRS_NAME.format(1, 1, 1, 0, 1, 0)
        apply_env(monkeypatch, rtc_cache, node)
        call_and_check(eng, node, seqs, want, "step 4: probe form after bitmaps and a kept run")
        l_want = (f0[0],) + LM.apply(f0[1], f0[2], f0[3], LM.limit(n, 0, *f0, 2))
        assert eng.prefilter_limit(2) == len(l_want[2])
        _same_csr(eng.prefilter_fetch(), l_want, "step 4: the prefilter's result limited to 2 a genome")
        again = eng.kept_fetch(0, len(k0))
        assert again.tobytes() == k0.tobytes(), "step 4: the kept pairs after a lists run"
        w = [L.cluster_weight("tani", r["x"], r["y"], r["lines"], lens[r["a"]], lens[r["b"]]) for r in k0]
        rep, cl, clusters = L.cluster_host(n, L.cluster_edges(k0["a"], k0["b"], w), "single")
        assert 1 < clusters < n                                                     # (by the host statement alone)
        assert eng.cluster_run("single") == clusters
        c0 = eng.cluster_fetch()
        assert np.array_equal(c0[0], rep) and np.array_equal(c0[1], cl), ("step 4: clusters", c0, rep, cl)
        # 5. a split run
        rec = _dense(eng, U._INST_FORM_ENV["split"], monkeypatch, rtc_cache, seqs, prm, want, "step 5: split form")
        assert len(rec) == 2 and all(x.startswith("split ") for x in rec), rec
        c1 = eng.cluster_fetch()
        assert np.array_equal(c1[0], c0[0]) and np.array_equal(c1[1], c0[1]), "step 5: the clusters after a split run"
        assert eng.kept_fetch(0, len(k0)).tobytes() == k0.tobytes(), "step 5: the kept pairs after a split run"
        _same_csr(eng.prefilter_fetch(), l_want, "step 5: the prefilter's result after a split run")
        l1_want = (f0[0],) + LM.apply(*l_want[1:], LM.limit(n, 0, *l_want, 1))        # (2 a genome cuts nothing of this set, 1 does)
        assert eng.prefilter_limit(1) == len(l1_want[2]) < len(l_want[2])
        _same_csr(eng.prefilter_fetch(), l1_want, "step 5: the prefilter's result limited to 1 a genome")
        # 6. another genome set: all three are gone, and the set runs as if it were the first
        seqs_n, want_n = U.instantiation_set("small N"), oracle_of("small N", "defaults")
        eng.set_genomes(seqs_n)
        for call in (eng.prefilter_fetch, lambda: eng.kept_fetch(0, 1), eng.cluster_fetch, eng.cluster_add_kept):
            with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
                call()
        rec = _dense(eng, U._INST_FORM_ENV["bitmaps"], monkeypatch, rtc_cache, seqs_n, prm, want_n, "step 6: bitmap form on the new set")
        assert all("nfree=0" in x and "cand=2" in x for x in rec), rec
    finally:
        eng.close()
