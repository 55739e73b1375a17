"""GPU: the split path's repair loop -- void segments, resumes, the give-up round -- on the smallest inputs that have one.

The inputs are the finds of tools/split_void_search.py (U.SPLIT_REPAIR_TABLE): sets of 2-4 genomes of 4-9 kbp whose split
run at cuts every 512 positions has void stitches on the host model.  Every expected value is made on the CPU
(tests/test_split_repair.py checks them there): the oracle's results, and the model's counts of the device's round
structure (U.model_split_rounds), which the device reports through Engine.split_stats().  The counts are equal by
construction -- the model's wave and the device's run the same PairMachine, the stitch is the same function, and which
segment is resumed follows from the segments' records alone.

Forced as tests/test_gpu_envelope.py forces its split form: LZANI_RTC=0, LZANI_PM_MIN_ROWS=1, LZANI_SPLIT=1,
LZANI_SPLIT_SEGLEN=512, LZANI_SPLIT_ALL=1."""
import numpy as np
import pytest

import lzani_ctypes as L
import util as U

pytestmark = pytest.mark.gpu

FORM_ENV = ("LZANI_RTC", "LZANI_RTC_MIN_PAIRS", "LZANI_PM", "LZANI_PM_MIN_ROWS", "LZANI_PM_MIN_SHARE", "LZANI_PM_MAX_BYTES",
            "LZANI_JOIN_MIN_BYTES", "LZANI_NO_JOIN", "LZANI_BLOCK_KERNEL", "LZANI_SPLIT", "LZANI_SPLIT_SEGLEN", "LZANI_SPLIT_ALL",
            "LZANI_SPLIT_S", "LZANI_SPLIT_THR", "LZANI_SPLIT_GIVE_UP", "LZANI_LPT", "LZANI_NO_TAGWORDS", "LZANI_NO_BUCKETS",
            "LZANI_NO_FILTER", "LZANI_FILTER_MAX_BITS", "LZANI_BK_MAX_DIRBITS", "LZANI_MAX_SLOTS", "LZANI_PM_FROM_INDEX")
COUNTS = ("pairs_cut", "rounds", "resumed", "given_up", "voids")


def _engine(monkeypatch, prm, seqs, env):
    for k in FORM_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = L.Engine(prm)
    eng.set_genomes(seqs)
    return eng


def _counts(st):
    return {k: st[k] for k in COUNTS}


def _diff(got, want):
    bad = np.argwhere((got != want).any(axis=2))
    return f"{len(bad)} pairs differ, first {bad[:3].tolist()}: {[got[tuple(b)].tolist() for b in bad[:3]]} != {[want[tuple(b)].tolist() for b in bad[:3]]}"


@pytest.mark.parametrize("entry", U.SPLIT_REPAIR_TABLE, ids=U.SPLIT_REPAIR_IDS)
def test_voids_resumes_and_the_give_up_round(monkeypatch, entry):
    """One entry at the device's own give-up rule, then with LZANI_SPLIT_GIVE_UP=0 (the first stitch is the last round:
    every pair with a void is given up) and =1 (one round of resumes first): all three fields of every pair equal to the
    oracle's, the launch record names the entry's split kernels (one launch of the segments' kernel a round), and the
    repair loop's counts equal the model's."""
    cls, seed = entry["cls"], entry["seed"]
    prm, seqs, want = U.split_repair_base(cls, seed)
    eng = _engine(monkeypatch, prm, seqs, U.SPLIT_REPAIR_ENV)
    try:
        for give_up in (-1, 0, 1):
            if give_up >= 0:
                monkeypatch.setenv("LZANI_SPLIT_GIVE_UP", str(give_up))
            _, model = U.split_repair_model(cls, seed, give_up)
            got = eng.all2all()
            st, rec, lay = eng.split_stats(), eng.kernel_launches(), eng.layout()
            what = (cls, seed, give_up)
            print(what, "device", _counts(st), "model", _counts(model))
            assert np.array_equal(got, want), (what, _diff(got, want))
            assert set(rec) == U.predict_kernels(seqs, prm, U.SPLIT_REPAIR_ENV) == {
                f"split nfree={entry['nfree']} defp={U.SPLIT_REPAIR_DEFP[cls]} mode={m}" for m in (0, 1)}, (what, rec)
            assert lay["split_launches"] == 1 and rec[f"split nfree={entry['nfree']} defp={U.SPLIT_REPAIR_DEFP[cls]} mode=1"] == st["rounds"], (what, lay, rec)
            assert _counts(st) == _counts(model), what
            assert sum(st["voids"]) > 0 and st["resumed"] + st["given_up"] == sum(st["voids"]), (what, st)
            if give_up < 0:
                assert _counts(st) == {k: entry[k] for k in COUNTS}, what
            else:
                # (give-up 0: every pair with a void is given up, so there is one; give-up 1: only a pair whose resumed segment
                # hands over to another void one is -- an entry with two resumes of one pair in a row has such a pair, an entry
                # of single voids has none, and the model's 0 is the expected value)
                assert st["rounds"] <= give_up + 2 and st["given_up"] == model["given_up"], (what, st)
                if give_up == 0 or entry["max_resumes_of_a_pair"] >= 2:
                    assert st["given_up"] > 0, (what, st)
    finally:
        eng.close()


@pytest.mark.parametrize("cls,seed", U.SPLIT_REPAIR_ONE_BATCH)
def test_counts_of_two_runs_and_of_two_batches(monkeypatch, cls, seed):
    """The counters, the finished flags and the disabled cuts of a batch do not reach the next one: a run with voids twice
    on one context gives the same results and counts twice; the same set in two batches of two references, of which only
    one has voids (tests/test_split_repair.py), gives the sums -- rounds: the most of a batch -- again twice.  The batches
    are cut by LZANI_PM_MAX_BYTES, room for the candidate bitmaps of six pairs: LZANI_MAX_SLOTS below the number of
    references takes a set of fewer than eight references off the bitmaps, and with them off the split."""
    prm, seqs, want = U.split_repair_base(cls, seed)
    _, model = U.split_repair_model(cls, seed)
    assert len(seqs) == 4
    six_pairs = 6 * 4 * ((max(len(s) for s in seqs) + prm["mrd"] + 320 + 1023) // 1024 * 32)
    for cap, batches in ((None, 1), (str(six_pairs), 2)):
        eng = _engine(monkeypatch, prm, seqs, dict(U.SPLIT_REPAIR_ENV, **({"LZANI_PM_MAX_BYTES": cap} if cap else {})))
        try:
            for run in (0, 1):
                got = eng.all2all()
                st, lay = eng.split_stats(), eng.layout()
                what = (cls, seed, cap, run)
                print(what, "device", _counts(st), "model", _counts(model))
                assert lay["batches_last_run"] == batches and lay["split_launches"] == batches, (what, lay)
                assert np.array_equal(got, want), (what, _diff(got, want))
                assert _counts(st) == _counts(model), what
        finally:
            eng.close()


@pytest.mark.parametrize("form", ("thr", "all0"))
def test_pairs_that_are_not_cut_stay_out_of_the_counts(monkeypatch, form):
    """Only the pairs whose candidates reach a threshold are cut (LZANI_SPLIT_THR; LZANI_SPLIT_ALL=0, whose threshold is the
    words of a pair's bitmap): the others are scanned whole by their segment 0 and never show in the void counts, a cut
    pair with a void still resumes.  Which pairs are cut follows on the CPU from the exact statement of the bitmaps."""
    prm, seqs, cnt, thr, env = U.split_partial_case(form)
    n = len(seqs)
    heavy = (cnt >= thr) & ~np.eye(n, dtype=bool)
    want = U.O.oracle_all2all(seqs, prm, threads=4)
    _, model = U.model_split_rounds(seqs, prm, seglen=512, heavy=heavy)
    eng = _engine(monkeypatch, prm, seqs, env)
    try:
        got = eng.all2all()
        st, rec = eng.split_stats(), eng.kernel_launches()
    finally:
        eng.close()
    print(form, "device", _counts(st), "model", _counts(model))
    assert np.array_equal(got, want), (form, _diff(got, want))
    assert set(rec) == {f"split nfree=1 defp=1 mode={m}" for m in (0, 1)}, rec
    assert st["pairs_cut"] == heavy.sum() < n * (n - 1)
    assert _counts(st) == _counts(model) and st["resumed"] >= 1 and st["given_up"] == 0, (form, st)
