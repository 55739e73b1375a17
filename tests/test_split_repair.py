"""CPU: the split path's repair loop on the host -- void segments, resumes, the give-up round.

- split_stitch on hand-made chains in a stand-alone program under the address and undefined-behaviour sanitizers
  (tests/model/split_stitch_check.cpp): the only place a broken chain (cause 5) and the exit without anything to retry
  can be tested;
- the table of the search's finds (U.SPLIT_REPAIR_TABLE, tools/split_void_search.py) holds what it is meant to hold, and
  every entry, regenerated, still gives the model's counts the table states: a change of the generator cannot empty it;
- the device's round structure on the host (U.model_split_rounds) equals the oracle on every entry at the device's
  give-up rule, at give-up 0 and at give-up 1.
tests/test_gpu_split_repair.py runs the same entries on the device against these expected values."""
import os
import subprocess

import numpy as np
import pytest

import util as U

TABLE = U.SPLIT_REPAIR_TABLE


def test_split_stitch_on_hand_made_chains_under_the_sanitizers(tmp_path):
    src = os.path.join(U.ROOT, "tests", "model", "split_stitch_check.cpp")
    exe = str(tmp_path / "split_stitch_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",      # (the runtime in the program: it runs beside any preloaded library)
                           src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) >= 100, r.stdout


def test_the_table_holds_what_the_gpu_tests_need():
    by = lambda d: [e for e in TABLE if U.SPLIT_REPAIR_DEFP[e["cls"]] == d]
    generic = by(0)
    for cause in (0, 1, 4):                               # each at least five times in all, on both NFREE instantiations
        assert sum(e["voids"][cause] for e in generic) >= 5, cause
        assert {e["nfree"] for e in generic if e["voids"][cause]} == {0, 1}, cause
    for cause in (2, 3):                                  # the search found these as well
        assert sum(e["voids"][cause] for e in generic) >= 1, cause
    assert max(e["max_resumes_of_a_pair"] for e in generic) >= 3
    assert any(e["given_up"] for e in generic)            # the device's own rule runs out of rounds
    assert len(by(1)) >= 6 and {e["nfree"] for e in by(1)} == {0, 1}
    assert len(by(2)) >= 2 and {e["nfree"] for e in by(2)} == {0, 1}
    assert all(sum(e["voids"]) > 0 and e["voids"][5] == 0 for e in TABLE)
    # pairs that are given up after one round of resumes (LZANI_SPLIT_GIVE_UP=1) on both NFREE instantiations
    assert {e["nfree"] for e in generic if e["max_resumes_of_a_pair"] >= 2} == {0, 1}
    assert all((cls, seed) in [(e["cls"], e["seed"]) for e in TABLE] for cls, seed in U.SPLIT_REPAIR_ONE_BATCH)


def test_split_plan_restates_the_forced_segment_length():
    """S and the segment length of U.SPLIT_REPAIR_ENV's form: a cut every 512 positions, as many as cover the longest
    genome + mrd, 64 at the most."""
    for dmax, want in ((512, (0, 0)), (513, (2, 512)), (1024, (2, 512)), (1025, (3, 512)), (9040, (18, 512)), (64 * 512, (64, 512)),
                       (64 * 512 + 1, (64, 512)), (200000, (64, 512))):
        assert U.split_plan(6, (dmax + 320 + 1023) // 1024 * 32, dmax, U.SPLIT_REPAIR_ENV) == want, dmax
    assert U.split_plan(6, 32, 9040, dict(U.SPLIT_REPAIR_ENV, LZANI_SPLIT_SEGLEN="100")) == (18, 512)       # 512 is the least
    assert U.split_plan(6, 32, 9040, dict(U.SPLIT_REPAIR_ENV, LZANI_SPLIT_SEGLEN="3000")) == (4, 3000)
    assert U.split_plan(56, 8192 * 20, 5_000_000, {}) == (64, 78125) and U.split_plan(5000, 65536, 2_000_000, {}) == (0, 0)


@pytest.mark.parametrize("entry", TABLE, ids=U.SPLIT_REPAIR_IDS)
def test_model_rounds_against_the_oracle(entry):
    cls, seed = entry["cls"], entry["seed"]
    prm, seqs, want = U.split_repair_base(cls, seed)
    n = len(seqs)
    nf = int(all((s < 4).all() for s in seqs))
    # the case is what the table says it is: the generator still makes it, the device would run it by that class's kernels,
    # and the model's cuts are the device's (every genome below 64 cuts of 512)
    assert nf == entry["nfree"] and 2 <= n <= 4 and all(4000 <= len(s) <= 9500 for s in seqs)
    assert max(len(s) for s in seqs) + prm["mrd"] < 64 * 512
    assert U.predict_kernels(seqs, prm, U.SPLIT_REPAIR_ENV) == {f"split nfree={nf} defp={U.SPLIT_REPAIR_DEFP[cls]} mode={m}" for m in (0, 1)}
    got, st = U.split_repair_model(cls, seed)
    assert {k: st[k] for k in entry if k not in ("cls", "seed", "nfree")} == {k: entry[k] for k in entry if k not in ("cls", "seed", "nfree")}
    assert np.array_equal(got, want)
    assert st["pairs_cut"] == n * (n - 1) and sum(st["voids"]) == st["resumed"] + st["given_up"] and st["pairs_with_void"] >= 1
    S, _ = U.split_plan(n * (n - 1), 32, max(len(s) for s in seqs) + prm["mrd"], U.SPLIT_REPAIR_ENV)
    assert st["rounds"] <= 6 + S // 4 + 2
    # give-up 0: the first stitch is the last round -- every pair with a void is given up, none resumed, and its result comes
    # from the stitch of its one segment
    got0, st0 = U.split_repair_model(cls, seed, 0)
    assert np.array_equal(got0, want)
    assert st0["given_up"] == st0["pairs_with_void"] == st["pairs_with_void"] == sum(st0["voids"]) and st0["resumed"] == 0 and st0["rounds"] == 2
    # give-up 1: one round of resumes, then the pairs still void are given up
    got1, st1 = U.split_repair_model(cls, seed, 1)
    assert np.array_equal(got1, want)
    assert st1["resumed"] == st["pairs_with_void"] and st1["given_up"] <= st["pairs_with_void"] and st1["rounds"] <= 3
    assert st1["given_up"] == sum(st1["voids"]) - st1["resumed"]
    if st["max_resumes_of_a_pair"] >= 2:
        assert st1["given_up"] >= 1 and st1["rounds"] == 3


@pytest.mark.parametrize("form", ("thr", "all0"))
def test_model_pairs_that_are_not_cut_have_no_voids(form):
    """A candidate threshold that cuts some pairs only: the others are scanned whole by their segment 0 and never show in
    the counts; a cut pair with a void still resumes."""
    prm, seqs, cnt, thr, _ = U.split_partial_case(form)
    n = len(seqs)
    off = ~np.eye(n, dtype=bool)
    heavy = (cnt >= thr) & off
    assert 0 < heavy.sum() < off.sum()
    _, base = U.split_repair_model("defaults", 2144)
    got, st = U.model_split_rounds(seqs, prm, seglen=512, heavy=heavy)
    assert np.array_equal(got, U.O.oracle_all2all(seqs, prm))
    assert st["pairs_cut"] == heavy.sum()
    assert (st["voids"], st["resumed"], st["given_up"], st["rounds"]) == (base["voids"], base["resumed"], base["given_up"], base["rounds"])
    assert st["resumed"] >= 1
    _, none = U.model_split_rounds(seqs, prm, seglen=512, heavy=np.zeros((n, n), bool))
    assert none["pairs_cut"] == 0 and sum(none["voids"]) == 0 and none["rounds"] == 1
    if form == "thr":                     # the family's pairs cut, the stranger's not, with room to spare
        assert heavy[:n - 1, :n - 1].sum() == (n - 1) * (n - 2) == heavy.sum()
        assert cnt[heavy].min() >= 2 * thr and cnt[off & ~heavy].max() * 1.8 <= thr, (cnt.tolist(), thr)
    else:                                 # some of the family's pairs left whole
        assert thr == (max(len(s) for s in seqs) + prm["mrd"] + 320 + 1023) // 1024 * 32
        assert heavy.sum() < (n - 1) * (n - 2) and not heavy[n - 1].any() and not heavy[:, n - 1].any()


@pytest.mark.parametrize("cls,seed", U.SPLIT_REPAIR_ONE_BATCH)
def test_model_voids_of_one_batch_only(cls, seed):
    """What the two-batch test on the device relies on: the voids of these entries lie in the rows of one half of the
    references, and the counts of the whole run are the sums over the halves (rounds: the most)."""
    prm, seqs, _ = U.split_repair_base(cls, seed)
    _, whole = U.split_repair_model(cls, seed)
    n = len(seqs)
    assert n == 4
    halves = []
    for rows in ((0, 1), (2, 3)):
        heavy = np.zeros((n, n), bool)
        heavy[list(rows), :] = True
        np.fill_diagonal(heavy, False)
        halves.append(U.model_split_rounds(seqs, prm, seglen=512, heavy=heavy)[1])
    assert sorted(sum(h["voids"]) > 0 for h in halves) == [False, True]
    assert [a + b for a, b in zip(halves[0]["voids"], halves[1]["voids"])] == whole["voids"]
    assert halves[0]["resumed"] + halves[1]["resumed"] == whole["resumed"] and max(h["rounds"] for h in halves) == whole["rounds"]
