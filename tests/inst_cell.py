"""GPU: the body of one instantiation cell (util.INST_CELLS), shared by tests/test_gpu_instantiations.py (the random sets),
tests/test_gpu_repeats.py (the repeat-structured sets) and tests/test_gpu_context_walk.py (the cells one after another on one
context).  A cell clears the LZANI_* switches, sets its own (apply_env), runs its call and asserts (call_and_check) that
- the launch record names exactly the cell's kernel (a split cell: both modes of its k_split) and no other pair kernel;
- the results are bit-equal to the oracle (the matching entries of its all2all for query lists);
- regions cells: every region of every pair equals O.oracle_pair(..., want_regions=True);
- run-time compiled cells: no compile failed, and rtc_info() reports the null chain as chain_params_ok says.
run_cell is the cell on a context of its own.  A node of tests/context_walk.py is a cell with three more keys: "kernels" (the
names of its launch record; None: not asserted), "blocks" (what residency() must count) and "limit"."""
import hashlib
import time

import numpy as np

import context_walk as W
import lzani_ctypes as L
import oracle as O
import util as U

FORM_ENV = ("LZANI_RTC", "LZANI_RTC_MIN_PAIRS", "LZANI_RTC_CACHE", "LZANI_PM", "LZANI_PM_MIN_ROWS", "LZANI_PM_MIN_SHARE",
            "LZANI_PM_MAX_BYTES", "LZANI_JOIN_MIN_BYTES", "LZANI_NO_JOIN", "LZANI_BLOCK_KERNEL", "LZANI_SPLIT", "LZANI_SPLIT_SEGLEN",
            "LZANI_SPLIT_ALL", "LZANI_SPLIT_S", "LZANI_SPLIT_THR", "LZANI_SPLIT_GIVE_UP", "LZANI_LPT", "LZANI_NO_TAGWORDS", "LZANI_NO_BUCKETS",
            "LZANI_NO_FILTER", "LZANI_FILTER_MAX_BITS", "LZANI_BK_MAX_DIRBITS", "LZANI_MAX_SLOTS")
REGION_COLS = ("ref_start", "ref_end", "seq_start", "seq_end", "num_matches", "num_mismatches")
_ORACLE, _REGIONS = {}, {}


def oracle_of(setname, prm_name):
    """The oracle's all2all of an instantiation set under a tuple of util.INST_PARAMS, made once."""
    key = (setname, prm_name)
    if key not in _ORACLE:
        _ORACLE[key] = O.oracle_all2all(U.instantiation_set(setname), U.INST_PARAMS[prm_name], threads=16)
    return _ORACLE[key]


def oracle_regions_of(seqs, prm_name):
    """{(r, q): the oracle's regions of the pair} of every ordered pair of the genome list seqs under a tuple of
    util.INST_PARAMS, made once per list (the lists of util.instantiation_set and of the repeat sets are made once)."""
    key = (id(seqs), prm_name)
    if key not in _REGIONS:
        prm = U.INST_PARAMS[prm_name]
        regs = {(r, q): O.oracle_pair(seqs[r], seqs[q], prm, want_regions=True)[1]
                for r in range(len(seqs)) for q in range(len(seqs)) if q != r}
        _REGIONS[key] = (seqs, regs)                    # (the list is kept: its id stays its own)
    return _REGIONS[key][1]


def diff(got, want):
    bad = np.argwhere((got != want).reshape(-1, 3).any(axis=1))
    return f"{len(bad)} of {len(want.reshape(-1, 3))} pairs differ, first {bad[:3].ravel().tolist()}"


def regions_of(regs, e):
    """The regions of pair e of a run_rows_regions call as rows of REGION_COLS."""
    mine = regs[regs["pair"] == e]
    return np.stack([mine[c] for c in REGION_COLS], axis=1) if len(mine) else np.zeros((0, 6), np.int32)


def apply_env(monkeypatch, rtc_cache, node):
    """The process environment of the node's calls: every switch of the set and run paths cleared, then the node's own."""
    for k in set(FORM_ENV + W.SET_ENV + W.RUN_ENV):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LZANI_RTC_CACHE", rtc_cache)
    for k, v in node["env"].items():
        monkeypatch.setenv(k, v)


def call_and_check(eng, node, seqs, want, where, seen=None):
    """The node's call on the engine eng, which holds the genome set seqs; want: the oracle's all2all of the set under the
    node's tuple; where: what every assertion message begins with.  Returns the number of pairs.  seen: a dict that gets the
    launch record ("kernels") and the SHA-256 of the result array ("digest") before anything is asserted."""
    prm = U.INST_PARAMS[node["prm"]]
    n = len(seqs)
    ref_ids, off, q = U.instantiation_rows(node, n)
    exp = np.concatenate([want[r, q[off[k]:off[k + 1]] if q is not None else [x for x in range(n) if x != r]]
                          for k, r in enumerate(ref_ids)])
    if node["form"] == "regions":
        out, regs = eng.run_rows_regions(ref_ids, off, None)
    else:
        out = eng.run_rows(ref_ids, off, q)
    rec, info = eng.kernel_launches(), eng.rtc_info()
    if seen is not None:
        seen.update(kernels=dict(rec), digest=hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest())
    kernels = node["kernels"] if "kernels" in node else U.kernel_names_of_cell(node)
    if kernels is not None:
        assert set(rec) == kernels, (where, rec)
    if "blocks" in node:
        assert eng.residency()["blocks"] == node["blocks"], (where, eng.residency())
    assert np.array_equal(out, exp), (where, diff(out, exp))
    if node["name"].startswith("rtc "):
        assert info["kernels_failed"] == 0 and info["kernels_built"] >= 1, (where, info)
        assert info["null_chain"] == U.chain_params_ok(prm), (where, info)
    if node["form"] == "regions":
        oracle_regs = oracle_regions_of(seqs, node["prm"])
        e = total = 0
        for r in range(n):
            for qq in range(n):
                if qq == r:
                    continue
                got = regions_of(regs, e)
                oregs = oracle_regs[(r, qq)]
                assert np.array_equal(got, oregs), (where, r, qq, got[:3].tolist(), oregs[:3].tolist())
                total += len(oregs)
                e += 1
        assert total == len(regs) and total > 0, (where, total, len(regs))
    return len(exp)


def run_cell(monkeypatch, rtc_cache, cell, seqs, want, seen=None):
    """One cell on the genome set seqs, on a context of its own; want: the oracle's all2all of the set under the cell's tuple;
    seen: see call_and_check."""
    apply_env(monkeypatch, rtc_cache, cell)
    t0 = time.time()
    eng = L.Engine(U.INST_PARAMS[cell["prm"]])
    try:
        eng.set_genomes(seqs)
        pairs = call_and_check(eng, cell, seqs, want, cell["id"], seen)
    finally:
        eng.close()
    print(f"cell {cell['id']}: set '{cell['set']}', {pairs} pairs, {time.time() - t0:.2f} s")
