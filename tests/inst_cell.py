"""GPU: the body of one instantiation cell (util.INST_CELLS), shared by tests/test_gpu_instantiations.py (the random sets) and
tests/test_gpu_repeats.py (the repeat-structured sets).  A cell clears the LZANI_* switches, sets its own, runs its call and
asserts that
- the launch record names exactly the cell's kernel (a split cell: both modes of its k_split) and no other pair kernel;
- the results are bit-equal to the oracle (the matching entries of its all2all for query lists);
- regions cells: every region of every pair equals O.oracle_pair(..., want_regions=True);
- run-time compiled cells: no compile failed, and rtc_info() reports the null chain as chain_params_ok says."""
import time

import numpy as np

import lzani_ctypes as L
import oracle as O
import util as U

FORM_ENV = ("LZANI_RTC", "LZANI_RTC_MIN_PAIRS", "LZANI_RTC_CACHE", "LZANI_PM", "LZANI_PM_MIN_ROWS", "LZANI_PM_MIN_SHARE",
            "LZANI_PM_MAX_BYTES", "LZANI_JOIN_MIN_BYTES", "LZANI_NO_JOIN", "LZANI_BLOCK_KERNEL", "LZANI_SPLIT", "LZANI_SPLIT_SEGLEN",
            "LZANI_SPLIT_ALL", "LZANI_SPLIT_S", "LZANI_SPLIT_THR", "LZANI_SPLIT_GIVE_UP", "LZANI_LPT", "LZANI_NO_TAGWORDS", "LZANI_NO_BUCKETS",
            "LZANI_NO_FILTER", "LZANI_FILTER_MAX_BITS", "LZANI_BK_MAX_DIRBITS", "LZANI_MAX_SLOTS")
REGION_COLS = ("ref_start", "ref_end", "seq_start", "seq_end", "num_matches", "num_mismatches")


def diff(got, want):
    bad = np.argwhere((got != want).reshape(-1, 3).any(axis=1))
    return f"{len(bad)} of {len(want.reshape(-1, 3))} pairs differ, first {bad[:3].ravel().tolist()}"


def regions_of(regs, e):
    """The regions of pair e of a run_rows_regions call as rows of REGION_COLS."""
    mine = regs[regs["pair"] == e]
    return np.stack([mine[c] for c in REGION_COLS], axis=1) if len(mine) else np.zeros((0, 6), np.int32)


def run_cell(monkeypatch, rtc_cache, cell, seqs, want):
    """One cell on the genome set seqs; want: the oracle's all2all of the set under the cell's tuple."""
    for k in FORM_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LZANI_RTC_CACHE", rtc_cache)
    for k, v in cell["env"].items():
        monkeypatch.setenv(k, v)
    t0 = time.time()
    prm = U.INST_PARAMS[cell["prm"]]
    n = len(seqs)
    ref_ids, off, q = U.instantiation_rows(cell, n)
    exp = np.concatenate([want[r, q[off[k]:off[k + 1]] if q is not None else [x for x in range(n) if x != r]]
                          for k, r in enumerate(ref_ids)])
    eng = L.Engine(prm)
    try:
        eng.set_genomes(seqs)
        if cell["form"] == "regions":
            out, regs = eng.run_rows_regions(ref_ids, off, None)
        else:
            out = eng.run_rows(ref_ids, off, q)
        rec, info = eng.kernel_launches(), eng.rtc_info()
    finally:
        eng.close()
    assert set(rec) == U.kernel_names_of_cell(cell), (cell["id"], rec)
    assert np.array_equal(out, exp), (cell["id"], diff(out, exp))
    if cell["name"].startswith("rtc "):
        assert info["kernels_failed"] == 0 and info["kernels_built"] >= 1, (cell["id"], info)
        assert info["null_chain"] == U.chain_params_ok(prm), (cell["id"], info)
    if cell["form"] == "regions":
        e = total = 0
        for r in range(n):
            for qq in range(n):
                if qq == r:
                    continue
                got = regions_of(regs, e)
                _, oregs = O.oracle_pair(seqs[r], seqs[qq], prm, want_regions=True)
                assert np.array_equal(got, oregs), (cell["id"], r, qq, got[:3].tolist(), oregs[:3].tolist())
                total += len(oregs)
                e += 1
        assert total == len(regs) and total > 0, (cell["id"], total, len(regs))
    print(f"cell {cell['id']}: set '{cell['set']}', {len(exp)} pairs, {time.time() - t0:.2f} s")
