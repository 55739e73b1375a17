"""GPU: one cell per pair-kernel instantiation of the launch record (util.INST_CELLS; tests/test_instantiations.py checks on
the CPU that the cells cover the table and lead the dispatch there).  Every cell clears the LZANI_* switches, sets its own,
runs its call and asserts that
- the launch record names exactly the cell's kernel (a split cell: both modes of its k_split) and no other pair kernel;
- the results are bit-equal to the oracle (the matching entries of its all2all for query lists);
- regions cells: every region of every pair equals O.oracle_pair(..., want_regions=True);
- run-time compiled cells: no compile failed, and rtc_info() reports the null chain as chain_params_ok says."""
import time

import numpy as np
import pytest

import lzani_ctypes as L
import oracle as O
import util as U

pytestmark = pytest.mark.gpu

FORM_ENV = ("LZANI_RTC", "LZANI_RTC_MIN_PAIRS", "LZANI_RTC_CACHE", "LZANI_PM", "LZANI_PM_MIN_ROWS", "LZANI_PM_MIN_SHARE",
            "LZANI_PM_MAX_BYTES", "LZANI_JOIN_MIN_BYTES", "LZANI_NO_JOIN", "LZANI_BLOCK_KERNEL", "LZANI_SPLIT", "LZANI_SPLIT_SEGLEN",
            "LZANI_SPLIT_ALL", "LZANI_SPLIT_S", "LZANI_SPLIT_THR", "LZANI_SPLIT_GIVE_UP", "LZANI_LPT", "LZANI_NO_TAGWORDS", "LZANI_NO_BUCKETS",
            "LZANI_NO_FILTER", "LZANI_FILTER_MAX_BITS", "LZANI_BK_MAX_DIRBITS", "LZANI_MAX_SLOTS")
_ORACLE = {}


@pytest.fixture(scope="module")
def rtc_cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("rtc_cache"))


def _oracle(setname, prm_name):
    key = (setname, prm_name)
    if key not in _ORACLE:
        _ORACLE[key] = O.oracle_all2all(U.instantiation_set(setname), U.INST_PARAMS[prm_name], threads=16)
    return _ORACLE[key]


def _diff(got, want):
    bad = np.argwhere((got != want).reshape(-1, 3).any(axis=1))
    return f"{len(bad)} of {len(want.reshape(-1, 3))} pairs differ, first {bad[:3].ravel().tolist()}"


@pytest.mark.parametrize("cell", U.INST_CELLS, ids=[c["id"] for c in U.INST_CELLS])
def test_instantiation_matches_the_oracle(monkeypatch, rtc_cache, cell):
    for k in FORM_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LZANI_RTC_CACHE", rtc_cache)
    for k, v in cell["env"].items():
        monkeypatch.setenv(k, v)
    t0 = time.time()
    prm = U.INST_PARAMS[cell["prm"]]
    seqs = U.instantiation_set(cell["set"])
    n = len(seqs)
    want = _oracle(cell["set"], cell["prm"])
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
    assert np.array_equal(out, exp), (cell["id"], _diff(out, exp))
    if cell["name"].startswith("rtc "):
        assert info["kernels_failed"] == 0 and info["kernels_built"] >= 1, (cell["id"], info)
        assert info["null_chain"] == U.chain_params_ok(prm), (cell["id"], info)
    if cell["form"] == "regions":
        cols = ("ref_start", "ref_end", "seq_start", "seq_end", "num_matches", "num_mismatches")
        e = total = 0
        for r in range(n):
            for qq in range(n):
                if qq == r:
                    continue
                mine = regs[regs["pair"] == e]
                got = np.stack([mine[c] for c in cols], axis=1) if len(mine) else np.zeros((0, 6), np.int32)
                _, oregs = O.oracle_pair(seqs[r], seqs[qq], prm, want_regions=True)
                assert np.array_equal(got, oregs), (cell["id"], r, qq, got[:3].tolist(), oregs[:3].tolist())
                total += len(oregs)
                e += 1
        assert total == len(regs) and total > 0, (cell["id"], total, len(regs))
    print(f"cell {cell['id']}: set '{cell['set']}', {len(exp)} pairs, {time.time() - t0:.2f} s")
