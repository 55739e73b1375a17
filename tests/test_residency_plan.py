"""CPU: the out-of-core block plan (lzani_plan_blocks, a pure host function) against its plain-Python statement
(tests/ooc_model.py), the `lz-ani --gpu-mem` flag, and the new exports."""
import os
import subprocess

import numpy as np
import pytest

import lzani_ctypes as L
import ooc_model as M
import util as U

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
NEW_EXPORTS = ("lzani_set_genome_memory", "lzani_plan_blocks", "lzani_get_residency", "lzani_group_set_genome_memory",
               "lzani_group_get_residency")

TUPLES = {"default": {}, "long": dict(mal=15, msl=9, reg=60), "nonfast": dict(mal=16, msl=16),
          "mrd0": dict(mrd=0, mqd=0), "mrd1000": dict(mrd=1000)}


@pytest.fixture(scope="module")
def lib():
    L.build_library()
    return L.load_library()


def _lens(st, n, lo, hi):
    return (lo + st.integers(0, hi - lo + 1, n)).astype(np.uint32)


@pytest.mark.parametrize("name", sorted(TUPLES))
def test_plan_matches_the_rule(lib, name):
    prm = TUPLES[name]
    st = np.random.default_rng(sum(map(ord, name)))
    for trial in range(6):
        n = int(st.integers(1, 60))
        lens = _lens(st, n, 0, 60_000)
        if trial == 5:
            lens[int(st.integers(0, n))] = 700_000        # a long genome: tag words of 8 MB, join lists at mal 11 / 15
        lo = M.min_limit(lens, prm)
        for limit in (lo, lo + 1, 2 * lo, 5 * lo + 12345, int(lens.astype(np.int64).sum()) * 600):
            nb, got = L.plan_blocks(lens, prm, limit)
            want = M.plan_blocks(lens, prm, limit)
            assert want is not None
            assert nb == int(want.max()) + 1 and np.array_equal(got, want), (name, trial, limit)
            assert max(M.block_bytes(lens, prm, want)) <= limit // 2
        with pytest.raises(L.LzaniError, match="ERR_ARG"):
            L.plan_blocks(lens, prm, lo - 1)
        assert M.plan_blocks(lens, prm, lo - 1) is None
        nb, got = L.plan_blocks(lens, prm, 0)
        assert nb == 1 and not got.any()


def test_plan_counts_join_lists_where_they_apply():
    lens = np.array([700_000, 650_000, 20_000], np.uint32)
    assert M.join_lists(lens, {}) and M.join_lists([2_200_000], TUPLES["long"])
    assert not M.join_lists(lens, TUPLES["long"])               # (mal 15: 9 tag bits, no tag words below ~2 Mbp)
    assert not M.join_lists(lens, TUPLES["nonfast"]) and not M.join_lists(lens[2:], {})
    # the minimum is twice the largest genome's tables, its join lists included
    w = (2 * 700_000 + 120 + 63) // 64 + 2
    assert M.min_limit(lens, {}) == 2 * (w * 536 + 8 * 700_000 + 20)
    nb, _ = L.plan_blocks(lens, {}, M.min_limit(lens, {}))
    assert nb == 2


def test_plan_refuses_bad_arguments(lib):
    arr, _ = L.params_array({})
    lens = np.array([5, 6], np.uint32)
    assert lib.lzani_plan_blocks(0, L._ptr(lens), arr, 1 << 30, None) == -1
    assert lib.lzani_plan_blocks(2, None, arr, 1 << 30, None) == -1
    bad, _ = L.params_array(dict(mqd=65))
    assert lib.lzani_plan_blocks(2, L._ptr(lens), bad, 1 << 30, None) == -2
    assert lib.lzani_plan_blocks(2, L._ptr(lens), arr, 1 << 30, None) == 1          # block_of may be NULL


def test_schedule_model_examples():
    """The documented order, by hand: 4 blocks of a dense all2all -- 16 tiles, 4 + 3 + 2 + 2 uploads."""
    bo = np.repeat(np.arange(4), 3).astype(np.uint32)
    ref, off = L.dense_rows(12)
    tiles, uploads, state = M.schedule(bo, ref, off, None)
    assert (tiles, uploads, state) == (16, 11, (3, 1))
    # filtered rows that stay inside their block: one tile and one upload per block, never a B upload
    q = np.array([(r + 1) % 3 + 3 * (r // 3) for r in range(12)], np.uint32)
    assert M.schedule(bo, ref, np.arange(13, dtype=np.uint64), q)[:2] == (4, 4)


def test_new_exports_are_present(lib):
    for name in NEW_EXPORTS:
        assert name in L.EXPORTS and getattr(lib, name) is not None
    assert [f for f, _ in L.ResidencyInfo._fields_] == ["limit", "blocks", "tiles", "block_uploads", "peak_resident_bytes",
                                                          "host_bytes", "upload_ms"]


@pytest.fixture(scope="module")
def host_binary():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])
    return EXE


def test_gpu_mem_flag_parsing(host_binary, tmp_path):
    """Bad --gpu-mem values are refused with exit 1 before any input is read; good ones get as far as the input."""
    missing = str(tmp_path / "missing.fna")
    for bad in ("", "abc", "12Q", "1.5G", "-1", "12KB", "G", "99999999999999999999", "17179869184G", " 5"):
        p = subprocess.run([host_binary, "all2all", "--in-fasta", missing, "--gpu-mem", bad], capture_output=True, text=True)
        assert p.returncode == 1 and f"Invalid value for --gpu-mem: {bad}" in p.stderr, (bad, p.stderr)
        assert "Loading sequences" not in p.stderr and "Cannot open file" not in p.stderr
    for good in ("0", "123", "64K", "2m", "1G", "16g"):
        p = subprocess.run([host_binary, "all2all", "--in-fasta", missing, "--gpu-mem", good], capture_output=True, text=True)
        assert p.returncode == 1 and "Invalid value" not in p.stderr and "Cannot open file" in p.stderr, (good, p.stderr)
    p = subprocess.run([host_binary, "all2all"], capture_output=True, text=True)
    assert "--gpu-mem <size>" in p.stderr
