"""CPU: the tile rule of sparse counting -- its Python statement (tests/prefilter_sparse_model.py) against
lzani_plan_sparse_tiles on the pass set's own rows, on random rows and on the error cases -- the new entry points of the
C-ABI without a GPU, and the host binary's --flt-kmers-counting."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lzani_ctypes as L
import prefilter_model as PM
import prefilter_pass_model as PP
import prefilter_sparse_model as SM
import synth_genomes as SG
import util as U

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
K12_ROWS = [14, 15, 10, 15, 9, 8, 11, 8, 8, 8, 10, 8, 8, 5, 3, 3, 0, 0, 4, 3, 2, 1, 1, 0]

_shared = {}


def shared_of(k):
    if k not in _shared:
        _shared[k] = PM.shared_matrix(PP.pass_set(), k)[1]
    return _shared[k]


def test_row_pairs_of_the_pass_set():
    """The figures the GPU tests of sparse counting stand on."""
    r8, r12, r21 = SM.row_pairs(shared_of(8)), SM.row_pairs(shared_of(12)), SM.row_pairs(shared_of(21))
    assert r8.dtype == np.uint64 and int(r8.sum()) == 231 and r8[:16].tolist() == list(range(21, 5, -1))
    assert r12.tolist() == K12_ROWS and int(r12.sum()) == 154
    assert int(r21.sum()) == 35 == int((np.triu(shared_of(21), 1) > 0).sum())
    for n_ref, pairs in ((9, 8), (13, 11)):
        rc = SM.row_pairs(shared_of(21), n_ref)
        assert len(rc) == n_ref and int(rc.sum()) == pairs


def test_row_pairs_equals_a_double_loop():
    r = lambda seed, n: (SG.splitmix64(seed, np.arange(n, dtype=np.uint64)) % np.uint64(4)).astype(np.uint8)
    base = r(1, 90)
    seqs = [base, np.concatenate((base[:50], r(2, 40))), r(3, 70), (3 - base[::-1]).astype(np.uint8), np.concatenate((r(4, 30), base[40:])), r(5, 6)]
    sets = [set(PM.kmer_set(s, 8).tolist()) for s in seqs]
    shared = PM.shared_matrix(seqs, 8)[1]
    n = len(seqs)
    assert SM.row_pairs(shared).tolist() == [sum(1 for b in range(a + 1, n) if sets[a] & sets[b]) for a in range(n)]
    assert sum(SM.row_pairs(shared).tolist()) > 0
    for n_ref in range(1, n):
        assert SM.row_pairs(shared, n_ref).tolist() == [sum(1 for b in range(n_ref, n) if sets[a] & sets[b]) for a in range(n_ref)]


@pytest.mark.parametrize("k, slots, tile_r0, attempts", [
    (8, 512, [0, 24], 1),                                   # 231 pairs under the limit of 256
    (12, 256, [0, 12, 24], 3),                              # 154 > 128; rows 0 .. 11 hold 124
    (12, 32, list(range(25)), 28),                          # 24, 12, 6, 3 rows overflow the limit of 16; then one row a tile
    (21, 2048, [0, 24], 1),
])
def test_the_plan_of_the_pass_set(k, slots, tile_r0, attempts):
    pairs = SM.row_pairs(shared_of(k))
    assert SM.plan(pairs, slots) == (tile_r0, attempts)
    got_r0, got_attempts = L.plan_sparse_tiles(pairs, slots)
    assert got_r0.dtype == np.uint32 and got_r0.tolist() == tile_r0 and got_attempts == attempts


def test_a_row_above_half_the_table_is_refused():
    pairs = SM.row_pairs(shared_of(12))
    assert SM.plan(pairs, 16) is None                       # row 0 holds 14 pairs, the limit is 8
    with pytest.raises(L.LzaniError, match="LZANI_ERR_NOMEM"):
        L.plan_sparse_tiles(pairs, 16)
    assert SM.plan([8], 16) == ([0, 1], 1) and L.plan_sparse_tiles([8], 16)[0].tolist() == [0, 1]      # exactly half fits
    assert SM.plan([9], 16) is None
    with pytest.raises(L.LzaniError, match="LZANI_ERR_NOMEM"):
        L.plan_sparse_tiles([9], 16)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_NOMEM"):
        L.plan_sparse_tiles([0, 0, 2 ** 64 - 1, 2 ** 64 - 1], 2 ** 40)


def test_random_rows_against_the_statement():
    rng = np.random.default_rng(20240611)
    seen_none, seen_many = 0, 0
    for _ in range(300):
        n = int(rng.integers(1, 70))
        slots = 1 << int(rng.integers(1, 12))
        top = int(rng.choice([1, slots // 8 + 1, slots // 2 + 1, slots]))
        pairs = rng.integers(0, top + 1, size=n).astype(np.uint64)
        want = SM.plan(pairs, slots)
        if want is None:
            seen_none += 1
            with pytest.raises(L.LzaniError, match="LZANI_ERR_NOMEM"):
                L.plan_sparse_tiles(pairs, slots)
            continue
        got_r0, got_attempts = L.plan_sparse_tiles(pairs, slots)
        assert (got_r0.tolist(), got_attempts) == want, (pairs.tolist(), slots)
        r0 = want[0]
        assert r0[0] == 0 and r0[-1] == n and all(a < b for a, b in zip(r0, r0[1:]))
        assert all(int(pairs[a:b].sum()) <= slots // 2 for a, b in zip(r0, r0[1:]))
        heights = [b - a for a, b in zip(r0, r0[1:])]
        assert all(x >= y for x, y in zip(heights, heights[1:]))               # the height never grows back
        seen_many += len(heights) > 2
    assert seen_none > 10 and seen_many > 10


def test_entry_points_without_a_gpu():
    L.build_library()
    lib = L.load_library()
    for name in ("lzani_set_prefilter_counting", "lzani_get_prefilter_sparse_info", "lzani_plan_sparse_tiles"):
        assert name in L.EXPORTS and getattr(lib, name) is not None
    assert C.sizeof(L.PrefilterSparseInfo) == 48 and L.PF_COUNTING == {"auto": 0, "dense": 1, "sparse": 2}
    info = L.PrefilterSparseInfo()
    assert lib.lzani_set_prefilter_counting(None, 2) == -1 and lib.lzani_get_prefilter_sparse_info(None, C.byref(info)) == -1
    pairs = np.array([1, 2, 3], dtype=np.uint64)
    p = pairs.ctypes.data_as(C.c_void_p)
    r0 = np.full(4, 77, dtype=np.uint32)
    att = C.c_uint32(77)
    for n_rows, ptr, slots in ((0, p, 16), (3, None, 16), (3, p, 0), (3, p, 1), (3, p, 24), (3, p, 2 ** 64 - 1)):
        assert lib.lzani_plan_sparse_tiles(n_rows, ptr, C.c_uint64(slots), r0.ctypes.data_as(C.c_void_p), C.byref(att)) == -1, (n_rows, slots)
    assert r0.tolist() == [77] * 4 and att.value == 77                          # nothing is written on an error
    assert lib.lzani_plan_sparse_tiles(3, p, C.c_uint64(16), None, None) == 1   # both outputs may be null
    assert lib.lzani_plan_sparse_tiles(3, p, C.c_uint64(8), None, None) == 3    # 6 > 4: three tiles of one row
    assert SM.plan([1, 2, 3], 8) == ([0, 1, 2, 3], 4) and L.plan_sparse_tiles(pairs, 8)[0].tolist() == [0, 1, 2, 3]


def test_the_tile_rule_under_the_sanitizers(tmp_path):
    """PfTiles and plan_sparse_tiles_impl (lzani_sparse_plan.h) in a stand-alone host program, built with the address and
    undefined-behaviour sanitizers and run on the CPU."""
    src = os.path.join(U.ROOT, "tests", "model", "sparse_plan_check.cpp")
    exe = str(tmp_path / "sparse_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",      # (the runtime in the program: it runs beside any preloaded library)
                           "-I" + os.path.join(U.ROOT, "include"), src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    plans, refused = (int(x) for x in r.stdout.split())
    assert plans > 1000 and refused > 1000


@pytest.fixture(scope="module")
def host_binary():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])
    return EXE


@pytest.mark.parametrize("mode", ["all2all", "query2ref"])
@pytest.mark.parametrize("value", ["x", "Sparse", "2", "dense,sparse"])
def test_the_binary_refuses_a_bad_counting_mode_before_reading_input(host_binary, tmp_path, mode, value):
    missing = str(tmp_path / "no_such_input.fa")
    args = [host_binary, mode, "--in-fasta", missing, "-o", str(tmp_path / "o.tsv"), "--flt-kmers", "21", "0.5", "--flt-kmers-counting", value]
    if mode == "query2ref":
        args += ["--query-fasta", missing]
    p = subprocess.run(args, capture_output=True, text=True)
    assert p.returncode == 1 and "Invalid value for --flt-kmers-counting: %s " % value in p.stderr, p.stderr
    assert "Cannot open file" not in p.stderr and "Loading sequences" not in p.stderr


@pytest.mark.parametrize("value", ["auto", "dense", "sparse"])
def test_good_counting_modes_reach_the_input(host_binary, tmp_path, value):
    missing = str(tmp_path / "no_such_input.fa")
    p = subprocess.run([host_binary, "all2all", "--in-fasta", missing, "-o", str(tmp_path / "o.tsv"), "--flt-kmers", "21", "0.5",
                        "--flt-kmers-counting", value], capture_output=True, text=True)
    assert p.returncode == 1 and "Cannot open file: " + missing in p.stderr


def test_usage_names_the_flag(host_binary):
    p = subprocess.run([host_binary], capture_output=True, text=True)
    assert "--flt-kmers-counting <auto|dense|sparse>" in p.stderr
