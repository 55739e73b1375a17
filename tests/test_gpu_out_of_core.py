"""GPU: genome sets run out-of-core (lzani_set_genome_memory, lzani_ooc.h) -- tile by tile over (reference block, query
block) -- give the results of the in-core run and of the oracle, with the tiles and block uploads tests/ooc_model.py
predicts, within the genome-memory limit, through every run entry point, every candidate form, the group and the host
binary."""
import ctypes as C
import os

import numpy as np
import pytest

import lzani_ctypes as L
import ooc_model as M
import oracle as O
import synth_genomes as SG
import util as U

pytestmark = pytest.mark.gpu

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
ENV = ("LZANI_RTC", "LZANI_RTC_MIN_PAIRS", "LZANI_RTC_CACHE", "LZANI_JOIN_MIN_BYTES", "LZANI_FREE_BYTES", "LZANI_PM",
       "LZANI_PM_MIN_ROWS", "LZANI_PM_MIN_SHARE",
       "LZANI_TILE_MIN", "LZANI_TILE_ROWS", "LZANI_DEVICE_LIST")
_SETS, _INCORE = {}, {}


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def small_set(with_n):
    """21 genomes of 3-6 kbp in families of 4, one of 300 bp; with N runs (util._put_n_runs) or without."""
    if with_n not in _SETS:
        seqs = SG.make_set(20, 9117, lmin=3000, lmax=6000, fam=4)[1]
        if with_n:
            seqs = U._put_n_runs(seqs)
        st = SG.Stream(77)
        _SETS[with_n] = seqs + [(st.u64(300) % np.uint64(4)).astype(np.uint8)]
    return _SETS[with_n]


def engine(seqs, limit, prm=None):
    e = L.Engine(prm)
    e.set_genome_memory(limit)
    e.set_genomes(seqs)
    return e


def incore(with_n):
    if with_n not in _INCORE:
        e = engine(small_set(with_n), 0)
        _INCORE[with_n] = e.all2all()
        assert e.residency()["blocks"] == 1
        e.close()
    return _INCORE[with_n]


def check_residency(eng, lens, prm, limit, ref_ids, row_off, query_ids, blocks=None, state=(None, None)):
    bo = M.plan_blocks(lens, prm, limit)
    tiles, uploads, state = M.schedule(bo, ref_ids, row_off, query_ids, state)
    r = eng.residency()
    assert r["blocks"] == int(bo.max()) + 1 and (blocks is None or r["blocks"] == blocks), r
    assert (r["tiles"], r["block_uploads"]) == (tiles, uploads), (r, tiles, uploads)
    assert r["limit"] == limit and 0 < r["peak_resident_bytes"] <= limit, r
    assert r["host_bytes"] == int(np.sum(lens)) and (r["upload_ms"] > 0) == (uploads > 0), r
    assert eng.layout()["bytes_genomes"] <= limit
    assert set(eng.kernel_launches()) <= set(L.kernel_names())
    return state


@pytest.mark.parametrize("with_n", [False, True], ids=["nfree", "N"])
@pytest.mark.parametrize("blocks", [2, 3, 7])
def test_dense_all2all_in_blocks(blocks, with_n):
    seqs = small_set(with_n)
    lens = [len(s) for s in seqs]
    limit = M.limit_for_blocks(lens, None, blocks)
    eng = engine(seqs, limit)
    got = eng.all2all()
    assert np.array_equal(got, incore(with_n))
    assert np.array_equal(got, O.oracle_all2all(seqs, None, threads=8))
    check_residency(eng, lens, None, limit, *L.dense_rows(len(seqs)), None, blocks=blocks)
    assert eng.layout()["n_free"] == (not with_n)
    assert eng.timing()["pairs"] == len(seqs) * (len(seqs) - 1)
    eng.close()


def ragged_rows(n, seed):
    """Unsorted query lists of 0-12 queries, references repeated and out of order, empty rows among them."""
    st = np.random.default_rng(seed)
    refs, lists = [], []
    for k in range(40):
        r = int(st.integers(0, n))
        m = 0 if k % 7 == 3 else int(st.integers(1, 13))
        q = st.choice([x for x in range(n) if x != r], size=m, replace=False)
        refs.append(r)
        lists.append(q)
    off = np.zeros(len(refs) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    return np.array(refs, np.uint32), off, np.concatenate(lists).astype(np.uint32)


def _regions_raw(eng, ref, off, q, cap):
    out = np.zeros((int(off[-1]), 3), np.int32)
    regs = np.zeros(max(cap, 1), dtype=L.Engine.REGION_DTYPE)
    cnt = C.c_uint64(0)
    eng._check(eng.lib.lzani_run_rows_regions(eng.h, len(ref), L._ptr(ref), L._ptr(off), L._ptr(q), L._ptr(out), L._ptr(regs),
                                              cap, C.byref(cnt)), "regions")
    return out, int(cnt.value)


def test_filtered_rows_through_every_entry_point():
    import torch
    seqs = small_set(True)
    n, lens = len(seqs), [len(s) for s in seqs]
    ref, off, q = ragged_rows(n, 5)
    limit = M.limit_for_blocks(lens, None, 3)
    inc, ooc = engine(seqs, 0), engine(seqs, limit)
    want = inc.run_rows(ref, off, q)
    assert np.array_equal(ooc.run_rows(ref, off, q), want)
    state = check_residency(ooc, lens, None, limit, ref, off, q, blocks=3)
    buf = torch.full((int(off[-1]), 3), -7, dtype=torch.int32, device="cuda:0")
    ooc.run_rows_device(ref, off, q, buf.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), want)
    state = check_residency(ooc, lens, None, limit, ref, off, q, state=state)        # (the halves kept their blocks)
    res_i, reg_i = inc.run_rows_regions(ref, off, q)
    res_o, reg_o = ooc.run_rows_regions(ref, off, q)
    assert np.array_equal(res_i, want) and np.array_equal(res_o, want)
    assert len(reg_i) > 20 and sorted(map(tuple, reg_o.tolist())) == sorted(map(tuple, reg_i.tolist()))
    # a buffer too small: the same count, the stored records a part of the full set with their pairs remapped
    _, cnt_i = _regions_raw(inc, ref, off, q, len(reg_i) // 3)
    out_o, cnt_o = _regions_raw(ooc, ref, off, q, len(reg_i) // 3)
    assert cnt_i == cnt_o == len(reg_i) and np.array_equal(out_o, want)
    inc.close()
    ooc.close()


def test_long_genome_forms_in_tiles(monkeypatch):
    """--mal 15 --msl 9 --reg 60 on genomes of 260-300 kbp: dense tiles by candidate bitmaps (from one row on: a tile here
    has two), split into segments; filtered rows of one query each at the defaults with join lists (the join threshold
    lowered to reach them at this size: tag words of 4 MB)."""
    monkeypatch.setenv("LZANI_PM_MIN_ROWS", "1")
    monkeypatch.setenv("LZANI_PM_MIN_SHARE", "1")
    seqs = SG.make_set(6, 4411, lmin=260_000, lmax=300_000, fam=3)[1]
    lens = [len(s) for s in seqs]
    prm = dict(mal=15, msl=9, reg=60)
    limit = M.limit_for_blocks(lens, prm, 3)
    want = engine(seqs, 0, prm).all2all()
    eng = engine(seqs, limit, prm)
    assert np.array_equal(eng.all2all(), want)
    lay = eng.layout()
    assert lay["split_launches"] > 0 and lay["bitmap_launches"] > 0, lay
    assert eng.residency()["blocks"] == 3
    monkeypatch.delenv("LZANI_PM_MIN_ROWS")
    monkeypatch.delenv("LZANI_PM_MIN_SHARE")
    monkeypatch.setenv("LZANI_JOIN_MIN_BYTES", str(1 << 20))
    ref = np.arange(6, dtype=np.uint32)
    off = np.arange(7, dtype=np.uint64)
    q = np.array([(r + 3) % 6 for r in range(6)], np.uint32)
    inc = engine(seqs, 0)
    want = inc.run_rows(ref, off, q)
    assert inc.layout()["join_lists"] == 1
    lim = M.limit_for_blocks(lens, None, 3, join=True)             # (the plan counts the join lists)
    nb, bo = L.plan_blocks(lens, None, lim)
    assert nb == 3 and np.array_equal(bo, M.plan_blocks(lens, None, lim, join=True))
    ooc = engine(seqs, lim)
    assert np.array_equal(ooc.run_rows(ref, off, q), want)
    assert ooc.layout()["join_lists"] == 1 and any("cand=1" in k for k in ooc.kernel_launches()), ooc.kernel_launches()
    assert ooc.residency()["blocks"] == nb


@pytest.mark.parametrize("prm", [dict(mal=16, msl=16), dict(reg=36)], ids=["nonfast", "rtc"])
def test_other_tuples_in_tiles(prm, monkeypatch, tmp_path):
    if prm.get("reg") == 36:                             # compiled at run time for this tuple, from the first pair on
        monkeypatch.setenv("LZANI_RTC_MIN_PAIRS", "0")
        monkeypatch.setenv("LZANI_RTC_CACHE", str(tmp_path))
    seqs = small_set(True)
    lens = [len(s) for s in seqs]
    limit = M.limit_for_blocks(lens, prm, 3)
    eng = engine(seqs, limit, prm)
    got = eng.all2all()
    assert np.array_equal(got, O.oracle_all2all(seqs, prm, threads=8))
    check_residency(eng, lens, prm, limit, *L.dense_rows(len(seqs)), None, blocks=3)
    if "reg" in prm:
        assert eng.layout()["rtc_launches"] > 0 and any(k.startswith("rtc ") for k in eng.kernel_launches())
    else:
        assert eng.layout()["kmer_words"] == 0


def test_group_with_a_limit_equals_the_single_context():
    seqs = small_set(False)
    lens = [len(s) for s in seqs]
    limit = M.limit_for_blocks(lens, None, 3)
    g = L.Group(None, (0, 0))
    g.set_genome_memory(limit)
    g.set_genomes(seqs)
    ref, off = L.dense_rows(len(seqs))
    got = g.run_rows(ref, off, None)
    want = incore(False)[~np.eye(len(seqs), dtype=bool)]
    assert np.array_equal(got, want)
    for d in (0, 1):
        r = g.residency(d)
        assert r["blocks"] == 3 and r["tiles"] > 0 and r["peak_resident_bytes"] <= limit
    g.close()


def test_fitting_set_stays_in_core_and_automatic_mode(monkeypatch):
    seqs = small_set(False)
    eng = engine(seqs, 0)
    r = eng.residency()
    assert (r["blocks"], r["host_bytes"], r["limit"], r["block_uploads"]) == (1, 0, 0, 0)
    eng.all2all()
    assert eng.residency()["tiles"] == 1
    # the automatic trigger: a device that (as the engine is told) has less free memory than the set's tables
    lens = [len(s) for s in seqs]
    tables = sum(M.genome_bytes(x, None, False) for x in lens)
    monkeypatch.setenv("LZANI_FREE_BYTES", str(tables * 3 // 4))
    auto = engine(seqs, 0)
    r = auto.residency()
    assert r["blocks"] > 1 and r["limit"] == tables * 3 // 4 // 2 and r["host_bytes"] == sum(lens), r
    assert np.array_equal(auto.all2all(), incore(False))
    assert auto.residency()["peak_resident_bytes"] <= r["limit"]


def test_limit_too_small_is_refused_and_the_context_recovers():
    seqs = small_set(True)
    lens = [len(s) for s in seqs]
    lo = M.min_limit(lens, None)
    eng = L.Engine()
    eng.set_genome_memory(lo - 1)
    with pytest.raises(L.LzaniError, match=f"ERR_ARG.*minimum of {lo} bytes"):
        eng.set_genomes(seqs)
    eng.set_genome_memory(lo)
    eng.set_genomes(seqs)
    assert eng.residency()["blocks"] == int(M.plan_blocks(lens, None, lo).max()) + 1 >= len(seqs) // 2
    with pytest.raises(L.LzaniError, match="ERR_STATE"):
        eng.debug_index(0)
    assert np.array_equal(eng.all2all(), incore(True))
    eng.set_genome_memory(0)
    eng.set_genomes(seqs)
    assert eng.residency()["blocks"] == 1 and np.array_equal(eng.all2all(), incore(True))


def _cli_limit(loader, blocks):
    names, seqs = U.reorder(*loader())
    return M.limit_for_blocks([len(s) for s in seqs], None, blocks)


def test_host_binary_with_gpu_mem(tmp_path):
    import subprocess
    run = lambda args, **kw: subprocess.run([EXE] + args, capture_output=True, text=True, **kw)
    out = str(tmp_path / "ani.tsv")
    vir = os.path.join(U.GOLD, "vir61")
    lim = _cli_limit(U.load_vir61, 4)
    p = run(["all2all", "--in-dir", vir, "--out", out, "--gpu-mem", str(lim), "-V", "2"])
    assert p.returncode == 0 and "out-of-core, 4 block(s)" in p.stderr, p.stderr
    assert open(out).read() == open(os.path.join(U.GOLD, "vir61.ani.tsv")).read()
    assert open(str(tmp_path / "ani.ids.tsv")).read() == open(os.path.join(U.GOLD, "vir61.ani.ids.tsv")).read()
    # the tiled all2all of the binary, on two contexts of one GPU
    env = dict(os.environ, LZANI_TILE_MIN="1", LZANI_TILE_ROWS="16", LZANI_DEVICE_LIST="0,0")
    p = run(["all2all", "--in-dir", vir, "--out", out, "--gpu-mem", str(lim), "-V", "2", "--gpus", "2"], env=env)
    assert p.returncode == 0 and "blocks of 16 rows" in p.stderr and "out-of-core, 4 block(s)" in p.stderr, p.stderr
    assert open(out).read() == open(os.path.join(U.GOLD, "vir61.ani.tsv")).read()
    fa = os.path.join(U.GOLD, "example", "multifasta.fna")
    names, seqs = U.reorder(*U.load_example())
    k = -(-M.min_limit([len(s) for s in seqs], None) // 1024)       # (a limit in K just above the minimum)
    nb = int(M.plan_blocks([len(s) for s in seqs], None, 1024 * k).max()) + 1
    assert nb >= 3
    p = run(["all2all", "--in-fasta", fa, "-o", out, "--gpu-mem", f"{k}K", "-V", "2"])
    assert p.returncode == 0 and f"out-of-core, {nb} block(s)" in p.stderr, p.stderr
    assert open(out).read() == open(os.path.join(U.GOLD, "example", "ani.tsv")).read()
    assert open(str(tmp_path / "ani.ids.tsv")).read() == open(os.path.join(U.GOLD, "example", "ani.ids.tsv")).read()
    aln = str(tmp_path / "ani.aln.tsv")
    p = run(["all2all", "--in-fasta", fa, "-o", out, "--out-alignment", aln, "--gpu-mem", f"{k}K", "-V", "2"])
    assert p.returncode == 0 and "out-of-core" in p.stderr, p.stderr
    got = open(aln).read().split("\n")
    gold = open(os.path.join(U.GOLD, "example", "ani.aln.tsv")).read().split("\n")
    assert got[0] == gold[0] and sorted(got[1:]) == sorted(gold[1:])
    assert open(out).read() == open(os.path.join(U.GOLD, "example", "ani.tsv")).read()
    # with the kmer-db filter: the same rows as the in-core run of the binary
    flt = ["--flt-kmerdb", os.path.join(U.GOLD, "example", "fltr.txt"), "0.9", "--out-format", "complete"]
    p = run(["all2all", "--in-fasta", fa, "-o", str(tmp_path / "a.tsv")] + flt)
    assert p.returncode == 0, p.stderr
    p = run(["all2all", "--in-fasta", fa, "-o", str(tmp_path / "b.tsv"), "--gpu-mem", f"{k}K", "-V", "2"] + flt)
    assert p.returncode == 0 and "out-of-core" in p.stderr, p.stderr
    a = open(str(tmp_path / "a.tsv")).read()
    assert a == open(str(tmp_path / "b.tsv")).read() and len(a.split("\n")) == 28
