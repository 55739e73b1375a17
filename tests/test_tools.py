"""CPU: the seeded workload generator is byte-stable, and bench.py's byte accounting is SURVEY 8(d)'s."""
import hashlib
import importlib.util
import os

import numpy as np

import shard as SH
import synth_genomes as SG
import util as U


def test_generator_is_byte_stable():
    names, seqs = SG.make_set(12, 1)
    assert names[0] == "g000000_f0_m0" and names[11] == "g000011_f1_m1"
    assert [len(s) for s in seqs[:4]] == [40307, 40278, 40461, 40500]
    h = hashlib.sha256(b"".join(s.tobytes() for s in seqs)).hexdigest()
    assert h == hashlib.sha256(b"".join(s.tobytes() for s in SG.make_set(12, 1)[1])).hexdigest()
    assert h != hashlib.sha256(b"".join(s.tobytes() for s in SG.make_set(12, 2)[1])).hexdigest()
    assert all(s.dtype == np.uint8 and s.max() <= 3 for s in seqs)
    # member 0 of a family is the ancestor, members differ from it by substitutions and indels
    same = (seqs[0][:100] == seqs[1][:100]).mean()          # before the first indel shifts the frame
    assert 0.7 < same <= 1.0 and not np.array_equal(seqs[0], seqs[1])


def test_splitmix_reference_values():
    # splitmix64 with seed 0: first outputs of the published sequence
    v = SG.splitmix64(0, np.arange(3, dtype=np.uint64))
    assert [int(x) for x in v] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def test_bench_algorithmic_bytes_formula():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(U.ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    prm = dict(mal=11, msl=7, mrd=40, mqd=40, reg=35, aw=15, am=7, ar=3)
    lens = np.array([40000, 40000], dtype=np.int64)
    # 10,000 + 20,030 + 160,120 + 12 = 190,162 B per directed pair at Lq = Lr = 40,000
    assert bench.algorithmic_bytes(lens, [0], prm) == 190162
    assert bench.algorithmic_bytes(lens, [0, 1], prm) == 2 * 190162
    assert bench.host_cores() >= 1


def test_bench_algorithmic_bytes_of_filtered_rows():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(U.ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    prm = dict(mal=11, msl=7, mrd=40, mqd=40, reg=35, aw=15, am=7, ar=3)
    lens = np.array([40000, 40000, 36000], dtype=np.int64)
    # rows (0: queries 1, 2), (2: query 0): the same B_pair per directed pair as the dense form
    got = bench.algorithmic_bytes_csr(lens, [0, 2], [0, 2, 3], [1, 2, 0], prm)
    qb, rb = bench.pair_bytes(lens, prm)
    assert got == int(2 * rb[0] + qb[1] + qb[2] + rb[2] + qb[0])
    assert bench.algorithmic_bytes_csr(lens[:2], [0], [0, 1], [1], prm) == 190162


def test_bench_dump_outputs_layout_and_sample(tmp_path, monkeypatch):
    """bench.py --dump-outputs: dense rows as written, and past the size limit a seeded sample whose ids follow the
    dense row layout (query j of reference r is j for j < r, else j + 1)."""
    spec = importlib.util.spec_from_file_location("bench", os.path.join(U.ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n, rows = 401, np.array([2, 250, 400], dtype=np.uint32)
    res = np.zeros((len(rows), n - 1, 3), dtype=np.int32)
    for i, r in enumerate(rows):
        for j in range(n - 1):
            res[i, j] = (r, j if j < r else j + 1, 40000 + i)
    bench.dump_outputs(str(tmp_path / "full"), res, rows)
    got = np.load(str(tmp_path / "full" / "results.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, res) and np.load(str(tmp_path / "full" / "ref_ids.npy")).tolist() == rows.tolist()
    assert sorted(os.listdir(str(tmp_path / "full"))) == ["ref_ids.npy", "results.npy"]
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096 + 10 * 36)          # (4 KB for the .npy headers, then 36 B a pair)
    for k in range(2):
        bench.dump_outputs(str(tmp_path / f"s{k}"), res, rows)
    s = [{f[:-4]: np.load(str(tmp_path / f"s{k}" / f)) for f in os.listdir(str(tmp_path / f"s{k}"))} for k in range(2)]
    assert sorted(s[0]) == ["query_ids", "ref_ids", "results", "sample_index"]
    assert all(np.array_equal(s[0][key], s[1][key]) for key in s[0])
    assert len(s[0]["results"]) == 10 and np.all(np.diff(s[0]["sample_index"]) > 0)
    assert np.array_equal(s[0]["results"][:, 0], s[0]["ref_ids"]) and np.array_equal(s[0]["results"][:, 1], s[0]["query_ids"])
    assert np.array_equal(s[0]["results"], res.reshape(-1, 3)[s[0]["sample_index"].astype(np.int64)])
    # filtered rows: one record per pair, both ids beside it
    bench.dump_outputs(str(tmp_path / "csr"), res[0], np.full(n - 1, 2), np.arange(n - 1))
    assert np.load(str(tmp_path / "csr" / "query_ids.npy")).dtype == np.float64


def test_integration_stub_compiles_against_the_reference_headers():
    """INTEGRATION.md section 1 (the replacement body of CLZMatcher::do_matching) is the text that was compiled against the
    reference's own headers (its digest in tests/golden/ref_live_vectors.json, written by oracle/make_goldens.py); where
    oracle/_ref is built (`make -C oracle ref`, part of build() where the reference's sources exist), the object compiled
    from it must come from the current INTEGRATION.md and define the method."""
    import subprocess
    import integration_stub as IS
    stub = IS.stub_source(os.path.join(U.ROOT, "INTEGRATION.md"))
    assert hashlib.sha256(stub.encode()).hexdigest() == U.load_ref_live()["integration_stub"]["sha256"], \
        "INTEGRATION.md section 1 changed: compile it against the reference's headers (make -C oracle ref) and rerun oracle/make_goldens.py"
    obj = os.path.join(U.ROOT, "oracle", "_ref", "integration_stub.o")
    if os.path.exists(obj):
        with open(os.path.join(U.ROOT, "oracle", "_ref", "integration_stub.cpp")) as f:
            assert f.read() == stub, "stale oracle/_ref: run build() again"
        syms = subprocess.run(["nm", "-C", "--defined-only", obj], capture_output=True, text=True, check=True).stdout
        assert "CLZMatcher::do_matching()" in syms, syms
