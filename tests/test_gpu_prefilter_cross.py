"""GPU: the cross form of the k-mer prefilter (lzani_prefilter_cross, lzani_prefilter_codes_cross) -- a query set against
a reference set -- against the numpy statement (tests/prefilter_cross_model.py) and against the all-pairs form of the same
process restricted to the cross pairs; the row builder cross_rows through the pair engine against the oracle; the mode
`lz-ani query2ref` of the host binary against all2all.  Every comparison is total and exact."""
import os
import subprocess

import numpy as np
import pytest

import lzani_ctypes as L
import oracle as O
import prefilter_cross_model as XM
import prefilter_model as PM
import prefilter_pass_model as PP
import synth_genomes as SG
import util as U

pytestmark = pytest.mark.gpu

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
EXAMPLE = os.path.join(U.GOLD, "example", "multifasta.fna")
INDEX_FREE = "query,reference,qlen,rlen,tani,gani,ani,qcov,rcov,len_ratio,nt_match,nt_mismatch,num_alns"
SPLITS_A = (1, 40, 64, 100, 159)            # of a run of 158 postings: its first posting, inside its first wave, a wave
                                            # boundary, its second wave, its last posting
THRESHOLDS = ((1, 0.0), (3, 0.2))           # 0.2 is selective: the common block alone gives ratios of about 0.12 .. 0.27


def _rc(s):
    return (3 - s[::-1]).astype(np.uint8)


def _rand(seed, n):
    return (SG.splitmix64(seed, np.arange(n, dtype=np.uint64)) % np.uint64(4)).astype(np.uint8)


def set_a():
    """160 genomes of 400-900 random bases that all hold one common block of 120 bases at a seeded offset, the odd ids as
    it is and the even ids its reverse complement: its k-mers are runs of 158 postings, longer than two waves.  Genome 7
    is all N, genome 150 is 9 bases (shorter than every k), genome 151 a copy of genome 3."""
    block = _rand(500, 120)
    seqs = []
    for g in range(160):
        n = 400 + int(SG.splitmix64(900, np.array([g], dtype=np.uint64))[0] % np.uint64(501))
        s = _rand(1000 + g, n)
        off = int(SG.splitmix64(901, np.array([g], dtype=np.uint64))[0] % np.uint64(n - 120))
        s[off:off + 120] = block if g % 2 else _rc(block)
        seqs.append(s)
    seqs[7] = np.full(300, 5, dtype=np.uint8)
    seqs[150] = _rand(77, 9)
    seqs[151] = seqs[3].copy()
    return seqs


def set_b():
    """The 102 genomes of tests/test_gpu_prefilter.py: 96 of 3-6 kbp in families of 8, an all-N genome, one shorter than
    every k, a reverse-complement copy, one with N runs, and the pair (100, 101) that shares exactly half of the smaller
    k-mer set at k = 21."""
    _, seqs = SG.make_set(96, 11, lmin=3000, lmax=6000, fam=8)
    seqs = [np.array(s) for s in seqs]
    seqs.append(np.full(200, 5, dtype=np.uint8))
    seqs.append(_rand(71, 6))
    seqs.append(_rc(seqs[3]))
    g = seqs[9].copy()
    g[100:140] = 5
    g[1000:1003] = 4
    g[-5:] = 5
    seqs.append(g)
    x = _rand(72, 1000)
    seqs.append(x)
    seqs.append(np.concatenate((x[:510], np.full(1, 5, dtype=np.uint8), _rand(73, 600))))
    return seqs


SETS = {"A": (set_a, SPLITS_A), "B": (set_b, (101,))}
_engines = {}
_model_cache = {}


@pytest.fixture(scope="module")
def engines():
    """name -> (seqs, engine holding them); made on first use, closed at the end of the module."""
    def get(name):
        if name not in _engines:
            seqs = SETS[name][0]()
            eng = L.Engine()
            eng.set_genomes(seqs)
            _engines[name] = (seqs, eng)
        return _engines[name]
    yield get
    for _, eng in _engines.values():
        eng.close()
    _engines.clear()


def _model(name, seqs, k, smax):
    key = (name, k, smax)
    if key not in _model_cache:
        _model_cache[key] = PM.shared_matrix(seqs, k, smax)
    return _model_cache[key]


def _same(got, want, what):
    for name, g, w in zip(("kmers_of", "row_off", "ids", "shared"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, g[:8], w[:8])


def _check_cross_info(eng, n, n_ref):
    ci = eng.prefilter_cross_info()
    assert (ci["n_ref"], ci["n_query"]) == (n_ref, n - n_ref)
    assert 1 <= ci["tile_rows"] <= n_ref and ci["matrix_bytes"] == ci["tile_rows"] * ci["n_query"] * 4
    return ci


@pytest.mark.parametrize("smax", [PM.SAMPLE_ALL, 1 << 62])
@pytest.mark.parametrize("k", [8, 16, 21, 31])
@pytest.mark.parametrize("name", ["A", "B"])
def test_cross_equals_the_model_and_the_restricted_all_pairs_result(engines, name, k, smax):
    seqs, eng = engines(name)
    n = len(seqs)
    kmers_of, shared = _model(name, seqs, k, smax)
    if name == "A" and smax == PM.SAMPLE_ALL and k in (8, 16, 31):         # the common block's runs of 158 postings
        sets = np.concatenate([PM.kmer_set(s, k) for s in seqs])
        _, c = np.unique(sets, return_counts=True)
        assert int((c == 158).sum()) == {8: 113, 16: 105, 31: 90}[k] and c.max() == 158
    for min_shared, min_ratio in THRESHOLDS + (((1, 0.5),) if name == "B" and k == 21 else ()):
        all_want = (kmers_of.astype(np.uint32),) + PM.kept_pairs(kmers_of, shared, min_shared, min_ratio)
        assert eng.prefilter(k, smax, min_shared, min_ratio) == len(all_want[2])
        all_got = eng.prefilter_fetch()
        _same(all_got, all_want, (name, k, smax, min_shared, min_ratio, "all pairs"))
        if name == "A" and k == 16 and smax == PM.SAMPLE_ALL and (min_shared, min_ratio) == (1, 0.0):
            assert len(all_want[2]) == 12403
        for n_ref in SETS[name][1]:
            what = (name, k, smax, min_shared, min_ratio, n_ref)
            want = (all_want[0],) + XM.kept_pairs(kmers_of, shared, n_ref, min_shared, min_ratio)
            cnt = eng.prefilter_cross(k, n_ref, smax, min_shared, min_ratio)
            got = eng.prefilter_fetch()
            _same(got, want, what)
            _same(got, (all_got[0],) + XM.restrict(all_got[1], all_got[2], all_got[3], n_ref), what + ("restricted all pairs",))
            assert np.array_equal(got[1][n_ref:], np.full(n - n_ref + 1, cnt, dtype=np.uint64))       # empty rows from n_ref on
            info = eng.prefilter_info()
            assert cnt == len(want[2]) == info["entries"] and info["k"] == k and info["tiles"] == 1, what
            assert info["postings"] == int(kmers_of.sum())
            assert _check_cross_info(eng, n, n_ref)["tile_rows"] == n_ref
            if name == "A" and k == 16 and smax == PM.SAMPLE_ALL and (min_shared, min_ratio) == (1, 0.0):
                assert cnt == {1: 157, 40: 4641, 64: 5985, 100: 5841, 159: 157}[n_ref]
            if name == "B" and k == 21 and smax == PM.SAMPLE_ALL and min_ratio == 0.5:
                assert (kmers_of[100], kmers_of[101], shared[100, 101]) == (980, 1070, 490)
                assert got[2][int(got[1][100]):int(got[1][101])].tolist() == [101]      # the exact-half pair straddles the split


def _cross_want(name, seqs, k, smax, n_ref, min_shared, min_ratio):
    kmers_of, shared = _model(name, seqs, k, smax)
    return (kmers_of.astype(np.uint32),) + XM.kept_pairs(kmers_of, shared, n_ref, min_shared, min_ratio)


@pytest.mark.parametrize("n_ref", [40, 159])
@pytest.mark.parametrize("rows", [1, 7])
def test_forced_tiles(engines, monkeypatch, rows, n_ref):
    seqs, eng = engines("A")
    monkeypatch.setenv("LZANI_PREFILTER_TILE_ROWS", str(rows))
    for k, smax, (min_shared, min_ratio) in ((16, PM.SAMPLE_ALL, THRESHOLDS[0]), (8, 1 << 62, THRESHOLDS[1])):
        eng.prefilter_cross(k, n_ref, smax, min_shared, min_ratio)
        _same(eng.prefilter_fetch(), _cross_want("A", seqs, k, smax, n_ref, min_shared, min_ratio), (rows, n_ref, k))
        assert eng.prefilter_info()["tiles"] == (n_ref + rows - 1) // rows
        assert eng.prefilter_pass_info()["key_sweeps"] == 3               # one pass: every tile counts from the same postings
        assert _check_cross_info(eng, len(seqs), n_ref)["tile_rows"] == min(rows, n_ref)
    monkeypatch.setenv("LZANI_PREFILTER_TILE_ROWS", "1000")                  # above n_ref: clipped to it
    eng.prefilter_cross(16, n_ref)
    assert _check_cross_info(eng, len(seqs), n_ref)["tile_rows"] == n_ref and eng.prefilter_info()["tiles"] == 1


@pytest.mark.parametrize("n_ref", [40, 100])
def test_forced_passes_and_tiles(engines, monkeypatch, n_ref):
    seqs, eng = engines("A")
    monkeypatch.setenv("LZANI_PREFILTER_PASSES", "3")
    monkeypatch.setenv("LZANI_PREFILTER_TILE_ROWS", "7")
    for k, (min_shared, min_ratio) in ((16, THRESHOLDS[0]), (31, THRESHOLDS[1])):
        windows = PP.pass_windows(PP.histogram(seqs, k, PM.SAMPLE_ALL), PP.forced_plan(3))
        eng.prefilter_cross(k, n_ref, PM.SAMPLE_ALL, min_shared, min_ratio)
        _same(eng.prefilter_fetch(), _cross_want("A", seqs, k, PM.SAMPLE_ALL, n_ref, min_shared, min_ratio), (n_ref, k))
        assert eng.prefilter_pass_info()["passes"] == 3 and eng.prefilter_info()["tiles"] == (n_ref + 6) // 7
        assert eng.prefilter_pass_info()["key_sweeps"] == PP.key_sweeps((n_ref + 6) // 7, windows)
        assert eng.prefilter_info()["postings"] == int(_model("A", seqs, k, PM.SAMPLE_ALL)[0].sum())
        _check_cross_info(eng, len(seqs), n_ref)


def test_streamed_cross_and_the_contexts_own_set(monkeypatch):
    seqs = set_a()
    n, k, slice_bytes = len(seqs), 16, 20000
    ns, slice_of = L.plan_slices([len(s) for s in seqs], slice_bytes)
    _, own = SG.make_set(12, 7, lmin=3000, lmax=5000, fam=4)
    own.append(np.full(100, 5, dtype=np.uint8))
    rows = L.cross_rows(len(own), 5)
    eng = L.Engine()
    try:
        eng.set_genomes(own)
        before = eng.run_rows(*rows)
        lay0, res0 = eng.layout(), eng.residency()
        for n_ref in (40, 100):
            assert ns >= 4 and slice_of[n_ref - 1] == slice_of[n_ref]      # several slices, none of them ends at the split
            for passes in (None, "3"):
                if passes:
                    monkeypatch.setenv("LZANI_PREFILTER_PASSES", passes)
                else:
                    monkeypatch.delenv("LZANI_PREFILTER_PASSES", raising=False)
                for min_shared, min_ratio in THRESHOLDS:
                    cnt = eng.prefilter_codes_cross(seqs, k, n_ref, PM.SAMPLE_ALL, min_shared, min_ratio, slice_bytes=slice_bytes)
                    want = _cross_want("A", seqs, k, PM.SAMPLE_ALL, n_ref, min_shared, min_ratio)
                    _same(eng.prefilter_fetch(), want, (n_ref, passes, min_shared, min_ratio))
                    assert cnt == len(want[2]) == eng.prefilter_info()["entries"]
                    assert eng.prefilter_stream_info()["slices"] == ns and eng.prefilter_pass_info()["passes"] == (3 if passes else 1)
                    _check_cross_info(eng, n, n_ref)
                assert eng.layout() == lay0 and eng.residency() == res0
        monkeypatch.delenv("LZANI_PREFILTER_PASSES", raising=False)
        assert np.array_equal(eng.run_rows(*rows), before)
        assert eng.layout()["bytes_genomes"] == lay0["bytes_genomes"] and eng.residency()["blocks"] == res0["blocks"]
    finally:
        eng.close()


def test_edges():
    seqs = set_a()[:12]
    eng = L.Engine()
    try:
        eng.set_genomes(seqs)
        assert eng.prefilter_cross(16, 5) > 0
        for bad in (0, len(seqs)):
            with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
                eng.prefilter_cross(16, bad)
            with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):     # the failed call left no result
                eng.prefilter_fetch()
            with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
                eng.prefilter_cross_info()
            with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
                eng.prefilter_codes_cross(seqs, 16, bad)
            with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
                eng.prefilter_fetch()
        assert eng.prefilter(16) > 0
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):         # an all-pairs result is no cross result
            eng.prefilter_cross_info()
        eng.prefilter_codes(seqs, 16)
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            eng.prefilter_cross_info()
        # two genomes
        two = [seqs[1], seqs[3]]
        eng.set_genomes(two)
        assert eng.prefilter_cross(16, 1) == 1
        _same(eng.prefilter_fetch(), XM.prefilter_cross(two, 16, 1), "two genomes")
        assert eng.prefilter_cross_info() == dict(n_ref=1, n_query=1, tile_rows=1, matrix_bytes=4)
        assert eng.prefilter_codes_cross(two, 16, 1) == 1
        _same(eng.prefilter_fetch(), XM.prefilter_cross(two, 16, 1), "two genomes, streamed")
        # no window is kept: all N, and shorter than k
        none = [np.full(50, 5, dtype=np.uint8), _rand(3, 12), np.full(20, 4, dtype=np.uint8)]
        eng.set_genomes(none)
        for run in (lambda: eng.prefilter_cross(16, 2), lambda: eng.prefilter_codes_cross(none, 16, 2)):
            assert run() == 0
            got = eng.prefilter_fetch()
            assert got[0].tolist() == [0, 0, 0] and got[1].tolist() == [0, 0, 0, 0] and len(got[2]) == 0 and len(got[3]) == 0
            info, ci = eng.prefilter_info(), eng.prefilter_cross_info()
            assert (info["positions"], info["postings"], info["entries"], info["tiles"]) == (0, 0, 0, 0)
            assert ci == dict(n_ref=2, n_query=1, tile_rows=0, matrix_bytes=0)
    finally:
        eng.close()


def test_cross_rows_through_the_pair_engine():
    seqs = set_b()[:24]
    n, n_ref = len(seqs), 10
    want = O.oracle_all2all(seqs, None, threads=8)
    ref_ids, row_off, query_ids = L.cross_rows(n, n_ref)
    eng = L.Engine()
    try:
        eng.set_genomes(seqs)
        got = eng.run_rows(ref_ids, row_off, query_ids)
        dense = eng.all2all()
        # the rows of the kept pairs of the cross prefilter, too
        eng.prefilter_cross(16, n_ref, min_ratio=0.05)
        _, pair_off, pair_ids, _ = eng.prefilter_fetch()
        kept_rows = L.cross_rows(n, n_ref, pair_off, pair_ids)
        got_kept = eng.run_rows(*kept_rows)
    finally:
        eng.close()
    r = np.repeat(ref_ids.astype(np.int64), np.diff(row_off.astype(np.int64)))
    q = query_ids.astype(np.int64)
    assert len(q) == 2 * n_ref * (n - n_ref) and ((r < n_ref) != (q < n_ref)).all()
    assert np.array_equal(got, want[r, q]) and np.array_equal(got, dense[r, q])
    assert (got[:, 0] > 0).any()
    r = np.repeat(kept_rows[0].astype(np.int64), np.diff(kept_rows[1].astype(np.int64)))
    q = kept_rows[2].astype(np.int64)
    assert 0 < len(q) == 2 * len(pair_ids) < 2 * n_ref * (n - n_ref) and np.array_equal(got_kept, want[r, q])


def test_binary_query2ref_against_all2all(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])
    recs = [b">" + x for x in open(EXAMPLE, "rb").read().split(b">")[1:]]
    ref, qry = str(tmp_path / "ref.fna"), str(tmp_path / "qry.fna")
    n_ref = 5                                           # the split of tests/test_host_cli_query2ref.py: inside the family of records 4 .. 6
    open(ref, "wb").write(b"".join(recs[:n_ref]))
    open(qry, "wb").write(b"".join(recs[n_ref:]))
    names, seqs = U.load_example()
    ref_names, n = set(names[:n_ref]), len(names)
    kmers_of, shared = PM.shared_matrix(seqs, 16)
    kept = len(XM.kept_pairs(kmers_of, shared, n_ref, 1, 0.1)[1])
    assert 0 < kept < n_ref * (n - n_ref)

    def lines(path, cross_only):
        out = [ln for ln in open(path).read().split("\n")[1:] if ln]
        if cross_only:
            out = [ln for ln in out if (ln.split("\t")[0] in ref_names) != (ln.split("\t")[1] in ref_names)]
        return sorted(out)

    for tag, extra, pairs in (("dense", [], n_ref * (n - n_ref)), ("flt", ["--flt-kmers", "16", "0.1"], kept)):
        q_out, a_out = str(tmp_path / (tag + ".q2r.tsv")), str(tmp_path / (tag + ".all.tsv"))
        p = subprocess.run([EXE, "query2ref", "--in-fasta", ref, "--query-fasta", qry, "-o", q_out, "-V", "2", "--out-format", INDEX_FREE] + extra,
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        assert "GPU 0: %d pairs" % (2 * pairs) in p.stderr, p.stderr[-2000:]
        if extra:
            assert "Filter size: %d" % (2 * pairs) in p.stderr, p.stderr[-2000:]
            assert "k-mer filter on device" in p.stderr and "; %d x %d" % (n_ref, n - n_ref) in p.stderr, p.stderr[-2000:]
        a = subprocess.run([EXE, "all2all", "--in-fasta", EXAMPLE, "-o", a_out, "--out-format", INDEX_FREE] + extra, capture_output=True, text=True)
        assert a.returncode == 0, a.stderr[-2000:]
        got = lines(q_out, False)
        assert got == lines(a_out, True) and len(got) == 2 * pairs
