"""GPU: the device k-mer prefilter (lzani_prefilter) against the numpy statement of its definitions
(tests/prefilter_model.py).  Every comparison is total and exact: kmers_of, row_off, ids and shared of the whole set."""
import os
import subprocess

import numpy as np
import pytest

import lzani_ctypes as L
import ooc_model as OM
import prefilter_model as PM
import synth_genomes as SG
import util as U

pytestmark = pytest.mark.gpu

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
HALF_K = 21                     # the k at which the planted pair below shares exactly half of the smaller k-mer set


def _rc(s):
    return (3 - s[::-1]).astype(np.uint8)


def _rand(seed, n):
    return (SG.splitmix64(seed, np.arange(n, dtype=np.uint64)) % np.uint64(4)).astype(np.uint8)


def small_set():
    """96 genomes of 3-6 kbp in families of 8, an all-N genome, one shorter than every k, an exact reverse-complement
    copy, one with N runs, and a pair X, Y with shared / min = 1/2 at k = 21: X is 1,000 random bases (980 windows), Y
    the first 510 of them (490 windows), an N, and 600 other random bases (580 windows)."""
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


@pytest.fixture(scope="module")
def small():
    seqs = small_set()
    eng = L.Engine()
    eng.set_genomes(seqs)
    yield seqs, eng
    eng.close()


_model_cache = {}


def _model(seqs, k, smax):
    key = (k, smax)
    if key not in _model_cache:
        _model_cache[key] = PM.shared_matrix(seqs, k, smax)
    return _model_cache[key]


def _same(got, want, what):
    for name, g, w in zip(("kmers_of", "row_off", "ids", "shared"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, g[:8], w[:8])


@pytest.mark.parametrize("smax", [PM.SAMPLE_ALL, 1 << 62])
@pytest.mark.parametrize("k", [8, 15, 16, 21, 31])
def test_small_set_equals_the_numpy_statement(small, k, smax):
    seqs, eng = small
    kmers_of, shared = _model(seqs, k, smax)
    n = len(seqs)
    assert kmers_of[96] == 0 and kmers_of[97] == 0                      # all N; shorter than k
    assert shared[3, 98] == kmers_of[3] == kmers_of[98] > 0              # the reverse-complement copy shares everything
    if k == HALF_K and smax == PM.SAMPLE_ALL:
        assert (kmers_of[100], kmers_of[101], shared[100, 101]) == (980, 1070, 490)      # exactly one half
    for min_shared in (1, 5):
        for min_ratio in (0.0, 0.5):
            want = (kmers_of.astype(np.uint32),) + PM.kept_pairs(kmers_of, shared, min_shared, min_ratio)
            cnt = eng.prefilter(k, smax, min_shared, min_ratio)
            got = eng.prefilter_fetch()
            _same(got, want, (k, smax, min_shared, min_ratio))
            info = eng.prefilter_info()
            assert cnt == len(want[2]) == info["entries"] and info["k"] == k and info["tiles"] == 1
            assert info["postings"] == int(kmers_of.sum())
            if k == HALF_K and smax == PM.SAMPLE_ALL:
                row = got[2][int(got[1][100]):int(got[1][101])]
                assert 101 in row.tolist()                                # a ratio equal to the threshold is kept
    assert n == 102


def test_forced_tiling_gives_the_same_result(small, monkeypatch):
    seqs, eng = small
    for k, smax, min_shared, min_ratio in ((16, PM.SAMPLE_ALL, 1, 0.0), (21, 1 << 62, 1, 0.5)):
        kmers_of, shared = _model(seqs, k, smax)
        want = (kmers_of.astype(np.uint32),) + PM.kept_pairs(kmers_of, shared, min_shared, min_ratio)
        monkeypatch.delenv("LZANI_PREFILTER_TILE_ROWS", raising=False)
        eng.prefilter(k, smax, min_shared, min_ratio)
        whole = eng.prefilter_fetch()
        assert eng.prefilter_info()["tiles"] == 1
        pi = eng.prefilter_pass_info()
        assert (pi["passes"], pi["key_sweeps"], pi["hist_ms"]) == (1, 3, 0)
        monkeypatch.setenv("LZANI_PREFILTER_TILE_ROWS", "7")
        eng.prefilter(k, smax, min_shared, min_ratio)
        tiled = eng.prefilter_fetch()
        assert eng.prefilter_info()["tiles"] == (len(seqs) + 6) // 7 > 1
        pi = eng.prefilter_pass_info()                                   # one pass: the tiles count from the same postings
        assert (pi["passes"], pi["key_sweeps"], pi["hist_ms"]) == (1, 3, 0)
        _same(tiled, whole, "tiled against whole")
        _same(tiled, want, "tiled against the model")


def test_larger_family_set():
    """2,000 genomes of 36-44 kbp in families of 50, k = 21, every fifth k-mer: about 16 M postings.  The generator's
    divergence is at most 10 % from the ancestor here: the numpy statement then gives every same-family pair at least 43
    shared sampled 21-mers and a ratio of at least 0.0058 (at 15 % some same-family pairs share none), and 201 pairs of
    different families share at least one.  Thresholds of 5 shared k-mers and a ratio of 0.003 sit between the two."""
    n, fam = 2000, 50
    _, seqs = SG.make_set(n, 5, fam=fam, dmax=0.10)
    smax = L.sample_max_of(0.2)
    kmers_of, shared = PM.shared_matrix(seqs, 21, smax)
    want = (kmers_of.astype(np.uint32),) + PM.kept_pairs(kmers_of, shared, 5, 0.003)
    a = np.repeat(np.arange(n), np.diff(want[1]).astype(np.int64))
    same = a // fam == want[2].astype(np.int64) // fam
    assert int(same.sum()) == n * (fam - 1) // 2                         # every same-family pair is kept
    assert int((~same).sum()) < 0.01 * len(same)
    eng = L.Engine()
    try:
        eng.set_genomes(seqs)
        eng.prefilter(21, smax, 5, 0.003)
        got = eng.prefilter_fetch()
        info = eng.prefilter_info()
    finally:
        eng.close()
    print("larger set:", info)
    _same(got, want, "2000 genomes")
    assert info["postings"] == int(kmers_of.sum()) > 15_000_000


def test_context_untouched():
    _, seqs = SG.make_set(12, 7, lmin=3000, lmax=5000, fam=4)
    seqs.append(np.full(100, 5, dtype=np.uint8))
    eng = L.Engine()
    try:
        eng.set_genomes(seqs)
        before = eng.all2all()
        lay0 = eng.layout()
        eng.prefilter(16)
        lay1 = eng.layout()
        after = eng.all2all()
        eng.prefilter(21, 1 << 63, 2, 0.1)
        again = eng.all2all()
    finally:
        eng.close()
    assert np.array_equal(before, after) and np.array_equal(before, again)
    assert lay0["bytes_genomes"] == lay1["bytes_genomes"] and lay0["slots"] == lay1["slots"]


def test_error_paths():
    _, seqs = SG.make_set(8, 3, lmin=3000, lmax=4000, fam=4)
    eng = L.Engine()
    try:
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            eng.prefilter(21)
        eng.set_genomes(seqs)
        for k in (7, 32):
            with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
                eng.prefilter(k)
        for ratio in (float("nan"), -0.5):
            with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
                eng.prefilter(21, min_ratio=ratio)
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            eng.prefilter_fetch()
        assert eng.prefilter(21) > 0
    finally:
        eng.close()
    eng = L.Engine()
    try:
        eng.set_genome_memory(4 * max(OM.genome_bytes(len(s), None, False) for s in seqs))     # blocks of two genomes
        eng.set_genomes(seqs)
        assert eng.residency()["blocks"] > 1
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            eng.prefilter(21)
        ooc = eng.all2all()
    finally:
        eng.close()
    eng = L.Engine()
    try:
        eng.set_genomes(seqs)
        assert np.array_equal(eng.all2all(), ooc)
    finally:
        eng.close()


def test_binary_builds_the_filter_a_kmerdb_file_would_give(tmp_path):
    """`lz-ani --flt-kmers k thr` against `--flt-kmerdb file thr` with the file written from the numpy statement's values
    (the ratio shared / min as repr prints it): the TSV and the ids file are byte-identical."""
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])
    names, seqs = SG.make_set(24, 13, lmin=3000, lmax=6000, fam=6)
    seqs.append(_rc(seqs[2]))
    names.append("rc_of_2")
    k, thr = 15, 0.1
    kmers_of, shared = PM.shared_matrix(seqs, k)
    n = len(seqs)
    a, b = np.triu_indices(n, 1)
    s = shared[a, b]
    val = s[s > 0] / np.minimum(kmers_of[a], kmers_of[b])[s > 0]
    assert np.abs(val - thr).min() > 1e-9 and (val >= thr).any() and (val < thr).any()
    fa, flt = str(tmp_path / "in.fa"), str(tmp_path / "flt.txt")
    SG.write_fasta(fa, names, seqs)
    with open(flt, "w") as f:
        f.write("kmer-length: %d fraction: 1 ,%s,\n" % (k, ",".join(names)))
        for i in range(n):
            cells = ["%d:%s" % (j + 1, repr(float(shared[i, j] / min(kmers_of[i], kmers_of[j])))) for j in range(i + 1, n) if shared[i, j] > 0]
            f.write(",".join([names[i]] + cells) + "\n")
    outs = []
    for tag, extra in (("file", ["--flt-kmerdb", flt, repr(thr)]), ("device", ["--flt-kmers", str(k), repr(thr)])):
        out = str(tmp_path / (tag + ".tsv"))
        p = subprocess.run([EXE, "all2all", "--in-fasta", fa, "-o", out, "-V", "2", "--out-format", "complete"] + extra,
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        assert "Filter size: %d" % (2 * int((val >= thr).sum())) in p.stderr, p.stderr[-2000:]
        outs.append((open(out, "rb").read(), open(str(tmp_path / (tag + ".ids.tsv")), "rb").read()))
        if tag == "device":
            assert "k-mer filter on device" in p.stderr and "K-mer filter :" in p.stderr
    assert outs[0] == outs[1] and outs[0][0].count(b"\n") > 1
