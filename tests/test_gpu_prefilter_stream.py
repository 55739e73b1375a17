"""GPU: the streamed k-mer prefilter (lzani_prefilter_codes) -- genomes from host memory through a staging buffer, slice by
slice -- against the numpy statement of the definitions (tests/prefilter_model.py) and against lzani_prefilter on the same
set held in-core.  Every comparison is total and exact.  The set is the smallest that can break the key kernel: lengths
around its chunk of 4,096 positions and around k, N's at the chunk boundary, genomes at odd byte offsets of the buffer."""
import os
import subprocess

import numpy as np
import pytest

import lzani_ctypes as L
import ooc_model as M
import prefilter_model as PM
import synth_genomes as SG
import util as U

pytestmark = pytest.mark.gpu

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
CHUNK = 4096                    # PF_CHUNK
KS = (8, 16, 21, 31)


def _rc(s):
    return (3 - s[::-1]).astype(np.uint8)


def _rand(seed, n):
    return (SG.splitmix64(seed, np.arange(n, dtype=np.uint64)) % np.uint64(4)).astype(np.uint8)


def edge_set(k):
    """31 genomes.  Id 0 is the longest, 8,197 (alone in a slice of 8,197 bytes); then k - 1, an empty genome, k and the
    lengths around the chunk; twelve 3-6 kbp genomes in families of four; an all-N genome; N at positions 4095 and 4096 of
    an 8,000-long genome; an N run at the end of a genome that ends just
    behind a chunk; the reverse complement of a family member; and a pair whose second genome starts with the k-mer the
    first one -- which ends inside the halo of its only chunk -- ends with."""
    seqs = [_rand(901, 8197), _rand(909, k - 1), _rand(900, 0)]
    for i, n in enumerate((k, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + k - 2, CHUNK + k - 1)):
        seqs.append(_rand(910 + i, n))
    _, fam = SG.make_set(12, 17, lmin=3000, lmax=6000, fam=4)
    seqs += [np.array(s, dtype=np.uint8) for s in fam]
    seqs.append(np.full(300, 5, dtype=np.uint8))
    g = _rand(920, 8000)
    g[CHUNK - 1] = 4
    g[CHUNK] = 7
    seqs.append(g)
    g = _rand(921, CHUNK + 40)
    g[-45:] = 5
    seqs.append(g)
    seqs.append(_rc(seqs[11]))
    a = _rand(922, CHUNK - 6)
    seqs.append(a)
    seqs.append(np.concatenate((a[-k:], _rand(923, 2500))))
    seqs.append(_rand(924, 3))
    seqs.append(_rand(925, 5000))
    seqs.append(np.concatenate((_rand(926, 700), seqs[9][100:2100], _rand(927, 333))))      # shares 2,000 bases with a family member
    seqs.append(_rand(928, 2 * CHUNK))                                                     # two whole chunks
    assert len(seqs) == 31
    return seqs


_sets, _engines, _models, _sizes = {}, {}, {}, {}


def slice_sizes(k):
    """The three slice plans of the tests: everything in one slice; 8,197 bytes (many slices, the longest genome alone);
    the smallest size from a third of the set on that gives three slices."""
    if k not in _sizes:
        lens = [len(s) for s in the_set(k)]
        total = sum(lens)
        three = next(sb for sb in range(max(max(lens), total // 3), total) if L.plan_slices(lens, sb)[0] == 3)
        _sizes[k] = dict(one=total, many=8197, three=three)
    return _sizes[k]


def the_set(k):
    if k not in _sets:
        _sets[k] = edge_set(k)
    return _sets[k]


@pytest.fixture(scope="module")
def resident():
    """A second context per k that holds the set in-core, for lzani_prefilter."""
    def get(k):
        if k not in _engines:
            _engines[k] = L.Engine()
            _engines[k].set_genomes(the_set(k))
        return _engines[k]
    yield get
    for e in _engines.values():
        e.close()
    _engines.clear()


@pytest.fixture(scope="module")
def streamer():
    eng = L.Engine()                   # holds no genome set at all
    yield eng
    eng.close()


def model(k, smax):
    if (k, smax) not in _models:
        _models[(k, smax)] = PM.shared_matrix(the_set(k), k, smax)
    return _models[(k, smax)]


def _same(got, want, what):
    for name, g, w in zip(("kmers_of", "row_off", "ids", "shared"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, g[:8], w[:8])


COUNTS = ("k", "positions", "distinct_kmers", "postings", "entries")


def staged_bytes_of(lens, slice_of, ns, sweeps=3):
    """Bytes of the slices copied: up, down without the last, up without the first."""
    b = np.bincount(slice_of, weights=lens, minlength=ns).astype(np.int64)
    if sweeps == 1 or ns == 1:
        return int(b.sum())
    return int(3 * b.sum() - b[-1] - b[0])


@pytest.mark.parametrize("plan", ["one", "many", "three"])
@pytest.mark.parametrize("smax", [PM.SAMPLE_ALL, 1 << 62])
@pytest.mark.parametrize("k", KS)
def test_streamed_equals_the_numpy_statement_and_the_resident_prefilter(streamer, resident, k, smax, plan):
    seqs = the_set(k)
    lens = [len(s) for s in seqs]
    sb = slice_sizes(k)[plan]
    ns, slice_of = L.plan_slices(lens, sb)
    assert {"one": ns == 1, "many": ns > 8 and (slice_of == 0).sum() == 1, "three": ns == 3}[plan]
    kmers_of, shared = model(k, smax)
    assert kmers_of[1] == kmers_of[2] == kmers_of[21] == 0                               # k - 1 long, empty, all N
    assert kmers_of[3] == 1 if smax == PM.SAMPLE_ALL else kmers_of[3] <= 1               # k long: one window
    assert shared[11, 24] == kmers_of[11] == kmers_of[24] > 0                            # the reverse-complement copy
    res = resident(k)
    for min_shared, min_ratio in ((1, 0.0), (3, 0.05)):
        want = (kmers_of.astype(np.uint32),) + PM.kept_pairs(kmers_of, shared, min_shared, min_ratio)
        cnt = streamer.prefilter_codes(seqs, k, smax, min_shared, min_ratio, slice_bytes=sb)
        got = streamer.prefilter_fetch()
        _same(got, want, (k, smax, plan, "model"))
        assert cnt == len(want[2]) > 0
        res.prefilter(k, smax, min_shared, min_ratio)
        _same(got, res.prefilter_fetch(), (k, smax, plan, "resident"))
        a, b = streamer.prefilter_info(), res.prefilter_info()
        assert [a[f] for f in COUNTS] == [b[f] for f in COUNTS] and a["postings"] == int(kmers_of.sum()) and a["positions"] > 0
        si = streamer.prefilter_stream_info()
        assert si["slices"] == ns and si["slice_uploads"] == 3 * ns - 2
        assert si["staged_bytes"] == staged_bytes_of(lens, slice_of, ns)
        assert 0 < si["stage_bytes"] <= sb and si["stage_bytes"] == np.bincount(slice_of, weights=lens).max()


def test_no_kept_window_runs_the_count_sweep_only(streamer):
    k = 16
    seqs = [_rand(950 + i, n) for i, n in enumerate((15, 0, 7, 15, 1, 15, 14, 0, 15))] + [np.full(40, 4, dtype=np.uint8)]
    lens = [len(s) for s in seqs]
    ns, slice_of = L.plan_slices(lens, 40)
    assert ns == 4
    assert streamer.prefilter_codes(seqs, k, slice_bytes=40) == 0
    kmers_of, row_off, ids, shared = streamer.prefilter_fetch()
    assert kmers_of.tolist() == [0] * 10 and row_off.tolist() == [0] * 11 and len(ids) == len(shared) == 0
    info, si = streamer.prefilter_info(), streamer.prefilter_stream_info()
    assert (info["positions"], info["distinct_kmers"], info["postings"], info["entries"]) == (0, 0, 0, 0)
    assert si["slices"] == si["slice_uploads"] == ns and si["staged_bytes"] == sum(lens)
    # not one base at all
    assert streamer.prefilter_codes([_rand(1, 0), _rand(2, 0)], k) == 0
    assert streamer.prefilter_stream_info()["slice_uploads"] == 1 and len(streamer.prefilter_fetch()[0]) == 2


def test_forced_tiling_with_several_slices_gives_the_same_result(streamer, monkeypatch):
    k, smax = 21, 1 << 62
    seqs = the_set(k)
    lens = [len(s) for s in seqs]
    kmers_of, shared = model(k, smax)
    want = (kmers_of.astype(np.uint32),) + PM.kept_pairs(kmers_of, shared, 1, 0.0)
    monkeypatch.setenv("LZANI_PREFILTER_TILE_ROWS", "7")
    streamer.prefilter_codes(seqs, k, smax, slice_bytes=slice_sizes(k)["three"])
    assert streamer.prefilter_info()["tiles"] == (len(seqs) + 6) // 7 and streamer.prefilter_stream_info()["slices"] == 3
    _same(streamer.prefilter_fetch(), want, "tiled, three slices")
    # one pass: the tiles count from the same postings, so the sweeps and the uploads are those of the untiled run
    assert streamer.prefilter_pass_info()["key_sweeps"] == 3 and streamer.prefilter_stream_info()["slice_uploads"] == 3 * 3 - 2
    # the environment's slice size overrides the argument
    monkeypatch.setenv("LZANI_PREFILTER_SLICE_BYTES", "8197")
    streamer.prefilter_codes(seqs, k, smax, slice_bytes=sum(lens))
    si = streamer.prefilter_stream_info()
    assert si["slices"] == L.plan_slices(lens, 8197)[0]
    assert streamer.prefilter_pass_info()["key_sweeps"] == 3 and si["slice_uploads"] == 3 * si["slices"] - 2
    _same(streamer.prefilter_fetch(), want, "tiled, many slices")


@pytest.mark.parametrize("ooc", [False, True])
def test_the_contexts_own_set_is_untouched(ooc):
    """A context with a genome set of its own, in-core or out-of-core in three blocks: the streamed prefilter of OTHER
    genomes (another n) leaves its results, its layout and its residency as they were, and fetch is sized by the
    prefilter's n; the next lzani_set_genomes clears the result."""
    _, own = SG.make_set(12, 7, lmin=3000, lmax=5000, fam=4)
    own.append(np.full(100, 5, dtype=np.uint8))
    k = 16
    seqs = the_set(k)
    lens = [len(s) for s in seqs]
    kmers_of, shared = model(k, PM.SAMPLE_ALL)
    want = (kmers_of.astype(np.uint32),) + PM.kept_pairs(kmers_of, shared, 1, 0.0)
    eng = L.Engine()
    try:
        if ooc:
            eng.set_genome_memory(M.limit_for_blocks([len(s) for s in own], None, 3))
        eng.set_genomes(own)
        before = eng.all2all()
        lay0, res0 = eng.layout(), eng.residency()
        assert res0["blocks"] == (3 if ooc else 1)
        eng.prefilter_codes(seqs, k, slice_bytes=slice_sizes(k)["three"])
        assert eng.layout() == lay0 and eng.residency() == res0
        got = eng.prefilter_fetch()
        assert len(got[0]) == len(seqs) != len(own) and len(got[1]) == len(seqs) + 1
        _same(got, want, "with a set of its own")
        after = eng.all2all()
        assert np.array_equal(before, after)
        assert eng.residency()["blocks"] == res0["blocks"] and eng.layout()["bytes_genomes"] == lay0["bytes_genomes"]
        _same(eng.prefilter_fetch(), want, "after a run")                  # the result outlives a run
        if ooc:
            with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):     # lzani_prefilter still refuses the out-of-core set
                eng.prefilter(k)
        eng.set_genomes(own)
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            eng.prefilter_fetch()
        with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
            eng.prefilter_stream_info()
    finally:
        eng.close()


def test_error_paths(streamer, resident):
    seqs = the_set(16)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG.*minimum of 8197 bytes"):
        streamer.prefilter_codes(seqs, 16, slice_bytes=8196)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):           # a failed call leaves no result
        streamer.prefilter_fetch()
    for k in (7, 32):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            streamer.prefilter_codes(seqs, k)
    for ratio in (float("nan"), -0.5):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            streamer.prefilter_codes(seqs, 16, min_ratio=ratio)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        streamer.prefilter_codes([], 16)
    lens = np.array([4], dtype=np.uint32)
    assert streamer.lib.lzani_prefilter_codes(streamer.h, 1, None, lens.ctypes.data, 16, 0, 1, 0.0, 0, None) == -1
    assert streamer.lib.lzani_prefilter_codes(None, 1, None, lens.ctypes.data, 16, 0, 1, 0.0, 0, None) == -1
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        streamer.prefilter_stream_info()
    res = resident(16)
    res.prefilter(16)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):           # a plain lzani_prefilter's result is not a streamed one
        res.prefilter_stream_info()
    assert streamer.prefilter_codes(seqs, 16) > 0 and streamer.prefilter_stream_info()["slices"] == 1      # automatic slice size


def test_binary_streams_the_filter_under_gpu_mem(tmp_path):
    """`lz-ani --flt-kmers 15 0.1 --gpu-mem <limit>`, the filter's slices forced down to at least three: TSV and ids file
    byte-identical to the run without --gpu-mem."""
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])
    names, seqs = SG.make_set(24, 13, lmin=3000, lmax=6000, fam=6)
    seqs.append(_rc(seqs[2]))
    names.append("rc_of_2")
    fa = str(tmp_path / "in.fa")
    SG.write_fasta(fa, names, seqs)
    lens = [len(s) for s in U.reorder(names, seqs)[1]]                  # (the ids of the binary)
    limit = M.limit_for_blocks(lens, None, 3)
    sb = sum(lens) // 3
    ns = L.plan_slices(lens, sb)[0]
    assert ns >= 3 and sb < limit
    outs = []
    for tag, extra, env in (("plain", [], {}), ("mem", ["--gpu-mem", str(limit)], {"LZANI_PREFILTER_SLICE_BYTES": str(sb)})):
        out = str(tmp_path / (tag + ".tsv"))
        p = subprocess.run([EXE, "all2all", "--in-fasta", fa, "-o", out, "-V", "2", "--out-format", "complete", "--flt-kmers", "15", "0.1"] + extra,
                           capture_output=True, text=True, env=dict(os.environ, **env))
        assert p.returncode == 0, p.stderr[-2000:]
        assert "k-mer filter on device" in p.stderr
        assert ("streamed: %d slice(s), %d upload(s)" % (ns, 3 * ns - 2) in p.stderr) == (tag == "mem"), p.stderr[-2000:]
        assert ("streamed: " in p.stderr) == (tag == "mem")
        outs.append((open(out, "rb").read(), open(str(tmp_path / (tag + ".ids.tsv")), "rb").read()))
    assert outs[0] == outs[1] and outs[0][0].count(b"\n") > 1
