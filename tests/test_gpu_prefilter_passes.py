"""GPU: the prefilter in several k-mer passes (LZANI_PREFILTER_PASSES, LZANI_PREFILTER_MAX_WINDOWS) against the numpy
statement of the definitions (tests/prefilter_model.py, tests/prefilter_pass_model.py) and against the one-pass run of
the same context, byte for byte -- resident and streamed, with and without matrix tiles.  The set is small and has what a
pass boundary can get wrong: families whose k-mers must meet in one pass, genomes without a window in a pass, a genome
with a run of N, one shorter than k, an empty one, a reverse complement."""
import os
import subprocess

import numpy as np
import pytest

import lzani_ctypes as L
import ooc_model as M
import prefilter_model as PM
import prefilter_pass_model as PP
import synth_genomes as SG
import util as U

pytestmark = pytest.mark.gpu

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
FIFTH = L.sample_max_of(0.2)
ENV = ("LZANI_PREFILTER_PASSES", "LZANI_PREFILTER_MAX_WINDOWS", "LZANI_PREFILTER_TILE_ROWS", "LZANI_PREFILTER_SLICE_BYTES")
THRESHOLDS = ((1, 0.0), (3, 0.05))
COUNTS = ("k", "positions", "distinct_kmers", "postings", "entries")

_set, _models, _hists, _base = [], {}, {}, {}


def the_set():
    if not _set:
        _set.extend(PP.pass_set())
    return _set


def model(k, smax):
    """(kmers_of, shared matrix) of the numpy statement: computed once, never changed."""
    if (k, smax) not in _models:
        _models[(k, smax)] = PM.shared_matrix(the_set(), k, smax)
    return _models[(k, smax)]


def want_of(k, smax, min_shared, min_ratio):
    kmers_of, shared = model(k, smax)
    return (kmers_of.astype(np.uint32),) + PM.kept_pairs(kmers_of, shared, min_shared, min_ratio)


def hist_of(k, smax):
    if (k, smax) not in _hists:
        _hists[(k, smax)] = PP.histogram(the_set(), k, smax)
    return _hists[(k, smax)]


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def resident():
    eng = L.Engine()
    eng.set_genomes(the_set())
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def streamer():
    eng = L.Engine()                   # holds no genome set at all
    yield eng
    eng.close()


def baseline(eng, k, smax, min_shared, min_ratio):
    """The same context's result without any forced plan: one pass (the set is far below any cap)."""
    key = (k, smax, min_shared, min_ratio)
    if key not in _base:
        assert "LZANI_PREFILTER_PASSES" not in os.environ and "LZANI_PREFILTER_MAX_WINDOWS" not in os.environ
        eng.prefilter(k, smax, min_shared, min_ratio)
        pi = eng.prefilter_pass_info()
        assert pi["passes"] == 1 and pi["key_sweeps"] == 3 and pi["hist_ms"] == 0 and eng.prefilter_pass_plan().tolist() == [0, PP.BINS]
        _base[key] = (eng.prefilter_fetch(), eng.prefilter_info())
    return _base[key]


def _same(got, want, what):
    for name, g, w in zip(("kmers_of", "row_off", "ids", "shared"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, g[:8], w[:8])


def _bytes_equal(got, want, what):
    for name, g, w in zip(("kmers_of", "row_off", "ids", "shared"), got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, name)


def test_the_set_is_what_the_passes_need():
    seqs = the_set()
    lens = [len(s) for s in seqs]
    assert len(seqs) == 24 and lens[17] == 0 and lens[16] < 8 and (seqs[15] >= 4).sum() == 300
    assert 80000 < int(hist_of(21, PM.SAMPLE_ALL).sum()) < 100000
    kmers_of, shared = model(21, PM.SAMPLE_ALL)
    assert kmers_of[16] == kmers_of[17] == 0 and shared[6, 18] == kmers_of[6] == kmers_of[18] > 0
    assert shared[0, 1] > 0 and shared[5, 6] > 0 and shared[10, 11] > 0 and shared[0, 5] == 0
    # a forced plan of 4,096 passes would leave most passes empty and most genomes without a window in a pass; already
    # with 7 the two shortest genomes have none in any, and every pass holds windows of every family
    for k, smax in ((8, FIFTH), (21, PM.SAMPLE_ALL), (31, FIFTH)):
        assert min(PP.pass_windows(hist_of(k, smax), PP.forced_plan(7))) > 0


@pytest.mark.parametrize("P", [1, 2, 3, 7])
@pytest.mark.parametrize("smax", [PM.SAMPLE_ALL, FIFTH], ids=["all", "fifth"])
@pytest.mark.parametrize("k", [8, 21, 31])
def test_forced_passes_equal_the_numpy_statement_and_one_pass(resident, monkeypatch, k, smax, P):
    hist = hist_of(k, smax)
    plan = PP.forced_plan(P)
    windows = PP.pass_windows(hist, plan)
    for min_shared, min_ratio in THRESHOLDS:
        base, base_info = baseline(resident, k, smax, min_shared, min_ratio)
        monkeypatch.setenv("LZANI_PREFILTER_PASSES", str(P))
        cnt = resident.prefilter(k, smax, min_shared, min_ratio)
        monkeypatch.delenv("LZANI_PREFILTER_PASSES")
        got = resident.prefilter_fetch()
        want = want_of(k, smax, min_shared, min_ratio)
        _same(got, want, (k, smax, P, "model"))
        _bytes_equal(got, base, (k, smax, P, "one pass"))
        assert cnt == len(want[2]) > 0
        info, pi = resident.prefilter_info(), resident.prefilter_pass_info()
        assert pi["passes"] == P and resident.prefilter_pass_plan().tolist() == plan
        assert [info[f] for f in COUNTS] == [base_info[f] for f in COUNTS] and info["tiles"] == base_info["tiles"] == 1
        assert sum(windows) == info["positions"] > 0 and max(windows) == pi["largest_pass"]
        assert pi["key_sweeps"] == PP.key_sweeps(1, windows) and (pi["hist_ms"] > 0) == (P > 1)
        assert pi["workspace_bytes"] >= 24 * pi["largest_pass"]


@pytest.mark.parametrize("k,smax", [(21, PM.SAMPLE_ALL), (8, FIFTH)], ids=["k21-all", "k8-fifth"])
def test_automatic_plan_under_a_window_cap(resident, monkeypatch, k, smax):
    hist = hist_of(k, smax)
    cap = int(hist.sum()) // 7
    assert int(hist.max()) <= cap
    base, base_info = baseline(resident, k, smax, 1, 0.0)
    monkeypatch.setenv("LZANI_PREFILTER_MAX_WINDOWS", str(cap))
    resident.prefilter(k, smax, 1, 0.0)
    got = resident.prefilter_fetch()
    _same(got, want_of(k, smax, 1, 0.0), (k, "model"))
    _bytes_equal(got, base, (k, "one pass"))
    pi, info = resident.prefilter_pass_info(), resident.prefilter_info()
    plan = PP.plan(hist, cap)
    windows = PP.pass_windows(hist, plan)
    assert pi["passes"] == len(plan) - 1 >= 7 and resident.prefilter_pass_plan().tolist() == plan
    assert pi["cap"] == cap and pi["largest_pass"] == max(windows) <= cap
    assert pi["key_sweeps"] == PP.key_sweeps(1, windows) and pi["hist_ms"] > 0
    assert [info[f] for f in COUNTS] == [base_info[f] for f in COUNTS]
    # a cap the set fits: one pass, no histogram -- the variable is read, and a large value is not a plan
    monkeypatch.setenv("LZANI_PREFILTER_MAX_WINDOWS", str(int(hist.sum())))
    resident.prefilter(k, smax, 1, 0.0)
    pi = resident.prefilter_pass_info()
    assert (pi["passes"], pi["key_sweeps"], pi["cap"], pi["hist_ms"]) == (1, 3, int(hist.sum()), 0)
    _bytes_equal(resident.prefilter_fetch(), base, (k, "fits"))


def test_a_bin_above_the_cap_is_refused_and_the_context_unharmed(resident, monkeypatch):
    k, smax = 21, PM.SAMPLE_ALL
    base, _ = baseline(resident, k, smax, 1, 0.0)
    hist = hist_of(k, smax)
    bad = next(b for b in range(PP.BINS) if hist[b] > 1)
    monkeypatch.setenv("LZANI_PREFILTER_MAX_WINDOWS", "1")
    with pytest.raises(L.LzaniError, match=r"LZANI_ERR_ARG.*bin %d .* holds %d sampled" % (bad, int(hist[bad]))):
        resident.prefilter(k, smax, 1, 0.0)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):           # a failed call leaves no result
        resident.prefilter_fetch()
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        resident.prefilter_pass_info()
    monkeypatch.delenv("LZANI_PREFILTER_MAX_WINDOWS")
    for bad_p in ("0", "4097"):
        monkeypatch.setenv("LZANI_PREFILTER_PASSES", bad_p)
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG.*LZANI_PREFILTER_PASSES"):
            resident.prefilter(k, smax, 1, 0.0)
    monkeypatch.delenv("LZANI_PREFILTER_PASSES")
    resident.prefilter(k, smax, 1, 0.0)
    assert resident.prefilter_pass_info()["passes"] == 1
    _bytes_equal(resident.prefilter_fetch(), base, "after the refusals")


def test_matrix_tiles_with_passes(resident, monkeypatch):
    k, smax = 21, FIFTH
    windows = PP.pass_windows(hist_of(k, smax), PP.forced_plan(3))
    for min_shared, min_ratio in THRESHOLDS:
        base, base_info = baseline(resident, k, smax, min_shared, min_ratio)
        monkeypatch.setenv("LZANI_PREFILTER_TILE_ROWS", "7")
        monkeypatch.setenv("LZANI_PREFILTER_PASSES", "3")
        resident.prefilter(k, smax, min_shared, min_ratio)
        got = resident.prefilter_fetch()
        _same(got, want_of(k, smax, min_shared, min_ratio), "tiles and passes, model")
        _bytes_equal(got, base, "tiles and passes, one pass")
        info, pi = resident.prefilter_info(), resident.prefilter_pass_info()
        assert info["tiles"] == 4 and pi["passes"] == 3 and pi["key_sweeps"] == PP.key_sweeps(4, windows) == 38
        assert [info[f] for f in COUNTS] == [base_info[f] for f in COUNTS]          # the sums over one tile's passes
        monkeypatch.delenv("LZANI_PREFILTER_TILE_ROWS")
        monkeypatch.delenv("LZANI_PREFILTER_PASSES")


def three_slices():
    lens = [len(s) for s in the_set()]
    total = sum(lens)
    return next(sb for sb in range(max(max(lens), total // 3), total) if L.plan_slices(lens, sb)[0] == 3)


@pytest.mark.parametrize("tile_rows", [None, 7], ids=["one-tile", "tiles"])
def test_streamed_in_two_passes(streamer, resident, monkeypatch, tile_rows):
    k, smax = 21, FIFTH
    seqs = the_set()
    windows = PP.pass_windows(hist_of(k, smax), PP.forced_plan(2))
    base, base_info = baseline(resident, k, smax, 1, 0.0)
    monkeypatch.setenv("LZANI_PREFILTER_PASSES", "2")
    if tile_rows:
        monkeypatch.setenv("LZANI_PREFILTER_TILE_ROWS", str(tile_rows))
    T = (len(seqs) + tile_rows - 1) // tile_rows if tile_rows else 1
    streamer.prefilter_codes(seqs, k, smax, 1, 0.0, slice_bytes=three_slices())
    got = streamer.prefilter_fetch()
    _same(got, want_of(k, smax, 1, 0.0), "streamed, model")
    _bytes_equal(got, base, "streamed, resident one pass")
    info, pi, si = streamer.prefilter_info(), streamer.prefilter_pass_info(), streamer.prefilter_stream_info()
    W = PP.key_sweeps(T, windows)
    assert W == 2 + 3 * T * 2
    assert info["tiles"] == T and pi["passes"] == 2 and pi["key_sweeps"] == W
    assert si["slices"] == 3 and si["slice_uploads"] == W * (3 - 1) + 1
    assert [info[f] for f in COUNTS] == [base_info[f] for f in COUNTS]


@pytest.mark.parametrize("ooc", [False, True])
def test_the_contexts_own_set_is_untouched_by_streamed_passes(monkeypatch, ooc):
    """What test_the_contexts_own_set_is_untouched (test_gpu_prefilter_stream.py) checks, under two passes."""
    _, own = SG.make_set(12, 7, lmin=3000, lmax=5000, fam=4)
    own.append(np.full(100, 5, dtype=np.uint8))
    k = 21
    seqs = the_set()
    want = want_of(k, FIFTH, 1, 0.0)
    eng = L.Engine()
    try:
        if ooc:
            eng.set_genome_memory(M.limit_for_blocks([len(s) for s in own], None, 3))
        eng.set_genomes(own)
        before = eng.all2all()
        lay0, res0 = eng.layout(), eng.residency()
        assert res0["blocks"] == (3 if ooc else 1)
        monkeypatch.setenv("LZANI_PREFILTER_PASSES", "2")
        eng.prefilter_codes(seqs, k, FIFTH, slice_bytes=three_slices())
        monkeypatch.delenv("LZANI_PREFILTER_PASSES")
        assert eng.prefilter_pass_info()["passes"] == 2 and eng.prefilter_stream_info()["slice_uploads"] == 8 * 2 + 1
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
            eng.prefilter_pass_plan()
    finally:
        eng.close()


def test_no_kept_window_under_forced_passes(resident, streamer, monkeypatch):
    k = 21
    seqs = the_set()
    assert int(hist_of(k, 0).sum()) == 0                                   # sample_max 0: no k-mer of the set hashes to 0
    monkeypatch.setenv("LZANI_PREFILTER_PASSES", "3")
    for eng, run in ((resident, lambda: resident.prefilter(k, 0)), (streamer, lambda: streamer.prefilter_codes(seqs, k, 0, slice_bytes=three_slices()))):
        assert run() == 0
        kmers_of, row_off, ids, shared = eng.prefilter_fetch()
        assert kmers_of.tolist() == [0] * 24 and row_off.tolist() == [0] * 25 and len(ids) == len(shared) == 0
        info, pi = eng.prefilter_info(), eng.prefilter_pass_info()
        assert (info["positions"], info["distinct_kmers"], info["postings"], info["entries"]) == (0, 0, 0, 0)
        assert (pi["passes"], pi["key_sweeps"], pi["largest_pass"]) == (3, PP.key_sweeps(1, [0, 0, 0]), 0)
        assert eng.prefilter_pass_plan().tolist() == PP.forced_plan(3)
    assert streamer.prefilter_stream_info()["slice_uploads"] == 3


def test_binary_writes_the_same_files_in_three_passes(tmp_path):
    """`lz-ani all2all --flt-kmers 21 0.3 -V 2` with LZANI_PREFILTER_PASSES=3: TSV and ids file byte-identical to the run
    without the variable; the verbose line says `; 3 passes`."""
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])
    seqs = the_set()
    names = ["p%02d" % i for i in range(len(seqs))]
    fa = str(tmp_path / "in.fa")
    SG.write_fasta(fa, names, seqs)
    env0 = {k: v for k, v in os.environ.items() if k not in ENV}
    outs = []
    for tag, env in (("plain", {}), ("passes", {"LZANI_PREFILTER_PASSES": "3"})):
        out = str(tmp_path / (tag + ".tsv"))
        p = subprocess.run([EXE, "all2all", "--in-fasta", fa, "-o", out, "-V", "2", "--out-format", "complete", "--flt-kmers", "21", "0.3"],
                           capture_output=True, text=True, env=dict(env0, **env))
        assert p.returncode == 0, p.stderr[-2000:]
        line = next(x for x in p.stderr.splitlines() if "k-mer filter on device" in x)
        assert line.endswith("; 3 passes") == (tag == "passes") and ("passes" in line) == (tag == "passes"), line
        outs.append((open(out, "rb").read(), open(str(tmp_path / (tag + ".ids.tsv")), "rb").read()))
    assert outs[0] == outs[1] and outs[0][0].count(b"\n") > 1
