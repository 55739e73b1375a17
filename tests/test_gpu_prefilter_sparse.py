"""GPU: sparse counting of the k-mer prefilter (lzani_set_prefilter_counting, LZANI_PREFILTER_TABLE_SLOTS) against the dense
one-pass result of the same context, byte for byte, and against the numpy statement of the definitions
(tests/prefilter_model.py, tests/prefilter_cross_model.py); the tiles and attempts against the statement of the tile rule
(tests/prefilter_sparse_model.py).  All four entry points, one pass and several, a table that is nearly full, tables of several
compaction blocks and scan steps, tables that
overflow and halve the tile, one that cannot hold a row, and the host binary."""
import os
import subprocess

import numpy as np
import pytest

import lzani_ctypes as L
import prefilter_cross_model as XM
import prefilter_model as PM
import prefilter_pass_model as PP
import prefilter_sparse_model as SM
import synth_genomes as SG
import util as U

pytestmark = pytest.mark.gpu

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
FIFTH = L.sample_max_of(0.2)
ENV = ("LZANI_PREFILTER_PASSES", "LZANI_PREFILTER_MAX_WINDOWS", "LZANI_PREFILTER_TILE_ROWS", "LZANI_PREFILTER_SLICE_BYTES",
       "LZANI_PREFILTER_TABLE_SLOTS")
THRESHOLDS = ((1, 0.0), (3, 0.05))
COUNTS = ("k", "positions", "distinct_kmers", "postings", "entries")
DENSE_INFO = dict(sparse=0, attempts=0, pass_runs=0, slots=0, table_bytes=0, pairs_seen=0, max_fill=0)

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


def want_of(k, smax, min_shared, min_ratio, n_ref=0):
    kmers_of, shared = model(k, smax)
    if n_ref:
        return (kmers_of.astype(np.uint32),) + XM.kept_pairs(kmers_of, shared, n_ref, min_shared, min_ratio)
    return (kmers_of.astype(np.uint32),) + PM.kept_pairs(kmers_of, shared, min_shared, min_ratio)


def pairs_of(k, smax, n_ref=0):
    return SM.row_pairs(model(k, smax)[1], n_ref)


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


@pytest.fixture(autouse=True)
def automatic_again(resident, streamer):
    yield
    resident.set_prefilter_counting("auto")
    streamer.set_prefilter_counting("auto")


def baseline(eng, k, smax, min_shared, min_ratio, n_ref=0):
    """The same context's dense result in one pass, without any variable: (fetch, info)."""
    key = (k, smax, min_shared, min_ratio, n_ref)
    if key not in _base:
        assert not any(name in os.environ for name in ENV)
        eng.set_prefilter_counting("dense")
        if n_ref:
            eng.prefilter_cross(k, n_ref, smax, min_shared, min_ratio)
        else:
            eng.prefilter(k, smax, min_shared, min_ratio)
        pi = eng.prefilter_pass_info()
        assert pi["passes"] == 1 and pi["key_sweeps"] == 3 and eng.prefilter_sparse_info() == DENSE_INFO
        _base[key] = (eng.prefilter_fetch(), eng.prefilter_info())
    return _base[key]


def _same(got, want, what):
    for name, g, w in zip(("kmers_of", "row_off", "ids", "shared"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, g[:8], w[:8])


def _bytes_equal(got, want, what):
    for name, g, w in zip(("kmers_of", "row_off", "ids", "shared"), got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, name)


def _check(eng, k, smax, min_shared, min_ratio, base, base_info, what, n_ref=0):
    got = eng.prefilter_fetch()
    _bytes_equal(got, base, (what, "dense"))
    _same(got, want_of(k, smax, min_shared, min_ratio, n_ref), (what, "model"))
    info = eng.prefilter_info()
    assert [info[f] for f in COUNTS] == [base_info[f] for f in COUNTS], what
    return info


def test_mode_and_info(resident, monkeypatch):
    """The test that fails without the feature: the default stays dense on this set, the mode brings the table."""
    k, smax = 21, PM.SAMPLE_ALL
    n = len(the_set())
    seen = int(pairs_of(k, smax).sum())
    assert seen == 35 == int((np.triu(model(k, smax)[1], 1) > 0).sum())
    for min_shared, min_ratio in THRESHOLDS:
        base, base_info = baseline(resident, k, smax, min_shared, min_ratio)
        resident.set_prefilter_counting("auto")
        resident.prefilter(k, smax, min_shared, min_ratio)                 # one matrix tile fits: automatic is dense
        info, pi = resident.prefilter_info(), resident.prefilter_pass_info()
        assert resident.prefilter_sparse_info() == DENSE_INFO and info["tiles"] == 1 and pi["key_sweeps"] == 3
        _bytes_equal(resident.prefilter_fetch(), base, "automatic")
        resident.set_prefilter_counting("sparse")
        cnt = resident.prefilter(k, smax, min_shared, min_ratio)
        info = _check(resident, k, smax, min_shared, min_ratio, base, base_info, "sparse")
        si, pi = resident.prefilter_sparse_info(), resident.prefilter_pass_info()
        assert cnt == info["entries"] > 0 and info["tiles"] == 1 and pi["key_sweeps"] == 3
        slots = 2048                                                       # the smallest power of two >= 2 * 24 * 24
        assert slots // 2 < 2 * n * n <= slots
        assert si == dict(sparse=1, attempts=1, pass_runs=1, slots=slots, table_bytes=12 * slots, pairs_seen=seen, max_fill=seen)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        resident.set_prefilter_counting(3)
    # a forced tile height is a statement about the matrix: automatic stays dense under it, and the mode does not listen to it
    base, base_info = baseline(resident, k, smax, 1, 0.0)
    monkeypatch.setenv("LZANI_PREFILTER_TILE_ROWS", "7")
    resident.set_prefilter_counting("auto")
    resident.prefilter(k, smax, 1, 0.0)
    assert resident.prefilter_sparse_info() == DENSE_INFO and resident.prefilter_info()["tiles"] == 4
    resident.set_prefilter_counting("sparse")
    resident.prefilter(k, smax, 1, 0.0)
    assert resident.prefilter_sparse_info()["sparse"] == 1 and resident.prefilter_info()["tiles"] == 1
    _bytes_equal(resident.prefilter_fetch(), base, "sparse under a tile height")


def test_a_full_table(resident, monkeypatch):
    """231 pairs in 512 slots, the limit is 256: probing and the wrap at the table's end at a load of 0.45."""
    k, smax = 8, PM.SAMPLE_ALL
    assert int(pairs_of(k, smax).sum()) == 231
    for min_shared, min_ratio in THRESHOLDS:
        base, base_info = baseline(resident, k, smax, min_shared, min_ratio)
        resident.set_prefilter_counting("sparse")
        monkeypatch.setenv("LZANI_PREFILTER_TABLE_SLOTS", "512")
        resident.prefilter(k, smax, min_shared, min_ratio)
        monkeypatch.delenv("LZANI_PREFILTER_TABLE_SLOTS")
        info = _check(resident, k, smax, min_shared, min_ratio, base, base_info, "full table")
        si = resident.prefilter_sparse_info()
        assert info["tiles"] == 1 and si == dict(sparse=1, attempts=1, pass_runs=1, slots=512, table_bytes=12 * 512, pairs_seen=231, max_fill=231)


@pytest.mark.parametrize("slots, n_ref", [(4096, 0), (8192, 0), (1 << 22, 0), (1 << 23, 0), (8192, 9), (1 << 23, 9)])
def test_a_table_of_several_blocks(resident, monkeypatch, slots, n_ref):
    """The compaction of the table over more than one block of 4,096 slots, and the scan of its block counts over more
    than one step of 1,024.  4096: one full block, its loop never breaks; 8192: two blocks, the second writes from a
    non-zero offset; 2^22: 1,024 block counts, exactly one scan step; 2^23: 2,048, the scan's carry is used."""
    k, smax = 21, PM.SAMPLE_ALL
    seen = int(pairs_of(k, smax, n_ref).sum())
    assert seen == (8 if n_ref else 35)
    for min_shared, min_ratio in THRESHOLDS:
        base, base_info = baseline(resident, k, smax, min_shared, min_ratio, n_ref)
        resident.set_prefilter_counting("sparse")
        monkeypatch.setenv("LZANI_PREFILTER_TABLE_SLOTS", str(slots))
        if n_ref:
            resident.prefilter_cross(k, n_ref, smax, min_shared, min_ratio)
        else:
            resident.prefilter(k, smax, min_shared, min_ratio)
        monkeypatch.delenv("LZANI_PREFILTER_TABLE_SLOTS")
        info = _check(resident, k, smax, min_shared, min_ratio, base, base_info, ("several blocks", slots, n_ref), n_ref)
        si = resident.prefilter_sparse_info()
        assert info["tiles"] == 1 and si == dict(sparse=1, attempts=1, pass_runs=1, slots=slots, table_bytes=12 * slots, pairs_seen=seen, max_fill=seen)


@pytest.mark.parametrize("slots, tiles, attempts", [(256, 2, 3), (32, 24, 28)])
def test_halving(resident, monkeypatch, slots, tiles, attempts):
    k, smax = 12, PM.SAMPLE_ALL
    pairs = pairs_of(k, smax)
    tile_r0, plan_attempts = SM.plan(pairs, slots)
    assert (len(tile_r0) - 1, plan_attempts) == (tiles, attempts)
    assert (L.plan_sparse_tiles(pairs, slots)[0].tolist(), L.plan_sparse_tiles(pairs, slots)[1]) == (tile_r0, attempts)
    fill = max(int(pairs[a:b].sum()) for a, b in zip(tile_r0, tile_r0[1:]))
    for min_shared, min_ratio in THRESHOLDS:
        base, base_info = baseline(resident, k, smax, min_shared, min_ratio)
        resident.set_prefilter_counting("sparse")
        monkeypatch.setenv("LZANI_PREFILTER_TABLE_SLOTS", str(slots))
        resident.prefilter(k, smax, min_shared, min_ratio)
        monkeypatch.delenv("LZANI_PREFILTER_TABLE_SLOTS")
        info = _check(resident, k, smax, min_shared, min_ratio, base, base_info, ("halving", slots))
        si, pi = resident.prefilter_sparse_info(), resident.prefilter_pass_info()
        assert info["tiles"] == tiles and si["attempts"] == attempts and pi["key_sweeps"] == 3 and si["pass_runs"] == 1
        assert si["pairs_seen"] == int(pairs.sum()) == 154 and si["max_fill"] == fill and si["slots"] == slots


def test_a_row_the_table_cannot_hold(resident, monkeypatch):
    k, smax = 12, PM.SAMPLE_ALL
    assert int(pairs_of(k, smax)[0]) == 14 and SM.plan(pairs_of(k, smax), 16) is None
    base, _ = baseline(resident, k, smax, 1, 0.0)
    resident.set_prefilter_counting("sparse")
    monkeypatch.setenv("LZANI_PREFILTER_TABLE_SLOTS", "16")
    with pytest.raises(L.LzaniError, match=r"LZANI_ERR_NOMEM.*row 0 .*16 slots.*dense"):
        resident.prefilter(k, smax, 1, 0.0)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):           # a failed call leaves no result
        resident.prefilter_fetch()
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        resident.prefilter_sparse_info()
    for bad in ("0", "1", "24", "1000"):
        monkeypatch.setenv("LZANI_PREFILTER_TABLE_SLOTS", bad)
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG.*LZANI_PREFILTER_TABLE_SLOTS"):
            resident.prefilter(k, smax, 1, 0.0)
    monkeypatch.setenv("LZANI_PREFILTER_TABLE_SLOTS", "16")
    resident.set_prefilter_counting("dense")                              # the way out the message names
    resident.prefilter(k, smax, 1, 0.0)
    assert resident.prefilter_sparse_info() == DENSE_INFO
    _bytes_equal(resident.prefilter_fetch(), base, "dense after the refusal")


@pytest.mark.parametrize("smax", [PM.SAMPLE_ALL, FIFTH], ids=["all", "fifth"])
@pytest.mark.parametrize("k", [8, 21, 31])
def test_seven_passes_in_one_tile(resident, monkeypatch, k, smax):
    windows = PP.pass_windows(hist_of(k, smax), PP.forced_plan(7))
    held = sum(1 for x in windows if x)
    assert held > 1
    base, base_info = baseline(resident, k, smax, 1, 0.0)
    monkeypatch.setenv("LZANI_PREFILTER_PASSES", "7")
    resident.set_prefilter_counting("sparse")
    resident.prefilter(k, smax, 1, 0.0)
    info = _check(resident, k, smax, 1, 0.0, base, base_info, "seven passes, sparse")
    si, pi = resident.prefilter_sparse_info(), resident.prefilter_pass_info()
    assert info["tiles"] == 1 and si["attempts"] == 1 and si["pass_runs"] == held and pi["passes"] == 7
    assert pi["key_sweeps"] == 2 + 3 * held == PP.key_sweeps(1, windows)
    assert si["pairs_seen"] == si["max_fill"] == int(pairs_of(k, smax).sum())
    resident.set_prefilter_counting("dense")
    monkeypatch.setenv("LZANI_PREFILTER_TILE_ROWS", "5")
    resident.prefilter(k, smax, 1, 0.0)
    info = _check(resident, k, smax, 1, 0.0, base, base_info, "seven passes, dense tiles")
    assert info["tiles"] == 5 and resident.prefilter_pass_info()["key_sweeps"] == 2 + 3 * 5 * held and resident.prefilter_sparse_info() == DENSE_INFO


def test_passes_with_an_abandoned_attempt(resident, monkeypatch):
    """The first attempt (all rows, 154 pairs against a limit of 128) runs some of its passes and is abandoned: no pass adds
    its |K(g)| twice, and every pass that was run is in the sweeps."""
    k, smax = 12, PM.SAMPLE_ALL
    pairs = pairs_of(k, smax)
    windows = PP.pass_windows(hist_of(k, smax), PP.forced_plan(7))
    held = sum(1 for x in windows if x)
    for min_shared, min_ratio in THRESHOLDS:
        base, base_info = baseline(resident, k, smax, min_shared, min_ratio)
        monkeypatch.setenv("LZANI_PREFILTER_PASSES", "7")
        monkeypatch.setenv("LZANI_PREFILTER_TABLE_SLOTS", "256")
        resident.set_prefilter_counting("sparse")
        resident.prefilter(k, smax, min_shared, min_ratio)
        monkeypatch.delenv("LZANI_PREFILTER_PASSES")
        monkeypatch.delenv("LZANI_PREFILTER_TABLE_SLOTS")
        info = _check(resident, k, smax, min_shared, min_ratio, base, base_info, "abandoned attempt")
        assert np.array_equal(resident.prefilter_fetch()[0], model(k, smax)[0].astype(np.uint32))
        si, pi = resident.prefilter_sparse_info(), resident.prefilter_pass_info()
        assert (info["tiles"], si["attempts"]) == (2, 3) == (len(SM.plan(pairs, 256)[0]) - 1, SM.plan(pairs, 256)[1])
        assert si["attempts"] > info["tiles"] and pi["key_sweeps"] == 2 + 3 * si["pass_runs"]
        assert 2 * held < si["pass_runs"] <= 3 * held                     # two whole attempts and a part of the abandoned one
        assert si["pairs_seen"] == 154 and si["max_fill"] == 124


@pytest.mark.parametrize("n_ref, seen", [(9, 8), (13, 11)])
def test_cross(resident, monkeypatch, n_ref, seen):
    k, smax = 21, PM.SAMPLE_ALL
    n = len(the_set())
    assert int(pairs_of(k, smax, n_ref).sum()) == seen
    for min_shared, min_ratio in THRESHOLDS:
        base, base_info = baseline(resident, k, smax, min_shared, min_ratio, n_ref)
        resident.set_prefilter_counting("sparse")
        for slots in (None, 8):                                            # automatic; and a table that halves the tile
            if slots:
                monkeypatch.setenv("LZANI_PREFILTER_TABLE_SLOTS", str(slots))
            resident.prefilter_cross(k, n_ref, smax, min_shared, min_ratio)
            monkeypatch.delenv("LZANI_PREFILTER_TABLE_SLOTS", raising=False)
            info = _check(resident, k, smax, min_shared, min_ratio, base, base_info, ("cross", n_ref, slots), n_ref)
            row_off = resident.prefilter_fetch()[1]
            assert row_off[n_ref:].tolist() == [info["entries"]] * (n - n_ref + 1)
            si, ci = resident.prefilter_sparse_info(), resident.prefilter_cross_info()
            tile_r0, attempts = SM.plan(pairs_of(k, smax, n_ref), slots or si["slots"])
            assert si["sparse"] == 1 and si["pairs_seen"] == seen and (info["tiles"], si["attempts"]) == (len(tile_r0) - 1, attempts)
            assert (ci["n_ref"], ci["n_query"]) == (n_ref, n - n_ref)
            if not slots:
                assert si["slots"] == 1 << int(np.ceil(np.log2(2 * n_ref * (n - n_ref)))) and attempts == 1
            else:
                assert attempts > 1


def three_slices():
    lens = [len(s) for s in the_set()]
    total = sum(lens)
    return next(sb for sb in range(max(max(lens), total // 3), total) if L.plan_slices(lens, sb)[0] == 3)


@pytest.mark.parametrize("passes", [1, 7])
@pytest.mark.parametrize("n_ref", [0, 9], ids=["all-pairs", "cross"])
def test_streamed(streamer, resident, monkeypatch, n_ref, passes):
    k, smax = 21, FIFTH
    seqs = the_set()
    base, base_info = baseline(resident, k, smax, 1, 0.0, n_ref)
    windows = PP.pass_windows(hist_of(k, smax), PP.forced_plan(passes))
    monkeypatch.setenv("LZANI_PREFILTER_PASSES", str(passes))
    slots = 8 if n_ref else 32                                             # tiles and abandoned attempts, streamed
    monkeypatch.setenv("LZANI_PREFILTER_TABLE_SLOTS", str(slots))
    streamer.set_prefilter_counting("sparse")
    if n_ref:
        streamer.prefilter_codes_cross(seqs, k, n_ref, smax, 1, 0.0, slice_bytes=three_slices())
    else:
        streamer.prefilter_codes(seqs, k, smax, 1, 0.0, slice_bytes=three_slices())
    info = _check(streamer, k, smax, 1, 0.0, base, base_info, ("streamed", n_ref, passes), n_ref)
    si, pi, st = streamer.prefilter_sparse_info(), streamer.prefilter_pass_info(), streamer.prefilter_stream_info()
    tile_r0, attempts = SM.plan(pairs_of(k, smax, n_ref), slots)
    assert si["sparse"] == 1 and (info["tiles"], si["attempts"]) == (len(tile_r0) - 1, attempts) and attempts > info["tiles"] > 1
    W = pi["key_sweeps"]
    assert W == (3 if passes == 1 else 2 + 3 * si["pass_runs"]) and pi["passes"] == passes
    if passes > 1:
        assert si["pass_runs"] >= info["tiles"] * sum(1 for x in windows if x)
    assert st["slices"] == 3 and st["slice_uploads"] == W * (3 - 1) + 1


def _rand(seed, n):
    return (SG.splitmix64(seed, np.arange(n, dtype=np.uint64)) % np.uint64(4)).astype(np.uint8)


def test_edges(resident, streamer):
    k = 21
    streamer.set_prefilter_counting("sparse")
    resident.set_prefilter_counting("sparse")
    # one genome: nothing to count, no table
    assert streamer.prefilter_codes([_rand(901, 3000)], k) == 0
    kmers_of, row_off, ids, shared = streamer.prefilter_fetch()
    assert kmers_of.tolist() == [2980] and row_off.tolist() == [0, 0] and len(ids) == len(shared) == 0
    assert streamer.prefilter_sparse_info() == DENSE_INFO and streamer.prefilter_info()["tiles"] == 0
    # no pair shares a k-mer: a table that stays empty
    lonely = [_rand(910 + i, 2000 + 300 * i) for i in range(5)]
    assert int(np.triu(PM.shared_matrix(lonely, k)[1], 1).sum()) == 0
    assert streamer.prefilter_codes(lonely, k) == 0
    kmers_of, row_off, ids, shared = streamer.prefilter_fetch()
    assert kmers_of.tolist() == [len(s) - k + 1 for s in lonely] and row_off.tolist() == [0] * 6 and len(ids) == len(shared) == 0
    si = streamer.prefilter_sparse_info()
    assert (si["sparse"], si["attempts"], si["pairs_seen"], si["max_fill"], si["slots"]) == (1, 1, 0, 0, 64) and streamer.prefilter_info()["tiles"] == 1
    # no kept window at all (sample_max 0: no k-mer of the set hashes to 0): the stage ends before the count
    assert resident.prefilter(k, 0) == 0
    kmers_of, row_off, ids, shared = resident.prefilter_fetch()
    assert kmers_of.tolist() == [0] * 24 and row_off.tolist() == [0] * 25 and len(ids) == len(shared) == 0
    assert resident.prefilter_sparse_info() == DENSE_INFO and resident.prefilter_pass_info()["key_sweeps"] == 1
    # min_shared above every count: the table holds the pairs, none is kept
    top = int(np.triu(model(k, PM.SAMPLE_ALL)[1], 1).max())
    assert resident.prefilter(k, PM.SAMPLE_ALL, top + 1, 0.0) == 0
    kmers_of, row_off, ids, shared = resident.prefilter_fetch()
    assert np.array_equal(kmers_of, model(k, PM.SAMPLE_ALL)[0].astype(np.uint32)) and row_off.tolist() == [0] * 25 and len(ids) == 0
    si = resident.prefilter_sparse_info()
    assert (si["sparse"], si["pairs_seen"], si["max_fill"]) == (1, 35, 35) and resident.prefilter_info()["tiles"] == 1
    assert resident.prefilter(k, PM.SAMPLE_ALL, top, 0.0) == 1            # ... and the fullest pair alone at its own count
    assert resident.prefilter_fetch()[3].tolist() == [top]


def test_binary_writes_the_same_files(tmp_path):
    """`lz-ani all2all --flt-kmers 21 0.3 --flt-kmers-counting sparse` under LZANI_PREFILTER_TABLE_SLOTS=256: TSV and ids
    file byte-identical to the dense run's; the same for query2ref.  The verbose line names the form."""
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])
    seqs = the_set()
    names = ["p%02d" % i for i in range(len(seqs))]
    fa, ref, qry = str(tmp_path / "in.fa"), str(tmp_path / "ref.fa"), str(tmp_path / "qry.fa")
    SG.write_fasta(fa, names, seqs)
    SG.write_fasta(ref, names[:9], seqs[:9])
    SG.write_fasta(qry, names[9:], seqs[9:])
    env = dict({k: v for k, v in os.environ.items() if k not in ENV}, LZANI_PREFILTER_TABLE_SLOTS="256")
    for mode, inputs in (("all2all", ["--in-fasta", fa]), ("query2ref", ["--in-fasta", ref, "--query-fasta", qry])):
        outs = []
        for form in ("dense", "sparse"):
            out = str(tmp_path / ("%s.%s.tsv" % (mode, form)))
            p = subprocess.run([EXE, mode] + inputs + ["-o", out, "-V", "2", "--out-format", "complete", "--flt-kmers", "21", "0.3", "--flt-kmers-counting", form],
                               capture_output=True, text=True, env=env)
            assert p.returncode == 0, p.stderr[-2000:]
            line = next(x for x in p.stderr.splitlines() if "k-mer filter on device" in x)
            assert ("; sparse counting: 1 attempt(s), 256 slots" in line) == (form == "sparse") and " 1 tile(s)" in line, line
            outs.append((open(out, "rb").read(), open(str(tmp_path / ("%s.%s.ids.tsv" % (mode, form))), "rb").read()))
        assert outs[0] == outs[1] and outs[0][0].count(b"\n") > 1, mode
