"""GPU: the bitmap-form refill of the pair kernel (DevWave::refill, lzani_kernels_pairs.h), which makes a candidate's mal-mer
word from the query text instead of reading it from the k-mer words.  Every case runs through the C-ABI, must have run
the form it is about (layout / launch record), and compares bit-exactly with the CPU oracle.  The shapes are the smallest
at which the refill can be wrong:
- queues that overflow by chance (the next refill starts at the surplus candidate, not at a block end);
- related pairs, whose extensions carry the scan past the blocks a refill has read (refills that start anywhere);
- query ends one below / at / above a multiple of 64 and of 4,096, queries shorter than a block and than mal, candidates
  at all 16 symbol offsets of a text word (a tandem repeat against itself, shifted);
- N runs (the kernel that consults the N mask), ending 0..mal symbols in front of candidates;
- the other readers of the same code: parameter set 2 with a matrix of fewer rows than k-mers (rshift != 0: bits the
  refill must find dead), with and without the split, and the join form (CAND 1).
The host-side statement of the hash itself is tests/test_refill_hash.py (no GPU)."""
import numpy as np
import pytest

import index_model as M
import lzani_ctypes as L
import oracle as O
import synth_genomes as SG
import util as U

pytestmark = pytest.mark.gpu

AQ_CAP = 64                       # lzani_kernels_pairs.h: candidates a queue takes
BLOCK = 4096                      # query positions of one bitmap block of a refill
FORM_ENV = ("LZANI_RTC", "LZANI_RTC_MIN_PAIRS", "LZANI_PM", "LZANI_PM_MIN_ROWS", "LZANI_PM_MIN_SHARE", "LZANI_PM_MAX_BYTES",
            "LZANI_JOIN_MIN_BYTES", "LZANI_NO_JOIN", "LZANI_BLOCK_KERNEL", "LZANI_SPLIT", "LZANI_SPLIT_SEGLEN", "LZANI_SPLIT_ALL",
            "LZANI_SPLIT_S", "LZANI_SPLIT_THR", "LZANI_SPLIT_GIVE_UP", "LZANI_LPT", "LZANI_NO_TAGWORDS", "LZANI_NO_BUCKETS", "LZANI_NO_FILTER",
            "LZANI_FILTER_MAX_BITS", "LZANI_BK_MAX_DIRBITS", "LZANI_MAX_SLOTS", "LZANI_PM_FROM_INDEX")
BITMAPS = {"LZANI_PM_MIN_ROWS": "1", "LZANI_SPLIT": "0", "LZANI_RTC": "0"}
JOIN = {"LZANI_JOIN_MIN_BYTES": "1", "LZANI_PM": "0", "LZANI_RTC": "0"}
SPLIT = {"LZANI_PM_MIN_ROWS": "1", "LZANI_SPLIT": "1", "LZANI_RTC": "0"}
LONG = dict(mal=15, msl=9, reg=60)


def _run(monkeypatch, seqs, prm, env):
    for k in FORM_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = L.Engine(prm)
    try:
        eng.set_genomes(seqs)
        got = eng.all2all()
        return got, eng.layout(), eng.kernel_launches()
    finally:
        eng.close()


def _check(got, want, what):
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.shape[0] * (got.shape[0] - 1)} pairs differ from the oracle, first {bad[:4].tolist()}"


def _family_set():
    """6 genomes of 9-13 kbp in families of 3 at <= 5 % divergence, two more for _put_n_runs."""
    return [np.ascontiguousarray(s) for s in SG.make_set(8, 7101, lmin=9000, lmax=13000, fam=3, dmin=0.01, dmax=0.05)[1]]


def test_queues_that_overflow_by_chance(monkeypatch):
    seqs = [np.ascontiguousarray(s) for s in SG.make_set(6, 7100, lmin=36000, lmax=44000, fam=1)[1]]
    mrd, mal = U.DEFAULTS["mrd"], U.DEFAULTS["mal"]
    # candidates of the first block of every pair, from the raw sequences (exact mal-mer matches: a lower bound of the
    # bits a hashed matrix sets): a pair's first refill starts at position 0 and reads [0, 4096)
    first = [int(M.popcounts(M.plain_bitmap(seqs[r], seqs[q], mrd, mal, M.cand_words(len(seqs[q]), mrd))[:BLOCK // 32]))
             for r in range(len(seqs)) for q in range(len(seqs)) if q != r]
    print("candidates in the first block of the 30 pairs:", sorted(first))
    assert max(first) > AQ_CAP, first
    got, lay, rec = _run(monkeypatch, seqs, None, BITMAPS)
    assert lay["bitmap_launches"] > 0 and any("cand=2" in k for k in rec), (lay, rec)
    _check(got, O.oracle_all2all(seqs, None, threads=16), "unrelated 36-44 kbp")


def test_related_pairs_whose_extensions_outrun_the_blocks(monkeypatch):
    seqs = _family_set()[:6]
    got, lay, rec = _run(monkeypatch, seqs, None, BITMAPS)
    assert lay["bitmap_launches"] > 0 and any("nfree=1" in k and "cand=2" in k for k in rec), (lay, rec)
    want = O.oracle_all2all(seqs, None, threads=16)
    assert want[0, 1, 0] > 5000 and want[0, 5, 0] < 500, want[0, :, 0].tolist()         # related and unrelated pairs
    _check(got, want, "families of 3")


def _edge_set():
    st = SG.Stream(7102)
    base = (st.u64(8600) % np.uint64(4)).astype(np.uint8)
    mrd = U.DEFAULTS["mrd"]
    seqs = [base]
    for D in (4096, 2 * 4096, 4096 + 64, 64 * 33):                 # L + mrd one below, at, one above a multiple of 4,096 / of 64
        for d in (-1, 0, 1):
            seqs.append(SG.mutate(base, 0.03, st)[:D - mrd + d].copy())
    seqs.append(base[5000:5700].copy())                             # shorter than one block
    seqs.append(base[100:100 + 60].copy())                          # shorter than one bitmap word
    seqs.append(base[300:300 + 7].copy())                           # shorter than mal
    unit = (st.u64(97) % np.uint64(4)).astype(np.uint8)
    rep = np.tile(unit, 7)
    seqs += [rep[:600].copy(), rep[5:5 + 590].copy()]               # a tandem repeat against itself, shifted: candidates at every offset
    return [np.ascontiguousarray(s) for s in seqs]


def test_query_ends_and_symbol_offsets(monkeypatch):
    seqs = _edge_set()
    mrd, mal = U.DEFAULTS["mrd"], U.DEFAULTS["mal"]
    a, b = seqs[-2], seqs[-1]
    bits = np.unpackbits(M.plain_bitmap(a, b, mrd, mal, 32).view(np.uint8), bitorder="little")
    offs = {int(p) & 15 for p in np.nonzero(bits)[0]}
    assert offs == set(range(16)), sorted(offs)
    got, lay, rec = _run(monkeypatch, seqs, None, BITMAPS)
    assert lay["bitmap_launches"] > 0 and any("cand=2" in k for k in rec), (lay, rec)
    _check(got, O.oracle_all2all(seqs, None, threads=16), "query ends and offsets")


def _n_set():
    seqs = U._put_n_runs(_family_set())
    g = seqs[0].copy()                                             # 0, 1, 2 are one family: nearly every position is a candidate,
    for k in range(16):                                             # so these runs end 0 .. mal symbols in front of one
        p = 3000 + 131 * k
        g[p:p + 1 + k % 5] = 5
    seqs[0] = g
    h = seqs[2].copy()
    h[:3] = 5
    h[len(h) - 2:] = 5
    seqs[2] = h
    return [np.ascontiguousarray(s) for s in seqs]


def test_n_runs_in_front_of_candidates(monkeypatch):
    seqs = _n_set()
    got, lay, rec = _run(monkeypatch, seqs, None, BITMAPS)
    assert lay["bitmap_launches"] > 0 and any("nfree=0" in k and "cand=2" in k for k in rec), (lay, rec)
    _check(got, O.oracle_all2all(seqs, None, threads=16), "N runs")


_LONG = {}


def _long_set():
    if not _LONG:
        st = SG.Stream(7103)
        base = (st.u64(300_000) % np.uint64(4)).astype(np.uint8)
        seqs = [base, SG.mutate(base, 0.04, st), (st.u64(290_000) % np.uint64(4)).astype(np.uint8)]
        _LONG["seqs"] = [np.ascontiguousarray(s) for s in seqs]
        _LONG["want"] = O.oracle_all2all(_LONG["seqs"], LONG, threads=16)
    return _LONG["seqs"], _LONG["want"]


@pytest.mark.parametrize("split", (False, True), ids=("whole_pairs", "split"))
def test_parameter_set_2_with_a_folded_matrix(monkeypatch, split):
    seqs, want = _long_set()
    for k in FORM_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in (SPLIT if split else BITMAPS).items():
        monkeypatch.setenv(k, v)
    n = len(seqs)
    eng = L.Engine(LONG)
    try:
        eng.set_genomes(seqs)
        out, _, _, plan = eng.debug_run_candidates(np.arange(n, dtype=np.uint32), np.arange(n + 1, dtype=np.uint64) * np.uint64(n - 1), None, words=32)
        lay, rec = eng.layout(), eng.kernel_launches()
    finally:
        eng.close()
    assert plan["pm"] and plan["rshift"] != 0, plan                 # fewer matrix rows than k-mers: set bits the refill finds dead
    assert lay["bitmap_launches"] > 0, lay
    assert any("split " in k for k in rec) == split and all("defp=2" in k for k in rec), rec
    exp = np.concatenate([want[r, [q for q in range(n) if q != r]] for r in range(n)])
    assert np.array_equal(out, exp), (out.tolist(), exp.tolist())


def test_join_form(monkeypatch):
    seqs = _family_set()[:6]
    got, lay, rec = _run(monkeypatch, seqs, None, JOIN)
    assert rec and all("cand=1" in k for k in rec), (lay, rec)
    _check(got, O.oracle_all2all(seqs, None, threads=16), "join form")
