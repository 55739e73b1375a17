"""GPU: the resolve of the pair kernel's refill from one fetch of each text (DevWave::refill; lzani_core.h: text_words5,
resolve_diff, null_ext_record_diff): the 32-symbol compare and both windows of a candidate's null-extension record come
out of the five dwords around the query position and around the reference position.  Every case runs through the C-ABI,
is bit-exact against the CPU oracle on every pair, asserts that the form it is about ran (layout / launch record), and
asserts from the raw sequences, before it runs, that the candidates it is aimed at exist:
(a) candidates at all 256 combinations of (qp & 15, pos & 15): the funnels of both texts at every shift;
(b) matches of every length 11..40 between mismatching symbols: 15/16/17 (the compare's word boundary), 31/32/33 (the
    lane's cap: longer candidates go to the wave), the forward window at every offset of the words; at the defaults and
    at mal 15, msl 9, reg 60;
(c) candidates that start at 0..33 of either text and matches that end within 48 symbols of a strand's or the query's
    end: the lanes that build validity masks, the front word that is not read in front of a text; one genome shorter
    than 64 symbols;
(d) N runs next to the matches: the kernel that consults the N masks, which keeps the windowed record;
(e) the other readers of the same code on the set of (b): the join form, the split, one run-time compiled tuple.
The host-side statement of the arithmetic is tests/test_refill_resolve.py (no GPU)."""
import numpy as np
import pytest

import index_model as M
import lzani_ctypes as L
import oracle as O
import synth_genomes as SG
import util as U

pytestmark = pytest.mark.gpu

FORM_ENV = ("LZANI_RTC", "LZANI_RTC_MIN_PAIRS", "LZANI_RTC_CACHE", "LZANI_PM", "LZANI_PM_MIN_ROWS", "LZANI_PM_MIN_SHARE", "LZANI_PM_MAX_BYTES",
            "LZANI_JOIN_MIN_BYTES", "LZANI_NO_JOIN", "LZANI_BLOCK_KERNEL", "LZANI_SPLIT", "LZANI_SPLIT_SEGLEN", "LZANI_SPLIT_ALL",
            "LZANI_SPLIT_S", "LZANI_SPLIT_THR", "LZANI_SPLIT_GIVE_UP", "LZANI_LPT", "LZANI_NO_TAGWORDS", "LZANI_NO_BUCKETS", "LZANI_NO_FILTER",
            "LZANI_FILTER_MAX_BITS", "LZANI_BK_MAX_DIRBITS", "LZANI_MAX_SLOTS", "LZANI_PM_FROM_INDEX")
BITMAPS = {"LZANI_PM_MIN_ROWS": "1", "LZANI_SPLIT": "0", "LZANI_RTC": "0"}
JOIN = {"LZANI_JOIN_MIN_BYTES": "1", "LZANI_PM": "0", "LZANI_RTC": "0"}
SPLIT = {"LZANI_PM_MIN_ROWS": "1", "LZANI_SPLIT": "1", "LZANI_SPLIT_SEGLEN": "1500", "LZANI_SPLIT_ALL": "1", "LZANI_RTC": "0"}
LONG = dict(mal=15, msl=9, reg=60)
MRD = U.DEFAULTS["mrd"]
CAP = 32                          # lzani_kernels_pairs.h: AQ_LANE_CAP, the symbols a lane compares


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
    assert got.shape == want.shape, (what, got.shape, want.shape)      # every directed pair
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.shape[0] * (got.shape[0] - 1)} pairs differ from the oracle, first {bad[:4].tolist()}"


def _candidates(ref, qry, mal, mrd=MRD):
    """(qp, pos, length) of the query positions whose mal-mer occurs exactly once in the reference's text (what a lane
    resolves alone): the position in either text and the number of equal symbols from there on, counted up to 48."""
    rt, qt = M.ref_text(ref, mrd), M.ref_text(qry, mrd)[:len(qry) + mrd]
    rv, rk = M.kmer_keys(rt, mal)
    qv, qk = M.kmer_keys(qt, mal)
    uk, first, cnt = np.unique(rk[rv], return_index=True, return_counts=True)
    rpos = np.nonzero(rv)[0][first]
    j = np.minimum(np.searchsorted(uk, qk), len(uk) - 1)
    hit = qv & (uk[j] == qk) & (cnt[j] == 1)
    qp, pos = np.nonzero(hit)[0], rpos[j[hit]]
    rp, qq = np.concatenate([rt, np.full(64, 4, np.uint8)]), np.concatenate([qt, np.full(64, 5, np.uint8)])
    ln, run = np.zeros(len(qp), np.int64), np.ones(len(qp), bool)
    for k in range(48):
        run &= (rp[pos + k] == qq[qp + k]) & (rp[pos + k] < 4)
        ln += run
    return qp, pos, ln


def _rand(st, n):
    return (st.u64(n) % np.uint64(4)).astype(np.uint8)


def _plant(dst, at, src, st, every=(9, 30)):
    """src laid into dst at `at`, a substitution every 9..30 symbols: matches of a few to a few dozen symbols"""
    seg = src.copy()
    k = st.randint(*every)
    while k < len(seg):
        seg[k] = (seg[k] + 1 + st.randint(0, 2)) % 4
        k += 1 + st.randint(*every)
    dst[at:at + len(seg)] = seg


# ---- (a) symbol offsets ---------------------------------------------------------------------------------------------

def _offset_set():
    st = SG.Stream(7201)
    base = _rand(st, 6000)
    seqs = [base]
    for k in range(1, 16):                                          # 6 % substitutions and a few indels, k symbols in front
        seqs.append(np.concatenate([_rand(st, k), SG.mutate(base, 0.06, st)]))
    seqs.append(_rand(st, 5800))
    return [np.ascontiguousarray(s) for s in seqs]


def test_every_symbol_offset_of_both_texts(monkeypatch):
    seqs = _offset_set()
    mal = U.DEFAULTS["mal"]
    seen = np.zeros((16, 16), np.int64)
    for q in range(1, 16):                                          # the candidates a lane compares and records: mal <= length <= 32
        for r in (0, (q % 15) + 1):
            qp, pos, ln = _candidates(seqs[r], seqs[q], mal)
            keep = (ln >= mal) & (ln <= CAP) & (qp >= 32) & (pos >= 32)
            np.add.at(seen, (qp[keep] & 15, pos[keep] & 15), 1)
    print("candidates per (qp & 15, pos & 15): min", int(seen.min()), "max", int(seen.max()))
    assert seen.min() > 0, np.argwhere(seen == 0).tolist()
    got, lay, rec = _run(monkeypatch, seqs, None, BITMAPS)
    assert lay["bitmap_launches"] > 0 and any("nfree=1" in k and "cand=2" in k for k in rec), (lay, rec)
    _check(got, O.oracle_all2all(seqs, None, threads=16), "symbol offsets")


# ---- (b) match lengths ----------------------------------------------------------------------------------------------

_LEN = {}


def _length_set():
    """Two unrelated genomes of ~8.6 kbp, and a third that carries, every 90 symbols, a match of m = 11..40 symbols with the
    first (thrice each, at varying word offsets) between symbols that differ; the oracle's answers at both tuples."""
    if not _LEN:
        st = SG.Stream(7202)
        a, b, c = _rand(st, 8600), _rand(st, 8500), _rand(st, 8400)
        plants = []
        at = 150
        for rep in range(3):
            for m in range(11, 41):
                pa = 200 + 91 * len(plants) + st.randint(0, 15)
                pb = at + st.randint(0, 15)
                b[pb:pb + m] = a[pa:pa + m]
                b[pb - 1] = (a[pa - 1] + 1 + st.randint(0, 2)) % 4
                b[pb + m] = (a[pa + m] + 1 + st.randint(0, 2)) % 4
                plants.append((pb, pa, m))
                at += 90
        _LEN["seqs"] = [np.ascontiguousarray(s) for s in (a, b, c)]
        _LEN["plants"] = plants
        _LEN["want"] = {None: O.oracle_all2all(_LEN["seqs"], None, threads=16)}
    return _LEN["seqs"], _LEN["plants"]


def _length_want(prm):
    key = None if prm is None else tuple(sorted(prm.items()))
    if key not in _LEN["want"]:
        _LEN["want"][key] = O.oracle_all2all(_LEN["seqs"], prm, threads=16)
    return _LEN["want"][key]


def _assert_planted_lengths(seqs, plants, mal):
    qp, pos, ln = _candidates(seqs[0], seqs[1], mal)
    have = {(int(a), int(b), int(c)) for a, b, c in zip(qp, pos, ln)}
    missing = [p for p in plants if p[2] >= mal and p not in have]
    assert not missing, missing[:5]
    assert {m for _, _, m in plants if m >= mal} == set(range(mal, 41))


@pytest.mark.parametrize("prm", (None, LONG), ids=("defaults", "mal15"))
def test_every_match_length_across_the_lane_cap(monkeypatch, prm):
    seqs, plants = _length_set()
    _assert_planted_lengths(seqs, plants, U.full_params(prm)["mal"])
    got, lay, rec = _run(monkeypatch, seqs, prm, BITMAPS)
    assert lay["bitmap_launches"] > 0 and all("cand=2" in k and f"defp={2 if prm else 1}" in k for k in rec), (lay, rec)
    _check(got, _length_want(prm), "match lengths")


# ---- (c) text edges -------------------------------------------------------------------------------------------------

def _edge_set():
    st = SG.Stream(7203)
    a, b, c, d = _rand(st, 3100), _rand(st, 4700), _rand(st, 2300), _rand(st, 2000)
    rc = lambda x: (3 - x[::-1]).astype(np.uint8)
    _plant(b, 0, a[1000:1090], st)              # query start   <- reference interior
    _plant(b, 600, a[:90], st)                  # reference start
    _plant(b, 900, a[-90:], st)                 # reference end: matches that end in front of L
    _plant(b, 1200, rc(a[-90:]), st)            # start of the reverse-complement strand (rc0 ..)
    _plant(b, 1500, rc(a[:90]), st)             # its end: matches that end in front of rc0 + L
    _plant(b, len(b) - 90, a[2000:2090], st)    # query end     <- reference interior
    _plant(c, 0, a[:90], st)                    # both starts at once, both ends at once
    _plant(c, len(c) - 90, a[-90:], st)
    _plant(d, 0, rc(a[-90:]), st)               # query start against the strand's start, query end against the strand's end
    _plant(d, len(d) - 90, rc(a[:90]), st)
    tiny = a[500:550].copy()                    # shorter than 64 symbols (and than one bitmap word)
    tiny[25] = (tiny[25] + 1) % 4
    return [np.ascontiguousarray(s) for s in (a, b, c, d, tiny)]


def test_candidates_at_the_ends_of_the_texts(monkeypatch):
    seqs = _edge_set()
    mal = U.DEFAULTS["mal"]
    La, rc0 = len(seqs[0]), len(seqs[0]) + 2 * MRD
    near = lambda end, e: (end - e >= 0) & (end - e <= 48)
    for q in (1, 2, 3):
        qp, pos, ln = _candidates(seqs[0], seqs[q], mal)
        ok = (ln >= mal) & (ln <= CAP)
        qp, pos, ln = qp[ok], pos[ok], ln[ok]
        Lq = len(seqs[q])
        facts = {"qp <= 33": qp <= 33, "match ends at the query's end": near(Lq, qp + ln)}
        if q == 1:
            facts.update({"pos <= 33": pos <= 33, "ends in front of L": near(La, pos + ln), "pos at rc0 .. rc0 + 33": (pos >= rc0) & (pos <= rc0 + 33),
                          "ends in front of rc0 + L": near(rc0 + La, pos + ln)})
        if q == 2:
            facts.update({"both starts": (qp <= 33) & (pos <= 33), "both ends": near(Lq, qp + ln) & near(La, pos + ln)})
        if q == 3:
            facts.update({"query start, strand start": (qp <= 33) & (pos >= rc0) & (pos <= rc0 + 33), "query end, strand end": near(Lq, qp + ln) & near(rc0 + La, pos + ln)})
        counts = {k: int(v.sum()) for k, v in facts.items()}
        print("query", q, counts)
        assert all(counts.values()), (q, counts)
    qp, pos, ln = _candidates(seqs[0], seqs[4], mal)
    assert len(seqs[4]) < 64 and ((ln >= mal) & (ln <= CAP)).sum() >= 2, (qp, pos, ln)
    got, lay, rec = _run(monkeypatch, seqs, None, BITMAPS)
    assert lay["bitmap_launches"] > 0 and any("nfree=1" in k and "cand=2" in k for k in rec), (lay, rec)
    _check(got, O.oracle_all2all(seqs, None, threads=16), "text edges")


# ---- (d) N runs -----------------------------------------------------------------------------------------------------

def test_n_runs_next_to_the_matches(monkeypatch):
    seqs, plants = _length_set()
    seqs = [s.copy() for s in seqs]
    b = seqs[1]
    for k, (pb, _, m) in enumerate(plants):                         # in front of a match, behind it, both, neither
        if k % 4 in (0, 2):
            b[pb - 2 - k % 5:pb - 1] = 5
        if k % 4 in (1, 2):
            b[pb + m + 1:pb + m + 2 + k % 7] = 5
    mal = U.DEFAULTS["mal"]
    qp, pos, ln = _candidates(seqs[0], b, mal)
    have = {(int(x), int(y), int(z)) for x, y, z in zip(qp, pos, ln)}
    assert all(p in have for p in plants), [p for p in plants if p not in have][:5]
    isn = np.nonzero(b > 3)[0]
    assert all(np.any((isn >= pb - 16) & (isn < pb + m + 16)) for k, (pb, _, m) in enumerate(plants) if k % 4 != 3)
    got, lay, rec = _run(monkeypatch, seqs, None, BITMAPS)
    assert lay["bitmap_launches"] > 0 and any("nfree=0" in k and "cand=2" in k for k in rec), (lay, rec)
    _check(got, O.oracle_all2all(seqs, None, threads=16), "N runs next to the matches")


# ---- (e) the other readers of the same code -------------------------------------------------------------------------

def test_join_form(monkeypatch):
    seqs, plants = _length_set()
    _assert_planted_lengths(seqs, plants, U.DEFAULTS["mal"])
    got, lay, rec = _run(monkeypatch, seqs, None, JOIN)
    assert rec and all("cand=1" in k for k in rec), (lay, rec)
    _check(got, _length_want(None), "join form")


def test_split_forced(monkeypatch):
    seqs, plants = _length_set()
    _assert_planted_lengths(seqs, plants, U.DEFAULTS["mal"])
    got, lay, rec = _run(monkeypatch, seqs, None, SPLIT)
    n = len(seqs)
    assert lay["split_launches"] >= 1 and lay["split_segments"] >= 2 * n * (n - 1) and any("split " in k for k in rec), (lay, rec)
    _check(got, _length_want(None), "split")


def test_run_time_compiled_tuple(monkeypatch, tmp_path):
    seqs, plants = _length_set()
    prm = dict(reg=36)
    _assert_planted_lengths(seqs, plants, U.full_params(prm)["mal"])
    env = {"LZANI_RTC_MIN_PAIRS": "0", "LZANI_RTC_CACHE": str(tmp_path), "LZANI_PM_MIN_ROWS": "1"}
    got, lay, rec = _run(monkeypatch, seqs, prm, env)
    assert lay["rtc_launches"] >= 1 and rec and all(k.startswith("rtc ") for k in rec), (lay, rec)
    _check(got, _length_want(prm), "run-time compiled tuple")
