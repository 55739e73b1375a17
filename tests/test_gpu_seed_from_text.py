"""GPU: in the kernels of the hand-written loops the tracking rounds of a pair without N take the query's seed words from the
packed query text at msl <= 7 (DevWave::query_seed_word and form T of the loops' loads, lzani_kernels_pairs.h; lzani_core.h: kms_from_syms,
kms_valid_nfree_head) -- two text dwords, a funnel shift by 2 ((i + lane) & 15), a mask, and KM_INVALID where the msl-mer would
run beyond the query's last symbol.  Every case runs through the C-ABI, is bit-exact against the CPU oracle on every pair and
asserts from the launch record that the kernel it is about ran.
(a) Text-word seams and the query's end: 32 random genomes without N whose lengths run through 16 consecutive values (every
    L mod 16) and two of 70..130 bp.  Asserted from the raw sequences before the run: the set holds matches of mal symbols
    and more that END 8..47 symbols in front of the query's end -- the 41 tracking steps behind each reach beyond Lq - msl --
    and matches that end nearer still; their ends cover every i mod 16.  Which of those rounds the null chain takes is not
    a fact of the sequences (it leaves where nothing is queued behind the match), so it is counted: pairs laid out for it
    (tests/seed_text_cover.py) run on the coverage library with and without a second match behind the first, and the
    chain's own counters must show that it committed the second one -- behind a round that starts 15..35 symbols in front
    of the query's end -- and that without it the round was not the chain's.  Those pairs also hold the reference window
    "the query's last symbols + zero bits", the one a step without KM_INVALID would take for a seed candidate.
(b) Related genomes: the same lengths as two families at 5 % divergence (seed events, close matches); and two families of
    8.4 kbp, the shortest texts whose index has tag words without candidate bitmaps: the probe form's kernel with the anchor
    queue, the one with the stretch chain at the defaults.  (The probe form of (a)'s set has no tag words: its kernel has
    neither hand-written loop and keeps the kmS load in every round, find_event_round's -- run as one of (c).)
(c) Paths that keep the load: one genome of the set carries an N run (the kernels with NFREE false keep the kmS load) beside the
    N-free context of (a); the set at msl 9 (the word carries hash bits: the kmS load); a run-time compiled tuple at msl 7.
The host-side statement of the word and its validity rule is tests/test_seed_word.py (no GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import index_model as M
import lzani_ctypes as L
import oracle as O
import path_cover as PC
import seed_text_cover as STC
import synth_genomes as SG
import util as U

pytestmark = pytest.mark.gpu

FORM_ENV = ("LZANI_RTC", "LZANI_RTC_MIN_PAIRS", "LZANI_RTC_CACHE", "LZANI_PM", "LZANI_PM_MIN_ROWS", "LZANI_PM_MIN_SHARE", "LZANI_PM_MAX_BYTES",
            "LZANI_JOIN_MIN_BYTES", "LZANI_NO_JOIN", "LZANI_BLOCK_KERNEL", "LZANI_SPLIT", "LZANI_SPLIT_SEGLEN", "LZANI_SPLIT_ALL",
            "LZANI_SPLIT_S", "LZANI_SPLIT_THR", "LZANI_SPLIT_GIVE_UP", "LZANI_LPT", "LZANI_NO_TAGWORDS", "LZANI_NO_BUCKETS", "LZANI_NO_FILTER",
            "LZANI_FILTER_MAX_BITS", "LZANI_BK_MAX_DIRBITS", "LZANI_MAX_SLOTS", "LZANI_PM_FROM_INDEX")
BITMAPS = {"LZANI_PM_MIN_ROWS": "1", "LZANI_SPLIT": "0", "LZANI_RTC": "0"}       # candidate bitmaps: the dense rows' kernel
PROBE = {"LZANI_PM": "0", "LZANI_NO_JOIN": "1", "LZANI_SPLIT": "0", "LZANI_RTC": "0"}   # a probe per query position; with tag words: the stretch chain
MAL, MSL, MRD, MQD = (U.DEFAULTS[k] for k in ("mal", "msl", "mrd", "mqd"))
L0 = 2992                          # lengths L0 .. L0 + 15, two genomes each
L0P = 8400                         # (b), probe form: 2 L + 3 mrd > 2^14, i.e. 15 directory bits and 7-bit tags (tests/util.py: index_form)

_SETS = {}


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


def _rand(st, n):
    return (st.u64(n) % np.uint64(4)).astype(np.uint8)


def _match_ends(ref, qry, mal=MAL, mrd=MRD):
    """query positions behind the matches of mal symbols and more that start at a query position whose mal-mer occurs once in
    the reference's text (what the anchor queue resolves): where the tracking round behind such a match starts, at the least"""
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
    keep = (ln >= mal) & (ln < 48)
    return np.unique(qp[keep] + ln[keep])


def _seam_set():
    """(a): random genomes; genome k carries, 8 + k symbols in front of its end, 12..20 symbols of genome k + 1 between
    symbols that differ -- a match whose tracking round reaches beyond the query's last msl-mer -- and half of them a
    second one 1..7 symbols in front of the end"""
    if "seam" not in _SETS:
        st = SG.Stream(7301)
        seqs = [_rand(st, L0 + k // 2) for k in range(32)]
        for k in range(32):
            q, r = seqs[k], seqs[(k + 1) % 32]
            m = 12 + k % 9
            at = len(q) - (8 + k) - m
            src = 400 + 37 * k
            q[at:at + m] = r[src:src + m]
            q[at - 1] = (r[src - 1] + 1 + st.randint(0, 2)) % 4
            q[at + m] = (r[src + m] + 1 + st.randint(0, 2)) % 4
            if k % 2:
                d = 1 + (k // 2) % 7
                at = len(q) - d - 14
                q[at:at + 14] = r[1500 + k:1514 + k]
                q[at - 1] = (r[1499 + k] + 1 + st.randint(0, 2)) % 4
                q[at + 14] = (r[1514 + k] + 1 + st.randint(0, 2)) % 4
        seqs += [_rand(st, 83), _rand(st, 127)]
        seqs[32][20:60] = seqs[0][100:140]                 # the short ones share a stretch with a long one and with each other
        seqs[33][50:110] = seqs[32][10:70]
        seqs[33][80] = (seqs[33][80] + 1) % 4
        _SETS["seam"] = [np.ascontiguousarray(s) for s in seqs]
        _SETS["seam_want"] = {}
    return _SETS["seam"]


def _want(name, seqs, prm=None):
    key = None if prm is None else tuple(sorted(prm.items()))
    store = _SETS.setdefault(name + "_want", {})
    if key not in store:
        store[key] = O.oracle_all2all(seqs, prm, threads=16)
    return store[key]


def _assert_rounds_at_the_end(seqs):
    chain, general, starts = 0, 0, set()               # (the zones the round behind a match falls into, by position alone)
    for k in range(32):
        q, r = seqs[k], seqs[(k + 1) % 32]
        end = _match_ends(r, q)
        Lq = len(q)
        beyond = end + MQD > Lq - MSL                      # the round's last step has no msl-mer
        in_chain = beyond & (end <= Lq - 8)                # i <= iend - (mqd + 1), iend = Lq + mrd - msl
        chain += int(in_chain.sum())
        general += int((beyond & ~in_chain & (end < Lq)).sum())
        starts |= {int(e) & 15 for e in end[in_chain]}
    print("matches whose round reaches beyond Lq - msl: ending at or before Lq - 8", chain, "nearer the end", general, "i mod 16 among the first", sorted(starts))
    assert chain >= 24 and general >= 12 and len(starts) == 16, (chain, general, sorted(starts))      # (a second plant may overwrite the first of its genome)
    assert sorted({len(s) % 16 for s in seqs[:32]}) == list(range(16)) and all(70 <= len(s) <= 130 for s in seqs[32:])


def test_text_word_seams_and_the_querys_end(monkeypatch):
    seqs = _seam_set()
    _assert_rounds_at_the_end(seqs)
    got, lay, rec = _run(monkeypatch, seqs, None, BITMAPS)
    assert lay["bitmap_launches"] > 0 and rec and all("nfree=1" in k and "cand=2" in k and "defp=1" in k for k in rec), (lay, rec)
    _check(got, _want("seam", seqs), "seams and the query's end, bitmap form")


def test_text_word_seams_probe_form(monkeypatch):
    seqs = _seam_set()
    got, lay, rec = _run(monkeypatch, seqs, None, PROBE)
    assert rec and all("nfree=1" in k and "bk=0 cand=0" in k for k in rec), (lay, rec)
    _check(got, _want("seam", seqs), "seams and the query's end, probe form")


def _related_set(form):
    """two families at 5 % divergence from their ancestors, the lengths l0 .. l0 + 15 in each (probe form: 8 a family, each length once)"""
    name = "rel_" + form
    if name not in _SETS:
        st = SG.Stream(7302 if form == "bitmaps" else 7303)
        l0, per = (L0, 16) if form == "bitmaps" else (L0P, 8)
        seqs = []
        for fam in range(2):
            anc = _rand(st, l0 + 40)
            for k in range(per):
                g = SG.mutate(anc, 0.05, st)
                n = l0 + (k if per == 16 else 8 * fam + k)
                g = g[:n] if len(g) >= n else np.concatenate([g, _rand(st, n - len(g))])
                seqs.append(np.ascontiguousarray(g.astype(np.uint8)))
        _SETS[name] = seqs
    return name, _SETS[name]


@pytest.mark.parametrize("form", ("bitmaps", "probe"))
def test_related_genomes(monkeypatch, form):
    name, seqs = _related_set(form)
    per = len(seqs) // 2
    assert sorted({len(s) % 16 for s in seqs}) == list(range(16)) and all(int(s.max()) < 4 for s in seqs)
    got, lay, rec = _run(monkeypatch, seqs, None, BITMAPS if form == "bitmaps" else PROBE)
    assert rec and all("nfree=1" in k and "defp=1" in k and ("bk=1 cand=2" if form == "bitmaps" else "bk=1 cand=0") in k for k in rec), (lay, rec)
    want = _want(name, seqs)
    assert want[0, 1, 0] > len(seqs[0]) // 2 and want[0, per + 1, 0] < len(seqs[0]) // 10, (want[0, 1], want[0, per + 1])      # a family shares most of its symbols, two families next to none
    _check(got, want, "related genomes, " + form)


def test_a_genome_with_an_n_run_keeps_the_load(monkeypatch):
    seqs = [s.copy() for s in _seam_set()]
    seqs[5][1000:1030] = 5
    got, lay, rec = _run(monkeypatch, seqs, None, BITMAPS)
    assert lay["bitmap_launches"] > 0 and rec and all("nfree=0" in k and "cand=2" in k for k in rec), (lay, rec)
    _check(got, _want("seam_n", seqs), "one genome with an N run")


def test_msl_9_keeps_the_load(monkeypatch):
    seqs = _seam_set()
    prm = dict(msl=9)
    got, lay, rec = _run(monkeypatch, seqs, prm, BITMAPS)
    assert rec and all("nfree=1" in k for k in rec), (lay, rec)
    _check(got, _want("seam", seqs, prm), "msl 9")


def test_run_time_compiled_tuple(monkeypatch, tmp_path):
    seqs = _seam_set()
    prm = dict(reg=36)
    env = {"LZANI_RTC_MIN_PAIRS": "0", "LZANI_RTC_CACHE": str(tmp_path), "LZANI_PM_MIN_ROWS": "1"}
    got, lay, rec = _run(monkeypatch, seqs, prm, env)
    assert lay["rtc_launches"] >= 1 and rec and all(k.startswith("rtc ") for k in rec), (lay, rec)
    _check(got, _want("seam", seqs, prm), "run-time compiled tuple")


def test_the_chain_commits_behind_rounds_that_reach_beyond_the_last_msl_mer():
    """tests/seed_text_cover.py: the child's lines, one per pair.  A pair shows it if its two runs differ by exactly the second
    match -- 2 commits of the chain more (one per direction), no event more by the general path.  At least half of the 16
    pairs must (a chance hit or a forward extension of the first match into the second changes a pair's picture); every run
    is the candidate-bitmap kernel for genomes without N and equals the oracle."""
    lib = L.build_diag_library()              # (built by __graft_entry__.build(); here only if it is missing or stale)
    env = dict(os.environ, LZANI_LIB=lib)
    p = subprocess.run(["timeout", "-k", "10", "200", sys.executable, os.path.join(STC.HERE, "seed_text_cover.py")], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    rows = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert [r["k"] for r in rows] == list(range(STC.CASES))
    C, G, N = (PC.CHAIN_SLOTS.index(x) for x in ("commits", "events_general", "exit_nothing"))
    shown = []
    for r in rows:
        assert r["with_ok"] and r["without_ok"], r
        for key in ("with_kernels", "without_kernels"):
            assert r[key] and all("nfree=1" in k and "defp=1" in k and "cand=2" in k for k in r[key]), r
        d = [a - b for a, b in zip(r["with"], r["without"])]
        print("pair", r["k"], "commits", r["without"][C], "->", r["with"][C], "events_general", r["without"][G], "->", r["with"][G],
              "exit_nothing", r["without"][N], "->", r["with"][N])
        if d[C] == 2 and d[G] == 0:
            shown.append(r["k"])
    assert len(shown) >= STC.CASES // 2, shown
