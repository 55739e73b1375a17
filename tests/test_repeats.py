"""CPU: the pair path on repeat-structured genomes (tests/repeat_genomes.py, tests/repeat_ties.py).

The random genomes of the other tests hold a k-mer once; here at least 15 % of the 11-mers of a genome of 8 kbp or more occur
more than once, one of them 16 times or more, and at least 10 % of the 21-mers do (asserted below).  This file pins
everything the GPU tests of tests/test_gpu_repeats.py compare the device with:
- the generator: the conditions on its output, and a checksum of every named set;
- the reference build (where oracle/_ref is built; its recorded answers of tests/golden/repeat_vectors.json everywhere), the
  oracle, the host model of the kernels and the model's two split runs agree on every named set and on 24 seeded sets, under
  six parameter tuples, regions of the related pairs included;
- the tie cases: which occurrence of a repeated k-mer the parse takes, stated case by case and asserted from the regions;
- the conditions that make the prefilter's GPU test meaningful."""
import json
import os
import time

import numpy as np
import pytest

import oracle as O
import prefilter_model as PM
import repeat_genomes as RG
import repeat_ties as RT
import synth_genomes as SG
import util as U

PRM_NAMES = ("defaults", "long", "rtc_chain", "generic", "slow", "chain")
N_FUZZ = 24
CHECKSUMS = {"small": 1148848280, "small N": 4041387137, "split": 760150264, "split N": 1040223856, "mid": 1780726521,
             "mid N": 1322096561, "long": 3166499075, "long N": 1698580550}
EXIT_CHECKSUMS = {"exits": 2987010118, "exits N": 1291578073}
_SPLIT_STATS = {}


def params_of(name, seed):
    """The six tuples: five of util.INST_PARAMS and a seeded tuple of util.fuzz_params_chain."""
    return U.fuzz_params_chain(SG.Stream(0xC4A1 + seed)) if name == "chain" else U.INST_PARAMS[name]


def load_recorded():
    with open(os.path.join(U.GOLD, "repeat_vectors.json")) as f:
        return json.load(f)


# ---- the generator ---------------------------------------------------------------------------------------------------------
def test_named_sets_do_not_drift():
    assert {name: RG.checksum(RG.repeat_set(name)) for name in RG.SET_NAMES} == CHECKSUMS


def test_exit_sets_do_not_drift_and_hold_their_motifs():
    """The exit sets' bytes depend on the seed alone; the relative differs from its ancestor in the bursts alone, at every
    symbol of a burst; a 'several' motif's seed stands twice in the ancestor, 30 apart; only the last genome of 'exits N'
    holds N; the stranger carries the reverse complement of the ancestor's first 30 symbols; host model and oracle agree."""
    assert {name: RG.checksum(RG.exit_set(name)) for name in RG.EXIT_SET_NAMES} == EXIT_CHECKSUMS
    g, h, x, m = RG.exit_set("exits")
    L = len(g)
    assert L == len(h) == RG.EXIT_LEN
    kinds = list(RG.EXIT_MOTIFS)
    starts = list(range(RG.EXIT_FIRST, L - RG.EXIT_STEP - 200, RG.EXIT_STEP))
    assert len(starts) >= 3 * len(kinds)
    burst = np.zeros(L, bool)
    for k, s in enumerate(starts):
        for a, b in RG.EXIT_MOTIFS[kinds[k % len(kinds)]]:
            burst[s + a:s + b] = True
        if kinds[k % len(kinds)] == "several":
            assert np.array_equal(g[s + 78:s + 88], g[s + 108:s + 118])
    for a, b in RG.EXIT_TAIL:
        burst[L + a:L + b] = True
    assert np.array_equal(g != h, burst)
    assert np.array_equal(x[3000:3030], RG.rc(g[:30])) and np.array_equal(x[3330:3360], g[5000:5030])
    gn = RG.exit_set("exits N")
    assert [bool((s > 3).any()) for s in gn] == [False, False, False, True] and gn[3][0] > 3 and gn[3][-1] > 3
    assert all(np.array_equal(a, b) for a, b in zip(gn[:3], (g, h, x)))
    for name in RG.EXIT_SET_NAMES:
        for pn in ("defaults", "long"):
            want = O.oracle_all2all(RG.exit_set(name), U.INST_PARAMS[pn], threads=8)
            assert np.array_equal(U.model_all2all(RG.exit_set(name), U.INST_PARAMS[pn]), want), (name, pn)


@pytest.mark.parametrize("name", RG.SET_NAMES)
def test_named_sets_mirror_the_instantiation_sets(name):
    """Same genome count, every length in the range of the random set's genome at that place, the 300 bp genome last; N-free
    without ' N'; with it the runs of util._put_n_runs and one inside a repeat copy; a family with an exact copy and one with
    a whole-genome reverse complement; every genome of 8 kbp or more repeat-rich: 11-mer share >= 0.15 with a multiplicity
    >= 16, 21-mer share >= 0.10."""
    seqs, rnd = RG.repeat_set(name), U.instantiation_set(name)
    base = name.split(" ")[0]
    assert len(seqs) == len(rnd) and len(seqs[-1]) == 300
    off = 2 if base in RG.BIG_LEN else 0
    lo, hi = RG.SET_RANGES["split" if base == "split" else "small"]
    assert all(lo <= len(s) <= hi for s in seqs[off:-1]), [len(s) for s in seqs]
    if off:
        # the relative: one family copy gained and one lost (an element is 12,000 symbols at the most), units and indels
        assert len(seqs[0]) == RG.BIG_LEN[base] == len(rnd[0]) and abs(len(seqs[1]) - len(seqs[0])) < 12000 + 0.01 * len(seqs[0])
    same = lambda a, b: len(a) == len(b) and np.array_equal(a[(a < 4) & (b < 4)], b[(a < 4) & (b < 4)])      # (but for N runs)
    assert same(seqs[off], seqs[off + 3]) and same(seqs[off + 6], RG.rc(seqs[off + 4]))
    if name.endswith(" N"):
        i, a, ln, (s0, s1) = RG.repeat_set_info(name)["n_in_repeat"]
        with_n = lambda group: {k for k, s in enumerate(group) if (s > 3).any()}
        assert with_n(seqs) == with_n(rnd) | {i} and len(seqs) - len(with_n(seqs)) >= 2
        assert s0 < a and a + ln < s1 and (seqs[i][a:a + ln] > 3).all() and (seqs[i][s0:a] < 4).all()
        assert any(s[0] > 3 for s in seqs) and any(s[-1] > 3 for s in seqs)
    else:
        assert all((s < 4).all() for s in seqs)
    for s in seqs:
        if len(s) >= 8000:
            share11, mult11 = RG.repeat_stats(s, 11)
            share21, _ = RG.repeat_stats(s, 21)
            assert share11 >= 0.15 and mult11 >= 16 and share21 >= 0.10, (name, len(s), share11, mult11, share21)


def test_random_genomes_hold_a_kmer_once():
    """The measurement the repeat sets answer: the random sets stay below 1 % with multiplicity 2 (3 at most), no 21-mer."""
    for s in U.instantiation_set("small")[:-1]:
        share, mult = RG.repeat_stats(s, 11)
        assert share < 0.01 and mult <= 3 and RG.repeat_stats(s, 21) == (0.0, 1)
    assert RG.repeat_stats(np.zeros(10, np.uint8), 4) == (1.0, 7)                     # AAAA seven times, TTTT seven times
    assert RG.repeat_stats(np.array([0, 1, 2, 3], np.uint8), 4) == (1.0, 2)           # ACGT is its own reverse complement
    assert RG.repeat_stats(np.array([0, 0, 0, 1, 5, 0, 0, 0, 1, 2], np.uint8), 4) == (4 / 6, 2)   # AAAC, N, AAAC, AACG and the other strand's three


@pytest.mark.parametrize("seed", range(N_FUZZ))
def test_structured_genomes_meet_the_conditions_and_the_caps(seed):
    st = SG.Stream(5000 + seed)
    L = st.randint(8000, 40000)
    lay = RG.structured_layout(st, L)
    g = lay.codes()
    assert len(g) == L and (g < 4).all()
    share11, mult11 = RG.repeat_stats(g, 11)
    assert share11 >= 0.15 and mult11 >= 16 and RG.repeat_stats(g, 21)[0] >= 0.10
    rel = RG.relative_layout(lay, st, 0.15)
    for lay_ in (lay, rel):
        fam = {}
        for kind, ident, x in lay_.pieces:
            if kind == "homo":
                assert len(x) <= RG.MAX_HOMO
            if kind == "tan":
                assert len(x) <= RG.MAX_ARRAY
            if kind == "fam":
                fam[ident] = fam.get(ident, 0) + 1
        assert fam and max(fam.values()) <= RG.MAX_COPIES and min(fam.values()) >= 2
    kinds = {p[0] for p in lay.pieces}
    assert kinds == {"bb", "fam", "tan", "homo", "dup", "pal", "term"}
    # N runs at the relative's repeat copies (its copy-number and array changes: the next test)
    for k, p in enumerate(rel.pieces):
        rel.pieces[k] = (p[0], p[1], p[2].copy())
    runs = RG.put_n_at_repeat(rel, st)
    h = rel.codes()
    assert len(runs) == 2 and all((h[a:a + n] > 3).all() for a, n in runs) and int((h > 3).sum()) == sum(n for _, n in runs)
    spans = rel.spans()
    assert any(a < runs[0][0] and runs[0][0] + runs[0][1] < b for a, b in spans)         # inside a copy
    assert any(runs[1][0] + runs[1][1] == a for a, _ in spans)                             # ends where a copy starts


def test_relatives_gain_and_lose_copies_and_units():
    """Each change of a relative on its own, from what relative_layout says it did and checked on the pieces: over the seeds
    a family gains a copy, a family loses one (never the same family: the two would cancel), a tandem array gets more whole
    units and another one fewer."""
    seen = set()
    for seed in range(N_FUZZ):
        st = SG.Stream(5000 + seed)
        lay = RG.structured_layout(st, st.randint(8000, 40000))
        rel = RG.relative_layout(lay, st, 0.05)
        ch = rel.changes
        copies = lambda la: np.array([sum(1 for p in la.pieces if p[:2] == ("fam", i)) for i in range(len(la.elements))])
        dc = copies(rel) - copies(lay)
        want = np.zeros(len(dc), dtype=np.int64)
        if ch["gained"] is not None:
            want[ch["gained"]] += 1
        if ch["lost"] is not None:
            want[ch["lost"]] -= 1
        assert np.array_equal(dc, want) and (ch["gained"] is None or ch["gained"] != ch["lost"]), (seed, dc, ch)
        seen |= {k for k in ("gained", "lost") if ch[k] is not None}
        arrays = {p[1]: len(p[2]) for p in rel.pieces if p[0] == "tan"}
        for ident, (before, after) in ch["units"].items():
            unit = arrays[ident] // after                                     # the relative's own unit, indels included
            assert arrays[ident] == after * unit and abs(unit - len(lay.units[ident])) <= 12, (seed, ident)
            assert before == sum(len(p[2]) for p in lay.pieces if p[:2] == ("tan", ident)) // len(lay.units[ident])
            seen |= {"expansion"} if after > before else {"contraction"} if after < before else set()
        assert sum(a != b for b, a in ch["units"].values()) <= 2
    assert seen == {"gained", "lost", "expansion", "contraction"}, seen


def test_width_units_are_in_the_sets():
    """Tandem units of exactly 16, 32 and 64 bp occur over the seeded sets."""
    seen = set()
    for seed in range(N_FUZZ):
        lay = RG.structured_layout(SG.Stream(9000 + seed), 9000)
        seen |= {len(u) for u in lay.units}
    assert set(RG.WIDTH_UNITS) <= seen


def test_oracle_time_on_the_named_sets():
    """A pair must not go quadratic: the oracle's all2all of a set within 2 s on 16 threads, the 2.2 Mbp sets within 10 s."""
    for name in RG.SET_NAMES:
        seqs = RG.repeat_set(name)
        for pn in ("defaults", "long"):
            t0 = time.time()
            O.oracle_all2all(seqs, U.INST_PARAMS[pn], threads=16)
            dt = time.time() - t0
            print(f"oracle all2all of '{name}' under {pn}: {dt:.2f} s")
            assert dt < (10.0 if name.startswith("long") else 2.0), (name, pn, dt)


def test_every_cell_still_selects_its_kernel():
    for c in U.INST_CELLS:
        seqs = RG.repeat_set(c["set"])
        ref_ids, off, q = U.instantiation_rows(c, len(seqs))
        got = U.predict_kernels(seqs, U.INST_PARAMS[c["prm"]], c["env"], c["form"], pairs_per_row=int(off[1] - off[0]),
                                n_rows=len(ref_ids), rtc_ready=c["name"].startswith("rtc "))
        assert got == U.kernel_names_of_cell(c), (c["id"], got)
        if "nfree=" in c["name"]:
            assert int("nfree=1" in c["name"]) == int(all((s < 4).all() for s in seqs)), c["id"]


# ---- reference build, oracle, host model, split models ---------------------------------------------------------------------
def agree(seqs, prm, related, what):
    """oracle == reference build (where built) == model == both split models at cuts every 512 positions; regions of the
    related pairs: model == oracle (== reference build).  Returns the split run's counts."""
    want = O.oracle_all2all(seqs, prm, threads=16)
    if O.lib_ref() is not None:
        assert np.array_equal(O.ref_all2all(seqs, prm, threads=16), want), what
    assert np.array_equal(U.model_all2all(seqs, prm), want), what
    s1, _ = U.model_split_all2all(seqs, prm, 512)
    s2, stats = U.model_split_rounds(seqs, prm, 512)
    assert np.array_equal(s1, want) and np.array_equal(s2, want), what
    n_regs = 0
    for r, q in related:
        res, regs = O.oracle_pair(seqs[r], seqs[q], prm, want_regions=True)
        mres, mregs = U.model_pair_regions(seqs[r], seqs[q], prm)
        assert res == mres == tuple(want[r, q]) and np.array_equal(regs, mregs), (what, r, q)
        if O.lib_ref() is not None:
            rres, rregs = O.ref_pair(seqs[r], seqs[q], prm, want_regions=True)
            assert rres == res and np.array_equal(rregs, regs), (what, r, q)
        n_regs += len(regs)
    assert n_regs > 0, what
    return stats


@pytest.mark.parametrize("pn", PRM_NAMES)
@pytest.mark.parametrize("name", [n for n in RG.SET_NAMES if not n.startswith("long")])
def test_named_sets_agree(name, pn):
    prm = params_of(pn, RG.SET_NAMES.index(name))
    _SPLIT_STATS[(name, pn)] = agree(RG.repeat_set(name), prm, RG.related_pairs(name), (name, pn, prm))


@pytest.mark.parametrize("seed", range(N_FUZZ))
def test_fuzz_sets_agree(seed):
    seqs = RG.fuzz_set(seed)
    assert all(8000 <= len(s) <= 45000 for s in seqs) and np.array_equal(seqs[0], seqs[4])
    related = [(r, q) for r in (0, 1, 2, 4) for q in (0, 1, 2, 4) if r != q]
    for pn in PRM_NAMES:
        prm = params_of(pn, 100 + seed)
        _SPLIT_STATS[(seed, pn)] = agree(seqs, prm, related, (seed, pn, prm))


@pytest.mark.parametrize("name", ["long", "long N"])
def test_long_sets_one_related_pair(name):
    """The 2.2 Mbp genome and its relative, both directions, under the two tuples the long cells run."""
    seqs = RG.repeat_set(name)[:2]
    for pn in ("defaults", "long"):
        prm = U.INST_PARAMS[pn]
        want = O.oracle_all2all(seqs, prm, threads=2)
        assert np.array_equal(U.model_all2all(seqs, prm), want) and want[0, 1, 0] > 1_000_000, (name, pn)
        if O.lib_ref() is not None:
            assert np.array_equal(O.ref_all2all(seqs, prm, threads=2), want), (name, pn)
        res, regs = O.oracle_pair(seqs[0], seqs[1], prm, want_regions=True)
        mres, mregs = U.model_pair_regions(seqs[0], seqs[1], prm)
        assert res == mres and 0 < len(regs) < 4096 and np.array_equal(regs, mregs), (name, pn)


def test_the_split_model_gets_voids_by_itself():
    """Over the sets above, by the model alone: void segments of at least two classes, and ten resumes or more in some set."""
    if len(_SPLIT_STATS) < 6 * 6 + N_FUZZ * 6:                              # (run alone: make the counts)
        for name in [n for n in RG.SET_NAMES if not n.startswith("long")]:
            for pn in PRM_NAMES:
                _SPLIT_STATS.setdefault((name, pn), U.model_split_rounds(RG.repeat_set(name), params_of(pn, RG.SET_NAMES.index(name)), 512)[1])
        for seed in range(N_FUZZ):
            for pn in PRM_NAMES:
                _SPLIT_STATS.setdefault((seed, pn), U.model_split_rounds(RG.fuzz_set(seed), params_of(pn, 100 + seed), 512)[1])
    voids = np.sum([st["voids"] for st in _SPLIT_STATS.values()], axis=0)
    most = max(_SPLIT_STATS.items(), key=lambda kv: kv[1]["resumed"])
    print("voids by class", voids.tolist(), "most resumes", most[0], most[1]["resumed"])
    assert int((voids > 0).sum()) >= 2 and most[1]["resumed"] >= 10


# ---- tie cases ---------------------------------------------------------------------------------------------------------------
TIES = RT.tie_cases()


def test_tie_cases_cover_the_rules():
    names = [c["name"] for c in TIES]
    assert len(set(names)) == len(names) and {n[0] for n in names} == set("abcdefg")
    assert {n for n in names if n[0] == "g"} == {"g_tandem_unit%d_shift%d" % (u, s) for u in (16, 32, 64) for s in range(1, u)}
    for c in TIES:
        assert U.index_form([c["ref"], c["qry"]], None)["tag_words"], c["name"]
    f = {c["name"]: c for c in TIES if c["name"][0] == "f"}
    assert [c["col"] for c in f.values()] == ["ref_end", "ref_at"]                        # either side of the crossover
    T = 2 * 10000 + 120
    assert not RT.anchor_beats_seed(12, 8, 14, T, 40) and RT.anchor_beats_seed(13, 8, 14, T, 40)


@pytest.mark.parametrize("case", TIES, ids=[c["name"] for c in TIES])
def test_tie_case_takes_the_stated_occurrence(case):
    """The oracle takes the stated copy, which differs from the other copy; the host model and (where built) the reference
    build give the same regions; everywhere the reference build's recorded regions."""
    res, regs = O.oracle_pair(case["ref"], case["qry"], None, want_regions=True)
    assert RT.occurrence(case, regs) == case["want"] != case["other"], (case["name"], regs[:3].tolist())
    mres, mregs = U.model_pair_regions(case["ref"], case["qry"], None)
    assert mres == res and np.array_equal(mregs, regs), case["name"]
    rec = load_recorded()["ties"][case["name"]]
    assert tuple(rec["res"]) == res and np.array_equal(np.array(rec["regions"], np.int32).reshape(-1, 6), regs), case["name"]
    if O.lib_ref() is not None:
        rres, rregs = O.ref_pair(case["ref"], case["qry"], None, want_regions=True)
        assert rres == res and np.array_equal(rregs, regs), case["name"]


def test_recorded_reference_results():
    """tests/golden/repeat_vectors.json (oracle/make_goldens.py --repeats-only): the reference build's triples of the 'small'
    repeat sets under the defaults and 'generic'; the oracle is held to them where oracle/_ref is absent too.  The file
    records results only and stays below ref_vectors.json in size."""
    rec = load_recorded()
    assert os.path.getsize(os.path.join(U.GOLD, "repeat_vectors.json")) <= os.path.getsize(os.path.join(U.GOLD, "ref_vectors.json"))
    assert set(rec["ties"]) == {c["name"] for c in TIES}
    for name in ("small", "small N"):
        assert rec["checksums"][name] == CHECKSUMS[name]
        for pn in ("defaults", "generic"):
            want = np.array(rec["sets"][f"{name}/{pn}"]["res"], dtype=np.int32)
            assert rec["sets"][f"{name}/{pn}"]["params"] == U.INST_PARAMS[pn]
            assert np.array_equal(O.oracle_all2all(RG.repeat_set(name), U.INST_PARAMS[pn], threads=16), want), (name, pn)


# ---- what makes the prefilter's GPU test meaningful ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "split", "split N"])
@pytest.mark.parametrize("k", [16, 21, 25])
def test_prefilter_model_sees_the_repeats(name, k):
    """A k-mer repeated inside a genome counts once: for some genome |K(g)| is at least 10 % below its valid windows; and a
    k-mer occurs on both strands of one genome (the hairpin)."""
    seqs = RG.repeat_set(name)
    kmers_of, shared = PM.shared_matrix(seqs, k)
    windows = np.array([int(PM.window_values(s, k)[2].sum()) for s in seqs])
    assert (kmers_of <= windows).all() and (kmers_of[:-1] <= 0.9 * windows[:-1]).any(), (kmers_of, windows)
    both = 0
    for s in seqs:
        v, r, valid = PM.window_values(s, k)
        both += len(np.intersect1d(v[valid], r[valid]))
    assert both > 0
    a, b = np.triu_indices(len(seqs), 1)
    assert (shared[a, b] <= np.minimum(kmers_of[a], kmers_of[b])).all() and shared[0, 3] == kmers_of[0] == kmers_of[3]
