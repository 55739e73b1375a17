"""CPU: the alignment-region stage as the library states it on the host (lzani_regions_host, csrc/lzani_regions.h and
lzani_aln_rule.h) against tests/aln_regions_model.py -- seeded made-up calls, the edges of the rule, the refusals -- and the
example set: the oracle's regions of all 132 pairs through lzani_regions_host and a restatement of the file's line format,
against tests/golden/example/ani.aln.tsv."""
import os

import numpy as np
import pytest

import aln_regions_model as M
import lzani_ctypes as L
import oracle as O
import util as U


@pytest.fixture(scope="module", autouse=True)
def lib():
    L.build_library()
    return L.load_library()


def same(got, want):
    assert got.dtype == L.REGION_DTYPE == M.REGION_DTYPE and got.dtype.itemsize == 32
    assert len(got) == len(want)
    assert got.tobytes() == want.tobytes()


def check(call, flt):
    n, aln_len, ref, off, q, regs = call
    want, info, stays, _ = M.order(n, aln_len, ref, off, q, regs, flt)
    got, ginfo = L.regions_host(n, aln_len, ref, off, q, regs, flt)
    same(got, want)
    assert {k: ginfo[k] for k in info} == info, (ginfo, info)
    return want, info


def test_regions_host_agrees_with_the_model_on_seeded_calls():
    kinds, empty_entries, tied, medians = set(), 0, 0, 0
    for seed in range(300):
        call = M.random_call(20270 + seed)
        n, aln_len, ref, off, q, regs = call
        kinds.add("dense" if q is None else "lists")
        every, info = check(call, None)
        assert len(every) == len(regs) and info["entries_dropped"] == 0
        empty_entries += info["entries"] > info["entries_with_regions"]
        key = np.stack((regs["pair"].astype(np.int64), regs["seq_start"], regs["seq_end"]), axis=1)
        tied += len(np.unique(key, axis=0)) < len(key)
        none, info = check(call, {"ani": 2.0})
        assert len(none) == 0 and info["entries_dropped"] == info["entries_with_regions"]
        for field, flt in M.median_filters(*call).items():
            if flt is None or info["entries_with_regions"] < 4:
                continue
            some, minfo = check(call, flt)
            assert 0 < minfo["entries_dropped"] < minfo["entries_with_regions"], (seed, field)     # some entries stay and some go
            assert 0 < len(some) < len(regs)
            medians += 1
    assert kinds == {"dense", "lists"} and empty_entries > 100 and tied > 100 and medians > 600


def test_ties_keep_their_input_order():
    ref, off, q = M.dense(3)
    regs = np.zeros(6, dtype=M.REGION_DTYPE)
    regs["pair"], regs["seq_start"], regs["seq_end"] = 4, 10, 30
    regs["ref_start"] = [5, 4, 3, 2, 1, 0]                                   # told apart by a field that is no key
    regs["ref_end"] = regs["ref_start"] + 20
    got, _ = L.regions_host(3, [100, 100, 100], ref, off, q, regs)
    assert got["ref_start"].tolist() == [5, 4, 3, 2, 1, 0]


def one_entry(mat, lit, length, flt):
    """the regions that stay of the call with one entry (ref 0, query 1) that owns one region of these counts"""
    ref, off, q = M.lists([(0, [1])])
    regs = np.zeros(1, dtype=M.REGION_DTYPE)
    regs["seq_end"], regs["ref_end"], regs["num_matches"], regs["num_mismatches"] = 50, 50, mat, lit
    call = (2, np.array([7, length], dtype=np.uint32), ref, off, q, regs)
    return len(check(call, flt)[0])


def test_rule_edges():
    # a length of 0: gani and qcov are inf (or NaN where the sums are 0), below nothing
    assert one_entry(30, 5, 0, {"gani": 1e308, "qcov": 1e308}) == 1
    assert one_entry(0, 0, 0, {"gani": 1e308, "qcov": 1e308}) == 1
    assert one_entry(0, 0, 0, {"ani": 1e-300}) == 0                           # ... but ani of mat + lit = 0 is 0
    assert one_entry(0, 0, 100, {"ani": 0.0}) == 1 and one_entry(0, 0, 100, {}) == 1
    # a value exactly equal to its minimum stays, the next double above drops it
    for field, v in (("gani", 30 / 97), ("ani", 30 / 37), ("qcov", 37 / 97)):
        assert one_entry(30, 7, 97, {field: v}) == 1, field
        assert one_entry(30, 7, 97, {field: float(np.nextafter(v, np.inf))}) == 0, field
        assert one_entry(30, 7, 97, {field: float(np.nextafter(v, 0))}) == 1, field
    # min_tani and min_rcov are not read
    assert one_entry(30, 7, 97, {"tani": 2.0, "rcov": 2.0}) == 1
    assert one_entry(30, 7, 97, {"tani": float("nan"), "rcov": float("nan")}) == 1
    # the length is the query's (genome 1), not the reference's
    assert one_entry(30, 7, 97, {"qcov": 37 / 97}) == 1 and one_entry(30, 7, 98, {"qcov": 37 / 97}) == 0
    # the sums are 32-bit: two regions whose matches wrap
    ref, off, q = M.lists([(0, [1])])
    regs = np.zeros(2, dtype=M.REGION_DTYPE)
    regs["seq_end"], regs["ref_end"], regs["num_matches"] = 50, 50, 2**30 + 5
    regs["seq_start"] = [0, 1]
    for flt in ({"gani": 0.0}, {"qcov": 0.0}, None):
        check((2, np.array([7, 1000], dtype=np.uint32), ref, off, q, regs), flt)
    assert len(M.order(2, [7, 1000], ref, off, q, regs, {"gani": 0.0})[0]) == 0       # (the sum is negative)


def test_refusals():
    ref, off, q = M.lists([(0, [1, 2]), (1, [0, 2]), (2, [0, 1])])
    al = np.array([100, 100, 100], dtype=np.uint32)
    good = M.random_regions(np.random.default_rng(1), 6, 10, 50)
    assert len(L.regions_host(3, al, ref, off, q, good)[0]) == 10

    def refused(*args):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            L.regions_host(*args)

    for k in M.FIELDS:
        refused(3, al, ref, off, q, good, {k: float("nan")})                 # a NaN minimum
    for field, value in (("pair", 6), ("seq_end", 0), ("seq_start", -1), ("ref_start", -1), ("ref_end", -1), ("num_matches", -1), ("num_mismatches", -1)):
        bad = good.copy()
        bad[field][3] = value                                               # a pair out of range; an empty region; a negative field
        if field == "seq_end":
            bad["seq_start"][3] = 0
        refused(3, al, ref, off, q, bad)
    bad = good.copy()
    bad["seq_start"][3], bad["seq_end"][3] = 9, 8                           # a negative length
    refused(3, al, ref, off, q, bad)
    refused(3, al, *M.lists([(0, [1, 2]), (1, [0, 2]), (0, [1])]), good[good["pair"] < 5])      # a genome leads two rows
    refused(3, al, *M.lists([(0, [2, 1]), (1, [0, 2]), (2, [0, 1])]), good)                     # a list that descends
    refused(3, al, *M.lists([(0, [1, 1]), (1, [0, 2]), (2, [0, 1])]), good)                     # ... and one that names a query twice


# ---- the example set ---------------------------------------------------------------------------------------------------
COLS = ("ref_start", "ref_end", "seq_start", "seq_end", "num_matches", "num_mismatches")


@pytest.fixture(scope="module")
def example():
    """names and genomes in the file's order, the dense rows, the oracle's regions of all 132 pairs in a shuffled order,
    and the golden file's lines"""
    names, seqs = U.reorder(*U.load_example())
    n = len(seqs)
    ref, off, _ = M.dense(n)
    parts, e = [], 0
    for r in range(n):
        for x in range(n):
            if x == r:
                continue
            w = O.oracle_pair(seqs[r], seqs[x], None, want_regions=True)[1]
            p = np.zeros(len(w), dtype=M.REGION_DTYPE)
            p["pair"] = e
            for k, c in enumerate(COLS):
                p[c] = w[:, k]
            parts.append(p)
            e += 1
    regs = np.concatenate(parts)
    regs = regs[np.random.default_rng(5).permutation(len(regs))]            # as a run leaves them: in no order
    gold = open(os.path.join(U.GOLD, "example", "ani.aln.tsv")).read().split("\n")
    assert gold[-1] == "" and gold[0].startswith("query\treference\tpident")
    return names, seqs, ref, off, regs, gold[1:-1]


def lines_of(names, seqs, ref, off, regs):
    r_of, q_of = M.M.entries_of(len(seqs), ref, off, None)
    return [M.aln_line(names[q_of[int(x["pair"])]], names[r_of[int(x["pair"])]], x, len(seqs[r_of[int(x["pair"])]]), 40) for x in regs]


def test_example_set_gives_the_golden_alignment_file(example):
    names, seqs, ref, off, regs, gold = example
    n, lens = len(seqs), np.array([len(s) for s in seqs], dtype=np.uint32)
    assert n == 12 and int(off[-1]) == 132 and len(regs) == 5693
    got, info = L.regions_host(n, lens, ref, off, None, regs)
    same(got, M.order(n, lens, ref, off, None, regs)[0])
    assert info["kept"] == 5693 and info["entries_dropped"] == 0
    mine = lines_of(names, seqs, ref, off, got)
    assert sorted(mine) == sorted(gold)                                      # the golden file as a multiset
    by_pair = {}
    for ln in gold:                                                          # each pair's lines in the statement's order
        by_pair.setdefault(tuple(ln.split("\t")[:2]), []).append(ln)
    mine_by_pair = {}
    for ln in mine:
        mine_by_pair.setdefault(tuple(ln.split("\t")[:2]), []).append(ln)
    assert mine_by_pair == by_pair
    per = np.bincount(got["pair"].astype(np.int64), minlength=132)
    assert per.min() == 3 and per.max() == 264


def test_example_set_under_the_medians_of_its_own_pairs(example):
    names, seqs, ref, off, regs, gold = example
    n, lens = len(seqs), np.array([len(s) for s in seqs], dtype=np.uint32)
    flt = {}
    for k, v in M.median_filters(n, lens, ref, off, None, regs).items():
        flt.update(v)
    assert abs(flt["gani"] - 0.0231) < 5e-4 and abs(flt["ani"] - 0.579) < 5e-3 and abs(flt["qcov"] - 0.0400) < 5e-4, flt
    want, info, stays, _ = M.order(n, lens, ref, off, None, regs, flt)
    assert 0 < info["entries_dropped"] < 132 and 0 < len(want) < len(regs)
    got, ginfo = L.regions_host(n, lens, ref, off, None, regs, flt)
    same(got, want)
    assert ginfo["entries_dropped"] == info["entries_dropped"]
    r_of, q_of = M.M.entries_of(n, ref, off, None)
    keep_names = {(names[q_of[e]], names[r_of[e]]) for e in np.flatnonzero(stays)}
    assert sorted(lines_of(names, seqs, ref, off, got)) == sorted(ln for ln in gold if tuple(ln.split("\t")[:2]) in keep_names)
