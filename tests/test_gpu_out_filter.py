"""GPU: the output filter on the device.  The stage alone (lzani_debug_filter_results) on made-up integers, record by
record against tests/out_filter_model.py, at the shapes at which it can go wrong; then lzani_run_rows_kept on a small
genome set -- dense rows, lists, the group, an out-of-core context -- against lzani_run_rows put through the model."""
import numpy as np
import pytest

import lzani_ctypes as L
import ooc_model as OM
import out_filter_model as M
import synth_genomes as SG

pytestmark = pytest.mark.gpu

CHUNK = 4096                                            # entries a block of the compaction takes


def same(got, want):
    assert got.dtype == L.KEPT_DTYPE and got.dtype.itemsize == M.KEPT_DTYPE.itemsize == 36
    assert len(got) == len(want)
    for k in ("a", "b", "x", "y", "lines"):
        assert np.array_equal(got[k], want[k]), k
    assert got.tobytes() == want.tobytes()


def lists(rows):
    """[(ref, [queries])] -> ref_ids, row_off, query_ids"""
    ref = np.array([r for r, _ in rows], dtype=np.uint32)
    off = np.cumsum([0] + [len(q) for _, q in rows]).astype(np.uint64)
    q = np.array([x for _, qs in rows for x in qs], dtype=np.uint32)
    return ref, off, q


def made_up(n, ref, off, q, seed, zero_len=()):
    """Printed lengths and one made-up result per directed entry: the aligned part at most the query, matches at least half
    of it, each direction drawn on its own -- so that the lines of a pair fall on both sides of a median."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(2000, 5000, n).astype(np.uint32)
    lens[list(zero_len)] = 0
    _, qq = M.entries_of(n, ref, off, q)
    al = (rng.random(len(qq)) * np.maximum(lens[qq], 1)).astype(np.int64)
    m = (al * (0.5 + 0.5 * rng.random(len(qq)))).astype(np.int64)
    return lens, np.stack((m, al - m, rng.integers(0, 30, len(qq))), axis=1).astype(np.int32)


def median_minimum(n, lens, ref, off, q, res, field="gani", quant=0.5, above=-1.0):
    """A minimum at a quantile of the field over the lines of every paired pair (a value of the data itself); above: over
    the lines whose value exceeds it only."""
    rec = M.kept({}, n, lens, ref, off, q, res)[0]
    v = M.ratios(rec["x"], rec["y"], lens[rec["a"]], lens[rec["b"]])[field].ravel()
    v = np.sort(v[np.isfinite(v) & (v > above)])
    return {field: float(v[int(quant * (len(v) - 1))])}


def check(eng, n, lens, ref, off, q, res, flt, mixed=True):
    want, unpaired, leading, ln, _ = M.kept(flt, n, lens, ref, off, q, res)
    if mixed:                                           # the case shows a kept pair, a dropped pair and a pair with one line
        assert (ln == 0).any() and (ln == 3).any() and ((ln == 1) | (ln == 2)).any(), np.bincount(ln, minlength=4)
    got = eng.filter_results(n, lens, ref, off, q, res, flt)
    same(got, want)
    info = eng.kept_info()
    assert info["entries"] == int(off[-1]) and info["leading"] == leading and info["unpaired"] == unpaired, info
    assert info["kept_pairs"] == len(want) and info["kept_lines"] == int((ln & 1).sum() + (ln >> 1).sum()), info
    assert info["bytes_to_host"] == 36 * len(got) and (info["filter_ms"] > 0) == (int(off[-1]) > 0)
    return want


@pytest.fixture(scope="module")
def eng():
    e = L.Engine()                                      # the stage alone needs no genome set
    yield e
    e.close()


def test_no_result_yet():
    e = L.Engine()
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        e.kept_fetch(0, 0)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_STATE"):
        e.kept_info()
    e.close()


def symmetric_lists(n, seed, p=0.4):
    rng = np.random.default_rng(seed)
    adj = np.triu(rng.random((n, n)) < p, 1)
    adj = adj | adj.T
    return [(r, np.flatnonzero(adj[r]).tolist()) for r in range(n)]


def test_stage_on_small_calls(eng):
    n = 7
    ref, off = L.dense_rows(n)
    lens, res = made_up(n, ref, off, None, 1)
    flt = median_minimum(n, lens, ref, off, None, res)
    want = check(eng, n, lens, ref, off, None, res, flt)                     # a dense 7 x 7 call
    assert 0 < len(want) < 21
    # ranges of the records; one past the end
    same(eng.kept_fetch(1, len(want) - 1), want[1:])
    same(eng.kept_fetch(len(want), 0), want[:0])
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        eng.kept_fetch(1, len(want))
    assert eng.kept_info()["bytes_to_host"] == 36 * (2 * len(want) - 1)
    # a genome of printed length 0: its lines divide by zero
    lens0, res0 = made_up(n, ref, off, None, 2, zero_len=(3,))
    assert lens0[3] == 0
    check(eng, n, lens0, ref, off, None, res0, median_minimum(n, lens0, ref, off, None, res0))
    check(eng, n, lens0, ref, off, None, res0, median_minimum(n, lens0, ref, off, None, res0, "rcov"))
    # a subset of dense rows: the mates of the others are missing
    sub, soff = L.dense_rows(n, [0, 2, 3, 6])
    slens, sres = made_up(n, sub, soff, None, 3)
    sflt = median_minimum(n, slens, sub, soff, None, sres, "qcov")
    check(eng, n, slens, sub, soff, None, sres, sflt)
    assert eng.kept_info()["unpaired"] == 3 + 2 + 2                          # rows 0, 2, 3 against the genomes 1, 4, 5 above them
    # symmetric lists
    n = 12
    rows = symmetric_lists(n, 5)
    ref, off, q = lists(rows)
    lens, res = made_up(n, ref, off, q, 6)
    for field in M.FIELDS:                              # (tani is the same for both lines: a second minimum halves pairs)
        also = median_minimum(n, lens, ref, off, q, res, "gani", 0.3) if field == "tani" else {}
        check(eng, n, lens, ref, off, q, res, dict(median_minimum(n, lens, ref, off, q, res, field), **also))
    check(eng, n, lens, ref, off, q, res, dict(median_minimum(n, lens, ref, off, q, res, "ani", 0.3), **median_minimum(n, lens, ref, off, q, res, "qcov", 0.3)))
    assert eng.kept_info()["unpaired"] == 0
    # lists with unpaired leading entries and entries that only trail; empty rows; the rows out of order
    rng = np.random.default_rng(22)
    order = [5, 11, 2, 9, 0, 7, 3, 10, 1]                                    # (4, 6 and 8 lead no row)
    rows = [(r, [] if r in (9, 3) else sorted(rng.choice([x for x in range(n) if x != r], 8, replace=False).tolist())) for r in order]
    ref, off, q = lists(rows)
    lens, res = made_up(n, ref, off, q, 8)
    want = check(eng, n, lens, ref, off, q, res, median_minimum(n, lens, ref, off, q, res))
    info = eng.kept_info()
    assert 0 < info["unpaired"] < info["leading"] and len(want)
    assert want["a"].tolist() != sorted(want["a"].tolist())                  # the order is the call's, not the ids'
    # a subset of the list rows
    ref2, off2, q2 = lists(rows[2:7])
    lens2, res2 = made_up(n, ref2, off2, q2, 9)
    check(eng, n, lens2, ref2, off2, q2, res2, median_minimum(n, lens2, ref2, off2, q2, res2), mixed=False)


def test_threshold_edges_on_real_entries(eng):
    """A minimum equal to a pair's own ratio keeps its line, the next double above drops it: for each of the five values,
    on the entry whose value is the median, so that the call keeps, drops and halves pairs around it."""
    n = 12
    ref, off, q = lists(symmetric_lists(n, 15, 0.6))
    lens, res = made_up(n, ref, off, q, 16)
    rec = M.kept({}, n, lens, ref, off, q, res)[0]
    for field in M.FIELDS:
        # a mild second minimum (tani alone never halves a pair); the target is the median among the lines that pass it
        base = median_minimum(n, lens, ref, off, q, res, "qcov" if field == "gani" else "gani", 0.25)
        passing = M.lines(base, rec["x"], rec["y"], lens[rec["a"]], lens[rec["b"]])
        v = M.ratios(rec["x"], rec["y"], lens[rec["a"]], lens[rec["b"]])[field]
        ok = np.stack((passing & 1, passing >> 1), axis=1).astype(bool)
        flat = np.sort(v[ok])
        target = flat[len(flat) // 2]
        p, line = (int(t[0]) for t in np.nonzero((v == target) & ok))
        at = check(eng, n, lens, ref, off, q, res, dict(base, **{field: float(target)}))
        hit = at[(at["a"] == rec["a"][p]) & (at["b"] == rec["b"][p])]
        assert len(hit) == 1 and int(hit["lines"][0]) & (1 << line)
        above = check(eng, n, lens, ref, off, q, res, dict(base, **{field: float(np.nextafter(target, np.inf))}))
        hit = above[(above["a"] == rec["a"][p]) & (above["b"] == rec["b"][p])]
        assert len(hit) == 0 or not int(hit["lines"][0]) & (1 << line)


def band_rows(entries):
    """Genome i lists i - 2, i - 1, i + 1, i + 2, the rows from the highest id down (a leading entry's mate lies in an earlier
    row), cut after `entries` directed entries.  Behind the first two rows every row has four entries, the last two of them
    leading: the entries 4095 and 4096, 8191 and 8192 are leading ones."""
    n = entries // 4 + 8
    rows, left = [], entries
    for i in range(n - 1, -1, -1):
        qs = [x for x in (i - 2, i - 1, i + 1, i + 2) if 0 <= x < n][:left]
        rows.append((i, qs))
        left -= len(qs)
        if not left:
            break
    return n, rows


@pytest.mark.parametrize("entries", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_chunk_edges_of_the_compaction(eng, entries):
    n, rows = band_rows(entries)
    ref, off, q = lists(rows)
    assert int(off[-1]) == entries
    lens, res = made_up(n, ref, off, q, entries)
    r_of, q_of = M.entries_of(n, ref, off, q)
    at = {(int(r), int(x)): e for e, (r, x) in enumerate(zip(r_of, q_of))}
    edges = [e for e in sorted({CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK} | set(range(entries - 4, entries))) if 0 <= e < entries and q_of[e] > r_of[e]]
    assert edges and (entries <= CHUNK or {CHUNK - 1, CHUNK} <= set(edges)) and (entries <= 2 * CHUNK or {2 * CHUNK - 1, 2 * CHUNK} <= set(edges))
    for e in edges:                                     # a perfect pair at every edge: all its ratios are 1
        m = at[(int(q_of[e]), int(r_of[e]))]
        res[e] = (lens[q_of[e]], 0, 1)
        res[m] = (lens[r_of[e]], 0, 1)
    flt = median_minimum(n, lens, ref, off, q, res)
    assert flt["gani"] < 1
    want, _, _, ln, lead = M.kept(flt, n, lens, ref, off, q, res)
    kept_entries = set(lead[ln != 0].tolist())
    assert set(edges) <= kept_entries                   # kept entries on both sides of every edge
    for c in range((entries + CHUNK - 1) // CHUNK):
        assert any(c * CHUNK <= e < (c + 1) * CHUNK for e in kept_entries)
    check(eng, n, lens, ref, off, q, res, flt)


def test_nothing_passes_everything_passes_and_refusals(eng):
    n = 9
    ref, off = L.dense_rows(n)
    lens, res = made_up(n, ref, off, None, 21)
    none = check(eng, n, lens, ref, off, None, res, {"ani": 2.0}, mixed=False)
    assert len(none) == 0 and eng.kept_info()["kept_pairs"] == 0
    assert len(eng.kept_fetch(0, 0)) == 0               # an empty range of an empty result
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        eng.kept_fetch(0, 1)
    every = check(eng, n, lens, ref, off, None, res, {}, mixed=False)
    assert len(every) == n * (n - 1) // 2 and (every["lines"] == 3).all()
    assert len(check(eng, 3, lens[:3], *lists([(2, []), (0, [])]), res[:0], {}, mixed=False)) == 0      # no entry at all
    # refused, on the host, before anything runs: the result of the last call stays
    good = lists([(0, [1, 2]), (1, [0, 2]), (2, [0, 1])])
    gl, gr = made_up(3, *good, 22)
    for bad, flt in ((lists([(0, [1, 2]), (1, [0, 2]), (0, [1])]), {}),             # a genome leads two rows
                     (lists([(0, [2, 1]), (1, [0, 2]), (2, [0, 1])]), {}),          # a descending list
                     (lists([(0, [1, 1]), (1, [0, 2]), (2, [0, 1])]), {}),          # ... and one that names a query twice
                     (good, {"qcov": float("nan")})):
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            eng.filter_results(3, gl, *bad, gr[:len(bad[2])], flt)
    assert eng.kept_info()["kept_pairs"] == 0 and eng.kept_info()["entries"] == 0
    check(eng, 3, gl, *good, gr, {}, mixed=False)


def test_stage_on_a_device_buffer(eng):
    import torch
    n = 7
    ref, off = L.dense_rows(n)
    lens, res = made_up(n, ref, off, None, 31)
    flt = median_minimum(n, lens, ref, off, None, res, "tani")
    buf = torch.from_numpy(res).to("cuda:0")
    torch.cuda.synchronize()
    got = eng.filter_results(n, lens, ref, off, None, int(buf.data_ptr()), flt)
    same(got, M.kept(flt, n, lens, ref, off, None, res)[0])


# ---- lzani_run_rows_kept on genomes ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def genomes():
    seqs = SG.make_set(20, 4711, lmin=2000, lmax=4000, fam=3)[1]
    seqs += [np.full(2500, 5, dtype=np.uint8), np.zeros(0, np.uint8)]                 # all N; empty
    e = L.Engine()
    e.set_genomes(seqs)
    full = e.all2all()                                  # the reference of every case below: computed once, left unchanged
    full.setflags(write=False)
    yield seqs, e, full
    e.close()


def rows_of(full, ref, off, q):
    """the results lzani_run_rows gives for a call, read from the all2all"""
    r, x = M.entries_of(full.shape[0], ref, off, q)
    return full[r, x]


def genome_cases(n):
    dense = L.dense_rows(n) + (None,)
    sym = lists(symmetric_lists(n, 41, 0.5))
    rng = np.random.default_rng(42)
    def row(r):                                         # the genomes of r's family of three, and six others
        fam = [x for x in range(r // 3 * 3, r // 3 * 3 + 3) if x != r and x < 20 and r < 20]
        return sorted(set(fam) | set(rng.choice([x for x in range(n) if x != r], 6, replace=False).tolist()))
    ragged = lists([(int(r), row(int(r))) for r in rng.permutation(n)[:16]])
    return dict(dense=dense, lists=sym, ragged=ragged)


def minima_of(n, lens, ref, off, q, res):
    """minima among the lines of related pairs (unrelated genomes align next to nothing): the medians of their values"""
    return dict(median_minimum(n, lens, ref, off, q, res, "ani", 0.5, above=0.5), **median_minimum(n, lens, ref, off, q, res, "qcov", 0.5, above=0.2))


@pytest.mark.parametrize("case", ["dense", "lists", "ragged"])
def test_run_rows_kept_against_run_rows_through_the_model(genomes, case):
    seqs, eng, full = genomes
    n, lens = len(seqs), np.array([len(s) for s in seqs], dtype=np.uint32)
    ref, off, q = genome_cases(n)[case]
    res = eng.run_rows(ref, off, q)
    assert np.array_equal(res, rows_of(full, ref, off, q))
    flt = minima_of(n, lens, ref, off, q, res)
    want, unpaired, leading, ln, _ = M.kept(flt, n, lens, ref, off, q, res)
    assert (ln == 0).any() and (ln == 3).any() and ((ln == 1) | (ln == 2)).any()
    got = eng.run_rows_kept(ref, off, q, flt)
    same(got, want)
    info = eng.kept_info()
    assert (info["entries"], info["leading"], info["unpaired"], info["kept_pairs"]) == (int(off[-1]), leading, unpaired, len(want))
    assert info["bytes_to_host"] == 36 * len(got)
    assert (unpaired > 0) == (case == "ragged")
    # printed lengths that differ from the genomes' own
    rl = lens + np.uint32(40)
    same(eng.run_rows_kept(ref, off, q, flt, report_len=rl), M.kept(flt, n, rl, ref, off, q, res)[0])
    # a second, smaller call in the same context; then run_rows gives what it gave
    ref2, off2, q2 = lists([(3, [4, 5]), (5, [3, 4]), (4, [3, 5])])
    res2 = rows_of(full, ref2, off2, q2)
    small = eng.run_rows_kept(ref2, off2, q2, {})
    same(small, M.kept({}, n, lens, ref2, off2, q2, res2)[0])
    assert len(small) == 3 and eng.kept_info()["bytes_to_host"] == 36 * 3
    assert np.array_equal(eng.run_rows(ref, off, q), res)
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        eng.run_rows_kept(*lists([(3, [5, 4])]), {})
    assert np.array_equal(eng.run_rows(*lists([(3, [5, 4])])), rows_of(full, *lists([(3, [5, 4])])))       # run_rows still takes it


def test_group_rehearsal_and_out_of_core(genomes):
    seqs, eng, full = genomes
    n, lens = len(seqs), np.array([len(s) for s in seqs], dtype=np.uint32)
    cases = genome_cases(n)
    grp = L.Group(None, (0, 0, 0))
    grp.set_genomes(seqs)
    limit = OM.limit_for_blocks([int(x) for x in lens], None, 3)
    ooc = L.Engine()
    ooc.set_genome_memory(limit)
    ooc.set_genomes(seqs)
    assert ooc.residency()["blocks"] == 3
    for name, (ref, off, q) in cases.items():
        res = rows_of(full, ref, off, q)
        flt = minima_of(n, lens, ref, off, q, res)
        want, unpaired, leading, ln, _ = M.kept(flt, n, lens, ref, off, q, res)
        assert 0 < len(want) < leading - unpaired
        got = grp.run_rows_kept(ref, off, q, flt)
        same(got, want)
        gi = grp.kept_info()
        assert (gi["leading"], gi["unpaired"], gi["kept_pairs"], gi["bytes_to_host"]) == (leading, unpaired, len(want), 36 * len(want)), name
        assert np.array_equal(grp.run_rows(ref, off, q), res)
        same(ooc.run_rows_kept(ref, off, q, flt), want)
        assert ooc.residency()["tiles"] > 1 and ooc.kept_info()["unpaired"] == unpaired
    assert len(grp.run_rows_kept(*L.dense_rows(n, []), None, {})) == 0 and grp.kept_info()["entries"] == 0      # no rows at all
    assert np.array_equal(ooc.run_rows(*cases["dense"]), rows_of(full, *cases["dense"]))
    grp.close()
    ooc.close()
