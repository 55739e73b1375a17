"""CPU: the cut of a cluster level as a pure host function (lzani_cluster_cut_lines) against tests/cluster_cut_model.py --
random made-up integer records (lengths of 0, m + l == 0, negative values, every value of `lines`), every minimum at a
record's own value and one step above it, the maximum of num_alns at a line's value and one below, the all-zero cut, the
refusals, and the property that ties a level to a stricter output filter."""
import numpy as np
import pytest

import cluster_cut_model as CUT
import lzani_ctypes as L
import out_filter_model as M

REFUSED = 0xFFFFFFFF


@pytest.fixture(scope="module", autouse=True)
def lib():
    L.build_library()
    return L.load_library()


def made_up(count, seed):
    """x, y int32[count, 3], lines in 1..3, la, lb: plausible values mixed with zeros, negative values and m + l == 0"""
    rng = np.random.default_rng(seed)
    la, lb = rng.integers(1, 5000, count).astype(np.uint32), rng.integers(1, 5000, count).astype(np.uint32)
    x = np.stack((rng.integers(0, 5000, count), rng.integers(0, 800, count), rng.integers(0, 9, count)), axis=-1).astype(np.int32)
    y = np.stack((rng.integers(0, 5000, count), rng.integers(0, 800, count), rng.integers(0, 9, count)), axis=-1).astype(np.int32)
    odd = rng.random(count)
    la[odd < 0.05] = 0
    lb[(odd > 0.04) & (odd < 0.09)] = 0
    x[(odd > 0.10) & (odd < 0.15)] = 0                      # m + l == 0
    y[(odd > 0.13) & (odd < 0.18), :2] = 0
    neg = (odd > 0.20) & (odd < 0.30)
    x[neg] = rng.integers(-3000, 3000, (int(neg.sum()), 3))
    y[(odd > 0.25) & (odd < 0.35), 0] *= -1
    same = (odd > 0.40) & (odd < 0.45)
    lb[same] = la[same]
    return x, y, rng.integers(1, 4, count).astype(np.uint32), la, lb


def random_cut(rng):
    cut = {}
    for k in CUT.FIELDS[:-1]:
        if rng.random() < 0.5:
            cut[k] = float(rng.choice([0.0, 0.1, 0.5, 0.9, 1.0, rng.random()]))
    if rng.random() < 0.5:
        cut["num_alns"] = int(rng.integers(1, 9))
    return cut


def got(cut, x, y, lines, la, lb):
    return np.array([L.cluster_cut_lines(cut, x[i], y[i], lines[i], la[i], lb[i]) for i in range(len(x))], dtype=np.uint32)


def test_random_records_against_the_model():
    rng = np.random.default_rng(3)
    for seed in range(8):
        x, y, lines, la, lb = made_up(500, seed)
        cut = random_cut(rng)
        mine, want = got(cut, x, y, lines, la, lb), CUT.cut_lines(cut, x, y, lines, la, lb)
        assert np.array_equal(mine, want), (cut, np.flatnonzero(mine != want)[:5])
        assert ((mine & ~lines) == 0).all()                 # a subset of `lines`
    x, y, lines, la, lb = made_up(500, 99)
    # the all-zero cut returns `lines`: of every record whose values are not negative, and of every line that an output filter
    # with minima that are not negative kept (a negative made-up value is below the minimum 0, there as here)
    positive = ((x >= 0) & (y >= 0)).all(axis=1)
    assert positive.sum() > 300 and np.array_equal(got({}, x, y, lines, la, lb)[positive], lines[positive])
    kept = lines & M.lines({}, x, y, la, lb)
    assert (kept != lines).any() and np.array_equal(got({}, x, y, kept, la, lb), kept)
    assert len(set(lines.tolist())) == 3 and (la == 0).any() and (lb == 0).any() and (x < 0).any() and ((x[:, 0] + x[:, 1]) == 0).any()


def plausible(count, seed):
    """records whose values are all finite and positive: every minimum can be set at a line's own value"""
    rng = np.random.default_rng(seed)
    la, lb = rng.integers(500, 5000, count).astype(np.uint32), rng.integers(500, 5000, count).astype(np.uint32)
    x = np.stack((rng.integers(1, 400, count), rng.integers(1, 100, count), rng.integers(2, 9, count)), axis=-1).astype(np.int32)
    y = np.stack((rng.integers(1, 400, count), rng.integers(1, 100, count), rng.integers(2, 9, count)), axis=-1).astype(np.int32)
    return x, y, la, lb


@pytest.mark.parametrize("field", CUT.FIELDS[:-1])
def test_a_minimum_at_a_lines_own_value_and_one_step_above(field):
    x, y, la, lb = plausible(60, 5)
    r = M.ratios(x, y, la, lb)
    for i in range(len(x)):
        for line in (0, 1):
            v = float(CUT.len_ratio(la[i], lb[i])) if field == "len_ratio" else float(r[field][i, line])
            assert np.isfinite(v) and v > 0
            args = (x[i], y[i], 3, la[i], lb[i])
            at, above = L.cluster_cut_lines({field: v}, *args), L.cluster_cut_lines({field: float(np.nextafter(v, np.inf))}, *args)
            assert at >> line & 1 == 1 and above >> line & 1 == 0, (field, i, line, v, at, above)
            assert at == CUT.cut_lines({field: v}, *args) and above == CUT.cut_lines({field: float(np.nextafter(v, np.inf))}, *args)


def test_the_maximum_of_num_alns_at_a_lines_value_and_one_below():
    x, y, la, lb = plausible(60, 6)
    for i in range(len(x)):
        for line, own in ((0, x[i]), (1, y[i])):
            args = (x[i], y[i], 3, la[i], lb[i])
            at, below = L.cluster_cut_lines({"num_alns": int(own[2])}, *args), L.cluster_cut_lines({"num_alns": int(own[2]) - 1}, *args)
            assert at >> line & 1 == 1 and below >> line & 1 == 0, (i, line, own, at, below)
    # a negative made-up num_alns is below every maximum; no maximum passes everything
    assert L.cluster_cut_lines({"num_alns": 1}, (10, 1, -5), (10, 1, 2), 3, 100, 100) == 1
    assert L.cluster_cut_lines({}, (10, 1, 2**31 - 1), (10, 1, 2), 3, 100, 100) == 3


def test_equal_lengths_have_len_ratio_one():
    for length in (1, 77, 4_000_000_000):
        args = ((10, 1, 1), (10, 1, 1), 3, length, length)
        assert L.cluster_cut_lines({"len_ratio": 1.0}, *args) == 3
        assert L.cluster_cut_lines({"len_ratio": float(np.nextafter(1.0, 2.0))}, *args) == 0
    assert L.cluster_cut_lines({"len_ratio": 1e-300}, (10, 1, 1), (10, 1, 1), 3, 0, 50) == 0          # a length of 0: len_ratio 0


def test_refusals(lib):
    import ctypes as C
    x, y = L.Result(10, 1, 1), L.Result(10, 1, 1)
    for k in CUT.FIELDS[:-1]:
        assert L.cluster_cut_lines({k: float("nan")}, (10, 1, 1), (10, 1, 1), 3, 100, 100) == REFUSED
    assert L.cluster_cut_lines(L.cluster_cut({}, reserved=1), (10, 1, 1), (10, 1, 1), 3, 100, 100) == REFUSED
    cut = L.cluster_cut({})
    assert lib.lzani_cluster_cut_lines(None, C.byref(x), C.byref(y), 3, 100, 100) == REFUSED
    assert lib.lzani_cluster_cut_lines(C.byref(cut), None, C.byref(y), 3, 100, 100) == REFUSED
    assert lib.lzani_cluster_cut_lines(C.byref(cut), C.byref(x), None, 3, 100, 100) == REFUSED
    assert lib.lzani_cluster_cut_lines(C.byref(cut), C.byref(x), C.byref(y), 3, 100, 100) == 3


def test_a_level_under_stricter_minima_is_the_stricter_filter():
    """every minimum of F' >= that of F: the lines of F cut by F' are the lines of F' (passing F' implies passing F)"""
    rng = np.random.default_rng(17)
    x, y, _, la, lb = made_up(400, 41)
    for _ in range(10):
        f = {k: float(rng.choice([0.0, 0.05, 0.3, 0.7])) for k in M.FIELDS}
        g = {k: f[k] + float(rng.choice([0.0, 0.1, 0.25])) for k in M.FIELDS}
        loose, strict = M.lines(f, x, y, la, lb), M.lines(g, x, y, la, lb)
        assert ((strict & ~loose) == 0).all()
        for i in np.flatnonzero(loose):
            assert L.cluster_cut_lines(g, x[i], y[i], loose[i], la[i], lb[i]) == strict[i] == L.out_filter_lines(g, x[i], y[i], la[i], lb[i])
