"""CPU: the rule of the output filter as the library states it (lzani_out_filter_lines, csrc/lzani_out_filter.h) against
tests/out_filter_model.py -- seeded tuples and the edges -- the host emitter's two routes from a pair to its text (the table
of all pairs and a kept record, tests/model/emit_shim.cpp) against the model, and the host binary through its --results-in
seam, where the filter stays on the host."""
import os
import subprocess

import numpy as np
import pytest

import lzani_ctypes as L
import oracle as O
import out_filter_model as M
import util as U

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
REFUSED = 0xFFFFFFFF


@pytest.fixture(scope="module", autouse=True)
def lib():
    L.build_library()
    return L.load_library()


def tuples(seed, count):
    """(x, y, la, lb, filter) of made-up pairs: results that fit their lengths, a few that do not, some zeros."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        la, lb = (int(v) for v in rng.integers(1, 60000, 2))
        if rng.random() < 0.05:
            la = 0
        if rng.random() < 0.05:
            lb = 0
        def res(qlen):
            top = max(qlen, 1) if rng.random() < 0.9 else 3 * max(qlen, 1)
            al = int(rng.integers(0, top + 1)) if rng.random() < 0.9 else 0
            m = int(rng.integers(0, al + 1))
            return (m, al - m, int(rng.integers(0, 50)))
        x, y = res(lb), res(la)
        r = M.ratios(x, y, la, lb)
        flt = {}
        for k in M.FIELDS:
            mode = rng.random()
            if mode < 0.4:
                continue
            v = float(r[k][int(rng.integers(0, 2))]) if mode < 0.7 else float(rng.random())
            if np.isfinite(v):
                flt[k] = v if rng.random() < 0.5 else float(np.nextafter(v, np.inf))
        out.append((x, y, la, lb, flt))
    return out


def test_lines_agree_with_the_model_on_seeded_tuples():
    seen = set()
    for x, y, la, lb, flt in tuples(20261, 4000):
        want = int(M.lines(flt, x, y, la, lb))
        assert L.out_filter_lines(flt, x, y, la, lb) == want, (x, y, la, lb, flt)
        seen.add(want)
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("field", M.FIELDS)
def test_a_minimum_at_the_exact_ratio_keeps_the_line_and_the_next_double_drops_it(field):
    x, y, la, lb = (31337, 1201, 9), (29991, 4410, 12), 40013, 35117
    r = M.ratios(x, y, la, lb)
    for line in (0, 1):
        v = float(r[field][line])
        assert 0 < v < 1
        at, above = L.out_filter_lines({field: v}, x, y, la, lb), L.out_filter_lines({field: float(np.nextafter(v, np.inf))}, x, y, la, lb)
        assert at == int(M.lines({field: v}, x, y, la, lb)) and at & (1 << line)
        assert above == int(M.lines({field: float(np.nextafter(v, np.inf))}, x, y, la, lb)) and not above & (1 << line)
        assert L.out_filter_lines({field: float(np.nextafter(v, 0))}, x, y, la, lb) & (1 << line)


def test_edges():
    x, y = (500, 20, 3), (450, 70, 4)
    assert L.out_filter_lines({}, x, y, 1000, 900) == 3                           # all minima 0: both lines
    assert L.out_filter_lines({}, (0, 0, 0), (0, 0, 0), 0, 0) == 3                # NaN everywhere: below nothing
    # X.m + X.l == 0: ani of line 0 is 0, and so is its qcov and line 1's rcov
    z = (0, 0, 0)
    assert M.ratios(z, y, 1000, 900)["ani"][0] == 0
    for flt, want in (({"ani": 1e-300}, 2), ({"qcov": 1e-300}, 2), ({"rcov": 1e-300}, 1), ({"ani": 0.0}, 3)):
        assert L.out_filter_lines(flt, z, y, 1000, 900) == int(M.lines(flt, z, y, 1000, 900)) == want, flt
    # a printed length of 0: the line that divides by it has inf (never below) or NaN (0 / 0)
    for la, lb in ((0, 900), (1000, 0), (0, 0)):
        for flt in ({"gani": 0.9}, {"qcov": 2.0}, {"rcov": 0.99}, {"tani": 0.6}, {"gani": 1e308, "qcov": 1e308, "rcov": 1e308}):
            for xx, yy in ((x, y), (z, y), (x, z), (z, z)):
                assert L.out_filter_lines(flt, xx, yy, la, lb) == int(M.lines(flt, xx, yy, la, lb)), (la, lb, flt, xx, yy)
    assert L.out_filter_lines({"gani": 1e308}, x, y, 0, 900) == 2                 # line 1 divides by la = 0: inf passes, line 0 does not
    # a NaN minimum is refused, whatever the field; an inf minimum is a number
    for k in M.FIELDS:
        assert L.out_filter_lines({k: float("nan")}, x, y, 1000, 900) == REFUSED
    assert L.out_filter_lines({"ani": float("inf")}, x, y, 1000, 900) == 0
    # the sums are 32-bit: matches that wrap, lengths that wrap
    big = (2**31 - 5, 100, 1)
    assert L.out_filter_lines({"tani": 0.5}, big, big, 2**31, 2**31 + 7) == int(M.lines({"tani": 0.5}, big, big, 2**31, 2**31 + 7))


def test_results_in_seam_keeps_the_host_filter(tmp_path):
    """--results-in with an --out-filter: the device stage does not apply (there is no run), the host path writes what it
    wrote, and what it writes is what the model keeps."""
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])
    names, seqs = U.reorder(*U.load_example())
    res = O.oracle_all2all(seqs, None, threads=8)
    n, lens = len(seqs), [len(s) for s in seqs]
    raw = str(tmp_path / "raw.txt")
    with open(raw, "w") as f:
        for r in range(n):
            for q in range(n):
                if r != q:
                    f.write(f"{r} {q} {res[r, q, 0]} {res[r, q, 1]} {res[r, q, 2]}\n")
    fa = os.path.join(U.GOLD, "example", "multifasta.fna")
    cols = "qidx,ridx,query,reference,tani,gani,ani,qcov,rcov,num_alns,len_ratio,qlen,rlen,nt_match,nt_mismatch".split(",")
    full = U.emit_tsv(names, lens, res, cols).split("\n")
    for flt in ({"ani": 0.9, "qcov": 0.5}, {"tani": 0.3, "rcov": 0.4}):
        out = str(tmp_path / "f.tsv")
        args = ["all2all", "--in-fasta", fa, "-o", out, "--results-in", raw, "--out-format", "complete", "-V", "2"]
        for k, v in flt.items():
            args += ["--out-filter", k, repr(v)]
        p = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        assert "out-filter on the device" not in p.stderr
        want = [full[0]]
        for ln in full[1:]:
            if not ln:
                continue
            q, r = (int(v) for v in ln.split("\t")[:2])
            a, b = min(q, r), max(q, r)
            bits = int(M.lines(flt, res[a, b], res[b, a], lens[a], lens[b]))
            if bits & (1 if q == b else 2):
                want.append(ln)
        got = open(out).read().split("\n")
        assert got[:-1] == want and got[-1] == "" and 1 < len(want) < len(full) - 1


COMPLETE = "qidx,ridx,query,reference,tani,gani,ani,qcov,rcov,num_alns,len_ratio,qlen,rlen,nt_match,nt_mismatch".split(",")


@pytest.fixture(scope="module")
def format_pair():
    """host_format_pair of tests/model/emit_shim.cpp: (x, y, la, lb, filter or None, percent, kept lines) -> (the lines of the
    table route's record, its text through format_row, the text of a lzani_kept_pair through format_kept)."""
    import ctypes as C
    d = os.path.join(U.ROOT, "tests", "model")
    so = os.path.join(d, "libemit_pair_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", os.path.join(d, "emit_shim.cpp"), "-o", so, "-lz"])
    lib = C.CDLL(so)
    lib.host_format_pair.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_uint32, C.c_char_p, C.c_char_p, C.c_size_t]
    lib.host_format_pair.restype = C.c_uint32
    a, b = C.create_string_buffer(4096), C.create_string_buffer(4096)

    def call(x, y, la, lb, flt, percent, kept_lines):
        rx, ry = (C.c_int32 * 3)(*x), (C.c_int32 * 3)(*y)
        minima = None if flt is None else (C.c_double * 5)(*(flt.get(k, 0.0) for k in M.FIELDS))
        lines = lib.host_format_pair(rx, ry, la, lb, minima, int(percent), kept_lines, a, b, 4096)
        assert lines != REFUSED
        return lines, a.value.decode(), b.value.decode()
    return call


def test_printed_lines_and_filter_follow_the_model_on_seeded_tuples(format_pair):
    """The emitter's two routes to a pair's text -- the table of all pairs (format_row) and a kept record (format_kept, its
    `lines` from lzani_out_filter_lines as the device stage would set them) -- give the same bytes, and those are the lines
    of util.emit_tsv that out_filter_model.lines keeps: with a filter and without, in percent (every other tuple) and not.
    Tuples with a printed length of 0 are left out (a line then prints inf or NaN, which real_to_chars does not take): 9.75 %
    by construction."""
    all_tuples = tuples(20261, 4000)
    seen, used = set(), 0
    for i, (x, y, la, lb, flt) in enumerate(all_tuples):
        if la == 0 or lb == 0:
            continue
        used += 1
        percent = bool(i & 1)
        res = np.zeros((2, 2, 3), dtype=np.int64)
        res[0, 1], res[1, 0] = x, y
        both = U.emit_tsv(["A", "B"], [la, lb], res, COMPLETE, in_percent=percent).split("\n")[1:3]
        assert all(both) and both[0].startswith("1\t0\tB\tA\t") and both[1].startswith("0\t1\tA\tB\t")
        lines, by_table, by_record = format_pair(x, y, la, lb, None, percent, 3)
        assert lines == 3 and by_table == by_record == both[0] + "\n" + both[1] + "\n", (x, y, la, lb)
        want = int(M.lines(flt, x, y, la, lb))
        lines, by_table, by_record = format_pair(x, y, la, lb, flt, percent, L.out_filter_lines(flt, x, y, la, lb))
        assert lines == want, (x, y, la, lb, flt)
        assert by_table == by_record == "".join(both[k] + "\n" for k in (0, 1) if want >> k & 1), (x, y, la, lb, flt)
        seen.add(want)
    assert len(all_tuples) - used < 0.15 * len(all_tuples)
    assert seen == {0, 1, 2, 3}


def test_host_record_wraps_like_the_rule(format_pair):
    """The 32-bit wrap case of test_edges through the emitter's own record (lines only: the model prints no wrapped text)."""
    big = (2**31 - 5, 100, 1)
    la, lb = 2**31, 2**31 + 7
    for flt in ({"tani": 0.5}, {"qcov": 0.0}, {"gani": 0.25, "rcov": 0.25}):
        want = int(M.lines(flt, big, big, la, lb))
        assert format_pair(big, big, la, lb, flt, False, want)[0] == want == L.out_filter_lines(flt, big, big, la, lb), flt
    assert format_pair(big, big, la, lb, None, False, 3)[0] == 3
