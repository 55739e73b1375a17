"""CPU: the host side of the prefilter's k-mer passes.  The pass plan (lzani_plan_passes) against a Python statement of
its rule (tests/prefilter_pass_model.py) on random histograms, with the properties the rule promises; the bin of a k-mer
(pf_bin of csrc/lzani_prefilter_defs.h, compiled here into a host shim) against the numpy statement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lzani_ctypes as L
import prefilter_pass_model as PP
import synth_genomes as SG
import util as U

BINS = PP.BINS


def rand(seed, n, mod):
    return (SG.splitmix64(seed, np.arange(n, dtype=np.uint64)) % np.uint64(mod)).astype(np.uint64)


def histograms():
    """Random histograms: dense, sparse (most bins empty), a few heavy bins among light ones, all empty."""
    out = [rand(1, BINS, 1000), rand(2, BINS, 3)]
    h = rand(3, BINS, 50)
    h[rand(4, BINS, 97) != 0] = 0
    out.append(h)
    h = rand(5, BINS, 20)
    h[rand(6, BINS, 211) == 0] = 5000
    out.append(h)
    out.append(np.zeros(BINS, dtype=np.uint64))
    h = np.zeros(BINS, dtype=np.uint64)
    h[BINS - 1] = 17                                           # only the last bin
    out.append(h)
    return out


def test_new_symbols_are_exported():
    L.build_library()
    lib = L.load_library()
    for name in ("lzani_get_prefilter_pass_info", "lzani_prefilter_pass_plan", "lzani_plan_passes"):
        assert name in L.EXPORTS and getattr(lib, name) is not None
    assert C.sizeof(L.PrefilterPassInfo) == 40


@pytest.mark.parametrize("P", [1, 2, 3, 7, 4096])
def test_forced_plan_equals_the_rule(P):
    for hist in histograms()[:2]:
        got = L.plan_passes(hist, 0, forced=P).tolist()            # a forced plan reads neither the histogram nor cap
        assert got == PP.plan(hist, 0, P) == [BINS * p // P for p in range(P + 1)]
        assert got[0] == 0 and got[-1] == BINS and len(got) == P + 1 and all(a < b for a, b in zip(got, got[1:]))
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        L.plan_passes(histograms()[0], 1 << 40, forced=BINS + 1)


def test_automatic_plan_equals_the_rule_and_is_greedy():
    seen = set()
    for i, hist in enumerate(histograms()):
        total, top = int(hist.sum()), int(hist.max())
        caps = {total, total + 1, max(total - 1, top), max(-(-total // 2), top), max(total // 9, top), top, top + 1, (1 << 32) - 1, (1 << 64) - 1}
        for cap in sorted(caps):
            want = PP.plan(hist, cap)
            got = L.plan_passes(hist, cap).tolist()
            assert got == want, (i, cap)
            P = len(got) - 1
            seen.add(min(P, 3))
            assert got[0] == 0 and got[-1] == BINS and all(a < b for a, b in zip(got, got[1:]))          # 0 .. 4096 in order
            sums = PP.pass_windows(hist, got)
            assert sum(sums) == total and max(sums) <= cap                                             # every pass fits
            assert all(a + b > cap for a, b in zip(sums, sums[1:]))                                    # no two neighbours would
            assert (P == 1) == (total <= cap)
    assert seen == {1, 2, 3}                                                                           # one, two and many passes


def test_a_bin_above_cap_is_refused():
    lib = L.load_library()
    for hist in histograms()[:4]:
        top = int(hist.max())
        assert PP.plan(hist, top - 1) is None
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            L.plan_passes(hist, top - 1)
        with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
            L.plan_passes(hist, 0)
    hist = histograms()[0]
    assert lib.lzani_plan_passes(hist.ctypes.data, C.c_uint64(1 << 40), 0, None) == 1                  # bin_lo may be NULL
    assert lib.lzani_plan_passes(None, C.c_uint64(1 << 40), 0, None) == -1                             # automatic needs the histogram
    assert lib.lzani_plan_passes(None, C.c_uint64(0), 5, None) == 5


SHIM = r"""
#include <cstdio>
#include "lzani_prefilter_defs.h"
// stdin: u64 values; stdout: pf_bin of each, as u64
int main()
{
    unsigned long long x;
    while (fread(&x, 8, 1, stdin) == 1) {
        const unsigned long long b = lzani::pf_bin(x);
        fwrite(&b, 8, 1, stdout);
    }
    return lzani::PF_BINS == 4096 ? 0 : 1;
}
"""


def test_pf_bin_equals_the_numpy_statement(tmp_path):
    src, exe = tmp_path / "shim.cpp", tmp_path / "shim"
    src.write_text(SHIM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(U.ROOT, "lz-ani_amd", "csrc"), str(src), "-o", str(exe)])
    x = np.concatenate((np.arange(300, dtype=np.uint64), SG.splitmix64(77, np.arange(20000, dtype=np.uint64)),
                        np.array([(1 << 62) - 1, (1 << 64) - 1, 1 << 20, 1 << 32], dtype=np.uint64)))
    out = subprocess.run([str(exe)], input=x.tobytes(), capture_output=True, check=True).stdout
    got = np.frombuffer(out, dtype=np.uint64).astype(np.int64)
    want = ((PP.PM.splitmix64(x) >> np.uint64(20)) & np.uint64(4095)).astype(np.int64)
    assert np.array_equal(got, want) and np.array_equal(want, PP.bin_of(x))
    assert len(np.unique(got)) > 4000                                                                  # (the bins are used)
