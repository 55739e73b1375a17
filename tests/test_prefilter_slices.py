"""CPU: the host side of the streamed k-mer prefilter (lzani_prefilter_codes).  The slice plan (lzani_plan_slices) against
a Python statement of its rule; the two functions its kernel forms windows with -- the window value from packed symbol
codes and the reverse complement from the forward value (csrc/lzani_prefilter_defs.h, compiled here into a host shim)
-- against the numpy statement of the definitions (tests/prefilter_model.py); and the binary's usage text."""
import os
import subprocess

import numpy as np
import pytest

import lzani_ctypes as L
import prefilter_model as PM
import synth_genomes as SG
import util as U

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")


def plan(lens, slice_bytes):
    """The rule of include/lzani.h: genomes in id order; a new slice starts where the next genome would take the slice's
    sum of lengths above slice_bytes.  (number of slices, slice_of); None where a genome is longer than a slice."""
    if slice_bytes == 0:
        return 1, [0] * len(lens)
    if max(lens) > slice_bytes:
        return None
    s, cur, out = 0, 0, []
    for x in lens:
        if cur + x > slice_bytes:
            s, cur = s + 1, 0
        cur += x
        out.append(s)
    return s + 1, out


def rand(seed, n, mod=4):
    return (SG.splitmix64(seed, np.arange(n, dtype=np.uint64)) % np.uint64(mod)).astype(np.int64)


def test_new_symbols_are_exported():
    L.build_library()
    lib = L.load_library()
    for name in ("lzani_prefilter_codes", "lzani_plan_slices", "lzani_get_prefilter_stream_info"):
        assert name in L.EXPORTS and getattr(lib, name) is not None


def test_plan_equals_the_rule_on_random_lengths():
    for seed in range(40):
        n = 1 + int(rand(seed, 1)[0] * 17 + seed) % 60
        lens = rand(1000 + seed, n, 5000)
        lens[rand(2000 + seed, n, 5) == 0] = 0                        # every fifth genome or so is empty
        lo = int(lens.max())
        for sb in (0, max(lo, 1), lo + 1, lo + 777, 3 * lo + 5, int(lens.sum()), int(lens.sum()) + 1, 1 << 40):
            want = plan(lens.tolist(), sb)
            ns, slice_of = L.plan_slices(lens, sb)
            assert (ns, slice_of.tolist()) == want, (seed, sb)
            sums = np.bincount(slice_of, weights=lens, minlength=ns)
            assert sb == 0 or sums.max() <= sb


def test_plan_edge_cases():
    # a genome exactly slice_bytes long fits, and is alone with it unless its neighbours are empty
    assert L.plan_slices([3, 8, 0, 0, 1, 7, 0], 8)[1].tolist() == [0, 1, 1, 1, 2, 2, 2]
    # one longer: refused
    with pytest.raises(L.LzaniError, match="LZANI_ERR_ARG"):
        L.plan_slices([3, 9, 1], 8)
    # empty genomes join the current slice, also the first one and also a full one
    ns, slice_of = L.plan_slices([0, 0, 8, 0, 8], 8)
    assert ns == 2 and slice_of.tolist() == [0, 0, 0, 0, 1]
    assert L.plan_slices([0, 0, 0], 5)[0] == 1 and L.plan_slices([0, 0, 0], 0)[0] == 1
    # slice_bytes 0: one slice whatever the lengths
    ns, slice_of = L.plan_slices([5, 1 << 30, 7], 0)
    assert ns == 1 and slice_of.tolist() == [0, 0, 0]
    # one genome per slice
    ns, slice_of = L.plan_slices([5, 4, 5, 3, 5], 5)
    assert ns == 5 and slice_of.tolist() == [0, 1, 2, 3, 4]
    # no genomes, no lengths
    lib = L.load_library()
    assert lib.lzani_plan_slices(0, None, 8, None) == -1
    lens = np.array([1, 2], dtype=np.uint32)
    assert lib.lzani_plan_slices(2, None, 8, None) == -1
    assert lib.lzani_plan_slices(2, lens.ctypes.data, 8, None) == 1           # slice_of may be NULL


SHIM = r"""
#include <cstdio>
#include <vector>
#include "lzani_prefilter_defs.h"
// stdin: k, L, then L symbol codes; stdout: for every window 0 <= p <= L - k its validity, its value and the value of its
// reverse complement -- by the product's pf_pack16 / pf_window / pf_rc_of, the way the kernel uses them: the codes packed
// in groups of 16 (the last one cut at L), the windows formed from the groups
int main()
{
    unsigned long long k, L;
    if (fread(&k, 8, 1, stdin) != 1 || fread(&L, 8, 1, stdin) != 1) return 1;
    std::vector<unsigned char> c(L);
    if (L && fread(c.data(), 1, L, stdin) != L) return 1;
    const size_t groups = (L + 15) / 16 + 3;
    std::vector<lzani::u32> t2(groups);
    std::vector<unsigned short> nm(groups);
    for (size_t j = 0; j < groups; ++j) {
        const long long left = (long long)L - 16 * (long long)j;
        lzani::u32 sym, nb;
        lzani::pf_pack16(c.data() + (left > 0 ? 16 * j : 0), left < 0 ? 0 : (left > 16 ? 16 : (int)left), sym, nb);
        t2[j] = sym; nm[j] = (unsigned short)nb;
    }
    for (unsigned long long p = 0; p + k <= L; ++p) {
        lzani::u64 v = 0;
        const unsigned long long ok = lzani::pf_window(t2.data(), nm.data(), (int)p, (int)k, v);
        const unsigned long long f = ok ? v : 0, r = ok ? lzani::pf_rc_of(v, (int)k) : 0;
        fwrite(&ok, 8, 1, stdout); fwrite(&f, 8, 1, stdout); fwrite(&r, 8, 1, stdout);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("pfshim")
    src, exe = d / "shim.cpp", d / "shim"
    src.write_text(SHIM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(U.ROOT, "lz-ani_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("k", [8, 15, 16, 21, 31])
def test_windows_from_codes_and_their_reverse_complement_equal_the_numpy_statement(shim, k):
    for seed, n in ((1, 5000), (2, 4096 + k - 1), (3, k), (4, k - 1), (5, 0), (6, 33)):
        c = rand(10 * k + seed, n).astype(np.uint8)
        if n:
            c[rand(77 * k + seed, n, 61) == 0] = 4 + seed % 3          # N's of several codes, one in 61
        if n > 400:
            c[200:260] = 5                                             # a run of N's over several groups
            c[-3:] = 4                                                 # ... and at the end
        head = np.array([k, n], dtype=np.uint64).tobytes()
        out = subprocess.run([shim], input=head + c.tobytes(), capture_output=True, check=True).stdout
        got = np.frombuffer(out, dtype=np.uint64).reshape(-1, 3)
        v, rc, valid = PM.window_values(c, k)
        assert len(got) == len(v) == max(n - k + 1, 0)
        assert np.array_equal(got[:, 0].astype(bool), valid), (k, n)
        assert np.array_equal(got[valid, 1], v[valid]) and np.array_equal(got[valid, 2], rc[valid]), (k, n)
        if n == 5000:
            assert 0.2 * len(valid) < int(valid.sum()) < len(valid)


def test_usage_says_what_gpu_mem_means_for_the_kmer_filter():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])
    p = subprocess.run([EXE], capture_output=True, text=True)
    assert "--gpu-mem <size>" in p.stderr and "with --flt-kmers also the size of the filter's staging buffer" in p.stderr
