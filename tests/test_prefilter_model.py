"""CPU: the k-mer prefilter's definitions.  Hand-worked cases for the numpy statement (tests/prefilter_model.py), the
product's own canon / keep (csrc/lzani_prefilter_defs.h, compiled here into a host shim) against it, and the refusals
of the binary's --flt-kmers flags."""
import os
import subprocess

import numpy as np
import pytest

import prefilter_model as PM
import synth_genomes as SG
import util as U

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
CODE = {c: i for i, c in enumerate("ACGT")}


def seq(s):
    return np.array([CODE.get(c, 5) for c in s], dtype=np.uint8)


def rc(x):
    return (3 - x[::-1]).astype(np.uint8)


def rand(seed, n):
    return (SG.splitmix64(seed, np.arange(n, dtype=np.uint64)) % np.uint64(4)).astype(np.uint8)


def test_window_value_packs_the_first_symbol_lowest():
    v, r, valid = PM.window_values(seq("ACGTACGTA"), 8)
    # ACGTACGT = 0,1,2,3,0,1,2,3 -> sum c_j 4^j; it is its own reverse complement
    want = sum(c * 4 ** j for j, c in enumerate([0, 1, 2, 3, 0, 1, 2, 3]))
    assert valid.tolist() == [True, True] and int(v[0]) == want == int(r[0])
    # CGTACGTA: reverse complement TACGTACG
    assert int(v[1]) == sum(c * 4 ** j for j, c in enumerate([1, 2, 3, 0, 1, 2, 3, 0]))
    assert int(r[1]) == sum(c * 4 ** j for j, c in enumerate([3, 0, 1, 2, 3, 0, 1, 2]))


def test_a_genome_and_its_reverse_complement_share_everything():
    g = rand(1, 3000)
    for k in (8, 15, 16, 21, 31):
        kmers_of, shared = PM.shared_matrix([g, rc(g)], k)
        assert kmers_of[0] == kmers_of[1] == shared[0, 1] > 0
        assert np.array_equal(PM.kmer_set(g, k), PM.kmer_set(rc(g), k))


def test_a_palindromic_kmer_is_counted_once():
    # ACGTACGT is its own reverse complement: one window, one k-mer.  Twice in a row: nine windows over the four
    # rotations, of which CGTACGTA and TACGTACG are each other's reverse complement -- three k-mers
    assert len(PM.kmer_set(seq("ACGTACGT"), 8)) == 1
    assert len(PM.canon_windows(seq("ACGTACGTACGTACGT"), 8)) == 9 and len(PM.kmer_set(seq("ACGTACGTACGTACGT"), 8)) == 3
    kmers_of, shared = PM.shared_matrix([seq("ACGTACGT"), seq("TTACGTACGTTT")], 8)
    assert kmers_of.tolist() == [1, 5] and shared[0, 1] == 1


def test_a_window_with_an_n_is_void_and_short_genomes_have_none():
    g = rand(2, 100)
    h = g.copy()
    h[50] = 5
    for k in (8, 21):
        assert len(PM.canon_windows(g, k)) == 100 - k + 1
        assert len(PM.canon_windows(h, k)) == 100 - k + 1 - k              # the k windows over position 50
    assert len(PM.canon_windows(np.full(40, 4, dtype=np.uint8), 8)) == 0
    for L in (0, 1, 7):
        assert len(PM.kmer_set(rand(3, L), 8)) == 0
    kmers_of, shared = PM.shared_matrix([rand(3, 7), g], 8)
    assert kmers_of.tolist() == [0, 93] and shared[0, 1] == 0
    assert PM.kept_pairs(kmers_of, shared)[0].tolist() == [0, 0, 0]


@pytest.mark.parametrize("k", [15, 16, 21, 31])
def test_a_planted_40mer_is_shared_as_41_minus_k_kmers(k):
    # seeds 11 / 12 / 13: two random genomes of 2,000 bases and a random 40-mer; at k >= 15 nothing else is common
    # (asserted below without the plant)
    a, b, plant = rand(11, 2000), rand(12, 2000), rand(13, 40)
    assert PM.shared_matrix([a, b], k)[1][0, 1] == 0
    a[300:340] = plant
    b[1500:1540] = rc(plant)                                               # on the other strand
    b[1540], b[1499] = (4 - a[299]) % 4, (4 - a[340]) % 4                  # not the complements of a's flanks: the match ends there
    kmers_of, shared = PM.shared_matrix([a, b], k)
    assert shared[0, 1] == 41 - k
    row_off, ids, sh = PM.kept_pairs(kmers_of, shared, min_shared=41 - k)
    assert row_off.tolist() == [0, 1, 1] and ids.tolist() == [1] and sh.tolist() == [41 - k]
    assert len(PM.kept_pairs(kmers_of, shared, min_shared=42 - k)[1]) == 0


def test_kept_pairs_compare_the_ratio_in_double():
    kmers_of = np.array([980, 1070, 3, 0])
    shared = np.zeros((4, 4), dtype=np.int64)
    shared[0, 1], shared[0, 2], shared[1, 2] = 490, 1, 2
    assert PM.kept_pairs(kmers_of, shared, 1, 0.5)[1].tolist() == [1, 2]            # 490/980 = 0.5 is kept; 1/3 is not; 2/3 is
    assert PM.kept_pairs(kmers_of, shared, 2, 0.0)[1].tolist() == [1, 2]
    assert PM.kept_pairs(kmers_of, shared, 0, 0.0)[0].tolist() == [0, 2, 3, 3, 3]   # min_shared 0 means 1


def test_sampling_keeps_the_values_whose_hash_is_within_the_bound():
    # splitmix64's published sequence from state 0: outputs for the states 0, g, 2g (g = 0x9E3779B97F4A7C15), i.e.
    # the hash of 0, g and 2g here
    g = 0x9E3779B97F4A7C15
    xs = np.array([0, g, (2 * g) & PM.SAMPLE_ALL], dtype=np.uint64)
    hs = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert [int(h) for h in PM.splitmix64(xs)] == hs
    assert PM.keep(xs).tolist() == [True, True, True]
    assert PM.keep(xs, hs[1]).tolist() == [False, True, True]                  # <= the bound
    assert PM.keep(xs, hs[1] - 1).tolist() == [False, False, True]
    assert PM.keep(xs, 0).tolist() == [False, False, False]
    x = PM.canon_windows(rand(5, 5000), 16)
    kept = PM.kmer_set(rand(5, 5000), 16, 1 << 62)
    assert np.array_equal(kept, np.unique(x[PM.splitmix64(x) <= np.uint64(1 << 62)])) and 0.2 < len(kept) / len(np.unique(x)) < 0.3


SHIM = r"""
#include <cstdio>
#include <vector>
#include "lzani_prefilter_defs.h"
// stdin: k, n, sample_max, then n windows of k codes; stdout: canon and keep of every window, computed by the
// product's pf_canon / pf_keep from the two packed values made here digit by digit
int main()
{
    unsigned long long k, n, smax;
    if (fread(&k, 8, 1, stdin) != 1 || fread(&n, 8, 1, stdin) != 1 || fread(&smax, 8, 1, stdin) != 1) return 1;
    std::vector<unsigned char> c(k);
    for (unsigned long long i = 0; i < n; ++i) {
        if (fread(c.data(), 1, k, stdin) != k) return 1;
        lzani::u64 v = 0, r = 0;
        for (unsigned j = 0; j < k; ++j) { v |= (lzani::u64)c[j] << (2 * j); r |= (lzani::u64)(3 - c[k - 1 - j]) << (2 * j); }
        const unsigned long long x = lzani::pf_canon(v, r), kept = lzani::pf_keep(x, smax);
        fwrite(&x, 8, 1, stdout); fwrite(&kept, 8, 1, stdout);
    }
    return 0;
}
"""


def test_the_products_canon_and_keep_equal_the_numpy_statement(tmp_path):
    src, exe = tmp_path / "shim.cpp", tmp_path / "shim"
    src.write_text(SHIM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(U.ROOT, "lz-ani_amd", "csrc"), str(src), "-o", str(exe)])
    n = 100_000
    for k, smax in ((8, PM.SAMPLE_ALL), (16, 1 << 62), (31, 1 << 63), (31, 12345)):
        w = rand(100 + k, n * k).reshape(n, k)
        head = np.array([k, n, smax], dtype=np.uint64).tobytes()
        out = subprocess.run([str(exe)], input=head + w.tobytes(), capture_output=True, check=True).stdout
        got = np.frombuffer(out, dtype=np.uint64).reshape(n, 2)
        v, r, valid = PM.window_values(np.concatenate([np.concatenate((row, [5])) for row in w[:2000]]), k)
        want = np.minimum(v, r)[valid]
        assert len(want) == 2000 and np.array_equal(got[:2000, 0], want)          # through the sliding-window statement
        j = np.arange(k, dtype=np.uint64)
        vv = (w.astype(np.uint64) << (2 * j)).sum(axis=1, dtype=np.uint64)
        rr = ((3 - w[:, ::-1]).astype(np.uint64) << (2 * j)).sum(axis=1, dtype=np.uint64)
        canon = np.minimum(vv, rr)
        assert np.array_equal(got[:, 0], canon)
        assert np.array_equal(got[:, 1].astype(bool), PM.keep(canon, smax))


@pytest.fixture(scope="module")
def host_binary():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])
    return EXE


@pytest.mark.parametrize("args, message", [
    (["--flt-kmers", "21", "0.5", "--flt-kmerdb", "no_such_filter.txt", "0.5"], "--flt-kmers and --flt-kmerdb cannot be used together"),
    (["--flt-kmers", "7", "0.5"], "--flt-kmers 7 (k-mer lengths 8 .. 31 are supported)"),
    (["--flt-kmers", "32", "0.5"], "--flt-kmers 32 (k-mer lengths 8 .. 31 are supported)"),
    (["--flt-kmers", "21", "0.5", "--flt-kmers-fraction", "0"], "Invalid value for --flt-kmers-fraction: 0 "),
    (["--flt-kmers", "21", "0.5", "--flt-kmers-fraction", "1.01"], "Invalid value for --flt-kmers-fraction: 1.01 "),
    (["--flt-kmers", "21", "0.5", "--flt-kmers-fraction", "-0.5"], "Invalid value for --flt-kmers-fraction: -0.5 "),
    (["--flt-kmers", "21", "0.5", "--flt-kmers-fraction", "half"], "Invalid value for --flt-kmers-fraction: half "),
    (["--flt-kmers", "21", "0.5", "--flt-kmers-fraction", "nan"], "Invalid value for --flt-kmers-fraction: nan "),
])
def test_the_binary_refuses_bad_kmer_filter_flags_before_reading_input(host_binary, tmp_path, args, message):
    missing = str(tmp_path / "no_such_input.fa")
    p = subprocess.run([host_binary, "all2all", "--in-fasta", missing, "-o", str(tmp_path / "o.tsv")] + args, capture_output=True, text=True)
    assert p.returncode == 1 and message in p.stderr, p.stderr
    assert "Cannot open file" not in p.stderr and "Loading sequences" not in p.stderr


def test_good_kmer_filter_flags_reach_the_input(host_binary, tmp_path):
    missing = str(tmp_path / "no_such_input.fa")
    p = subprocess.run([host_binary, "all2all", "--in-fasta", missing, "-o", str(tmp_path / "o.tsv"), "--flt-kmers", "21", "0.5",
                        "--flt-kmers-fraction", "0.2"], capture_output=True, text=True)
    assert p.returncode == 1 and "Cannot open file: " + missing in p.stderr


def test_usage_names_the_flags(host_binary):
    p = subprocess.run([host_binary], capture_output=True, text=True)
    assert "--flt-kmers <k> <float>" in p.stderr and "--flt-kmers-fraction" in p.stderr
