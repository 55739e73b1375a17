"""The mal-mer word the pair kernel's refill makes from the packed query text (lzani_core.h: kml_from_syms, kmer_valid_n,
kmer_valid_nfree_head) equals k_kmers' statement -- kmer_at + mix_key -- at every position of random reference texts with and
without N runs, at mal 9, 11 and 15, and positions kmer_at rejects are rejected.  A stand-alone host program
(tests/model/refill_hash_check.cpp) does the comparison; its header says how to run it under the sanitizers."""
import os
import subprocess

import util as U


def test_hash_from_the_text_equals_the_kmer_words(tmp_path):
    src = os.path.join(U.ROOT, "tests", "model", "refill_hash_check.cpp")
    exe = str(tmp_path / "refill_hash_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    n, bad = (int(x) for x in r.stdout.split() if x.isdigit())
    assert n > 400_000 and bad == 0, r.stdout
