"""The seed word of a text position made from the packed text (lzani_core.h: kms_from_syms, kmer_valid_n, kms_valid_nfree_head)
equals k_kmers' statement -- kmer_at's key -- at every position of random reference texts with and without N runs, at msl 5,
6 and 7, every length mod 16, lengths below 64 and mrd 0 included, and positions kmer_at rejects are rejected.  A stand-alone
host program (tests/model/seed_word_check.cpp) does the comparison; its header says how to run it under the sanitizers."""
import os
import subprocess

import util as U


def test_seed_word_from_the_text_equals_the_kmer_words(tmp_path):
    src = os.path.join(U.ROOT, "tests", "model", "seed_word_check.cpp")
    exe = str(tmp_path / "seed_word_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    n, bad = (int(x) for x in r.stdout.split() if x.isdigit())
    assert n > 400_000 and bad == 0, r.stdout
