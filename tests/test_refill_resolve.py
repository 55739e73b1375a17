"""The pair kernel's refill resolves a candidate from one fetch of each text (lzani_core.h: text_words5, resolve_diff,
diff_same32, null_ext_record_diff).  A stand-alone host program (tests/model/refill_resolve_check.cpp) compares the
match length and the null-extension record these give with the statements they replace -- win2f's compare and
null_ext_record in both of its forms -- at every symbol offset, match length, text start and text end; its header lists
the cases and says how to run it under the sanitizers."""
import os
import subprocess

import util as U


def test_resolve_from_the_words_equals_the_window_statements(tmp_path):
    src = os.path.join(U.ROOT, "tests", "model", "refill_resolve_check.cpp")
    exe = str(tmp_path / "refill_resolve_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    n, bad, rec, masked, missing = (int(x.rstrip(";")) for x in r.stdout.split() if x.rstrip(";").isdigit())
    assert n > 400_000 and bad == 0 and missing == 0, r.stdout
    assert masked > 1000 and rec - masked > 100_000, r.stdout          # both branches of the record's validity
