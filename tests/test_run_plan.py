"""CPU: the pure decisions of a run (lz-ani_amd/csrc/lzani_run_plan.h: cut_batches, plan_queues, choose_split,
slab_bytes_per_slot) in a stand-alone host program under the address and undefined-behaviour sanitizers, and the split
decision it prints for a fixed grid against the rule as tests/util.py states it."""
import os
import subprocess

import util as U


def test_the_run_plan_under_the_sanitizers(tmp_path):
    src = os.path.join(U.ROOT, "tests", "model", "run_plan_check.cpp")
    exe = str(tmp_path / "run_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",      # (the runtime in the program: it runs beside any preloaded library)
                           src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    row_cases, split_cases, above_cap, empty_rows, splits = (int(x) for x in lines[-1].split())
    assert row_cases >= 3000 and split_cases >= 3000 and above_cap > 100 and empty_rows > 1000 and splits > 100
    grid = [l.split()[1:] for l in lines if l.startswith("grid ")]
    assert len(grid) == len(lines) - 1 == 6 * 3 * 3 * 6
    seen = set()
    for pairs, cb_words, dmax, split, split_s, seglen, got_S, got_seglen, got_lpt in (map(int, g) for g in grid):
        env = {"LZANI_SPLIT_S": str(split_s)}
        if split >= 0:
            env["LZANI_SPLIT"] = str(split)
        if seglen:
            env["LZANI_SPLIT_SEGLEN"] = str(seglen)
        want = U.split_rule(pairs, cb_words, dmax, env)
        assert (got_S >= 2) == want and got_S != 1, (pairs, cb_words, dmax, env, got_S)
        assert not want or (got_lpt == 1 and got_seglen >= 512)
        seen.add((split, want))
    assert seen == {(-1, False), (-1, True), (0, False), (1, False), (1, True)}       # both answers with and without the switch
    # the thresholds of the default rule, by name: 8 x 5 Mbp (56 pairs) and 16 x 5 Mbp (240) split, 32 x 5 Mbp (992) from
    # bitmaps of 65,536 words on, 5,000 pairs and bitmaps below 8,192 words never
    D = lambda cb: cb * 32 - 320
    assert U.split_rule(56, 8192, D(8192)) and U.split_rule(240, 8192, D(8192)) and U.split_rule(512, 8192, D(8192))
    assert not U.split_rule(513, 8192, D(8192)) and not U.split_rule(992, 8192, D(8192)) and U.split_rule(992, 65536, D(65536))
    assert U.split_rule(1024, 65536, D(65536)) and not U.split_rule(1025, 65536, D(65536))
    assert not U.split_rule(5000, 65536, D(65536)) and not U.split_rule(1, 4096, D(4096))
