"""CPU: the choice of a launch's pair kernel (lz-ani_amd/csrc/lzani_pair_dispatch.h: PAIR_KERNELS, pk_id,
choose_pair_kernel) in a stand-alone host program under the address and undefined-behaviour sanitizers, and what it chooses
for every consistent combination of the facts against the rule as tests/util.py states it (pair_kernel_choice, the last step
of predict_kernels)."""
import itertools
import os
import re
import subprocess

import util as U

FACTS = ("regions", "fast", "tw", "pm", "split", "join", "blk", "nfree", "dsel", "rtc")


def consistent(f):
    """The combinations a run can produce (lzani_hip.hip: run_batch, launch_pairs, run_rows_impl)."""
    return ((not f["blk"] or (f["fast"] and f["tw"] and not f["join"] and not f["pm"] and not f["regions"])) and
            (not f["split"] or f["pm"]) and (not f["join"] or not f["regions"]) and
            (not f["rtc"] or (f["dsel"] == 0 and f["fast"] and not f["regions"])))


def test_the_pair_dispatch_under_the_sanitizers(tmp_path):
    src = os.path.join(U.ROOT, "tests", "model", "pair_dispatch_check.cpp")
    exe = str(tmp_path / "pair_dispatch_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",      # (the runtime in the program: it runs beside any preloaded library)
                           src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    want = {}
    for v in itertools.product(*[(0, 1, 2) if k == "dsel" else (0, 1) for k in FACTS]):
        f = dict(zip(FACTS, v))
        if consistent(f):
            want[v] = U.pair_kernel_choice(**{k: (x if k == "dsel" else bool(x)) for k, x in f.items()})
    # by hand: without regions and with k-mer words, (pm, split, join, tw, blk) takes 3 * 2 * 2 + 1 = 13 values, (dsel, rtc) 4;
    # without regions or k-mer words 12 x 3; with regions (fast, tw, pm, split) 2 * 2 * 3 x 3; each with and without N
    assert len(want) == 2 * (13 * 4 + 12 * 3 + 12 * 3) == 248
    lines = r.stdout.splitlines()
    assert len(lines) == len(want)
    seen = set()
    for line in lines:
        facts, aot, rtc = line.split("\t")
        v = tuple(int(x) for x in facts.split())
        assert v in want and v not in seen, line
        seen.add(v)
        assert re.match(U.KERNEL_NAME_RE, aot) and (rtc == "-" or re.match(U.KERNEL_NAME_RE, rtc)), line
        assert (aot, None if rtc == "-" else rtc) == want[v], (line, want[v])
    # every name of the launch record is reached: the ahead-of-time ones chosen (a split's mode 1 with its mode 0), the
    # run-time compiled ones offered
    aots = {a for a, _ in want.values()}
    aots |= {a.replace("mode=0", "mode=1") for a in aots if a.startswith("split ")}
    assert aots | {x for _, x in want.values() if x} == set(U.expected_kernel_names())
