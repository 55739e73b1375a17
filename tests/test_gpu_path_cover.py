"""GPU: the oracle-compared cells reach every exit of the pair kernel's hand-written loops.

The coverage library (build/diag/liblzani_cover.so: the engine with -DLZANI_PATH_STATS -DLZANI_CHAIN_STATS) counts how
find_event found its events, how the null chain left and how the stretch chain left; tests/path_cover.py runs the cells of a
tuple on it in a child process (lzani_ctypes reads LZANI_LIB at import) and prints the raw totals per cell.  Two things are
asserted on every child's lines:
- parity of the diagnostic build: every cell launches its kernel and equals the oracle, as tests/inst_cell.py asserts it for
  the shipped library (which also keeps the diagnostic builds from rotting);
- coverage: per chain class -- (defaults | long) x (NFREE | N) x (bitmaps | join | probe | split) -- every slot of
  path_cover.REQUIRED is non-zero in the union of the class's cells, unless CANNOT_OCCUR gives the reason from the code why
  the class cannot count it.
Two limits of the diagnostic builds: the block kernel is compiled without its chain there, and run-time compiled
modules carry no counters, so every cell runs with LZANI_RTC=0 and there is no block-kernel class."""
import json
import os
import subprocess
import sys

import pytest

import lzani_ctypes as L
import path_cover as PC

pytestmark = pytest.mark.gpu

CHILD_LIMIT = 240            # seconds: a child runs 24 cells of well under a second each, and their oracles
STRETCH = [("ps", 23)] + [("pw", k) for k in range(1, 10)]
CHAIN = ([("ps", k) for k in (1, 16, 17, 18, 19)] + [("st", k) for k in range(2, 6)] + [("sr", k) for k in range(4)] +
         [("sw", k) for k in (0, 2, 3, 4, 5, 6)])
# (class, slot) pairs that cannot occur by construction: (tuple or None = both, form or None = every form, slots, the reason)
CANNOT_OCCUR = (
    ("defaults", "bitmaps", STRETCH, "DevWave::HAS_STRETCH_CHAIN: a JOIN wave (candidate bitmaps) has the stretch chain from mal 13 on, the defaults have mal 11"),
    ("defaults", "join", STRETCH, "DevWave::HAS_STRETCH_CHAIN: a JOIN wave has the stretch chain from mal 13 on, the defaults have mal 11"),
    ("defaults", "split", STRETCH, "split_body's wave is a JOIN wave: HAS_STRETCH_CHAIN needs mal 13, the defaults have mal 11"),
    ("long", "probe", STRETCH + CHAIN, "pair_kernel_choice: the probe forms run the long tuple generic (defp 0), chain_of(0) = 0: neither hand-written "
                                       "loop is compiled (null_chain's st, sr, sw, LZ_PS(16..19); find_event's `pre` of LZ_PS(1) is CHAIN && pre_round)"),
    # Dead code: the exit needs msl + 64 equal symbols at the seed.  That is mal symbols or more, so the seed's step
    # is a candidate of the queue, which covers the round's steps, and the round's seed steps end at the queue head (LZ_NC_SEEDS):
    # the seed stands AT the head.  A lane resolves 32 symbols (AQ_LANE_CAP): equal throughout, the candidate is AQ_LONG (or
    # complex, or at position 0), never plain, and the test before this one (LZ_NC_WHY(1): blen < 1) has handed the round back.
    (None, None, [("sw", 4)], "null_chain: a seed of msl + 64 symbols stands at a queued candidate that is AQ_LONG, not plain: LZ_NC_WHY(1) leaves first"),
)


def cannot_occur(cls, s):
    for t, form, slots, why in CANNOT_OCCUR:
        if t in (None, cls[0]) and form in (None, cls[2]) and s in slots:
            return why
    return None


@pytest.fixture(scope="module")
def cover_lib():
    return L.build_diag_library()              # (built by __graft_entry__.build(); here only if it is missing or stale)


_LINES = {}


def child_lines(lib, tuple_name):
    """{cell id: the child's JSON line} of a tuple's cells, one child per tuple, run once."""
    if tuple_name not in _LINES:
        env = dict(os.environ, LZANI_LIB=lib, LZANI_RTC="0")
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.join(PC.HERE, "path_cover.py"), tuple_name]
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0, (tuple_name, p.returncode, p.stderr[-2000:])
        rows = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
        _LINES[tuple_name] = {r["cell"]: r for r in rows}
    return _LINES[tuple_name]


@pytest.mark.parametrize("tuple_name", PC.TUPLES)
def test_diagnostic_build_equals_the_oracle(cover_lib, tuple_name):
    lines = child_lines(cover_lib, tuple_name)
    want = [c for c in PC.cells() if c["prm"] == tuple_name]
    assert sorted(lines) == sorted(c["id"] for c in want)
    for c in want:
        r = lines[c["id"]]
        assert r["ok"], (c["id"], r["error"])
        assert set(r["kernels"]) == c["kernels"] and r["digest"], (c["id"], r["kernels"])
        assert r["paths"][0] > 0 and len(r["paths"]) == len(PC.PATH_SLOTS) and len(r["chain"]) == len(PC.CHAIN_SLOTS), c["id"]


@pytest.mark.parametrize("cls", PC.CLASSES, ids=[PC.class_name(c).replace(" ", "_") for c in PC.CLASSES])
def test_every_exit_is_reached(cover_lib, cls):
    lines = child_lines(cover_lib, cls[0])
    mine = [c["id"] for c in PC.cells() if c["class"] == cls]
    assert mine
    total = {"paths": [0] * len(PC.PATH_SLOTS), "chain": [0] * len(PC.CHAIN_SLOTS)}
    for ident in mine:
        for vec in total:
            total[vec] = [a + b for a, b in zip(total[vec], lines[ident][vec])]
    missing, dead_but_counted = [], []
    for s in PC.REQUIRED:
        vec, k, label = PC.slot(*s)
        why = cannot_occur(cls, s)
        print(PC.class_name(cls), label, total[vec][k], "(cannot occur)" if why else "")
        if why is None and total[vec][k] == 0:
            missing.append(label)
        if why is not None and total[vec][k] != 0:
            dead_but_counted.append((label, total[vec][k], why))
    assert not missing, "class '{}': no cell reaches {}; cells run: {}".format(PC.class_name(cls), missing, mine)
    assert not dead_but_counted, "class '{}': counted although listed as impossible: {}".format(PC.class_name(cls), dead_but_counted)
