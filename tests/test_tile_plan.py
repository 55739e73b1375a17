"""CPU: the decisions of an out-of-core run (lz-ani_amd/csrc/lzani_tile_plan.h: the step list, the local tables of a
reference block's tiles, the local genome table, the upload tables) in a stand-alone host program under the address and
undefined-behaviour sanitizers -- it checks the tables itself -- and the step list it prints for every case against the
schedule as tests/ooc_model.py states it."""
import os
import subprocess

import numpy as np
import pytest

import lzani_ctypes as L
import ooc_model as M
import util as U

WHAT = ("keep", "trade", "upload")            # TileA


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    src = os.path.join(U.ROOT, "tests", "model", "tile_plan_check.cpp")
    out = str(tmp_path_factory.mktemp("tile_plan") / "tile_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",      # (the runtime in the program: it runs beside any preloaded library)
                           src, "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return r.stdout.splitlines()


def _state(a, b):
    return (None if a < 0 else a, None if b < 0 else b)


def _cases(lines):
    """The printed cases: (block_of, state, ref, off, q or None, [(i, what, [(j, up), ...]), ...], state after, tiles, uploads)."""
    at = 0
    while lines[at].startswith("case "):
        head = [int(x) for x in lines[at].split()[1:]]
        n, nb = head[:2]
        first, (sa, sb, dense, n_rows) = head[2:3 + nb], head[3 + nb:]
        ref, off, q = ([int(x) for x in lines[at + k].split()[1:]] for k in (1, 2, 3))
        assert (lines[at + 1].split()[0], lines[at + 2].split()[0], lines[at + 3].split()[0]) == ("ref", "off", "q")
        assert first[0] == 0 and first[-1] == n and len(ref) == n_rows and len(off) == n_rows + 1
        at += 4
        steps = []
        while lines[at].startswith("step "):
            v = [int(x) for x in lines[at].split()[1:]]
            steps.append((v[0], WHAT[v[1]], [(j, bool(up)) for j, up in zip(v[2::2], v[3::2])]))
            at += 1
        after = [int(x) for x in lines[at].split()[1:]]
        assert lines[at].startswith("after ")
        at += 1
        block_of = np.repeat(np.arange(nb), np.diff(first)).astype(np.uint32)
        yield (block_of, _state(sa, sb), np.array(ref, np.uint32), np.array(off, np.uint64), None if dense else np.array(q, np.uint32),
               steps, _state(*after[:2]), after[2], after[3])
    assert at == len(lines) - 1


def test_the_tile_plan_under_the_sanitizers_and_its_steps_against_the_python_schedule(lines):
    tot = dict(cases=0, keep=0, trade=0, upload=0, b_holds=0, self_tiles=0, skipped=0, dense_single=0)
    forms, carried = set(), 0
    for block_of, state, ref, off, q, steps, after, tiles, uploads in _cases(lines):
        case = (tot["cases"], block_of.tolist(), state)
        want, want_after = M.steps(block_of, ref, off, q, state)
        assert len(steps) == len(want), case
        for got_step, want_step in zip(steps, want):
            assert got_step == want_step, (case, got_step, want_step)
        assert after == want_after, case
        assert (tiles, uploads, after) == M.schedule(block_of, ref, off, q, state), case
        # what the case set must show, by the model alone
        size = np.bincount(block_of)
        nb = len(size)
        assert 2 <= nb <= 7 and len(block_of) <= 24 and len(ref) <= 40
        tot["cases"] += 1
        for i, what, qs in want:
            tot[what] += 1
            tot["b_holds"] += sum(j != i and not up for j, up in qs)
            tot["self_tiles"] += sum(j == i for j, _ in qs)
        tot["skipped"] += nb - len(want)
        if q is None:
            tot["dense_single"] += int(sum(size[block_of[r]] == 1 for r in ref))
            forms.add("dense all" if len(ref) == len(block_of) and sorted(ref) == list(range(len(ref))) else "dense subset")
        else:
            inside = all(block_of[x] == block_of[r] for k, r in enumerate(ref) for x in q[int(off[k]):int(off[k + 1])])
            forms.add("inside" if inside else "ragged")
        carried += state != (None, None)
    assert [int(x) for x in lines[-1].split()] == list(tot.values()), (lines[-1], tot)
    assert tot["cases"] >= 3000 and all(v > 0 for v in tot.values()), tot
    assert forms == {"dense all", "dense subset", "ragged", "inside"} and 0 < carried < tot["cases"]


def test_the_hand_worked_schedule():
    """4 blocks of a dense all2all -- 16 tiles, 4 + 3 + 2 + 2 uploads, state (3, 1) -- as steps."""
    bo = np.repeat(np.arange(4), 3).astype(np.uint32)
    ref, off = L.dense_rows(12)
    steps, state = M.steps(bo, ref, off, None)
    assert steps == [(0, "upload", [(0, False), (1, True), (2, True), (3, True)]),
                     (1, "upload", [(1, False), (3, False), (0, True), (2, True)]),
                     (2, "trade", [(2, False), (1, False), (0, True), (3, True)]),
                     (3, "trade", [(3, False), (2, False), (0, True), (1, True)])] and state == (3, 1)
    assert M.schedule(bo, ref, off, None) == (16, 11, (3, 1))
