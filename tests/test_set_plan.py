"""CPU: the pure layout decisions of a genome set (lz-ani_amd/csrc/lzani_set_plan.h: SetKnobs, set_layout_of, the genome
footprints, plan_blocks_impl, auto_genome_limit, slab_slot_count) in a stand-alone host program under the address and
undefined-behaviour sanitizers, and the layouts, footprints and block plans it prints for a fixed grid against the rules as
tests/util.py and tests/ooc_model.py state them."""
import os
import subprocess

import numpy as np
import pytest

import ooc_model as OM
import util as U

KEYS = ("mal", "msl", "mrd", "mqd", "reg", "aw", "am", "ar")
SWITCHES = {"LZANI_BK_MAX_DIRBITS": "11", "LZANI_NO_BUCKETS": "1", "LZANI_NO_TAGWORDS": "1", "LZANI_JOIN_MIN_BYTES": "12345",
            "LZANI_NO_JOIN": "1", "LZANI_SORT_INDEX_MIN_DIRBITS": "7", "LZANI_NO_SORT_INDEX": "1", "LZANI_FILTER_MAX_BITS": "13",
            "LZANI_NO_FILTER": "1", "LZANI_MAX_SLOTS": "5", "LZANI_FREE_BYTES": "99999999999"}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    src = os.path.join(U.ROOT, "tests", "model", "set_plan_check.cpp")
    out = str(tmp_path_factory.mktemp("set_plan") / "set_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",      # (the runtime in the program: it runs beside any preloaded library)
                           src, "-o", out])
    return out


def _run(exe, args=(), switches=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("LZANI_")}
    env.update(switches or {})
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return r.stdout.splitlines()


def test_the_set_plan_under_the_sanitizers_and_its_grid_against_the_python_statements(exe):
    lines = _run(exe)
    layouts, joins, filters, sorts, slot_cases, block_cases, refused, several, res_cases, in_core = (int(x) for x in lines[-1].split())
    assert layouts == 6 * 9 * 7 and joins and filters and sorts and slot_cases >= 20000 and block_cases >= 4000
    assert refused > 100 and several > 100 and res_cases >= 4000 and 100 < in_core < res_cases - 100
    grid = [[int(x) for x in l.split()[1:]] for l in lines if l.startswith("grid ")]
    blocks = [l.split()[1:] for l in lines if l.startswith("blocks ")]
    assert len(grid) == 6 * 9 * 3 and len(blocks) == 2 * 3 * 7 and len(grid) + len(blocks) == len(lines) - 1
    seen = set()
    for Lmax, n, *rest in grid:
        prm = dict(zip(KEYS, rest[:8]))
        kb, dirbits, posbits, bk, tw, fl, fmask, join, sort_build, max_slots, footprint = rest[8:]
        lens = [Lmax] * n
        want_join = OM.join_lists(lens, prm)
        f = U.index_form([range(Lmax)], prm, join=want_join)
        case = (Lmax, n, prm)
        assert (kb, dirbits, posbits) == (f["key_bits"], f["dir_bits"], f["pos_bits"]), case
        assert bk == (4 << dirbits if f["bucket_table"] else 0) and tw == (1 << dirbits if f["tag_words"] else 0), case
        assert bool(join) == want_join, case
        assert fl == ((1 << f["filter_bits"]) // 32 if f["filter_bits"] else 0) and fmask == f["filter_mask"], case
        assert bool(sort_build) == f["sort_build"] and max_slots == f["max_slots"], case
        assert footprint == OM.genome_bytes(Lmax, prm, want_join), case
        seen.add((bool(bk), bool(tw), bool(join), bool(fl), bool(sort_build), max_slots < 65535))
    # every decision both ways on the grid
    assert all({s[i] for s in seen} == {False, True} for i in range(6)), seen
    outcomes = set()
    for b in blocks:
        prm = dict(zip(KEYS, map(int, b[:8])))
        limit, n = int(b[8]), int(b[9])
        lens, got = [int(x) for x in b[10:10 + n]], b[11 + n:]
        assert b[10 + n] == ":"
        want = OM.plan_blocks(lens, prm, limit)
        if want is None:
            assert got == ["refused"], (prm, limit, lens)
        else:
            assert np.array_equal(np.array(got, np.uint32), want), (prm, limit, lens, got)
        outcomes.add("refused" if want is None else min(int(want.max()) + 1, 3))
    assert outcomes == {"refused", 1, 2, 3}


def test_set_knobs_reads_each_switch_into_its_own_field(exe):
    assert _run(exe, ["knobs"]) == ["knobs 26 1 1 8388608 1 20 1 18 1 0 -1"]
    assert _run(exe, ["knobs"], SWITCHES) == ["knobs 11 0 0 12345 0 7 0 13 0 5 99999999999"]
    for name, value in SWITCHES.items():          # one at a time: no switch reaches a second field
        want = "knobs 26 1 1 8388608 1 20 1 18 1 0 -1".split()
        at = 1 + list(SWITCHES).index(name)
        want[at] = value if not name.startswith("LZANI_NO_") else "0"
        assert _run(exe, ["knobs"], {name: value}) == [" ".join(want)], name
