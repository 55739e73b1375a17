"""CPU: the walk of tests/test_gpu_context_walk.py (tests/context_walk.py) is what it says.

Every tuple's circuit crosses each ordered pair of its nodes exactly once; the segments join end to start within their cap;
SET_ENV and RUN_ENV are the switches the library reads at lzani_set_genomes and at a run, by its source text; and the kinds of
edge the walk exists for -- another form on the same upload, N-free and N sets, longer and shorter texts, another set layout
of the same genomes, in-core and out-of-core, run-time compiled and ahead of time -- are among the edges."""
import os
import re

import pytest

import context_walk as W
import ooc_model as M
import util as U

CSRC = os.path.join(U.ROOT, "lz-ani_amd", "csrc")
ENV_RE = re.compile(r'env_(?:int|u64|is|flag)\("(LZANI_\w+)"')
GETENV_RE = re.compile(r'getenv\("(LZANI_\w+)"')
NODE_COUNTS = {"defaults": 15, "generic": 13, "long": 6, "slow": 2, "rtc_chain": 12, "rtc_plain": 12}


def _edges(prm):
    return [(a, b) for seg in W.segments(prm) for a, b in zip(seg, seg[1:])]


def _kinds(prm):
    out = set()
    for a, b in _edges(prm):
        out |= W.edge_kinds(a, b)
    return out


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_node_counts():
    assert set(NODE_COUNTS) == set(U.INST_PARAMS)
    cells = {prm: sum(c["prm"] == prm for c in U.INST_CELLS) for prm in U.INST_PARAMS}
    assert cells == {"defaults": 13, "generic": 13, "long": 6, "slow": 2, "rtc_chain": 6, "rtc_plain": 6}
    assert {prm: len(W.nodes(prm)) for prm in U.INST_PARAMS} == NODE_COUNTS
    assert sum(k * k for k in NODE_COUNTS.values()) == 169 + 36 + 4 + 144 + 144 + 225 == 722
    for prm in U.INST_PARAMS:
        ids = [x["id"] for x in W.nodes(prm)]
        assert ids == sorted(ids) and len(set(ids)) == len(ids)
        assert all(x["prm"] == prm for x in W.nodes(prm))


@pytest.mark.parametrize("prm", list(U.INST_PARAMS))
def test_circuit_crosses_every_ordered_pair_once(prm):
    ns, w = W.nodes(prm), W.walk(prm)
    k = len(ns)
    assert len(w) == k * k + 1 and w[0] is w[-1]
    pairs = [(a["id"], b["id"]) for a, b in zip(w, w[1:])]
    assert len(set(pairs)) == k * k == len(pairs)
    assert set(pairs) == {(a["id"], b["id"]) for a in ns for b in ns}
    assert W.walk(prm) == w                                                       # deterministic


@pytest.mark.parametrize("prm", list(U.INST_PARAMS))
def test_segments_join_end_to_start_within_the_cap(prm):
    segs, w = W.segments(prm), W.walk(prm)
    cap = W.CAP_OF.get(prm, W.CAP)
    assert 1 <= cap <= W.CAP == 48
    assert all(2 <= len(s) <= cap + 1 for s in segs)
    assert segs[0][0] is w[0] and segs[-1][-1] is w[-1]
    assert all(a[-1] is b[0] for a, b in zip(segs, segs[1:]))
    pairs = [(a["id"], b["id"]) for a, b in _edges(prm)]                          # no edge lost or doubled by the cuts
    assert pairs == [(a["id"], b["id"]) for a, b in zip(w, w[1:])]
    assert (prm, len(segs) - 1) in W.segment_ids() and (prm, len(segs)) not in W.segment_ids()


def test_all_722_ordered_pairs_are_in_the_segments():
    assert sum(len(_edges(prm)) for prm in U.INST_PARAMS) == 722
    assert len(W.segment_ids()) == sum(len(W.segments(prm)) for prm in U.INST_PARAMS)


def test_switch_lists_equal_the_source():
    set_plan, hip, rtc = _text("lzani_set_plan.h"), _text("lzani_hip.hip"), _text("lzani_rtc.h")
    assert set(W.SET_ENV) == set(ENV_RE.findall(set_plan)) and len(set(W.SET_ENV)) == len(W.SET_ENV)
    assert not GETENV_RE.findall(set_plan)
    knobs = hip[hip.index("struct Knobs {"):]
    knobs = knobs[:knobs.index("};")]
    run_knobs = set(ENV_RE.findall(knobs))
    assert len(run_knobs) >= 18 and run_knobs == set(ENV_RE.findall(hip))          # lzani_hip.hip reads switches nowhere else
    rtc_env = set(GETENV_RE.findall(rtc))
    assert rtc_env == {"LZANI_RTC", "LZANI_RTC_CACHE"}
    assert set(W.RUN_ENV) == run_knobs | rtc_env and len(set(W.RUN_ENV)) == len(W.RUN_ENV)
    assert not set(W.SET_ENV) & set(W.RUN_ENV)
    # what the run path reads besides: LZANI_TRACE (a log), and the stage headers' own switches (none of a pair run)
    assert set(GETENV_RE.findall(hip)) == {"LZANI_TRACE"}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".h", ".hip")) and name not in ("lzani_set_plan.h", "lzani_hip.hip", "lzani_rtc.h"):
            others = set(ENV_RE.findall(_text(name))) | set(GETENV_RE.findall(_text(name)))
            assert all(x.startswith("LZANI_PREFILTER_") for x in others), (name, others)


def test_every_switch_of_a_node_is_in_exactly_one_list():
    for prm in U.INST_PARAMS:
        for x in W.nodes(prm):
            for k in x["env"]:
                assert (k in W.SET_ENV) + (k in W.RUN_ENV) == 1, (x["id"], k)
    import inst_cell
    assert set(inst_cell.FORM_ENV) <= set(W.SET_ENV) | set(W.RUN_ENV)


def test_twins_and_out_of_core_nodes():
    for prm in W.RTC_TUPLES:
        ns = {x["id"]: x for x in W.nodes(prm)}
        twins = [x for x in ns.values() if "twin_of" in x]
        assert len(twins) == 6
        for t in twins:
            c = ns[t["twin_of"]]
            assert c["name"].startswith("rtc ") and t["env"]["LZANI_RTC"] == "0" and W.set_key(t) == W.set_key(c)
            assert len(t["kernels"]) == 1 and t["kernels"] != c["kernels"]
            (name,) = t["kernels"]
            cand = c["name"][-1]
            assert name == U.PAIRS_NAME.format(1, int("nfree=1" in c["name"]), 0, 0, 1, cand), (t["id"], name)
    ooc = [x for x in W.nodes("defaults") if x["limit"]]
    assert [(x["set"], x["form"], x["blocks"]) for x in ooc] == [("small", "lists", 2), ("small N", "all2all", 3)]
    for x in ooc:
        lens = [len(s) for s in U.instantiation_set(x["set"])]
        prm = U.INST_PARAMS["defaults"]
        assert int(M.plan_blocks(lens, prm, x["limit"]).max()) + 1 == x["blocks"] and x["kernels"] is None
        bo = M.plan_blocks(lens, prm, x["limit"] - 2)                        # the smallest such limit (limits count in halves)
        assert bo is None or int(bo.max()) + 1 > x["blocks"]
        assert not M.join_lists(lens, prm)
    assert all(x["limit"] == 0 and x["blocks"] == 1 for p in U.INST_PARAMS for x in W.nodes(p) if x["kernels"] is not None)


COMMON = {"form change on one upload", "N-free -> N", "N -> N-free"}
LENGTHS = {"longest text grows", "longest text shrinks"}


def test_edge_kinds_of_every_tuple_with_more_than_one_set():
    """Of the layout flips on the same genomes a tuple crosses those its cells hold: the join in every tuple but the long one
    (its join cells are alone on the 'long' sets, the others on the 'split' sets: stated below, so that a cell added there is
    noticed), tag words and bucket table off and on where cells set LZANI_NO_TAGWORDS / LZANI_NO_BUCKETS (defaults, generic).
    The longest text changes in every tuple but rtc_plain, whose two sets, 'small' and 'small N', are as long as each other."""
    many = [prm for prm in U.INST_PARAMS if len({x["set"] for x in W.nodes(prm)}) > 1]
    assert many == ["defaults", "long", "generic", "rtc_chain", "rtc_plain"]
    for prm in many:
        kinds = _kinds(prm)
        assert COMMON <= kinds, (prm, COMMON - kinds)
        if prm != "rtc_plain":
            assert LENGTHS <= kinds, (prm, LENGTHS - kinds)
        if prm != "long":
            assert {"join on", "join off"} <= kinds, (prm, kinds)
        if prm in ("defaults", "generic"):
            assert {"index tables off", "index tables on"} <= kinds, (prm, kinds)
    by_set = {}
    for x in W.nodes("long"):
        by_set.setdefault(x["set"], set()).add(tuple(sorted(W.layout_of(x).items())))
    assert all(len(v) == 1 for v in by_set.values()), by_set
    assert {x["set"] for x in W.nodes("rtc_plain")} == {"small", "small N"} and not LENGTHS & _kinds("rtc_plain")
    assert _kinds("slow") == {"form change on one upload"}


def test_in_core_out_of_core_and_rtc_twin_edges():
    assert {"in-core -> out-of-core", "out-of-core -> in-core"} <= _kinds("defaults")
    for prm in W.RTC_TUPLES:
        assert {"rtc -> twin", "twin -> rtc"} <= _kinds(prm), prm
        # ... and rtc -> ahead of time -> rtc with nothing between: the twin edge, then the edge back, somewhere in a row
        ids = [[x["id"] for x in seg] for seg in W.segments(prm)]
        assert any(s[i] == s[i + 2] and s[i + 1] == s[i] + "_aot" for s in ids for i in range(len(s) - 2)), prm


def test_layout_of_agrees_with_predict_kernels():
    """layout_of restates the first lines of util.predict_kernels; the kernel names say the same: cand=1 where the join is
    on, bk=1 where the tag words are."""
    for prm in U.INST_PARAMS:
        for x in W.nodes(prm):
            if x["kernels"] is None or x["form"] == "regions":
                continue
            f = W.layout_of(x)
            for name in x["kernels"]:
                if name.startswith("pairs "):
                    assert ("cand=1" in name) == (f["join"] and "cand=2" not in name), (x["id"], name, f)
                    if "fast=1" in name and "cand=0" in name:
                        assert ("bk=1" in name) == f["tw"], (x["id"], name, f)
