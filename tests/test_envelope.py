"""CPU: the LZ parameter envelope at its edges (U.EDGE_TUPLES): the oracle against the reference build's stored answers,
every host model of the kernel formulation against the oracle, and the refusal edge of params_supported through the model
and the host binary.  tests/test_gpu_envelope.py runs the same tuples through every form of the device path."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import synth_genomes as SG
import util as U

GOLDEN = os.path.join(U.GOLD, "ref_envelope_vectors.json")
EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
SETS = {"edge": U.edge_set, "family": U.envelope_family_set}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def sets():
    return {k: f() for k, f in SETS.items()}


def test_edge_table_rows():
    """The table holds the rows the envelope tests are written for, keeps mqd <= mrd everywhere, stays inside
    params_supported, and the restated predicates put the rows where their comments say."""
    T = U.EDGE_TUPLES
    want = {("mqd", "mrd"): [(0, 0), (0, 64), (24, 40), (63, 64), (63, 65), (64, 64), (64, 1000)],
            ("aw", "am", "ar"): [(1, 0, 0), (2, 0, 2), (2, 1, 0), (15, 15, 15), (15, 20, 0), (16, 7, 3), (64, 64, 64), (64, 64, -3)],
            ("mal", "msl"): [(1, 1), (15, 1), (9, 9), (7, 9), (15, 8), (15, 15), (16, 16), (31, 11), (32, 7), (32, 11), (32, 32)],
            ("reg",): [(-1,), (0,), (1,)]}
    for keys, rows in want.items():
        have = {tuple(p[k] for k in keys) for p in T.values()}
        assert set(rows) <= have, (keys, set(rows) - have)
    for name, p in T.items():
        assert p["mqd"] <= p["mrd"] and U.params_supported(p), name
        changed = {k for k in p if p[k] != U.DEFAULTS[k]}
        assert changed and any(changed <= set(g[next(iter(g))]) for g in U.EDGE_GROUPS.values()), name
    L = max(len(s) for f in SETS.values() for s in f())
    assert any(p["reg"] > L for p in T.values())                      # one region length beyond every genome
    assert len(T) == sum(len(g) for g in U.EDGE_GROUPS.values())      # (no name twice)
    inside = {"mqd0_mrd64", "mqd24_mrd40", "mqd62_mrd65", "aw2_am0_ar2", "aw2_am1_ar0", "aw15_am15_ar15", "aw15_am20_ar0",
              "mal1_msl1", "mal15_msl1", "mal9_msl9", "mal7_msl9", "mal15_msl8", "reg0", "reg1", "reg100000"}
    assert {n for n, p in T.items() if U.chain_params_ok(p)} == inside
    assert not any(U.is_aot(p) for p in T.values()) and all(U.is_aot(p) for p in U.AOT_SETS.values())
    assert {n for n, p in T.items() if not U.is_fast(p)} == {"mal16_msl16", "mal31_msl11", "mal32_msl7", "mal32_msl11", "mal32_msl32"}
    assert U.chain_params_ok(U.AOT_SETS["defaults"]) and U.chain_params_ok(U.AOT_SETS["long"])


def test_golden_file_covers_the_reference_rows(golden):
    names = [n for n, p in U.EDGE_TUPLES.items() if p["msl"] <= U.REF_MAX_MSL]
    assert sorted(golden["params"]) == sorted(names) and len(names) >= 25
    for name in names:
        assert golden["params"][name] == U.EDGE_TUPLES[name], name
    assert os.path.getsize(GOLDEN) < 256 * 1024


@pytest.mark.parametrize("name", [n for n, p in U.EDGE_TUPLES.items() if p["msl"] <= U.REF_MAX_MSL])
def test_oracle_equals_reference_at_the_edges(golden, sets, name):
    """The oracle against the reference build's answers stored in tests/golden/ref_envelope_vectors.json, and live
    against oracle/_ref where it has been built."""
    prm = U.EDGE_TUPLES[name]
    for k, seqs in sets.items():
        got = O.oracle_all2all(seqs, prm, threads=8)
        want = np.array(golden["res"][k][name], dtype=np.int32)
        bad = np.argwhere((got != want).any(axis=2))
        assert len(bad) == 0, (name, k, bad[:3].tolist())
        if O.lib_ref() is not None:
            assert np.array_equal(O.ref_all2all(seqs, prm, threads=8), got), (name, k, "live")


def _lane(seqs, prm, words):
    lib = U.model_lib()
    s, ptrs, lens = O._seq_table(seqs)
    out = np.zeros((len(s), len(s), 3), dtype=np.int32)
    assert lib.model_lane_all2all(len(s), ptrs, O._ptr(lens), O.params_array(prm), words, O._ptr(out)) == 0
    return out


def _queue(seqs, prm):
    lib = U.model_lib()
    s, ptrs, lens = O._seq_table(seqs)
    out = np.zeros((len(s), len(s), 3), dtype=np.int32)
    rc = lib.model_queue_all2all(len(s), ptrs, O._ptr(lens), O.params_array(prm), O._ptr(out))
    return out if rc == 0 else None


def _diff(got, want):
    bad = np.argwhere((got != want).any(axis=2))
    return f"{len(bad)} pairs differ, first {bad[:3].tolist()}" + (f": {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}" if len(bad) else "")


@pytest.mark.parametrize("name", list(U.EDGE_TUPLES))
def test_models_equal_oracle_at_the_edges(sets, name):
    """Every host model of the kernel formulation (lzani_core.h) against the oracle: the lane-emulating model, the
    lane-serial policy with and without word tricks, the anchor queue where it applies (k-mer words and exact tags),
    the split into segments at two segment lengths, and the region stream on pairs of both sets."""
    prm = U.EDGE_TUPLES[name]
    for k, seqs in sets.items():
        want = O.oracle_all2all(seqs, prm, threads=8)
        assert (got := U.model_all2all(seqs, prm)).tobytes() == want.tobytes(), (name, k, "model", _diff(got, want))
        for words in (0, 1):
            assert (got := _lane(seqs, prm, words)).tobytes() == want.tobytes(), (name, k, "lane", words, _diff(got, want))
        got = _queue(seqs, prm)
        form = U.index_form(seqs, prm)
        assert (got is not None) == (U.is_fast(prm) and form["exact"]), (name, k, "queue model applies")
        if got is not None:
            assert got.tobytes() == want.tobytes(), (name, k, "queue", _diff(got, want))
        for seglen in (150, 1100):
            got, _ = U.model_split_all2all(seqs, prm, seglen)
            assert got.tobytes() == want.tobytes(), (name, k, "split", seglen, _diff(got, want))
        n = len(seqs)
        for r, q in [(0, 1), (1, 0), (0, 2), (3, n - 1), (n - 2, 4), (2, 5)]:
            res, regs = U.model_pair_regions(seqs[r], seqs[q], prm)
            ores, oregs = O.oracle_pair(seqs[r], seqs[q], prm, want_regions=True)
            assert res == ores and np.array_equal(regs, oregs), (name, k, "regions", r, q)
            assert res == tuple(want[r, q]), (name, k, r, q)


def test_models_equal_oracle_on_edge_draws():
    """Random combinations of the edge rows (U.edge_params) on small random genomes: the model and the lane-serial policy
    against the oracle, the oracle against oracle/_ref where it has been built and can run the tuple."""
    st = SG.Stream(3232)
    ref = 0
    for it in range(60):
        prm = U.edge_params(st)
        _, seqs = U.fuzz_case(st)
        want = O.oracle_all2all(seqs, prm, threads=4)
        assert np.array_equal(U.model_all2all(seqs, prm), want), (it, prm)
        assert np.array_equal(_lane(seqs, prm, it & 1), want), (it, prm)
        got, _ = U.model_split_all2all(seqs, prm, 64 + 37 * (it % 7))
        assert np.array_equal(got, want), (it, prm, "split")
        if O.lib_ref() is not None and prm["msl"] <= U.REF_MAX_MSL:
            assert np.array_equal(O.ref_all2all(seqs, prm, threads=4), want), (it, prm)
            ref += 1
    assert O.lib_ref() is None or ref >= 30


BOUNDS = U.ENVELOPE_BOUNDS


def test_refusal_edge_through_the_model():
    """One step inside every bound the model runs (and equals the oracle), one step outside it refuses with the C-ABI's
    rule -- and the Python restatement of params_supported says the same."""
    seqs = [U.edge_set()[0][:300], U.edge_set()[2][:200], U.edge_set()[3][1450:1650]]
    for knob, ok, bad in BOUNDS:
        inside, outside = U.bound_pair(knob, ok, bad)
        assert U.params_supported(inside), (knob, ok)
        assert np.array_equal(U.model_all2all(seqs, inside), O.oracle_all2all(seqs, inside, threads=4)), (knob, ok)
        assert not U.params_supported(outside), (knob, bad)
        for f in (U.model_all2all, lambda s, p: U.model_split_all2all(s, p, 500), lambda s, p: U.model_pair_regions(s[0], s[1], p)):
            with pytest.raises(ValueError):
                f(seqs, outside)
    # no bound below ar, none above am or reg
    for extra in (dict(ar=-1000), dict(am=1000), dict(reg=1 << 30), dict(reg=-(1 << 30))):
        assert U.params_supported(extra)
        assert np.array_equal(U.model_all2all(seqs, extra), O.oracle_all2all(seqs, extra, threads=4)), extra


def test_refusal_edge_through_the_c_abi_needs_no_device():
    """lzani_create refuses a tuple outside params_supported with LZANI_ERR_PARAMS before it looks for a device (the
    inside half of the edge, which needs one, is in tests/test_gpu_envelope.py)."""
    import lzani_ctypes as L
    for knob, ok, bad in BOUNDS:
        _, outside = U.bound_pair(knob, ok, bad)
        with pytest.raises(L.LzaniError, match="LZANI_ERR_PARAMS"):
            L.Engine(outside)


def test_refusal_edge_through_the_host_binary(tmp_path):
    """The host binary's envelope (host/cli.h) at the same bounds: one step outside is "Unsupported value" and exit 1
    before any input is read, one step inside goes on to the input (here: a missing file)."""
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])
    flags = {"msl": "--msl", "mal": "--mal", "mrd": "--mrd", "mqd": "--mqd", "aw": "--aw", "ar": "--ar", "am": "--am"}

    def run(knob, val):
        return subprocess.run([EXE, "all2all", "--in-fasta", str(tmp_path / "does_not_exist.fna"), "-o", str(tmp_path / "o.tsv"),
                               flags[knob], str(val)], capture_output=True, text=True)
    for knob, ok, bad in BOUNDS:
        p = run(knob, bad)
        assert p.returncode == 1 and f"Unsupported value: {flags[knob]} {bad}" in p.stderr, (knob, bad, p.stderr)
        p = run(knob, ok)
        assert p.returncode == 1 and "Unsupported" not in p.stderr and "Cannot open file" in p.stderr, (knob, ok, p.stderr)
