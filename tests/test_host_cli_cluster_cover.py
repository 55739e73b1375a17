"""`lz-ani --cluster set-cover`: the cluster file of the host binary against tests/cluster_cover_model.py put over the pairs
that the run's own TSV lists (greedy set cover reads the graph alone -- no weight, so no rounded decimal, enters).
CPU half: through --results-in, which takes the host path (the sequential statement of lzani_cluster_plan.h); the
refusals.  GPU half: the device path (lzani_group_cluster_* behind the kept calls) and LZANI_OUT_FILTER=host write the
same bytes, those of the model."""
import os
import subprocess

import numpy as np
import pytest

import cluster_cover_model as CC
import util as U
from test_host_cli import _oracle_reordered, _raw_file
from test_host_cli_out_filter import CUTS, SETS

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
ENV = ("LZANI_OUT_FILTER", "LZANI_TILE_MIN", "LZANI_TILE_ROWS", "LZANI_DEVICE_LIST")


@pytest.fixture(scope="module", autouse=True)
def build_host():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])


def run(args, env=None, cwd=None):
    base = {k: v for k, v in os.environ.items() if k not in ENV}
    base.update(env or {})
    return subprocess.run([EXE] + args, capture_output=True, text=True, env=base, cwd=cwd)


def model_files(tsv, ids):
    """The cluster file by the model, with numbers and with representatives, from the TSV's pairs and the ids file's names;
    and the number of edges and of clusters."""
    names = [ln.split("\t")[0] for ln in open(ids).read().split("\n")[1:] if ln]
    rows = [ln.split("\t") for ln in open(tsv).read().split("\n") if ln]
    qi, ri = rows[0].index("qidx"), rows[0].index("ridx")
    edges = {(min(int(r[qi]), int(r[ri])), max(int(r[qi]), int(r[ri]))) for r in rows[1:]}
    rep = CC.cover(len(names), edges)
    cl, k = CC.number(rep)
    numbers = "object\tcluster\n" + "".join(f"{nm}\t{c}\n" for nm, c in zip(names, cl))
    reps = "object\trepresentative\n" + "".join(f"{nm}\t{names[r]}\n" for nm, r in zip(names, rep))
    return numbers, reps, len(edges), k


@pytest.mark.parametrize("cut", sorted(CUTS))
def test_cluster_file_through_results_in(tmp_path, cut):
    names, seqs, res = _oracle_reordered(U.load_example)
    n = len(names)
    raw = str(tmp_path / "raw.txt")
    _raw_file(raw, res)
    base = ["all2all"] + SETS["example"][0] + ["--results-in", raw] + CUTS[cut]
    plain = str(tmp_path / "plain.tsv")
    assert run(base + ["-o", plain]).returncode == 0
    numbers, reps, edges, k = model_files(plain, plain.replace(".tsv", ".ids.tsv"))
    assert 0 < edges < n * (n - 1) // 2 and 1 < k < n and numbers != reps, (edges, k)
    for tag, more, want in (("numbers", [], numbers), ("reps", ["--cluster-representatives"], reps),
                            ("gani", ["--cluster-measure", "gani"], numbers), ("ani", ["--cluster-measure", "ani"], numbers)):   # the measure: accepted, no effect
        out, cf = str(tmp_path / f"{tag}.tsv"), str(tmp_path / f"{tag}.clusters")
        p = run(base + ["-o", out, "-V", "2", "--cluster", "set-cover", "--cluster-out", cf] + more)
        assert p.returncode == 0, p.stderr[-1500:]
        assert open(cf).read() == want, tag
        assert f"clusters on the host: {k} of {n} sequences from {edges} pairs" in p.stderr, p.stderr[-600:]
        # the TSV and the ids file are those of the run without --cluster
        assert open(out, "rb").read() == open(plain, "rb").read()
        assert open(out.replace(".tsv", ".ids.tsv"), "rb").read() == open(plain.replace(".tsv", ".ids.tsv"), "rb").read()


def test_refusals_and_usage(tmp_path):
    fa = SETS["example"][0]
    raw = tmp_path / "raw.txt"
    raw.write_text("")
    common = ["-o", str(tmp_path / "o.tsv"), "--results-in", str(raw), "--cluster-out", str(tmp_path / "c.tsv")] + CUTS["ani_qcov"]
    for value in ("complete", "leiden", "set_cover", "3"):
        p = run(["all2all"] + fa + ["--cluster", value] + common)
        assert p.returncode == 1 and f"Unknown value for --cluster: {value}" in p.stderr and "set-cover" in p.stderr, p.stderr[-600:]
        assert not os.path.exists(str(tmp_path / "c.tsv"))
    p = run(["all2all"] + fa + ["--cluster", "set-cover", "--cluster-out", str(tmp_path / "c.tsv"), "-o", str(tmp_path / "o.tsv"), "--results-in", str(raw)])
    assert p.returncode == 1 and "--out-filter" in p.stderr                      # set cover needs the output filter like the others
    assert "set-cover" in run([]).stderr                                        # the usage text


# ---- GPU half ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("cut", sorted(CUTS))
def test_device_and_host_paths_write_the_models_file(tmp_path, cut):
    args, n, _ = SETS["example"]
    files = {}
    for reps in (False, True):
        for tag, env, line in (("device", dict(LZANI_TILE_ROWS="0"), "clusters on the device: "),
                               ("host", dict(LZANI_TILE_ROWS="0", LZANI_OUT_FILTER="host"), "clusters on the host: ")):
            d = tmp_path / f"{tag}{int(reps)}"
            d.mkdir()
            p = run(["all2all"] + args + CUTS[cut] + ["-o", "o.tsv", "-V", "2", "--cluster", "set-cover", "--cluster-out", "c.tsv"]
                    + (["--cluster-representatives"] if reps else []), env, cwd=str(d))
            assert p.returncode == 0, p.stderr[-1500:]
            assert line in p.stderr, p.stderr[-1500:]
            numbers, names, edges, k = model_files(str(d / "o.tsv"), str(d / "o.ids.tsv"))
            assert 0 < edges and 1 < k < n
            if tag == "device":
                assert f"clusters on the device: {k} of {n} sequences" in p.stderr and f"from {edges} pairs" in p.stderr, p.stderr[-1500:]
                assert f"set cover: {edges} distinct pairs (0 given again)" in p.stderr, p.stderr[-1500:]
            files[(tag, reps)] = ((d / "c.tsv").read_bytes(), (d / "o.tsv").read_bytes())
            assert files[(tag, reps)][0].decode() == (names if reps else numbers), (tag, reps)
        assert files[("device", reps)] == files[("host", reps)]
