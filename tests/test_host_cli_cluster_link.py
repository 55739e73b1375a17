"""`lz-ani --cluster complete-linkage`: the cluster file of the host binary against tests/cluster_link_model.py put over the
raw integers of the matching stage (never over the printed TSV: its decimals are rounded, and the order of the weights
would turn on the rounding).  CPU half: through --results-in, which takes the host path (the sequential statement of
lzani_cluster_plan.h), for the three measures; the refusals; the usage text.  GPU half: the device path
(lzani_group_cluster_* behind the kept calls), LZANI_OUT_FILTER=host and --results-in write the same bytes, those of the
model over a --results-out run's integers."""
import os
import subprocess

import numpy as np
import pytest

import cluster_link_model as LM
import cluster_model as CM
import out_filter_model as M
import util as U
from test_host_cli import _oracle_reordered, _raw_file
from test_host_cli_cluster import minima, raw_integers
from test_host_cli_out_filter import CUTS, SETS

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
ENV = ("LZANI_OUT_FILTER", "LZANI_TILE_MIN", "LZANI_TILE_ROWS", "LZANI_DEVICE_LIST")
ALGO = "complete-linkage"


@pytest.fixture(scope="module", autouse=True)
def build_host():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])


def run(args, env=None, cwd=None):
    base = {k: v for k, v in os.environ.items() if k not in ENV}
    base.update(env or {})
    return subprocess.run([EXE] + args, capture_output=True, text=True, env=base, cwd=cwd)


def model_files(names, lens, res, cut, measure):
    """The cluster file by the model, with numbers and with representatives: res[r, q] = the raw result of (ref r, query q),
    ids in the order of the ids file; and the number of edges, of clusters, and the largest cluster."""
    n = len(names)
    a, b = np.triu_indices(n, 1)
    lens = np.asarray(lens, dtype=np.uint32)
    x, y = res[a, b], res[b, a]
    ln = M.lines(minima(cut), x, y, lens[a], lens[b])
    keep = ln != 0
    w = CM.weight(measure, x[keep], y[keep], ln[keep], lens[a][keep], lens[b][keep])
    rep = LM.linkage(n, LM.edge_min(a[keep], b[keep], w))
    cl, k = LM.number(rep)
    numbers = "object\tcluster\n" + "".join(f"{nm}\t{c}\n" for nm, c in zip(names, cl))
    reps = "object\trepresentative\n" + "".join(f"{nm}\t{names[r]}\n" for nm, r in zip(names, rep))
    return numbers, reps, int(keep.sum()), k, int(np.bincount(rep).max())


@pytest.fixture(scope="module")
def example():
    names, seqs, res = _oracle_reordered(U.load_example)
    return names, [len(s) for s in seqs], res


@pytest.mark.parametrize("cut", sorted(CUTS))
def test_cluster_file_through_results_in(tmp_path, example, cut):
    names, lens, res = example
    n = len(names)
    raw = str(tmp_path / "raw.txt")
    _raw_file(raw, res)
    base = ["all2all"] + SETS["example"][0] + ["--results-in", raw] + CUTS[cut]
    plain = str(tmp_path / "plain.tsv")
    assert run(base + ["-o", plain]).returncode == 0
    for measure in CM.MEASURES:
        numbers, reps, edges, k, largest = model_files(names, lens, res, CUTS[cut], measure)
        assert 0 < edges < n * (n - 1) // 2 and 1 < k < n and largest >= 2 and numbers != reps, (edges, k)
        for tag, more, want in (("numbers", [], numbers), ("reps", ["--cluster-representatives"], reps)):
            out, cf = str(tmp_path / f"{measure}_{tag}.tsv"), str(tmp_path / f"{measure}_{tag}.clusters")
            p = run(base + ["-o", out, "-V", "2", "--cluster", ALGO, "--cluster-out", cf, "--cluster-measure", measure] + more)
            assert p.returncode == 0, p.stderr[-1500:]
            assert open(cf).read() == want, (measure, tag)
            assert f"clusters on the host: {k} of {n} sequences from {edges} pairs" in p.stderr, p.stderr[-600:]
            # the TSV and the ids file are those of the run without --cluster
            assert open(out, "rb").read() == open(plain, "rb").read()
            assert open(out.replace(".tsv", ".ids.tsv"), "rb").read() == open(plain.replace(".tsv", ".ids.tsv"), "rb").read()
    # without --cluster-measure: tani
    cf = str(tmp_path / "default.clusters")
    assert run(base + ["-o", str(tmp_path / "d.tsv"), "--cluster", ALGO, "--cluster-out", cf]).returncode == 0
    assert open(cf).read() == model_files(names, lens, res, CUTS[cut], "tani")[0]


def test_refusals_and_usage(tmp_path):
    fa = SETS["example"][0]
    raw = tmp_path / "raw.txt"
    raw.write_text("")
    common = ["-o", str(tmp_path / "o.tsv"), "--results-in", str(raw), "--cluster-out", str(tmp_path / "c.tsv")] + CUTS["ani_qcov"]
    for value in ("complete", "leiden", "6", "complete_linkage"):
        p = run(["all2all"] + fa + ["--cluster", value] + common)
        assert p.returncode == 1 and f"Unknown value for --cluster: {value}" in p.stderr and "complete-linkage" in p.stderr, p.stderr[-600:]
        assert not os.path.exists(str(tmp_path / "c.tsv"))
    p = run(["all2all"] + fa + ["--cluster", ALGO, "--cluster-out", str(tmp_path / "c.tsv"), "-o", str(tmp_path / "o.tsv"), "--results-in", str(raw)])
    assert p.returncode == 1 and "--out-filter" in p.stderr                      # complete linkage needs the output filter like the others
    usage = run([]).stderr
    assert "complete-linkage" in usage and "greedy-best and complete-linkage compare" in usage      # the value, and that the measure matters for it


# ---- GPU half ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("measure", CM.MEASURES)
def test_device_and_host_paths_write_the_models_file(tmp_path, tmp_path_factory, measure):
    names, lens, res = raw_integers(tmp_path_factory, "example")
    args, n, _ = SETS["example"]
    cut = "ani_qcov"
    numbers, reps, edges, k, largest = model_files(names, lens, res, CUTS[cut], measure)
    assert 0 < edges and 1 < k < n and largest >= 2
    raw = str(tmp_path / "raw.txt")
    _raw_file(raw, res)
    for with_reps in (False, True):
        files = {}
        for tag, more, env, line in (("device", [], dict(LZANI_TILE_ROWS="0"), "clusters on the device: "),
                                     ("host", [], dict(LZANI_TILE_ROWS="0", LZANI_OUT_FILTER="host"), "clusters on the host: "),
                                     ("results-in", ["--results-in", raw], {}, "clusters on the host: ")):
            d = tmp_path / f"{tag}{int(with_reps)}"
            d.mkdir()
            p = run(["all2all"] + args + more + CUTS[cut] + ["-o", "o.tsv", "-V", "2", "--cluster", ALGO, "--cluster-out", "c.tsv", "--cluster-measure", measure]
                    + (["--cluster-representatives"] if with_reps else []), env, cwd=str(d))
            assert p.returncode == 0, p.stderr[-1500:]
            assert line in p.stderr, p.stderr[-1500:]
            if tag == "device":
                assert f"clusters on the device: {k} of {n} sequences" in p.stderr and f"from {edges} pairs" in p.stderr, p.stderr[-1500:]
                assert f"complete linkage: {edges} distinct pairs (0 given again), {n - k} merges" in p.stderr, p.stderr[-1500:]
            files[tag] = ((d / "c.tsv").read_bytes(), (d / "o.tsv").read_bytes())
            assert files[tag][0].decode() == (reps if with_reps else numbers), (tag, with_reps)
        assert files["device"] == files["host"] and files["device"][0] == files["results-in"][0]
