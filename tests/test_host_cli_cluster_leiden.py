"""`lz-ani --cluster leiden-cpm`: the cluster file of the host binary against tests/cluster_leiden_model.py put over the raw
integers of the matching stage (never over the printed TSV: its decimals are rounded).  CPU half: through --results-in, which
takes the host path (the sequential form of lzani_cluster_plan.h), for the three measures, with and without
--cluster-representatives, with the default and with given parameters; the refusals; the usage text.  GPU half: the device
path (lzani_group_cluster_* behind the kept calls), LZANI_OUT_FILTER=host and --results-in write the same bytes, those of the
model over a --results-out run's integers."""
import os
import subprocess

import numpy as np
import pytest

import cluster_model as CM
import out_filter_model as M
import util as U
from test_cluster_leiden import model
from test_host_cli import _oracle_reordered, _raw_file
from test_host_cli_cluster import minima, raw_integers
from test_host_cli_out_filter import CUTS, SETS

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
ENV = ("LZANI_OUT_FILTER", "LZANI_TILE_MIN", "LZANI_TILE_ROWS", "LZANI_DEVICE_LIST")
ALGO = "leiden-cpm"


@pytest.fixture(scope="module", autouse=True)
def build_host():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])


def run(args, env=None, cwd=None):
    base = {k: v for k, v in os.environ.items() if k not in ENV}
    base.update(env or {})
    return subprocess.run([EXE] + args, capture_output=True, text=True, env=base, cwd=cwd)


def model_files(names, lens, res, cut, measure, gamma=0.7, iterations=2):
    """The cluster file by the model, with numbers and with representatives: res[r, q] = the raw result of (ref r, query q),
    ids in the order of the ids file; and the number of edges, and the model's result."""
    n = len(names)
    a, b = np.triu_indices(n, 1)
    lens = np.asarray(lens, dtype=np.uint32)
    x, y = res[a, b], res[b, a]
    ln = M.lines(minima(cut), x, y, lens[a], lens[b])
    keep = ln != 0
    w = CM.weight(measure, x[keep], y[keep], ln[keep], lens[a][keep], lens[b][keep])
    r = model(n, a[keep], b[keep], w, gamma, iterations)
    numbers = "object\tcluster\n" + "".join(f"{nm}\t{c}\n" for nm, c in zip(names, r["cluster_of"]))
    reps = "object\trepresentative\n" + "".join(f"{nm}\t{names[p]}\n" for nm, p in zip(names, r["rep_of"]))
    return numbers, reps, int(keep.sum()), r


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
    seen = set()
    for measure in CM.MEASURES:
        for gamma, it, flags in ((0.7, 2, []), (0.3, 1, ["--cluster-leiden-resolution", "0.3", "--cluster-leiden-iterations", "1"])):
            numbers, reps, edges, r = model_files(names, lens, res, CUTS[cut], measure, gamma, it)
            assert 0 < edges < n * (n - 1) // 2 and numbers != reps
            seen.add(r["clusters"])
            for tag, more, want in (("numbers", [], numbers), ("reps", ["--cluster-representatives"], reps)):
                out, cf = str(tmp_path / f"{measure}_{it}_{tag}.tsv"), str(tmp_path / f"{measure}_{it}_{tag}.clusters")
                p = run(base + ["-o", out, "-V", "2", "--cluster", ALGO, "--cluster-out", cf, "--cluster-measure", measure] + flags + more)
                assert p.returncode == 0, p.stderr[-1500:]
                assert open(cf).read() == want, (measure, tag, gamma)
                assert f"clusters on the host: {r['clusters']} of {n} sequences from {edges} pairs" in p.stderr, p.stderr[-600:]
                # the TSV and the ids file are those of the run without --cluster
                assert open(out, "rb").read() == open(plain, "rb").read()
                assert open(out.replace(".tsv", ".ids.tsv"), "rb").read() == open(plain.replace(".tsv", ".ids.tsv"), "rb").read()
    assert any(1 < k < n for k in seen) and len(seen) > 1, seen           # by the model alone: real clusters, and the parameters matter
    # without --cluster-measure: tani
    cf = str(tmp_path / "default.clusters")
    assert run(base + ["-o", str(tmp_path / "d.tsv"), "--cluster", ALGO, "--cluster-out", cf]).returncode == 0
    assert open(cf).read() == model_files(names, lens, res, CUTS[cut], "tani")[0]


def test_refusals_and_usage(tmp_path):
    fa = SETS["example"][0]
    raw = tmp_path / "raw.txt"
    raw.write_text("")
    cf = str(tmp_path / "c.tsv")
    common = ["-o", str(tmp_path / "o.tsv"), "--results-in", str(raw), "--cluster-out", cf] + CUTS["ani_qcov"]
    for value in ("leiden", "leiden_cpm", "8", "cpm"):                 # `leiden` alone is still unknown
        p = run(["all2all"] + fa + ["--cluster", value] + common)
        assert p.returncode == 1 and f"Unknown value for --cluster: {value}" in p.stderr and "complete-linkage or leiden-cpm" in p.stderr, p.stderr[-600:]
    # one step outside the ranges, before any input is read (the fasta does not exist)
    missing = ["--in-fasta", str(tmp_path / "missing.fa")]
    for flag, value in (("--cluster-leiden-resolution", "1.0001"), ("--cluster-leiden-resolution", "-0.0001"), ("--cluster-leiden-resolution", "nan"),
                        ("--cluster-leiden-resolution", "0.7x"), ("--cluster-leiden-iterations", "0"), ("--cluster-leiden-iterations", "17"),
                        ("--cluster-leiden-iterations", "2.5")):
        p = run(["all2all"] + missing + ["--cluster", ALGO, flag, value] + common)
        assert p.returncode == 1 and f"Unsupported value: {flag} {value}" in p.stderr, (flag, value, p.stderr[-600:])
    for flag, value in (("--cluster-leiden-resolution", "0"), ("--cluster-leiden-resolution", "1"), ("--cluster-leiden-iterations", "1"),
                        ("--cluster-leiden-iterations", "16")):      # the ends of the ranges pass the check (and the input is missed)
        p = run(["all2all"] + missing + ["--cluster", ALGO, flag, value] + common)
        assert "Unsupported value" not in p.stderr and "belong to" not in p.stderr, (flag, value, p.stderr[-600:])
    # either flag without leiden-cpm
    for flag, value in (("--cluster-leiden-resolution", "0.5"), ("--cluster-leiden-iterations", "3")):
        for algo in (["--cluster", "single"], []):
            p = run(["all2all"] + fa + algo + [flag, value] + (common if algo else ["-o", str(tmp_path / "o.tsv"), "--results-in", str(raw)]))
            assert p.returncode == 1 and "belong to --cluster leiden-cpm" in p.stderr, (flag, algo, p.stderr[-600:])
    assert not os.path.exists(cf)
    p = run(["all2all"] + fa + ["--cluster", ALGO, "--cluster-out", cf, "-o", str(tmp_path / "o.tsv"), "--results-in", str(raw)])
    assert p.returncode == 1 and "--out-filter" in p.stderr                      # Leiden needs the output filter like the others
    usage = run([]).stderr
    assert "leiden-cpm" in usage and "--cluster-leiden-resolution" in usage and "--cluster-leiden-iterations" in usage
    assert "complete-linkage compare and leiden-cpm sums" in usage                     # the measure matters for it


# ---- GPU half ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("measure", CM.MEASURES)
def test_device_and_host_paths_write_the_models_file(tmp_path, tmp_path_factory, measure):
    names, lens, res = raw_integers(tmp_path_factory, "example")
    args, n, _ = SETS["example"]
    cut = "ani_qcov"
    raw = str(tmp_path / "raw.txt")
    _raw_file(raw, res)
    for gamma, it, flags in ((0.7, 2, []), (0.3, 3, ["--cluster-leiden-resolution", "0.3", "--cluster-leiden-iterations", "3"])):
        numbers, reps, edges, r = model_files(names, lens, res, CUTS[cut], measure, gamma, it)
        assert 0 < edges
        for with_reps in (False, True):
            files = {}
            for tag, more, env, line in (("device", [], dict(LZANI_TILE_ROWS="0"), "clusters on the device: "),
                                         ("host", [], dict(LZANI_TILE_ROWS="0", LZANI_OUT_FILTER="host"), "clusters on the host: "),
                                         ("results-in", ["--results-in", raw], {}, "clusters on the host: ")):
                d = tmp_path / f"{tag}{it}{int(with_reps)}"
                d.mkdir()
                p = run(["all2all"] + args + more + CUTS[cut] + ["-o", "o.tsv", "-V", "2", "--cluster", ALGO, "--cluster-out", "c.tsv", "--cluster-measure", measure]
                        + flags + (["--cluster-representatives"] if with_reps else []), env, cwd=str(d))
                assert p.returncode == 0, p.stderr[-1500:]
                assert line in p.stderr, p.stderr[-1500:]
                if tag == "device":
                    assert f"clusters on the device: {r['clusters']} of {n} sequences" in p.stderr and f"from {edges} pairs" in p.stderr, p.stderr[-1500:]
                    assert (f"Leiden: {edges} distinct pairs (0 given again), {r['iterations']} iterations, {r['levels']} levels, {r['move_rounds']} moving and "
                            f"{r['refine_rounds']} refinement rounds, {r['moves']} moves, {r['merges']} merges, quality {r['quality']} / 2^20") in p.stderr, p.stderr[-1500:]
                files[tag] = ((d / "c.tsv").read_bytes(), (d / "o.tsv").read_bytes())
                assert files[tag][0].decode() == (reps if with_reps else numbers), (tag, with_reps, gamma)
            assert files["device"] == files["host"] and files["device"][0] == files["results-in"][0]
