"""`lz-ani --cluster-cut / --cluster-level`: several clusterings of one run, each cut at cluster time.  The files of the host
binary against tests/cluster_cut_model.py and the cluster models put over the raw integers of the matching stage.
CPU half: through --results-in, which takes the host path (cluster_on_host once per level); the TSV and the ids file with and
without the cluster flags; the refusals.  GPU half: the device path (the record store behind the kept calls, a level per file),
the tiled device path and LZANI_OUT_FILTER=host write the same three files, the model's, and the same TSV."""
import os

import numpy as np
import pytest

import cluster_cut_model as CUT
import cluster_link_model as KM
import cluster_model as CM
import out_filter_model as M
from test_cluster_leiden import model as leiden_model
from test_host_cli import _raw_file
from test_host_cli_cluster import build_host, oracle_sets, raw_integers, run  # noqa: F401  (fixtures and helpers, unchanged)
from test_host_cli_out_filter import SETS

FILTER = ["--out-filter", "tani", "0.2"]
# (algorithm, file, cut): the level of --cluster with its --cluster-cut flags, then the --cluster-level ones
LEVELS = (("single", "f1", dict(ani=0.9, qcov=0.5)), ("complete-linkage", "f2", dict(ani=0.95, qcov=0.85)), ("leiden-cpm", "f3", {}))


def level_flags(d=""):
    f = [os.path.join(d, name) for _, name, _ in LEVELS]
    return ["--cluster", "single", "--cluster-out", f[0], "--cluster-cut", "ani", "0.9", "--cluster-cut", "qcov", "0.5",
            "--cluster-level", "complete-linkage", f[1], "ani=0.95,qcov=0.85", "--cluster-level", "leiden-cpm", f[2], "none"]


def model_files(names, lens, res, measure="tani"):
    """{file: (text, clusters, records in, edges)} by the models: res[r, q] = the raw result of (ref r, query q)."""
    n = len(names)
    a, b = np.triu_indices(n, 1)
    lens = np.asarray(lens, dtype=np.uint32)
    x, y = res[a, b], res[b, a]
    ln = M.lines({"tani": 0.2}, x, y, lens[a], lens[b])
    out = {}
    for algo, name, cut in LEVELS:
        stay = CUT.cut_lines(cut, x, y, ln, lens[a], lens[b])
        keep = stay != 0
        ea, eb = a[keep], b[keep]
        w = CM.weight(measure, x[keep], y[keep], stay[keep], lens[ea], lens[eb])
        if algo == "single":
            rep = CM.cluster(n, CM.edge_set(ea, eb, w), algo)[0]
        elif algo == "complete-linkage":
            rep = KM.linkage(n, KM.edge_min(ea, eb, w))
        else:
            rep = leiden_model(n, ea, eb, w)["rep_of"]
        rep = np.asarray(rep, dtype=np.int64)
        cl, k = CM.number(rep)
        out[name] = ("object\tcluster\n" + "".join(f"{nm}\t{c}\n" for nm, c in zip(names, cl)), k, int((ln != 0).sum()), int(keep.sum()))
    return out


@pytest.mark.parametrize("name", sorted(SETS))
def test_level_files_through_results_in(tmp_path, oracle_sets, name):
    names, lens, res = oracle_sets[name]
    n = len(names)
    raw = str(tmp_path / "raw.txt")
    _raw_file(raw, res)
    base = ["all2all"] + SETS[name][0] + ["--results-in", raw, "--out-format", "complete"] + FILTER
    plain, out = str(tmp_path / "plain.tsv"), str(tmp_path / "o.tsv")
    assert run(base + ["-o", plain]).returncode == 0
    p = run(base + ["-o", out, "-V", "2"] + level_flags(str(tmp_path)))
    assert p.returncode == 0, p.stderr[-1500:]
    assert "cluster level" not in p.stderr and p.stderr.count("clusters on the host: ") == 3
    want = model_files(names, lens, res)
    texts = set()
    for _, f, _ in LEVELS:
        text, k, records, edges = want[f]
        assert open(str(tmp_path / f)).read() == text, f
        assert f"clusters on the host: {k} of {n} sequences from {edges} pairs" in p.stderr, (f, p.stderr[-1500:])
        if name == "vir61":
            assert 1 < k < n and 0 < edges <= records, (f, k, edges)
        texts.add(text)
    if name == "vir61":
        assert len(texts) == 3                          # three levels, three clusterings
    # the TSV and the ids file are those of the run without any cluster flag
    assert open(out, "rb").read() == open(plain, "rb").read()
    assert open(out.replace(".tsv", ".ids.tsv"), "rb").read() == open(plain.replace(".tsv", ".ids.tsv"), "rb").read()


def test_refusals(tmp_path):
    fa = SETS["example"][0]
    raw = tmp_path / "raw.txt"
    raw.write_text("")
    f = [str(tmp_path / x) for x in ("c1", "c2", "c3")]
    common = ["all2all"] + fa + ["-o", str(tmp_path / "o.tsv"), "--results-in", str(raw)] + FILTER
    cluster = ["--cluster", "single", "--cluster-out", f[0]]
    same_file = "--cluster-level: two levels write the same file"
    for args, text in (
            (["--cluster-cut", "ani", "0.9"], "--cluster-cut and --cluster-level belong to --cluster"),                 # without --cluster
            (["--cluster-level", "single", f[1], "none"], "--cluster-cut and --cluster-level belong to --cluster"),
            (cluster + ["--cluster-cut", "cov", "0.9"], "Invalid value for --cluster-cut: unknown parameter 'cov'"),    # an unknown par
            (cluster + ["--cluster-level", "single", f[1], "cov=0.9"], "Invalid value for --cluster-level: unknown parameter 'cov'"),
            (cluster + ["--cluster-level", "complete", f[1], "none"], "Unknown value for --cluster-level: complete"),   # an unknown algorithm
            (cluster + ["--cluster-cut", "ani", "high"], "Invalid value for --cluster-cut: ani takes a number, not 'high'"),   # values that do not parse
            (cluster + ["--cluster-cut", "ani", "0.9x"], "Invalid value for --cluster-cut: ani takes a number, not '0.9x'"),
            (cluster + ["--cluster-cut", "ani", "nan"], "Invalid value for --cluster-cut: ani takes a number, not 'nan'"),
            (cluster + ["--cluster-cut", "num_alns", "0"], "Invalid value for --cluster-cut: num_alns takes an integer >= 1, not '0'"),
            (cluster + ["--cluster-cut", "num_alns", "2.5"], "Invalid value for --cluster-cut: num_alns takes an integer >= 1, not '2.5'"),
            (cluster + ["--cluster-level", "single", f[1], "ani=high"], "Invalid value for --cluster-level: ani takes a number, not 'high'"),
            (cluster + ["--cluster-level", "single", f[1], "ani"], "Invalid value for --cluster-level: 'ani' is not of the form par=value"),
            (cluster + ["--cluster-level", "single", f[1], "ani=0.9,,qcov=0.5"], "Invalid value for --cluster-level: '' is not of the form par=value"),
            (cluster + ["--cluster-level", "single", f[1], ""], "Invalid value for --cluster-level: empty cuts"),
            (cluster + ["--cluster-level", "single", f[1], "none", "--cluster-level", "greedy-best", f[1], "ani=0.9"], same_file + ": " + f[1]),
            (cluster + ["--cluster-level", "greedy-best", f[0], "ani=0.9"], same_file + ": " + f[0]),                  # the file of --cluster-out
            (cluster + ["--cluster-level", "complete-linkage", f[1], "none", "--cluster-leiden-resolution", "0.5"],
             "--cluster-leiden-resolution and --cluster-leiden-iterations belong to --cluster leiden-cpm"),             # no level is leiden-cpm
            (cluster + ["--cluster-cut", "ani", "0.9", "--cluster-leiden-iterations", "3"],
             "--cluster-leiden-resolution and --cluster-leiden-iterations belong to --cluster leiden-cpm"),
            (cluster + [x for k in range(17) for x in ("--cluster-level", "single", str(tmp_path / f"l{k}"), "none")], "--cluster-level can be used at most 16 times")):
        p = run(common + args)
        assert p.returncode == 1 and text in p.stderr, (args, p.stderr[-600:])
        assert "Unknown parameter" not in p.stderr and "Usage:" not in p.stderr, (args, p.stderr[:300])      # the refusal meant, not the catch-all one
        assert not any(os.path.exists(x) for x in f) and "Loading sequences" not in p.stderr, args


def test_leiden_parameters_belong_to_any_leiden_level(tmp_path, oracle_sets):
    names, lens, res = oracle_sets["example"]
    raw = str(tmp_path / "raw.txt")
    _raw_file(raw, res)
    f = [str(tmp_path / x) for x in ("c1", "c2")]
    p = run(["all2all"] + SETS["example"][0] + ["--results-in", raw, "-o", str(tmp_path / "o.tsv")] + FILTER +
            ["--cluster", "single", "--cluster-out", f[0], "--cluster-level", "leiden-cpm", f[1], "none", "--cluster-leiden-resolution", "0.5"])
    assert p.returncode == 0 and all(os.path.exists(x) for x in f), p.stderr[-600:]


# ---- GPU half ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SETS))
def test_device_tiled_and_host_paths_write_the_models_files(tmp_path, tmp_path_factory, name):
    names, lens, res = raw_integers(tmp_path_factory, name)
    args, n, rows = SETS[name]
    want = model_files(names, lens, res)
    files = {}
    for tag, env in (("device", dict(LZANI_TILE_ROWS="0")), ("tiled", dict(LZANI_TILE_MIN="1", LZANI_TILE_ROWS=str(rows))),
                     ("host", dict(LZANI_TILE_ROWS="0", LZANI_OUT_FILTER="host"))):
        d = tmp_path / tag
        d.mkdir()
        p = run(["all2all"] + args + FILTER + ["-o", "o.tsv", "-V", "2"] + level_flags(), env, cwd=str(d))
        assert p.returncode == 0, p.stderr[-1500:]
        assert (f"blocks of {rows} rows" in p.stderr) == (tag == "tiled"), p.stderr[-1500:]
        assert p.stderr.count("cluster level ") == (0 if tag == "host" else 3), p.stderr[-1500:]          # the level line: the device paths only
        assert p.stderr.count("clusters on the device: " if tag != "host" else "clusters on the host: ") == 3
        for k, (_, f, _) in enumerate(LEVELS):
            text, clusters, records, edges = want[f]
            assert (d / f).read_text() == text, (tag, f)
            if tag != "host":
                level = f"cluster level {k} on the device ({f}): {records} records in, {edges} edges out"
                assert level in p.stderr and p.stderr.index(level) < p.stderr.index(f"clusters on the device: {clusters} of {n} sequences", p.stderr.index(level))
        files[tag] = (d / "o.tsv").read_bytes()
    plain = tmp_path / "plain"
    plain.mkdir()
    assert run(["all2all"] + args + FILTER + ["-o", "o.tsv"], dict(LZANI_TILE_ROWS="0"), cwd=str(plain)).returncode == 0
    assert files["device"] == files["tiled"] == files["host"] == (plain / "o.tsv").read_bytes()
