"""`lz-ani --cluster`: the cluster file of the host binary against tests/cluster_model.py put over the raw integers of the
matching stage (never over the printed TSV: its decimals are rounded, and greedy-best would turn on the rounding).
CPU half: through --results-in, which takes the host path (the emitter's own lines, the sequential statement of
lzani_cluster_plan.h); the refusals; the TSV with and without --cluster.  GPU half: the device path (lzani_group_cluster_*
behind the kept calls), the tiled device path and LZANI_OUT_FILTER=host write the same file, that of the model over a
--results-out run's integers."""
import os
import subprocess

import numpy as np
import pytest

import cluster_model as CM
import out_filter_model as M
import util as U
from test_host_cli import _oracle_reordered, _raw_file
from test_host_cli_out_filter import CUTS, SETS

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
ENV = ("LZANI_OUT_FILTER", "LZANI_TILE_MIN", "LZANI_TILE_ROWS", "LZANI_DEVICE_LIST")
LOADERS = {"example": U.load_example, "vir61": U.load_vir61}
MEASURE_OF_CUT = {"ani_qcov": "gani", "tani_rcov": "tani"}


@pytest.fixture(scope="module", autouse=True)
def build_host():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])


def run(args, env=None, cwd=None):
    base = {k: v for k, v in os.environ.items() if k not in ENV}
    base.update(env or {})
    return subprocess.run([EXE] + args, capture_output=True, text=True, env=base, cwd=cwd)


def minima(cut):
    return {cut[i + 1]: float(cut[i + 2]) for i in range(0, len(cut), 3)}


def model_file(names, lens, res, cut, algo, measure, representatives=False):
    """The cluster file by the model: res[r, q] = the raw result of (ref r, query q), ids in the order of the ids file."""
    n = len(names)
    a, b = np.triu_indices(n, 1)
    lens = np.asarray(lens, dtype=np.uint32)
    x, y = res[a, b], res[b, a]
    ln = M.lines(minima(cut), x, y, lens[a], lens[b])
    keep = ln != 0
    w = CM.weight(measure, x[keep], y[keep], ln[keep], lens[a][keep], lens[b][keep])
    rep, cl, st = CM.cluster(n, CM.edge_set(a[keep], b[keep], w), algo)
    col = [names[r] for r in rep] if representatives else [str(c) for c in cl]
    head = "object\t" + ("representative" if representatives else "cluster") + "\n"
    return head + "".join(f"{nm}\t{c}\n" for nm, c in zip(names, col)), st, int(keep.sum())


@pytest.fixture(scope="module")
def oracle_sets():
    out = {}
    for name, loader in LOADERS.items():
        names, seqs, res = _oracle_reordered(loader)
        out[name] = (names, [len(s) for s in seqs], res)
    return out


@pytest.mark.parametrize("cut", sorted(CUTS))
@pytest.mark.parametrize("name", sorted(SETS))
def test_cluster_file_through_results_in(tmp_path, oracle_sets, name, cut):
    names, lens, res = oracle_sets[name]
    n = len(names)
    raw = str(tmp_path / "raw.txt")
    _raw_file(raw, res)
    measure = MEASURE_OF_CUT[cut]
    base = ["all2all"] + SETS[name][0] + ["--results-in", raw, "--out-format", "complete"] + CUTS[cut]
    plain = str(tmp_path / "plain.tsv")
    assert run(base + ["-o", plain]).returncode == 0
    shown = set()
    for algo in CM.ALGOS:
        for reps in (False, True):
            out, cf = str(tmp_path / f"{algo}{int(reps)}.tsv"), str(tmp_path / f"{algo}{int(reps)}.clusters")
            p = run(base + ["-o", out, "--cluster", algo, "--cluster-out", cf, "--cluster-measure", measure] + (["--cluster-representatives"] if reps else []))
            assert p.returncode == 0, p.stderr[-1500:]
            want, st, edges = model_file(names, lens, res, CUTS[cut], algo, measure, reps)
            assert open(cf).read() == want, (algo, reps)
            assert 0 < edges < n * (n - 1) // 2 and 1 < st["clusters"] < n, (st, edges)
            shown.add(want)
            # the TSV and the ids file are those of the run without --cluster
            assert open(out, "rb").read() == open(plain, "rb").read()
            assert open(out.replace(".tsv", ".ids.tsv"), "rb").read() == open(plain.replace(".tsv", ".ids.tsv"), "rb").read()
    assert len(shown) >= 2                                # (numbers and representatives; the families here are near-cliques)


def test_default_measure_is_tani(tmp_path, oracle_sets):
    names, lens, res = oracle_sets["example"]
    raw = str(tmp_path / "raw.txt")
    _raw_file(raw, res)
    cf = str(tmp_path / "c.tsv")
    args = ["all2all"] + SETS["example"][0] + ["--results-in", raw, "-o", str(tmp_path / "o.tsv"), "--cluster", "greedy-best", "--cluster-out", cf]
    assert run(args + CUTS["ani_qcov"]).returncode == 0
    assert open(cf).read() == model_file(names, lens, res, CUTS["ani_qcov"], "greedy-best", "tani")[0]


def test_refusals(tmp_path):
    fa = SETS["example"][0]
    raw = tmp_path / "raw.txt"
    raw.write_text("")
    common = ["-o", str(tmp_path / "o.tsv"), "--results-in", str(raw), "--cluster-out", str(tmp_path / "c.tsv")]
    cut = CUTS["ani_qcov"]
    for mode, args, text in (
            ("all2all", fa + ["--cluster", "single"], "--out-filter"),                                   # no output filter
            ("query2ref", fa + ["--query-fasta", fa[1], "--cluster", "single"] + cut, "all2all"),
            ("all2all", fa + ["--cluster", "single", "--out-type", "single-txt"] + cut, "single-txt"),
            ("all2all", fa + ["--cluster", "complete"] + cut, "Unknown value for --cluster"),
            ("all2all", fa + ["--cluster", "single", "--cluster-measure", "qcov"] + cut, "Unknown value for --cluster-measure")):
        p = run([mode] + args + common)
        assert p.returncode == 1 and text in p.stderr, (args, p.stderr[-600:])
        assert not os.path.exists(str(tmp_path / "c.tsv"))
    p = run(["all2all"] + fa + ["--cluster", "single", "-o", str(tmp_path / "o.tsv"), "--results-in", str(raw)] + cut)
    assert p.returncode == 1 and "--cluster-out" in p.stderr


# ---- GPU half ----------------------------------------------------------------------------------------------------------

_raw = {}


def raw_integers(tmp_path_factory, name):
    """res[r, q] of a --results-out run of the binary (the matching stage on the GPU), and the ids file's names and lengths."""
    if name not in _raw:
        d = tmp_path_factory.mktemp("raw_" + name)
        p = run(["all2all"] + SETS[name][0] + ["-o", "o.tsv", "--results-out", "raw.txt"], cwd=str(d))
        assert p.returncode == 0, p.stderr[-1500:]
        ids = [ln.split("\t") for ln in (d / "o.ids.tsv").read_text().split("\n")[1:] if ln]
        n = len(ids)
        res = np.zeros((n, n, 3), dtype=np.int32)
        for ln in (d / "raw.txt").read_text().split("\n"):
            if ln:
                r, q, m, l, c = (int(v) for v in ln.split())
                res[r, q] = (m, l, c)
        _raw[name] = ([i[0] for i in ids], [int(i[1]) for i in ids], res)
    return _raw[name]


@pytest.mark.gpu
@pytest.mark.parametrize("algo", CM.ALGOS)
@pytest.mark.parametrize("cut", sorted(CUTS))
@pytest.mark.parametrize("name", sorted(SETS))
def test_device_tiled_and_host_paths_write_the_models_file(tmp_path, tmp_path_factory, name, cut, algo):
    names, lens, res = raw_integers(tmp_path_factory, name)
    args, n, rows = SETS[name]
    assert len(names) == n
    measure = MEASURE_OF_CUT[cut]
    want, st, edges = model_file(names, lens, res, CUTS[cut], algo, measure)
    assert 0 < edges and 1 < st["clusters"] < n
    files = {}
    for tag, env, line in (("device", dict(LZANI_TILE_ROWS="0"), "clusters on the device: "),
                           ("tiled", dict(LZANI_TILE_MIN="1", LZANI_TILE_ROWS=str(rows)), "clusters on the device: "),
                           ("host", dict(LZANI_TILE_ROWS="0", LZANI_OUT_FILTER="host"), "clusters on the host: ")):
        d = tmp_path / tag
        d.mkdir()
        p = run(["all2all"] + args + CUTS[cut] + ["-o", "o.tsv", "-V", "2", "--cluster", algo, "--cluster-out", "c.tsv", "--cluster-measure", measure],
                env, cwd=str(d))
        assert p.returncode == 0, p.stderr[-1500:]
        assert line in p.stderr and (f"blocks of {rows} rows" in p.stderr) == (tag == "tiled"), p.stderr[-1500:]
        if tag != "host":
            assert f"clusters on the device: {st['clusters']} of {n} sequences ({st['singletons']} singletons, the largest of {st['largest']}) from {edges} pairs" in p.stderr
        files[tag] = ((d / "c.tsv").read_text(), (d / "o.tsv").read_bytes())
        assert files[tag][0] == want, tag
    assert files["device"][1] == files["tiled"][1] == files["host"][1]
