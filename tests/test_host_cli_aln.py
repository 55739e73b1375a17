"""GPU: `lz-ani --out-alignment` on the example multifasta through the device's region stage (lzani_run_rows_aligned) against
the host path of the same binary (LZANI_OUT_ALN=host): the bytes of the alignment file, of the TSV and of the cluster file."""
import os
import subprocess

import pytest

import ooc_model as OM
import util as U

pytestmark = pytest.mark.gpu

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
FA = os.path.join(U.GOLD, "example", "multifasta.fna")
ON_DEVICE, ON_HOST = "alignment regions on the device", "alignment regions on the host"
MEDIANS = ["--out-filter", "gani", "0.0231", "--out-filter", "ani", "0.579", "--out-filter", "qcov", "0.04"]      # about the medians of the golden file's pairs


@pytest.fixture(scope="module", autouse=True)
def build_host():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])


def run(tmp, tag, extra, env=None):
    """(stderr, the bytes of the TSV, of the alignment file, of the cluster file or None) of one run"""
    out, aln, cl = (str(tmp / f"{tag}.{x}") for x in ("tsv", "aln.tsv", "clusters.tsv"))
    args = [EXE, "all2all", "--in-fasta", FA, "-o", out, "--out-alignment", aln, "-V", "2"] + [cl if x == "CLUSTERS" else x for x in extra]
    e = {k: v for k, v in os.environ.items() if k not in ("LZANI_OUT_ALN", "LZANI_DEVICE_LIST")}
    p = subprocess.run(args, capture_output=True, text=True, env=dict(e, **(env or {})))
    assert p.returncode == 0, p.stderr[-1500:]
    return p.stderr, open(out, "rb").read(), open(aln, "rb").read(), open(cl, "rb").read() if os.path.exists(cl) else None


def gpu_mem_for_three_blocks():
    lens = [len(s) for s in U.reorder(*U.load_example())[1]]
    return str(OM.limit_for_blocks(lens, None, 3))


CASES = {
    "plain": [],
    "medians": MEDIANS,
    "kmerdb": ["--flt-kmerdb", os.path.join(U.GOLD, "example", "fltr.txt"), "0.9"],
    "gpu_mem": None,                                    # (made in the test: --gpu-mem at 3 blocks)
    "cluster": MEDIANS + ["--cluster", "single", "--cluster-out", "CLUSTERS"],
}


@pytest.mark.parametrize("case", list(CASES))
def test_device_path_writes_the_bytes_of_the_host_path(tmp_path, case):
    extra = ["--gpu-mem", gpu_mem_for_three_blocks()] if case == "gpu_mem" else CASES[case]
    err_d, tsv_d, aln_d, cl_d = run(tmp_path, "dev", extra)
    err_h, tsv_h, aln_h, cl_h = run(tmp_path, "host", extra, {"LZANI_OUT_ALN": "host"})
    assert ON_DEVICE in err_d and ON_HOST not in err_d and ON_HOST in err_h and ON_DEVICE not in err_h      # -V 2 names the path taken
    assert err_d.count("GPU 0:") == 1 and err_h.count("GPU 0:") == 1
    assert aln_d == aln_h and tsv_d == tsv_h and cl_d == cl_h
    lines = aln_d.decode().split("\n")
    assert len(lines) > 3 and lines[-1] == ""
    gold = open(os.path.join(U.GOLD, "example", "ani.aln.tsv")).read().split("\n")
    if case in ("plain", "gpu_mem"):
        assert lines[0] == gold[0] and sorted(lines[1:]) == sorted(gold[1:])          # the golden file as a multiset
        assert " 1 run(s)" in err_d
    else:
        assert set(lines) < set(gold)                   # some pairs go, some stay
    if case == "gpu_mem":
        assert "out-of-core, 3 block(s)" in err_d
    if case == "medians":
        assert "out-filter on the device" in err_d      # the same call is the kept call
        assert "out-filter on the device" not in err_h
    if case == "cluster":
        # (with --cluster next to --out-alignment the binary keeps the output filter and the clustering on the host in both
        # runs, over the results the aligned call brought: the three files must still be equal, and the alignment's path is
        # the device's -- DESIGN 4f says what is left out)
        assert cl_d is not None and len(cl_d) > 20
        assert "clusters on the host" in err_d and "clusters on the host" in err_h and "out-filter on the device" not in err_d
    # the file's order: pairs by (reference, query) in the reordered ids, inside a pair the longer region first, then the smaller start
    names = U.reorder(*U.load_example())[0]
    at = {nm: i for i, nm in enumerate(names)}
    rows = [ln.split("\t") for ln in lines[1:-1]]
    keys = [(at[r[1]], at[r[0]], -int(r[3]), int(r[4])) for r in rows]
    assert keys == sorted(keys)


def test_a_nan_minimum_keeps_the_host_path_and_the_other_minima(tmp_path):
    """A minimum that is not a number drops nothing and leaves the others in force, as before the device path was there."""
    err, tsv, aln, _ = run(tmp_path, "nan", ["--out-filter", "ani", "nan", "--out-filter", "qcov", "0.04"])
    assert ON_HOST in err and ON_DEVICE not in err
    ref = run(tmp_path, "num", ["--out-filter", "qcov", "0.04"])
    assert ON_DEVICE in ref[0] and aln == ref[2]
    gold = open(os.path.join(U.GOLD, "example", "ani.aln.tsv")).read().split("\n")
    assert 3 < len(aln.decode().split("\n")) < len(gold)


def test_two_devices_take_the_host_path(tmp_path):
    err, tsv, aln, _ = run(tmp_path, "two", ["--gpus", "2"], {"LZANI_DEVICE_LIST": "0,0"})
    assert ON_HOST in err and ON_DEVICE not in err and err.count("GPU 0:") == 2
    one = run(tmp_path, "one", [])
    assert ON_DEVICE in one[0] and (tsv, aln) == (one[1], one[2])
    assert sorted(aln.decode().split("\n")) == sorted(open(os.path.join(U.GOLD, "example", "ani.aln.tsv")).read().split("\n"))
