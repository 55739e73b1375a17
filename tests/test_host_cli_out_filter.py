"""GPU: `lz-ani --out-filter` with the filter applied on the device (lzani_group_run_rows_kept; the kept forms of
do_matching and do_matching_tiled in lz-ani_amd/host/match.h) writes the bytes the host filter writes (LZANI_OUT_FILTER=host):
dense and with a kmer-db filter, untiled and in row blocks, all2all and query2ref, one shard and three."""
import os
import subprocess

import pytest

import util as U

pytestmark = pytest.mark.gpu

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
EXAMPLE = os.path.join(U.GOLD, "example", "multifasta.fna")
CUTS = {"ani_qcov": ["--out-filter", "ani", "0.9", "--out-filter", "qcov", "0.5"],
        "tani_rcov": ["--out-filter", "tani", "0.5", "--out-filter", "rcov", "0.6"]}
SETS = {"example": (["--in-fasta", EXAMPLE], 12, 5), "vir61": (["--in-dir", os.path.join(U.GOLD, "vir61")], 61, 16)}     # input, genomes, rows of a block
ENV = ("LZANI_OUT_FILTER", "LZANI_TILE_MIN", "LZANI_TILE_ROWS", "LZANI_DEVICE_LIST")
DEVICE_LINE = "out-filter on the device: "


@pytest.fixture(scope="module", autouse=True)
def build_host():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])


def both_paths(tmp_path, mode, args, complete_lines, env=None, expect=()):
    """The run with the filter on the device and the run with it on the host: the same files; the -V 2 line of the device's
    stage on the first only; some lines, not all.  Returns the device run's stderr."""
    base = {k: v for k, v in os.environ.items() if k not in ENV}
    base.update(env or {})
    got = {}
    for tag, e in (("device", base), ("host", dict(base, LZANI_OUT_FILTER="host"))):
        d = tmp_path / tag
        d.mkdir()
        p = subprocess.run([EXE, mode] + args + ["-o", "out.tsv", "--out-format", "complete", "-V", "2"], capture_output=True, text=True, env=e, cwd=str(d))
        assert p.returncode == 0, p.stderr[-1500:]
        assert (DEVICE_LINE in p.stderr) == (tag == "device"), p.stderr[-1500:]
        assert "All2all sparse" in p.stderr and "Storing results" in p.stderr and "GPU 0:" in p.stderr
        for text in expect:
            assert text in p.stderr, (text, p.stderr[-1500:])
        got[tag] = ((d / "out.tsv").read_bytes(), (d / "out.ids.tsv").read_bytes(), p.stderr)
    assert got["device"][0] == got["host"][0] and got["device"][1] == got["host"][1]
    lines = got["device"][0].count(b"\n") - 1
    assert 0 < lines < complete_lines, lines
    line = [ln for ln in got["device"][2].split("\n") if ln.startswith(DEVICE_LINE)]
    assert len(line) == 1
    assert f" {lines} lines kept of " in line[0], line                        # the stage's own count is the file's
    return got["device"][2], lines


@pytest.mark.parametrize("tiled", [False, True], ids=["untiled", "tiled"])
@pytest.mark.parametrize("cut", sorted(CUTS))
@pytest.mark.parametrize("name", sorted(SETS))
def test_dense_all2all(tmp_path, name, cut, tiled):
    args, n, rows = SETS[name]
    env = dict(LZANI_TILE_MIN="1", LZANI_TILE_ROWS=str(rows)) if tiled else dict(LZANI_TILE_ROWS="0")
    err, _ = both_paths(tmp_path, "all2all", args + CUTS[cut], n * (n - 1), env, expect=[f"blocks of {rows} rows"] if tiled else [])
    assert f"lines kept of {n * (n - 1) // 2} pairs, 0 unpaired" in err


@pytest.mark.parametrize("cut", sorted(CUTS))
def test_with_a_kmerdb_filter(tmp_path, cut):
    flt = os.path.join(U.GOLD, "example", "fltr.txt")
    err, _ = both_paths(tmp_path, "all2all", ["--in-fasta", EXAMPLE, "--flt-kmerdb", flt, "0.9"] + CUTS[cut], 26, expect=["Filter size: 26"])
    assert "lines kept of 13 pairs, 0 unpaired" in err


def test_query2ref(tmp_path):
    recs = [b">" + r for r in open(EXAMPLE, "rb").read().split(b">")[1:]]
    ref, qry = tmp_path / "ref.fna", tmp_path / "qry.fna"
    ref.write_bytes(b"".join(recs[:5]))                 # (the split of test_host_cli_query2ref.py: inside a family)
    qry.write_bytes(b"".join(recs[5:]))
    err, _ = both_paths(tmp_path, "query2ref", ["--in-fasta", str(ref), "--query-fasta", str(qry)] + CUTS["ani_qcov"], 2 * 5 * 7)
    assert "lines kept of 35 pairs, 0 unpaired" in err


def test_three_shards_on_one_device(tmp_path):
    err, lines = both_paths(tmp_path, "all2all", ["--in-fasta", EXAMPLE, "--gpus", "3"] + CUTS["ani_qcov"], 132, dict(LZANI_DEVICE_LIST="0,0,0"))
    assert err.count("GPU 0:") == 3 and lines == 25
