"""The host binary's --flt-kmers-max-seqs: on the CPU what it refuses before any input is read; on the GPU the TSV of a
limited run against the run without the flag and the definition in Python integers (tests/prefilter_limit_model.py)."""
import os
import subprocess

import pytest

import lzani_ctypes as L
import prefilter_limit_model as LM
import synth_genomes as SG
import util as U

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
INDEX_FREE = "query,reference,qlen,rlen,tani,gani,ani,qcov,rcov,len_ratio,nt_match,nt_mismatch,num_alns"


@pytest.fixture(scope="module")
def host_binary():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])
    return EXE


def _run(host_binary, mode, tmp_path, extra):
    missing = str(tmp_path / "no_such_input.fa")
    args = [host_binary, mode, "--in-fasta", missing, "-o", str(tmp_path / "o.tsv")] + extra
    if mode == "query2ref":
        args += ["--query-fasta", missing]
    return subprocess.run(args, capture_output=True, text=True), missing


@pytest.mark.parametrize("mode", ["all2all", "query2ref"])
@pytest.mark.parametrize("value", ["0", "-1", "x", "4.5", "4x", "+4", "4294967296", "99999999999999999999999"])
def test_the_binary_refuses_a_bad_value_before_reading_input(host_binary, tmp_path, mode, value):
    p, _ = _run(host_binary, mode, tmp_path, ["--flt-kmers", "16", "0.1", "--flt-kmers-max-seqs", value])
    assert p.returncode == 1 and "Invalid value for --flt-kmers-max-seqs: %s (an integer >= 1)" % value in p.stderr, p.stderr
    assert "Cannot open file" not in p.stderr and "Loading sequences" not in p.stderr


@pytest.mark.parametrize("mode,extra", [("all2all", []), ("all2all", ["--flt-kmerdb", "no_such_filter.txt", "0.5"]), ("query2ref", [])])
def test_the_flag_belongs_to_flt_kmers(host_binary, tmp_path, mode, extra):
    p, _ = _run(host_binary, mode, tmp_path, extra + ["--flt-kmers-max-seqs", "4"])
    assert p.returncode == 1 and "--flt-kmers-max-seqs belongs to --flt-kmers" in p.stderr, p.stderr
    assert "Cannot open file" not in p.stderr and "Loading sequences" not in p.stderr


@pytest.mark.parametrize("value", ["1", "4", "4294967295"])
def test_good_values_reach_the_input(host_binary, tmp_path, value):
    p, missing = _run(host_binary, "all2all", tmp_path, ["--flt-kmers-max-seqs", value, "--flt-kmers", "16", "0.1"])
    assert p.returncode == 1 and "Cannot open file: " + missing in p.stderr, p.stderr


def test_usage_names_the_flag(host_binary):
    p = subprocess.run([host_binary], capture_output=True, text=True)
    assert "--flt-kmers-max-seqs <int>" in p.stderr


# ---- GPU

def _lines(path):
    return [ln for ln in open(path).read().split("\n")[1:] if ln]


def _ids(path):
    return [ln.split("\t")[0] for ln in open(path).read().split("\n")[1:] if ln]


def _family_set():
    """96 genomes of 3-6 kbp in families of 12, at most 4 % from the ancestor: every two of a family share at least a
    quarter of their 16-mers (0.92^16), so every genome has 11 partners above the threshold of 0.1."""
    return SG.make_set(96, 29, lmin=3000, lmax=6000, fam=12, dmin=0.01, dmax=0.04)


def _binary(mode_args, out, extra):
    p = subprocess.run([EXE] + mode_args + ["-o", out, "-V", "2", "--out-format", INDEX_FREE, "--flt-kmers", "16", "0.1"] + extra,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stderr


def _survivors(order, seq_of, n_ref, N):
    """The engine's unlimited result for the genomes in the binary's order, and the name pairs the model lets survive."""
    eng = L.Engine()
    try:
        if n_ref:
            eng.prefilter_codes_cross([seq_of[x] for x in order], 16, n_ref, min_ratio=0.1)
        else:
            eng.prefilter_codes([seq_of[x] for x in order], 16, min_ratio=0.1)
        k_of, row_off, ids, shared = eng.prefilter_fetch()
    finally:
        eng.close()
    keep = LM.limit(len(order), n_ref, k_of, row_off, ids, shared, N)
    a, b = LM.pairs_of(row_off, ids)
    return len(ids), {frozenset((order[x], order[y])) for x, y in zip(a[keep == 1].tolist(), b[keep == 1].tolist())}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["all2all", "query2ref"])
def test_the_limited_tsv_holds_the_lines_of_the_surviving_pairs(host_binary, tmp_path, mode):
    names, seqs = _family_set()
    seq_of = dict(zip(names, seqs))
    N = 4
    if mode == "all2all":
        fa = str(tmp_path / "in.fa")
        SG.write_fasta(fa, names, seqs)
        mode_args, n_ref = ["all2all", "--in-fasta", fa], 0
    else:                                                   # the even genomes are the references: six of every family
        ref, qry = str(tmp_path / "ref.fa"), str(tmp_path / "qry.fa")
        SG.write_fasta(ref, names[0::2], seqs[0::2])
        SG.write_fasta(qry, names[1::2], seqs[1::2])
        mode_args, n_ref = ["query2ref", "--in-fasta", ref, "--query-fasta", qry], len(names) // 2
    plain, cut = str(tmp_path / "plain.tsv"), str(tmp_path / "cut.tsv")
    _binary(mode_args, plain, [])
    err = _binary(mode_args, cut, ["--flt-kmers-max-seqs", str(N)])
    ids_plain, ids_cut = str(tmp_path / "plain.ids.tsv"), str(tmp_path / "cut.ids.tsv")
    assert open(ids_plain, "rb").read() == open(ids_cut, "rb").read()                    # the ids file is unchanged
    order = _ids(ids_plain)
    assert sorted(order) == sorted(names) and (not n_ref or set(order[:n_ref]) == set(names[0::2]))
    entries, alive = _survivors(order, seq_of, n_ref, N)
    want = [ln for ln in _lines(plain) if frozenset(ln.split("\t")[:2]) in alive]
    got = _lines(cut)
    assert got == want and 0 < len(got) < len(_lines(plain))
    assert len(_lines(plain)) == 2 * entries and len(got) == 2 * len(alive)
    assert "Filter size: %d" % (2 * len(alive)) in err, err[-2000:]
    assert "; max-seqs %d: %d of %d pairs stay, " % (N, len(alive), entries) in err and " sequences cut, limit " in err, err[-2000:]


# ---- a library without the stage (CPU: a stub that exports the required symbols only, every call an error)

@pytest.fixture(scope="module")
def old_library(tmp_path_factory):
    import re
    hdr = open(os.path.join(U.ROOT, "lz-ani_amd", "host", "engine.h")).read()
    required = re.search(r"#define LZANI_ENGINE_REQUIRED\(X\)(.*?)\n#define", hdr, re.S).group(1)
    names = re.findall(r"X\((\w+)\)", required)
    assert "prefilter" in names and "prefilter_limit" not in names
    d = tmp_path_factory.mktemp("old_library")
    src, lib = str(d / "stub.c"), str(d / "liblzani_stub.so")
    with open(src, "w") as f:
        f.write("".join("int lzani_%s(void) { return -3; }\n" % x for x in names))
    subprocess.check_call(["gcc", "-shared", "-fPIC", src, "-o", lib])
    return lib


def test_a_library_without_the_stage_is_refused_only_with_the_flag(host_binary, old_library, tmp_path):
    fa = str(tmp_path / "in.fa")
    SG.write_fasta(fa, *SG.make_set(4, 3, lmin=300, lmax=400, fam=2))
    args = [host_binary, "all2all", "--in-fasta", fa, "-o", str(tmp_path / "o.tsv"), "--flt-kmers", "16", "0.1"]
    env = dict(os.environ, LZANI_LIB=old_library)
    p = subprocess.run(args + ["--flt-kmers-max-seqs", "4"], capture_output=True, text=True, env=env)
    assert p.returncode != 0 and "Missing symbol lzani_prefilter_limit" in p.stderr, p.stderr
    p = subprocess.run(args, capture_output=True, text=True, env=env)              # the library is taken; its create then fails
    assert p.returncode != 0 and "Missing symbol" not in p.stderr and "lzani_create failed with code -3" in p.stderr, p.stderr
