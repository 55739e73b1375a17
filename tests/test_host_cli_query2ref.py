"""The mode `lz-ani query2ref` of the host binary, on the CPU: the queries of one set of files against the references of
another, fed the matching stage's integers through --results-in (oracle numbers, listed by the mode's ids: the references
in their reordered order, then the queries in theirs)."""
import os
import subprocess

import pytest

import oracle as O
import util as U

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
EXAMPLE = os.path.join(U.GOLD, "example", "multifasta.fna")
N_REF_RECORDS = 5                                       # the first records of the example are the references, the rest the queries:
                                                        # a split inside a family of related genomes (records 4 .. 6)
INDEX_FREE = "query,reference,qlen,rlen,tani,gani,ani,qcov,rcov,len_ratio,nt_match,nt_mismatch,num_alns"


@pytest.fixture(scope="module", autouse=True)
def build_host():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])


def run(args, **kw):
    return subprocess.run([EXE] + args, capture_output=True, text=True, **kw)


def split_example(tmp_path):
    """The example's records as they lie in the file, the first N_REF_RECORDS into ref.fna and the rest into qry.fna."""
    recs = [b">" + r for r in open(EXAMPLE, "rb").read().split(b">")[1:]]
    ref, qry = str(tmp_path / "ref.fna"), str(tmp_path / "qry.fna")
    open(ref, "wb").write(b"".join(recs[:N_REF_RECORDS]))
    open(qry, "wb").write(b"".join(recs[N_REF_RECORDS:]))
    return ref, qry


def mode_order():
    """(names, seqs, n_ref) in the mode's ids: each side reordered on its own, references first."""
    names, seqs = U.load_example()
    rn, rs = U.reorder(names[:N_REF_RECORDS], seqs[:N_REF_RECORDS])
    qn, qs = U.reorder(names[N_REF_RECORDS:], seqs[N_REF_RECORDS:])
    return rn + qn, rs + qs, len(rn)


def cross_lines(path, ref_names):
    """The lines of an index-free TSV whose two names lie on different sides, sorted."""
    lines = open(path).read().split("\n")[1:]
    return sorted(ln for ln in lines if ln and (ln.split("\t")[0] in ref_names) != (ln.split("\t")[1] in ref_names))


@pytest.fixture(scope="module")
def example():
    names, seqs, n_ref = mode_order()
    assert 0 < n_ref < len(names) == 12
    return names, seqs, n_ref, O.oracle_all2all(seqs, None, threads=8)


def _raw_cross(path, res, n_ref):
    n = res.shape[0]
    with open(path, "w") as f:
        for r in range(n):
            for q in range(n):
                if (r < n_ref) != (q < n_ref):
                    f.write(f"{r} {q} {res[r, q, 0]} {res[r, q, 1]} {res[r, q, 2]}\n")


def test_query2ref_gives_the_cross_lines_of_all2all(tmp_path, example):
    names, seqs, n_ref, res = example
    ref, qry = split_example(tmp_path)
    raw = str(tmp_path / "raw.txt")
    _raw_cross(raw, res, n_ref)
    out = str(tmp_path / "q2r.tsv")
    p = run(["query2ref", "--in-fasta", ref, "--query-fasta", qry, "-o", out, "--results-in", raw, "--out-format", INDEX_FREE])
    assert p.returncode == 0, p.stderr
    # all2all on the whole file, fed the oracle's numbers in its own (whole-set) order
    an, aseqs = U.reorder(*U.load_example())
    ares = O.oracle_all2all(aseqs, None, threads=8)
    araw = str(tmp_path / "all.raw")
    with open(araw, "w") as f:
        for r in range(len(an)):
            for q in range(len(an)):
                if r != q:
                    f.write(f"{r} {q} {ares[r, q, 0]} {ares[r, q, 1]} {ares[r, q, 2]}\n")
    aout = str(tmp_path / "all.tsv")
    assert run(["all2all", "--in-fasta", EXAMPLE, "-o", aout, "--results-in", araw, "--out-format", INDEX_FREE]).returncode == 0
    ref_names = set(names[:n_ref])
    got = sorted(ln for ln in open(out).read().split("\n")[1:] if ln)
    want = cross_lines(aout, ref_names)
    assert got == want and len(got) == 2 * n_ref * (len(names) - n_ref)
    assert got == cross_lines(out, ref_names)                                   # (nothing but cross lines)


def test_query2ref_ids_follow_the_ids_file(tmp_path, example):
    names, seqs, n_ref, res = example
    ref, qry = split_example(tmp_path)
    raw = str(tmp_path / "raw.txt")
    _raw_cross(raw, res, n_ref)
    out, ids = str(tmp_path / "std.tsv"), str(tmp_path / "my.ids.tsv")
    p = run(["query2ref", "--in-fasta", ref, "--query-fasta", qry, "-o", out, "--results-in", raw, "--out-ids", ids,
             "--out-format", "standard,reference"])
    assert p.returncode == 0, p.stderr
    id_rows = [ln.split("\t") for ln in open(ids).read().split("\n")[1:] if ln]
    assert [r[0] for r in id_rows] == names and [int(r[1]) for r in id_rows] == [len(s) for s in seqs]
    rows = [ln.split("\t") for ln in open(out).read().split("\n")[1:] if ln]
    assert len(rows) == 2 * n_ref * (len(names) - n_ref)
    for r in rows:                                      # qidx, ridx, query, reference, ...
        q, ref_id = int(r[0]), int(r[1])
        assert names[q] == r[2] and names[ref_id] == r[3]
        assert (q < n_ref) != (ref_id < n_ref)
    assert open(out).read() == _expected_standard(names, [len(s) for s in seqs], res, n_ref)


def _expected_standard(names, lens, res, n_ref):
    """emit_tsv's lines of the cross pairs, in its order (reference rows ascending, their partners ascending)."""
    cols = U.STANDARD + ["reference"]
    full = U.emit_tsv(names, lens, res, cols).split("\n")
    keep = [full[0]] + [ln for ln in full[1:] if ln and (int(ln.split("\t")[0]) < n_ref) != (int(ln.split("\t")[1]) < n_ref)]
    return "\n".join(keep) + "\n"


def test_query2ref_refusals(tmp_path):
    ref, qry = split_example(tmp_path)
    out = str(tmp_path / "o.tsv")
    p = run(["query2ref", "--in-fasta", ref, "--query-fasta", qry, "-o", out, "--flt-kmerdb", os.path.join(U.GOLD, "example", "fltr.txt"), "0.9"])
    assert p.returncode == 1 and "--flt-kmerdb" in p.stderr
    p = run(["all2all", "--in-fasta", ref, "--query-fasta", qry, "-o", out])
    assert p.returncode == 1 and "query2ref" in p.stderr
    p = run(["query2ref", "--in-fasta", ref, "-o", out])
    assert p.returncode == 1 and "Query" in p.stderr
    assert not os.path.exists(out)
