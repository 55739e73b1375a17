"""GPU: the stages of lzani_group_run_rows (lzani_multi.h) at the smallest shapes at which they can go wrong -- empty
shards, empty rows, no rows at all, the group's buffers and events reused and grown from call to call -- against a single
context on the same rows, and the --out-alignment shards of the host binary on a device list.  Rehearsals on one GPU:
the group lists device 0 three times (shards move by device copies)."""
import os
import subprocess

import numpy as np
import pytest

import lzani_ctypes as L
import synth_genomes as SG
import util as U

pytestmark = pytest.mark.gpu

EXE = os.path.join(U.ROOT, "lz-ani_amd", "host", "lz-ani")
ZERO = ("index_ms", "pairs_ms", "pair_launches", "pairs", "cand_ms", "kmers_ms")      # a device's own figures in Group.timing


def test_group_stages_on_small_shapes():
    seqs = SG.make_set(5, 23, lmin=2000, lmax=4000, fam=3)[1]
    seqs += [np.full(2500, 5, dtype=np.uint8), np.zeros(0, np.uint8)]                 # all N; empty (a row of it costs nothing)
    n, lens, z = len(seqs), [len(s) for s in seqs], len(seqs) - 1
    eng = L.Engine()
    eng.set_genomes(seqs)
    grp = L.Group(None, (0, 0, 0))
    grp.set_genomes(seqs)

    def dense(rows):
        ref, off = L.dense_rows(n, rows)
        return ref, off, None, np.arange(len(rows)) % 3                               # the cyclic deal

    def lists(rows):
        ref = np.array([r for r, _ in rows], dtype=np.uint32)
        off = np.cumsum([0] + [len(q) for _, q in rows]).astype(np.uint64)
        q = np.array([x for _, qs in rows for x in qs], dtype=np.uint32)
        return ref, off, q, L.partition_rows(len(ref), 3, L.row_costs(ref, off, q, lens))

    def check(ref, off, q, part, want_part=None):
        if want_part is not None:
            assert part.tolist() == want_part
        got = grp.run_rows(ref, off, q)
        assert np.array_equal(got, eng.run_rows(ref, off, q))
        sizes = np.diff(off.astype(np.int64))
        for d in range(3):
            t = grp.timing(d)
            if not (part == d).any():
                assert all(t[k] == 0 for k in ZERO), (d, t)
            assert t["pairs"] == sizes[part == d].sum()
            assert (t["gather_ms"] > 0) == (len(ref) > 0)
        return got

    two = check(*dense([0, 1]))                                 # the third shard is empty; the group's buffers and events are made
    assert two.shape == (2 * (n - 1), 3) and two.any()
    assert np.array_equal(check(*dense([0, 1])), two)           # ... and used again
    check(*dense([3]))                                          # one row: two empty shards
    assert check(*dense([])).shape == (0, 3)                    # no rows: nothing runs, every figure is zero
    check(*lists([(0, [1, 2]), (4, []), (2, [0, 5, 3])]))       # an empty list between two others
    check(*lists([(1, [0, 2, 3]), (z, []), (z, [])]), want_part=[0, 1, 1])     # LPT: two rows on one shard, none on another
    four = lists([(0, [1, 2, 3, 4]), (1, [0]), (5, [2, 3]), (2, [4])])
    assert np.bincount(four[3], minlength=3).max() == 2         # ragged lists, two of them on one shard
    check(*four)
    full = check(*dense(list(range(n))))                        # more pairs than before: d_all / d_final grow
    assert np.array_equal(full[:2 * (n - 1)], two)
    assert np.array_equal(check(*dense([0, 1])), two)           # a small call in the grown buffers
    grp.close()
    eng.close()


def test_out_alignment_shards_on_a_device_list(tmp_path):
    """`lz-ani --out-alignment --gpus 2` takes its devices from LZANI_DEVICE_LIST like the group does: two shards on GPU 0
    write the same bytes as one."""
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE)])
    fa = os.path.join(U.GOLD, "example", "multifasta.fna")
    env = {k: v for k, v in os.environ.items() if k != "LZANI_DEVICE_LIST"}
    files = {}
    for tag, extra, e in (("one", ["--gpus", "1"], env), ("two", ["--gpus", "2"], dict(env, LZANI_DEVICE_LIST="0,0"))):
        out, aln = str(tmp_path / f"{tag}.tsv"), str(tmp_path / f"{tag}.aln.tsv")
        p = subprocess.run([EXE, "all2all", "--in-fasta", fa, "-o", out, "--out-alignment", aln, "-V", "2"] + extra,
                           capture_output=True, text=True, env=e)
        assert p.returncode == 0, p.stderr[-800:]
        assert p.stderr.count("GPU 0:") == (2 if tag == "two" else 1), p.stderr[-600:]
        files[tag] = (open(out, "rb").read(), open(aln, "rb").read())
    assert files["one"] == files["two"]
    assert files["one"][0] == open(os.path.join(U.GOLD, "example", "ani.tsv"), "rb").read() and len(files["one"][1]) > 1000
