"""CPU: the launch record of the pair kernels (lzani_debug_kernel_name) is complete.

Its names follow one grammar and equal the matrix tests/util.py writes from the dispatch rules; every k_pairs, k_pairs_blk and
k_split instance of the gfx950 code object in liblzani_hip.so has exactly one name and every name other than the run-time
compiled ones has a kernel; every name has a cell in tests/test_gpu_instantiations.py whose genome set, tuple, switches and call
lead the dispatch (as util.predict_kernels restates it) to that name.  An instantiation added without a name, or a name without
a cell, fails here."""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

import lzani_ctypes as L
import util as U

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SYM_RE = re.compile(r"^_ZN5lzani(7k_pairs|11k_pairs_blk|7k_split)I((?:L[bi]\d+E)+)EEvNS_\d+[A-Za-z]+")


@pytest.fixture(scope="module")
def names():
    L.build_library()
    return L.kernel_names()


def test_names_unique_follow_the_grammar_and_equal_the_dispatch_matrix(names):
    assert len(names) == len(set(names)), [k for k, v in collections.Counter(names).items() if v > 1]
    bad = [n for n in names if not re.match(U.KERNEL_NAME_RE, n)]
    assert not bad, bad
    want = U.expected_kernel_names()
    assert len(want) == len(set(want)) == 46
    assert set(names) == set(want), (sorted(set(names) - set(want)), sorted(set(want) - set(names)))
    lib = L.load_library()
    assert lib.lzani_debug_kernel_name(len(names)) is None and lib.lzani_debug_kernel_name(0xFFFFFFFF) is None
    assert lib.lzani_debug_kernel_launches(None, None, 0) == -1


def _symbol_name(kind, args):
    v = [int(x) for x in re.findall(r"L[bi](\d+)E", args)]
    if kind == "7k_pairs":
        assert len(v) == 6, args
        return U.PAIRS_NAME.format(*v)
    if kind == "11k_pairs_blk":
        assert len(v) == 2, args
        return "pairs_blk nfree={} defp={}".format(*v)
    assert len(v) == 3, args
    return "split nfree={} defp={} mode={}".format(*v)


def code_object_kernels(tmp_path):
    """Kernel symbols of the gfx950 code object in liblzani_hip.so: its offload bundle section, unbundled (the first bundle of the
    section is lzani_hip.hip's), then the symbol table."""
    bindir = os.path.join(ROCM, "llvm", "bin")
    fat, dev = str(tmp_path / "fatbin.bin"), str(tmp_path / "gfx950.o")
    subprocess.check_call([os.path.join(bindir, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, L.LIB_PATH,
                           str(tmp_path / "stripped.so")])
    subprocess.check_call([os.path.join(bindir, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + dev])
    syms = subprocess.check_output([os.path.join(bindir, "llvm-readelf"), "--syms", "--wide", dev], text=True)
    out = set()
    for line in syms.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC" and SYM_RE.match(f[7]):
            out.add(f[7])
    return out


def test_table_matches_the_code_object(names, tmp_path):
    syms = code_object_kernels(tmp_path)
    assert len(syms) >= 40, sorted(syms)
    mapped = collections.defaultdict(list)
    for s in syms:
        m = SYM_RE.match(s)
        mapped[_symbol_name(m.group(1), m.group(2))].append(s)
    unnamed = {k: v for k, v in mapped.items() if k not in names}
    assert not unnamed, f"kernels of the code object without a name in the launch record: {unnamed}"
    assert all(len(v) == 1 for v in mapped.values()), {k: v for k, v in mapped.items() if len(v) > 1}
    missing = [n for n in names if not n.startswith("rtc ") and n not in mapped]
    assert not missing, f"names without a kernel in the code object: {missing}"


def test_every_name_has_a_cell_that_reaches_it(names):
    cells = U.INST_CELLS
    assert len({c["id"] for c in cells}) == len(cells)
    covered = collections.Counter(c["name"] for c in cells)
    for n in names:
        if n.startswith("split ") and n.endswith("mode=1"):
            continue                                  # (a split cell runs both modes)
        assert covered[n] == (2 if n.startswith("rtc ") else 1), n
    for n in names:
        if n.startswith("rtc "):
            chain = [U.chain_params_ok(U.INST_PARAMS[c["prm"]]) for c in cells if c["name"] == n]
            assert sorted(chain) == [False, True], n
    for c in cells:
        prm = U.INST_PARAMS[c["prm"]]
        seqs = U.instantiation_set(c["set"])
        ref_ids, off, q = U.instantiation_rows(c, len(seqs))
        per_row = int(off[1] - off[0])
        assert all(int(off[k + 1] - off[k]) == per_row for k in range(len(ref_ids)))
        got = U.predict_kernels(seqs, prm, c["env"], c["form"], pairs_per_row=per_row, n_rows=len(ref_ids),
                                rtc_ready=c["name"].startswith("rtc "))
        assert got == U.kernel_names_of_cell(c), (c["id"], got)
        nf = int("nfree=1" in c["name"])
        if "nfree=" in c["name"]:
            assert nf == int(all((s < 4).all() for s in seqs)), c["id"]
        assert any(len(s) <= 500 for s in seqs), c["id"]


def test_sets_hold_what_the_cells_need():
    """N runs at the start, in the middle and at the end, N-free genomes beside them, a pair with N on both sides."""
    for name in ("small N", "split N", "mid N", "long N"):
        seqs = U.instantiation_set(name)
        hasn = [bool((s > 3).any()) for s in seqs]
        assert any(s[0] > 3 for s in seqs) and any(s[-1] > 3 for s in seqs), name
        assert any((s[len(s) // 4:-len(s) // 4] > 3).any() for s in seqs), name
        assert sum(hasn) >= 2 and hasn.count(False) >= 2, name
    for name in ("small", "split", "mid", "long"):
        assert all((s < 4).all() for s in U.instantiation_set(name)), name
    assert max(len(s) for s in U.instantiation_set("split")) >= 20_000
    assert U.index_form(U.instantiation_set("long"), U.INST_PARAMS["long"])["tag_words"]
    assert U.index_form(U.instantiation_set("mid"), U.INST_PARAMS["rtc_chain"])["tag_words"]
    assert U.index_form(U.instantiation_set("small"), U.INST_PARAMS["defaults"])["tag_words"]
