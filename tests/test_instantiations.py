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
import path_cover as PC
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


# ---- the counters of the diagnostic builds (tests/path_cover.py, tests/test_gpu_path_cover.py) ---------------------------
def _text(path):
    with open(path) as f:
        return f.read()


def test_counter_slots_are_the_headers():
    """The slot tables tests/test_gpu_path_cover.py goes by are the header's, number by number, and the statements that count
    use the numbers the tables name: a renumbered slot fails here, not on the GPU."""
    pairs = _text(PC.PAIRS_H)
    assert PC.header_slots(pairs, "LZ_PATH_SLOTS") == list(enumerate(PC.PATH_SLOTS))
    assert PC.header_slots(pairs, "LZ_CHAIN_SLOTS") == list(enumerate(PC.CHAIN_SLOTS))
    assert "unsigned ps[24] = {0};" in pairs and "unsigned pw[12] = {0};" in pairs and "unsigned st[8]" in pairs and "unsigned sw[8]" in pairs
    hip = _text(os.path.join(os.path.dirname(PC.PAIRS_H), "lzani_hip.hip"))
    assert "g_path_stats[{}];".format(len(PC.PATH_SLOTS)) in hip and "g_chain_stats[{}];".format(len(PC.CHAIN_SLOTS)) in hip
    for path, lines in PC.COUNTING_TEXT.items():
        text = _text(path)
        for line in lines:
            assert text.count(line) == 1, (os.path.basename(path), line, text.count(line))
    count = lambda rx: dict(collections.Counter(int(k) for k in re.findall(rx, pairs)))
    assert count(r"\bLZ_PS\((\d+)\)") == PC.LZ_PS_SITES
    assert count(r"\bLZ_NC_WHY\((\d+)\)") == PC.LZ_NC_WHY_SITES
    assert count(r"\bLZ_SC_WHY\((\d+)\)") == PC.LZ_SC_WHY_SITES
    assert re.findall(r"\bLZ_PSN\((\d+),", pairs) == ["23"]
    # every required slot is one the tables name, and has a name
    for s in PC.REQUIRED:
        vec, k, label = PC.slot(*s)
        assert (PC.PATH_SLOTS if vec == "paths" else PC.CHAIN_SLOTS)[k] != "-", label


def test_coverage_cells_select_their_class():
    """Every chain class has its cells, every cell's set, tuple and switches lead the dispatch (util.predict_kernels) to the
    class's kernel, and every exit set is some class's."""
    cells = PC.cells()
    assert len({c["id"] for c in cells}) == len(cells)
    for cls in PC.CLASSES:
        t, nf, form = cls
        mine = [c for c in cells if c["class"] == cls]
        assert len(mine) >= 2, cls
        d = {"defaults": 1, "long": 2}[t]
        if form == "split":
            want = {"split nfree={} defp={} mode={}".format(nf, d, m) for m in (0, 1)}
        elif form == "probe":
            want = {U.PAIRS_NAME.format(1, nf, d if d == 1 else 0, 0, 1, 0)}          # (the long tuple runs generic there)
        else:
            want = {U.PAIRS_NAME.format(1, nf, d, 0, 1, {"bitmaps": 2, "join": 1}[form])}
        for c in mine:
            assert c["kernels"] == want and c["env"]["LZANI_RTC"] == "0", (c["id"], c["kernels"])
    import repeat_genomes as RG
    assert {c["set"] for c in cells if c["set"].startswith("exits")} == set(RG.EXIT_SET_NAMES)


def test_parse_raw_sums_the_runs():
    text = ("[lzani paths] pairs=2, per pair: x=1.0;\n[lzani paths raw]" + " 1" * 36 + "\n[lzani chain raw]" + " 2" * 24 + "\n"
            "noise\n[lzani paths raw]" + " 3" * 36 + "\n")
    assert PC.parse_raw(text) == {"paths": [4] * 36, "chain": [2] * 24}
