"""CPU: which lines of lzani_core.h -- the machine the kernels and the host model share -- the suite's own inputs execute.

tests/model/lzani_model.cpp is built with g++ -O0 --coverage into a temporary directory; a child process (this file run as a
program) calls every entry point of the model the suite uses over the named genome sets and the tuples of util.INST_PARAMS;
gcov -b, run beside the sources, gives the counts.  A source line of lzani_core.h is reached if any instantiation executed
it.  Every executable line must be reached or be listed in tests/golden/core_unreached.txt, keyed by its enclosing function
and its stripped text (not its number) with a reason; a line that is newly unreached fails, and so does a stale entry.
`python tests/test_core_coverage.py --list` prints the unreached lines in the file's format (reason left open)."""
import collections
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODEL_DIR = os.path.join(HERE, "model")
CORE_H = os.path.join(ROOT, "lz-ani_amd", "csrc", "lzani_core.h")
UNREACHED = os.path.join(HERE, "golden", "core_unreached.txt")
SPLIT_TUPLES = ("defaults", "generic", "long")
REPAIR_CASES = (("wide", 85), ("generic", 46), ("generic", 16419), ("defaults", 2144), ("long", 3108))    # of util.SPLIT_REPAIR_TABLE: voids of every cause
REGION_PAIRS = ((0, 1), (1, 0), (0, 2), (3, 0), (0, 4), (12, 0), (0, 12), (13, 0), (7, 0), (0, 9))    # of util.edge_set()


def named_sets(with_exit_sets=True):
    import repeat_genomes as RG
    import util as U
    sets = {"edge": U.edge_set(), "small": U.instantiation_set("small"), "small N": U.instantiation_set("small N"),
            "split N[:5]": U.instantiation_set("split N")[:5], "family N": U.envelope_family_set(True),
            "family": U.envelope_family_set(False)}
    if with_exit_sets:
        sets.update({name: RG.exit_set(name) for name in RG.EXIT_SET_NAMES})
    return sets


def drive(so, with_exit_sets=True):
    """Every model entry point the suite uses, over the named sets and the tuples (the child: the counts are written at exit)."""
    import ctypes as C
    import numpy as np
    import oracle as O
    import util as U
    U._model = C.CDLL(so)
    lib = U._model
    for setname, seqs in named_sets(with_exit_sets).items():
        s, ptrs, lens = O._seq_table(seqs)
        n = len(s)
        for pn, prm in U.INST_PARAMS.items():
            want = U.model_all2all(seqs, prm)
            out = np.zeros((n, n, 3), dtype=np.int32)
            if lib.model_queue_all2all(n, ptrs, O._ptr(lens), O.params_array(prm), O._ptr(out)) == 0:
                assert np.array_equal(out, want), (setname, pn, "queue")
            for words in (0, 1):
                assert lib.model_lane_all2all(n, ptrs, O._ptr(lens), O.params_array(prm), words, O._ptr(out)) == 0
                assert np.array_equal(out, want), (setname, pn, "lane", words)
            if pn in SPLIT_TUPLES:
                for seglen in (1000, 3000):
                    assert np.array_equal(U.model_split_all2all(seqs, prm, seglen=seglen)[0], want), (setname, pn, "split", seglen)
                if setname != "edge":
                    assert np.array_equal(U.model_split_rounds(seqs, prm, seglen=512)[0], want), (setname, pn, "rounds")
                    assert np.array_equal(U.model_split_rounds(seqs, prm, seglen=512, give_up=1)[0], want), (setname, pn, "give up")
            pairs = REGION_PAIRS if setname == "edge" else ((0, 1), (1, 0), (0, n - 1))
            for r, q in pairs:
                assert tuple(int(x) for x in want[r, q]) == U.model_pair_regions(seqs[r], seqs[q], prm)[0], (setname, pn, r, q)
        # the index and the k-mer words of the set's first genomes; the two forms of the null-extension record
        maxlen = max(len(x) for x in seqs)
        for g in seqs[:3]:
            for pn in ("defaults", "long", "slow"):
                prm = U.INST_PARAMS[pn]
                n_ent = C.c_uint32(0)
                assert lib.model_index(O._ptr(g), len(g), maxlen, O.params_array(prm), None, None, None, None, C.byref(n_ent)) == 0
                T = 2 * len(g) + 3 * prm["mrd"]
                valid, h = np.zeros(T, np.uint8), np.zeros(T, np.uint64)
                for k in (prm["msl"], prm["mal"]):
                    assert lib.model_kmers(O._ptr(g), C.c_uint32(len(g)), O.params_array(prm), C.c_int32(k), O._ptr(valid), O._ptr(h)) == 0
        r, q = seqs[0], seqs[1]
        if len(r) > 100 and len(q) > 100:
            for prm in (U.INST_PARAMS["defaults"], U.INST_PARAMS["generic"], dict(U.DEFAULTS, aw=7, am=6, ar=3, mrd=25)):
                T = 2 * len(r) + 3 * prm["mrd"]
                k = np.arange(3000, dtype=np.int64)
                qp = ((k * 7919) % (len(q) + prm["mrd"])).astype(np.int32)
                rp = ((k * 104729) % T).astype(np.int32)
                al = (k % 41).astype(np.int32)
                assert lib.model_ext_records_agree(O._ptr(r), len(r), O._ptr(q), len(q), O.params_array(prm), len(k), O._ptr(qp), O._ptr(rp), O._ptr(al)) == 0


    # the split's repair loop: cases of util.SPLIT_REPAIR_TABLE (void segments, resumed segments, a pair given up)
    for cls, seed in REPAIR_CASES:
        prm, seqs = U.split_repair_case(cls, seed)
        want = U.model_all2all(seqs, prm)
        for give_up in (-1, 1):
            assert np.array_equal(U.model_split_rounds(seqs, prm, seglen=512, give_up=give_up)[0], want), (cls, seed, give_up)


# ---- the counts ------------------------------------------------------------------------------------------------------------
def build_and_run(tmp, with_exit_sets=True):
    so = os.path.join(tmp, "liblzani_model_cov.so")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "--coverage", "-fPIC", "-shared", "-ffp-contract=off",
                           os.path.join(MODEL_DIR, "lzani_model.cpp"), "-o", so], cwd=tmp)
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--drive", so, "1" if with_exit_sets else "0"], cwd=tmp)
    gcno = [f for f in os.listdir(tmp) if f.endswith(".gcno")]
    assert len(gcno) == 1, gcno
    # (beside the sources: from elsewhere gcov does not find the headers the unit includes by relative path)
    out = subprocess.run(["gcov", "-b", "-m", "--json-format", "--stdout", os.path.join(tmp, gcno[0])], cwd=MODEL_DIR,
                         stdout=subprocess.PIPE, check=True).stdout
    return json.loads(out)


def simple_name(demangled):
    """lzani::PairMachine<lzani::HostWave, false>::run(int*) -> PairMachine::run"""
    s, depth, out = demangled, 0, []
    for ch in s:
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif depth == 0:
            out.append(ch)
    s = "".join(out)
    s = s.split("(")[0].strip()
    s = s.split(" ")[-1]                       # (a return type before the name)
    return s.replace("lzani::", "").replace("(anonymous namespace)::", "")


def core_lines(report):
    """{line number: (reached, function, branches taken, branches)} of lzani_core.h, any instantiation."""
    files = [f for f in report["files"] if os.path.basename(f["file"]) == "lzani_core.h"]
    assert len(files) == 1, [f["file"] for f in report["files"]]
    f = files[0]
    names = {fn["name"]: simple_name(fn["demangled_name"]) for fn in f["functions"]}
    lines = {}
    for ln in f["lines"]:
        k = ln["line_number"]
        fn = names.get(ln.get("function_name"), "?")
        br = ln.get("branches", [])
        if k not in lines:
            lines[k] = [False, fn, [False] * len(br)]
        e = lines[k]
        e[0] = e[0] or ln["count"] > 0
        if len(e[2]) < len(br):
            e[2] += [False] * (len(br) - len(e[2]))
        for j, b in enumerate(br):
            e[2][j] = e[2][j] or b["count"] > 0
    return lines


def summary(lines):
    n = len(lines)
    hit = sum(1 for e in lines.values() if e[0])
    br = sum(len(e[2]) for e in lines.values())
    taken = sum(sum(e[2]) for e in lines.values())
    return {"lines": n, "lines_reached": hit, "line_pct": round(100.0 * hit / n, 1), "branches": br, "branches_taken": taken,
            "branch_pct": round(100.0 * taken / br, 1)}


def unreached_keys(lines):
    """[(function, stripped text)] of the unreached lines, in text order, each key once."""
    with open(CORE_H) as f:
        text = f.read().split("\n")
    out = []
    for k in sorted(lines):
        if not lines[k][0]:
            key = (lines[k][1], text[k - 1].strip())
            if key not in out:
                out.append(key)
    return out


def listed():
    """{(function, stripped text): reason} of tests/golden/core_unreached.txt: function <TAB> text <TAB> reason per line."""
    out = collections.OrderedDict()
    with open(UNREACHED) as f:
        for ln in f:
            ln = ln.rstrip("\n")
            if not ln or ln.startswith("#"):
                continue
            fn, text, reason = ln.split("\t")
            assert reason.strip() and (fn, text) not in out, ln
            out[(fn, text)] = reason
    return out


def test_every_line_of_the_core_is_reached_or_listed():
    with tempfile.TemporaryDirectory() as tmp:
        lines = core_lines(build_and_run(tmp))
    s = summary(lines)
    print(s)
    assert s["lines"] >= 500, s                                   # (the header's machine is there: not an empty report)
    missing = unreached_keys(lines)
    known = listed()
    new = [k for k in missing if k not in known]
    stale = [k for k in known if k not in missing]
    assert not new, "unreached and not listed in tests/golden/core_unreached.txt: {}".format(new)
    assert not stale, "listed in tests/golden/core_unreached.txt but reached (or gone): {}".format(stale)


if __name__ == "__main__":
    for _p in ("lz-ani_amd", "oracle", "tools", "tests"):
        sys.path.insert(0, os.path.join(ROOT, _p))
    if sys.argv[1] == "--drive":
        drive(sys.argv[2], sys.argv[3] == "1")
    else:                                                          # --list [0: without the exit sets]
        with tempfile.TemporaryDirectory() as tmp:
            lines = core_lines(build_and_run(tmp, with_exit_sets=sys.argv[2:3] != ["0"]))
        print("#", summary(lines))
        for fn, text in unreached_keys(lines):
            print("{}\t{}\t".format(fn, text))
