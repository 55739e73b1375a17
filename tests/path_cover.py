"""Which exits of the pair kernel's hand-written loops the oracle-compared cells take: the cells, the slot tables, the child.

The coverage library (lzani_ctypes.build_diag_library: -DLZANI_PATH_STATS -DLZANI_CHAIN_STATS) counts per wave how find_event
found its events (LZ_PS), how the null chain left (st, sr, sw) and how the stretch chain left (pw), and report_diagnostics
prints the totals of every run as two lines of raw 64-bit numbers.  lzani_ctypes reads LZANI_LIB at import, so the counting
runs are a child's: `python tests/path_cover.py TUPLE [CELL ...]` with LZANI_LIB set runs the tuple's cells -- all of them, or
the ones named as 'form,NFREE|N,set name' -- through tests/inst_cell.py's run_cell (the cell's switches, the launch record and
the oracle as in tests/test_gpu_instantiations.py; LZANI_RTC=0) and prints one JSON line per cell: its id, the kernels
launched, the digest of the result array, whether run_cell's assertions held, and the two counter vectors.
tests/test_gpu_path_cover.py starts one child per tuple and asserts on the lines.

The slot names live next to the counters (lzani_kernels_pairs.h: LZ_PATH_SLOTS, LZ_CHAIN_SLOTS); PATH_SLOTS and CHAIN_SLOTS
below restate them by number, and tests/test_instantiations.py checks the two against each other, and the counting
statements of the header against COUNTING_TEXT, without a GPU: a renumbered slot fails there.

A chain class is (tuple defaults | long) x (NFREE | N) x (bitmaps | join | probe | split); REQUIRED are the slots that must
be non-zero in the union of a class's cells unless CANNOT_OCCUR says why the class cannot count them."""
import contextlib
import json
import os
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PAIRS_H = os.path.join(ROOT, "lz-ani_amd", "csrc", "lzani_kernels_pairs.h")
SPLIT_H = os.path.join(ROOT, "lz-ani_amd", "csrc", "lzani_kernels_split.h")

PATH_SLOTS = (
    "find_event calls", "fe: seed straight from the chain's round", "fe: common call, plain candidate", "fe: light rounds",
    "fe: light round hit", "fe: light round without a hit", "fe: merge loop hit", "fe: jump to a plain candidate",
    "stretch calls", "stretch: not applicable", "stretch: no seed step", "stretch: anchor before the seed",
    "stretch: seed event", "stretch: ... with the masks", "stretch: sum of seed steps",
    "refills", "chain: nothing", "chain: round done", "chain: event found", "chain: seed event known",
    "events", "close events", "extension chunks", "stretch chain: events committed",
    "-", "text end", "no seed step", "several window positions", "seed bounds", "match of 64+",
    "anchor before the seed", "tag in two slots / overflow", "anchor elsewhere", "extension runs on", "-", "-")
CHAIN_SLOTS = (
    "chain_calls", "commits", "exit_nothing", "exit_seed", "exit_not_plain", "exit_event", "events_general", "refills",
    "cycles after exit_nothing", "cycles after round_done", "cycles after exit_event", "cycles inside the chain",
    "not null: close", "not null: region kept or none open", "not null: no forward record", "not null: backward side",
    "exit_seed: anchor's own step", "exit_seed: no window position", "exit_seed: several", "exit_seed: text end",
    "exit_seed: long seed", "exit_seed: other", "event known, commit left", "-")
# The statements that count, as the header writes them: where a slot number is used, not only where it is named.
COUNTING_TEXT = {
    PAIRS_H: (
        "for (int k = 0; k < 24; ++k) atomicAdd(&g[k], ln == 0 ? (unsigned long long)ps[k] : 0ULL);",
        "for (int k = 0; k < 12; ++k) atomicAdd(&g[24 + k], ln == 0 ? (unsigned long long)pw[k] : 0ULL);",
        "for (int k = 0; k < 8; ++k) atomicAdd(&g[k], ln == 0 ? (unsigned long long)st[k] : 0ULL);",
        "for (int k = 0; k < 4; ++k) atomicAdd(&g[8 + k], ln == 0 ? stc[k] : 0ULL);",
        "for (int k = 0; k < 4; ++k) atomicAdd(&g[12 + k], ln == 0 ? (unsigned long long)sr[k] : 0ULL);",
        "for (int k = 0; k < 8; ++k) atomicAdd(&g[16 + k], ln == 0 ? (unsigned long long)sw[k] : 0ULL);",
        "if (code == 0) LZ_PS(16); else if (code == 1) LZ_PS(17); else if (code == 2) LZ_PS(18); else LZ_PS(19);",
        "st[0] += 1; st[1] += ncnt; st[2] += code == 0; st[3] += code == 1 && seed != 0; st[4] += code == 1 && seed == 0; st[5] += code == 2;",
        "sr[0] += close; sr[1] += !close && kept; sr[2] += !close && !kept && nofwd; sr[3] += !close && !kept && !nofwd;",
        "sw[0] += why == 1; sw[2] += why == 2; sw[3] += why == 3; sw[4] += why == 4; sw[5] += why == 0;",
        "if (code == 4) sw[6] += 1;",
        "pw[why < 12 ? why : 0] += 1;",
        "LZ_PSN(23, ncm);",
        "w.flush_path_stats(g_path_stats, lane);",
        "w.flush_chain_stats(g_chain_stats, lane);"),
    SPLIT_H: ("w.flush_path_stats(g_path_stats, lane);", "w.flush_chain_stats(g_chain_stats, lane);"),
}
LZ_PS_SITES = {0: 1, 1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 6: 1, 7: 1, 15: 1, 16: 1, 17: 1, 18: 1, 19: 1}     # LZ_PS(k): uses in the header
LZ_NC_WHY_SITES = {1: 1, 2: 1, 3: 1, 4: 1, 5: 1}            # the null chain's LZ_NC_WHY(n): n is what sw[] goes by
LZ_SC_WHY_SITES = {1: 2, 2: 3, 3: 1, 4: 1, 5: 1, 6: 1, 7: 2, 8: 2, 9: 2, 10: 1}       # the stretch chain's LZ_SC_WHY(n): pw[n]


def header_slots(text, macro):
    """[(number, name)] of the X(number, "name") entries of a slot list macro of the header."""
    m = re.search(r"#define " + macro + r"\(X\)((?:[^\n]*\\\n)*[^\n]*)\n", text)
    assert m, macro
    return [(int(k), n) for k, n in re.findall(r'X\((\d+), "([^"]*)"\)', m.group(1))]


def slot(kind, k):
    """(vector, index, label) of a counter by the header's own name for it: slot("ps", 5), slot("sw", 2) ..."""
    vec, base, names = {"ps": ("paths", 0, PATH_SLOTS), "pw": ("paths", 24, PATH_SLOTS), "st": ("chain", 0, CHAIN_SLOTS),
                        "sr": ("chain", 12, CHAIN_SLOTS), "sw": ("chain", 16, CHAIN_SLOTS)}[kind]
    label = ("LZ_PS({})" if kind == "ps" else kind + "[{}]").format(k) + " '" + names[base + k] + "'"
    return vec, base + k, label


REQUIRED = ([("ps", k) for k in (0, 1, 2, 3, 4, 5, 6, 7, 15, 16, 17, 18, 19, 23)] + [("pw", k) for k in range(1, 10)] +
            [("st", k) for k in range(2, 7)] + [("sr", k) for k in range(4)] + [("sw", k) for k in (0, 2, 3, 4, 5, 6)])
TUPLES, FORMS = ("defaults", "long"), ("bitmaps", "join", "probe", "split")
CLASSES = [(t, nf, f) for t in TUPLES for nf in (1, 0) for f in FORMS]


def class_name(cls):
    return "{} {} {}".format(cls[0], "NFREE" if cls[1] else "N", cls[2])


# ---- the genome sets ------------------------------------------------------------------------------------------------------
def genome_set(name):
    """A cell's genome set by name: util.instantiation_set's names, 'repeat ' + a name of repeat_genomes.repeat_set, or one
    of repeat_genomes.EXIT_SET_NAMES (the pairs laid out for single exits)."""
    import repeat_genomes as RG
    import util as U
    if name.startswith("repeat "):
        return RG.repeat_set(name[len("repeat "):])
    if name in RG.EXIT_SET_NAMES:
        return RG.exit_set(name)
    return U.instantiation_set(name)


# ---- the cells -----------------------------------------------------------------------------------------------------------
def _sets_of(tuple_name, nf, form):
    """The genome sets of a class: the set of its instantiation cell (util.INST_CELLS), that set's repeat-structured
    counterpart and the exit set (repeat_genomes.exit_set; not where the two long sets reach everything by themselves).  The join and probe forms of the long tuple need tag words at mal 15 (without them find_event is
    find_event_round: no LZ_PS at all), which only the sets with the genome of 2.2 Mbp have."""
    suf = "" if nf else " N"
    if tuple_name == "long":
        base = {"bitmaps": "split", "split": "split", "join": "long", "probe": "long"}[form]
    else:
        base = "split" if form == "split" else "small"
    if base == "long":
        return [base + suf, "repeat " + base + suf]
    return [base + suf, "repeat " + base + suf, "exits" + suf]


_CELLS = []


def cells():
    """Every cell of the coverage run: dicts as util.INST_CELLS holds them (id, name, set, prm, env, form) plus "class" and
    "kernels" (what the launch record must hold: util.predict_kernels)."""
    import util as U
    if _CELLS:
        return _CELLS
    out = _CELLS
    for cls in CLASSES:
        t, nf, form = cls
        for setname in _sets_of(*cls):
            env = dict(U._INST_FORM_ENV[form], LZANI_RTC="0")
            if t == "long" and form == "probe":
                env["LZANI_NO_JOIN"] = "1"                      # (a set with tag words and a directory this large joins)
            seqs = genome_set(setname)
            names = U.predict_kernels(seqs, U.INST_PARAMS[t], env, "all2all")
            out.append({"id": "{} | {}".format(class_name(cls), setname), "class": cls, "name": sorted(names)[0], "kernels": set(names),
                        "set": setname, "prm": t, "env": env, "form": "all2all"})
    return out


# ---- the child -------------------------------------------------------------------------------------------------------------
RAW_RE = re.compile(r"^\[lzani (paths|chain) raw\]((?: \d+)+)\s*$", re.M)


def parse_raw(text):
    """{"paths": [36 totals], "chain": [24 totals]} summed over the runs whose stderr text holds."""
    acc = {"paths": [0] * len(PATH_SLOTS), "chain": [0] * len(CHAIN_SLOTS)}
    for kind, nums in RAW_RE.findall(text):
        v = [int(x) for x in nums.split()]
        assert len(v) == len(acc[kind]), (kind, len(v))
        acc[kind] = [a + b for a, b in zip(acc[kind], v)]
    return acc


@contextlib.contextmanager
def _stderr_to(path):
    """The process's file descriptor 2 into a file for the block: the library prints with fprintf(stderr)."""
    sys.stderr.flush()
    keep = os.dup(2)
    with open(path, "wb") as f:
        os.dup2(f.fileno(), 2)
        try:
            yield
        finally:
            sys.stderr.flush()
            os.dup2(keep, 2)
            os.close(keep)


def run_cells(tuple_name, only=(), out=sys.stdout):
    """The child's work: the tuple's cells one after another, a JSON line each.  only: cells as 'form,NFREE|N,set name'
    (e.g. 'split,N,exits N'); none given: every cell of the tuple."""
    import pytest
    import inst_cell as IC
    import oracle as O
    import util as U
    oracle = {}
    with tempfile.TemporaryDirectory() as tmp:
        for cell in cells():
            spec = "{},{},{}".format(cell["class"][2], "NFREE" if cell["class"][1] else "N", cell["set"])
            if cell["prm"] != tuple_name or (only and spec not in only):
                continue
            seqs = genome_set(cell["set"])
            if cell["set"] not in oracle:
                oracle[cell["set"]] = O.oracle_all2all(seqs, U.INST_PARAMS[tuple_name], threads=16)
            seen, err, log = {}, None, os.path.join(tmp, "stderr.txt")
            with pytest.MonkeyPatch.context() as mp, _stderr_to(log):
                try:
                    IC.run_cell(mp, os.path.join(tmp, "rtc"), cell, seqs, oracle[cell["set"]], seen)
                except AssertionError as e:
                    err = str(e)[:400]
            with open(log, errors="replace") as f:
                raw = parse_raw(f.read())
            print(json.dumps({"cell": cell["id"], "ok": err is None, "error": err, "kernels": seen.get("kernels"),
                              "digest": seen.get("digest"), "paths": raw["paths"], "chain": raw["chain"]}), file=out, flush=True)


if __name__ == "__main__":
    import torch  # noqa: F401  -- before the engine library: torch must load its own bundled HIP runtime first (same soname)
    for _p in ("lz-ani_amd", "oracle", "tools", "tests"):
        sys.path.insert(0, os.path.join(ROOT, _p))
    run_cells(sys.argv[1], tuple(sys.argv[2:]))
