"""The walk of tests/test_gpu_context_walk.py, without a GPU: which calls follow which on one warm context.

Nodes.  Per tuple of util.INST_PARAMS (a context has one tuple) the cells of util.INST_CELLS; for the two run-time compiled
tuples every cell also as a twin with LZANI_RTC=0, whose kernel util.predict_kernels names (the walk crosses rtc -> ahead of
time -> rtc on one context); for the defaults two nodes that run out-of-core under the smallest genome-memory limits
tests/ooc_model.py gives for 3 and 2 blocks.  A node is a cell (id, name, set, prm, env, form) plus
- limit: the genome-memory limit set before its lzani_set_genomes (0: in-core);
- kernels: the names its launch record must hold, or None (out-of-core nodes: results and blocks are asserted instead);
- blocks: what residency()["blocks"] must say.

The switches.  SET_ENV are read by lzani_set_genomes (lzani_set_plan.h: SetKnobs), RUN_ENV at the start of every run
(lzani_hip.hip: Knobs; lzani_rtc.h: LZANI_RTC, LZANI_RTC_CACHE).  set_key(node) is what a lzani_set_genomes depends on: two
nodes in a row with the same key run on one upload, two with different keys have a lzani_set_genomes between them.

The circuit.  walk(prm) is an Eulerian circuit of the complete directed graph with self-loops over the tuple's k nodes
(Hierholzer, nodes and out-edges in id order): k^2 edges, every ordered pair (a, b), (a, a) included, exactly once.
segments(prm) cuts it into pieces of at most CAP edges; a piece begins with the node the piece before it ended with, and each
piece gets a context of its own, so the only cold call of a piece is its first and no pair is crossed cold."""
import ooc_model as M
import util as U

SET_ENV = ("LZANI_BK_MAX_DIRBITS", "LZANI_NO_BUCKETS", "LZANI_NO_TAGWORDS", "LZANI_JOIN_MIN_BYTES", "LZANI_NO_JOIN",
           "LZANI_SORT_INDEX_MIN_DIRBITS", "LZANI_NO_SORT_INDEX", "LZANI_FILTER_MAX_BITS", "LZANI_NO_FILTER", "LZANI_MAX_SLOTS",
           "LZANI_FREE_BYTES")
RUN_ENV = ("LZANI_PM", "LZANI_PM_MIN_ROWS", "LZANI_PM_MAX_BYTES", "LZANI_PM_MIN_SHARE", "LZANI_PM_FAIL_CBITS", "LZANI_PM_FROM_INDEX",
           "LZANI_BLOCKS_PER_CU", "LZANI_BLOCK_KERNEL", "LZANI_RTC_MIN_PAIRS", "LZANI_LPT", "LZANI_SPLIT", "LZANI_SPLIT_S",
           "LZANI_SPLIT_SEGLEN", "LZANI_SPLIT_ALL", "LZANI_SPLIT_THR", "LZANI_SPLIT_GIVE_UP", "LZANI_NO_LDS_INDEX",
           "LZANI_LDS_INDEX_MAX_DIRBITS", "LZANI_RTC", "LZANI_RTC_CACHE")
RTC_TUPLES = ("rtc_chain", "rtc_plain")
# Edges of one context at the most: a condition (a test of a few seconds), not a measurement; per tuple where 48 edges take
# longer than the suite gives one test.  More, shorter segments lose no edge.
CAP = 48
# The run-time compiled tuples: a context's first rtc node of each (nfree, cand) compiles its kernel (1.4 s each on the
# MI355X with an empty disk cache), and the circuit's first 23 edges visit all twelve nodes: 48 edges took 9.2 s and 7.6 s
# (0.5-0.8 s the later segments, which load from the cache).  12 edges reach four of the six kernels.
CAP_OF = {"rtc_chain": 12, "rtc_plain": 12}
OOC_NODES = (("ooc3_small_N_all2all", "small N", "all2all", 3), ("ooc2_small_lists", "small", "lists", 2))

_NODES = {}


def rows_of(node):
    """(ref_ids, row_off, query_ids or None, rows, pairs per row) of the node's call."""
    n = len(U.instantiation_set(node["set"]))
    ref_ids, off, q = U.instantiation_rows(node, n)
    return ref_ids, off, q, len(ref_ids), int(off[1] - off[0])


def _twin(cell):
    env = dict(cell["env"], LZANI_RTC="0")
    seqs = U.instantiation_set(cell["set"])
    _, _, _, n_rows, per_row = rows_of(cell)
    names = U.predict_kernels(seqs, U.INST_PARAMS[cell["prm"]], env, cell["form"], pairs_per_row=per_row, n_rows=n_rows, rtc_ready=True)
    return dict(cell, id=cell["id"] + "_aot", name=sorted(names)[0], env=env, kernels=set(names), twin_of=cell["id"])


def _ooc(ident, setname, form, blocks):
    prm = U.INST_PARAMS["defaults"]
    lens = [len(s) for s in U.instantiation_set(setname)]
    limit = M.limit_for_blocks(lens, prm, blocks)
    assert limit is not None and int(M.plan_blocks(lens, prm, limit).max()) + 1 == blocks, (ident, limit)
    return dict(id=ident, name="out-of-core", set=setname, prm="defaults", env={"LZANI_RTC": "0"}, form=form, limit=limit,
                kernels=None, blocks=blocks)


def nodes(prm):
    """The nodes of tuple prm (a name of util.INST_PARAMS), in id order."""
    if prm not in _NODES:
        out = []
        for c in U.INST_CELLS:
            if c["prm"] != prm:
                continue
            out.append(dict(c, limit=0, kernels=U.kernel_names_of_cell(c), blocks=1))
            if prm in RTC_TUPLES:
                out.append(dict(_twin(c), limit=0, blocks=1))
        if prm == "defaults":
            out += [_ooc(*spec) for spec in OOC_NODES]
        assert len({x["id"] for x in out}) == len(out)
        _NODES[prm] = sorted(out, key=lambda x: x["id"])
    return _NODES[prm]


def set_key(node):
    """What the node's lzani_set_genomes depends on: the set's name, its SET_ENV items, its genome-memory limit."""
    return (node["set"], tuple(sorted((k, v) for k, v in node["env"].items() if k in SET_ENV)), node["limit"])


def euler_circuit(k):
    """Hierholzer on the complete directed graph with self-loops over 0 .. k - 1, from node 0, every node's out-edges taken in
    ascending order of their heads: a list of k^2 + 1 node numbers that begins and ends with 0."""
    nxt = [0] * k                                   # the next unused out-edge of every node is (v, nxt[v])
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < k:
            nxt[v] += 1
            stack.append(nxt[v] - 1)
        else:
            circuit.append(stack.pop())
    return circuit[::-1]


def walk(prm):
    """The circuit of tuple prm as a list of nodes (k^2 + 1 of them; the first is the last)."""
    ns = nodes(prm)
    return [ns[i] for i in euler_circuit(len(ns))]


def segments(prm):
    """The circuit cut into lists of nodes of at most CAP_OF[prm] (default CAP) edges each -- a list of e + 1 nodes has e
    edges; list s + 1 begins with the node list s ends with."""
    w, cap = walk(prm), CAP_OF.get(prm, CAP)
    return [w[a:a + cap + 1] for a in range(0, len(w) - 1, cap)]


def segment_ids():
    """(tuple, segment number) of every segment of every tuple: the parameters of the GPU test."""
    return [(prm, s) for prm in U.INST_PARAMS for s in range(len(segments(prm)))]


def layout_of(node):
    """The set layout lzani_set_genomes gives the node (lzani_set_plan.h: set_layout_of), from util.index_form and the node's
    SET_ENV items: dict(bk, tw, join) -- bucket table, tag words, join lists."""
    env, p = node["env"], U.INST_PARAMS[node["prm"]]
    seqs = U.instantiation_set(node["set"])
    g = U.index_form(seqs, p)
    on = lambda name: env.get(name, "")[:1] == "1"
    bk = g["bucket_table"] and not on("LZANI_NO_BUCKETS")
    tw = bk and g["tag_words"] and not on("LZANI_NO_TAGWORDS")
    join = bool(tw and 4 * (1 << g["dir_bits"]) >= int(env.get("LZANI_JOIN_MIN_BYTES", 8 << 20)) and p["mqd"] + p["mrd"] <= 128 and
                U._clog2(len(seqs) + 1) + g["key_bits"] + g["pos_bits"] <= 64 and not on("LZANI_NO_JOIN"))
    return dict(bk=bool(bk), tw=bool(tw), join=join)


def edge_kinds(a, b):
    """The kinds of the edge a -> b (the call of b on the context that a's call left), as a set of names."""
    kinds = set()
    same_key = set_key(a) == set_key(b)
    if same_key and a["kernels"] != b["kernels"]:
        kinds.add("form change on one upload")
    nfree = lambda x: not x["set"].endswith(" N")
    if nfree(a) != nfree(b):
        kinds.add("N-free -> N" if nfree(a) else "N -> N-free")
    la, lb = (max(len(s) for s in U.instantiation_set(x["set"])) for x in (a, b))
    if la != lb:
        kinds.add("longest text grows" if lb > la else "longest text shrinks")
    if a["set"] == b["set"]:
        fa, fb = layout_of(a), layout_of(b)
        if fa["join"] != fb["join"]:
            kinds.add("join on" if fb["join"] else "join off")
        if (fa["bk"], fa["tw"]) != (fb["bk"], fb["tw"]):
            kinds.add("index tables off" if (fb["bk"], fb["tw"]) < (fa["bk"], fa["tw"]) else "index tables on")
    if (a["limit"] != 0) != (b["limit"] != 0):
        kinds.add("in-core -> out-of-core" if b["limit"] else "out-of-core -> in-core")
    if a.get("twin_of") == b["id"]:
        kinds.add("twin -> rtc")
    if b.get("twin_of") == a["id"]:
        kinds.add("rtc -> twin")
    return kinds
