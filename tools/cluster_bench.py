#!/usr/bin/env python3
"""GPU box: the cluster stage on the family set of tools/related_bench.py (n genomes in families of `fam`, the rows hold the
same-family pairs) behind an output filter that keeps the related pairs.  One lzani_run_rows_kept, then per algorithm
begin -> add_kept -> run; lzani_cluster_host on the same edges for the wall time of the sequential statement, and its
answer compared; then complete linkage on its worst shape, a path of made-up edges with ascending ids and equal weights
(one merge a round), and Leiden on its two: that path at resolution 0.3, and one clique (one mover a round in both).  Prints
one JSON object (profiles/cluster_stage.json; with set cover, profiles/cluster_cover.json; with complete linkage,
profiles/cluster_link.json; with Leiden, profiles/cluster_leiden.json).  Usage: tools/cluster_bench.py [n] [fam] [dmax] [path nodes]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("lz-ani_amd", "oracle", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np
import lzani_ctypes as L
import cluster_model as CM
import synth_genomes as SG

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
fam = int(sys.argv[2]) if len(sys.argv) > 2 else 50
dmax = float(sys.argv[3]) if len(sys.argv) > 3 else 0.15
path_n = int(sys.argv[4]) if len(sys.argv) > 4 else 4000
flt = {"ani": 0.7, "qcov": 0.5}
t = time.perf_counter()
_, seqs = SG.make_set(n, 1, fam=fam, dmax=dmax)
print(f"{n} genomes made in {time.perf_counter() - t:.0f} s", file=sys.stderr, flush=True)
rows = [[q for q in range((r // fam) * fam, min(n, (r // fam + 1) * fam)) if q != r] for r in range(n)]
ref_ids = np.arange(n, dtype=np.uint32)
row_off = np.zeros(n + 1, dtype=np.uint64)
row_off[1:] = np.cumsum([len(r) for r in rows])
q = np.array([x for r in rows for x in r], dtype=np.uint32)
eng = L.Engine()
eng.set_genomes(seqs)
t = time.perf_counter()
kept = eng.run_rows_kept(ref_ids, row_off, q, flt, fetch=False)
wall = time.perf_counter() - t
tm, ki = eng.timing(), eng.kept_info()
print(f"run_rows_kept: {wall:.1f} s wall, pairs_ms {tm['pairs_ms']:.1f}, kept {kept} of {ki['leading']} pairs", file=sys.stderr, flush=True)
rec = eng.kept_fetch(0, kept)
lens = np.array([len(s) for s in seqs], dtype=np.uint32)
out = dict(workload=dict(genomes=n, family=fam, dmax=dmax, directed_pairs=int(len(q)), out_filter=flt, leading_pairs=int(ki["leading"]),
                         kept_pairs=int(kept)),
           pairs_ms=tm["pairs_ms"], index_ms=tm["index_ms"], filter_ms=ki["filter_ms"], algorithms={})
for algo in CM.ALGOS + ("set-cover", "complete-linkage", "leiden-cpm"):
    eng.cluster_begin(measure="tani")
    eng.cluster_add_kept()
    eng.cluster_run(algo)
    eng.cluster_run(algo)                                   # (the second run: no first-launch cost)
    info = eng.cluster_info()
    rep, cl = eng.cluster_fetch()
    edges = L.cluster_edges(rec["a"], rec["b"], CM.weight("tani", rec["x"], rec["y"], rec["lines"], lens[rec["a"]], lens[rec["b"]]))
    t = time.perf_counter()
    h_rep, h_cl, h_k = L.cluster_host(n, edges, algo)
    host_ms = (time.perf_counter() - t) * 1e3
    same = bool(np.array_equal(rep, h_rep) and np.array_equal(cl, h_cl))
    out["algorithms"][algo] = dict(edges=int(info["edges"]), add_ms=info["add_ms"], run_ms=info["run_ms"], rounds=int(info["rounds"]),
                                   clusters=int(info["clusters"]), singletons=int(info["singletons"]), largest=int(info["largest"]),
                                   edge_bytes=int(info["edge_bytes"]), cluster_host_wall_ms=host_ms, equals_cluster_host=same,
                                   below_pairs_ms=bool(info["add_ms"] + info["run_ms"] < tm["pairs_ms"]))
    if algo == "set-cover":                                 # what the run says of its distinct edges, and the ratio for the record
        cov = eng.cluster_cover_info()
        out["algorithms"][algo].update(distinct_edges=int(cov["distinct_edges"]), duplicate_edges=int(cov["duplicate_edges"]),
                                       workspace_bytes=int(cov["workspace_bytes"]), dedup_ms=cov["dedup_ms"], rounds_ms=cov["rounds_ms"],
                                       run_ms_over_greedy_first=info["run_ms"] / out["algorithms"]["greedy-first"]["run_ms"])
    if algo == "complete-linkage":
        lk = eng.cluster_link_info()
        out["algorithms"][algo].update(distinct_edges=int(lk["distinct_edges"]), duplicate_edges=int(lk["duplicate_edges"]), merges=int(lk["merges"]),
                                       table_slots=int(lk["table_slots"]), workspace_bytes=int(lk["workspace_bytes"]), dedup_ms=lk["dedup_ms"],
                                       rounds_ms=lk["rounds_ms"], run_ms_over_single=info["run_ms"] / out["algorithms"]["single"]["run_ms"],
                                       run_ms_over_set_cover=info["run_ms"] / out["algorithms"]["set-cover"]["run_ms"])
    if algo == "leiden-cpm":                                # the defaults: resolution 0.7, two iterations
        ld = eng.cluster_leiden_info()
        out["algorithms"][algo].update({k: (ld[k] if k.endswith("_ms") else int(ld[k])) for k in ld},
                                       run_ms_over_single=info["run_ms"] / out["algorithms"]["single"]["run_ms"],
                                       run_ms_over_complete_linkage=info["run_ms"] / out["algorithms"]["complete-linkage"]["run_ms"])
# the worst shape of complete linkage: path_n nodes in a path, path_n / 2 + 1 rounds of one merge each
eng.cluster_begin(path_n, np.ones(path_n, np.uint32))
eng.debug_cluster_add_edges(L.cluster_edges(np.arange(path_n - 1), np.arange(1, path_n), np.full(path_n - 1, 0.5)))
eng.cluster_run("complete-linkage")
eng.cluster_run("complete-linkage")
info, lk = eng.cluster_info(), eng.cluster_link_info()
out["complete_linkage_path"] = dict(nodes=path_n, edges=int(info["edges"]), rounds=int(info["rounds"]), merges=int(lk["merges"]), clusters=int(info["clusters"]),
                                    run_ms=info["run_ms"], rounds_ms=lk["rounds_ms"], dedup_ms=lk["dedup_ms"], ms_per_round=lk["rounds_ms"] / info["rounds"],
                                    workspace_bytes=int(lk["workspace_bytes"]))
# the worst shapes of Leiden: one mover a round -- the path at a resolution below its weight, and one clique
clique_n = 300
iu = np.triu_indices(clique_n, 1)
for name, nodes, edges, gamma in (("leiden_path", path_n, L.cluster_edges(np.arange(path_n - 1), np.arange(1, path_n), np.full(path_n - 1, 0.5)), 0.3),
                                  ("leiden_clique", clique_n, L.cluster_edges(iu[0], iu[1], np.full(len(iu[0]), 0.9)), 0.7)):
    eng.cluster_begin(nodes, np.ones(nodes, np.uint32))
    eng.debug_cluster_add_edges(edges)
    eng.set_cluster_leiden(gamma, 2)
    eng.cluster_run("leiden-cpm")
    eng.cluster_run("leiden-cpm")
    info, ld = eng.cluster_info(), eng.cluster_leiden_info()
    rounds = int(ld["move_rounds"] + ld["refine_rounds"])
    out[name] = dict(nodes=nodes, edges=int(info["edges"]), resolution=gamma, clusters=int(info["clusters"]), run_ms=info["run_ms"], ms_per_round=ld["rounds_ms"] / rounds,
                     **{k: (ld[k] if k.endswith("_ms") else int(ld[k])) for k in ld})
eng.close()
print(json.dumps(out, indent=1))
sys.exit(0 if all(a["equals_cluster_host"] for a in out["algorithms"].values()) else 1)
