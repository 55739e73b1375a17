#!/usr/bin/env python3
"""GPU box: the cost of running a genome set out-of-core (lzani_set_genome_memory) against the in-core run.

Two workloads, each in three engines of one process -- in-core, and with genome-memory limits that cut the set into 4 and
16 blocks -- whose runs alternate (rounds of in-core, 4, 16) so that clocks and the box's load hit them alike:
  dense    a 2,000-row dense slab of the 10k x 40 kbp set (bench.py --workload dense, seed 2): 20 M directed pairs;
  related  the 20,000-genome related set (families of 50, same-family rows only: what a kmer-db filter leaves).
One JSON line per (workload, mode): wall pairs/s (median of the rounds), pair-kernel ms, block uploads and their device
time, tiles; every out-of-core result is checked against the in-core one.
Usage: tools/ooc_bench.py [--rounds 3] [--out FILE] [--dense-genomes 10000] [--related-genomes 20000]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("lz-ani_amd", "oracle", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np

import lzani_ctypes as L
import synth_genomes as SG


def limit_for(lens, blocks):
    """The smallest limit whose block plan has at most `blocks` blocks (the plan's block count falls as the limit grows)."""
    lo = 1
    hi = 2 * int(sum(16.75 * x + 4096 for x in lens)) + (1 << 20)
    while lo < hi:
        mid = (lo + hi) // 2
        try:
            nb, _ = L.plan_blocks(lens, None, mid)
        except L.LzaniError:
            nb = 1 << 30
        if nb <= blocks:
            hi = mid
        else:
            lo = mid + 1
    return lo


def reordered(seqs, names):
    order = sorted(range(len(seqs)), key=lambda i: (-len(seqs[i]), names[i]))
    return [seqs[i] for i in order], [names[i] for i in order], order


def run_workload(name, seqs, rows, rounds, out):
    lens = np.array([len(s) for s in seqs], np.uint32)
    modes = [("in-core", 0), ("4 blocks", limit_for(lens, 4)), ("16 blocks", limit_for(lens, 16))]
    engines = []
    for label, limit in modes:
        e = L.Engine()
        e.set_genome_memory(limit)
        t = time.perf_counter()
        e.set_genomes(seqs)
        engines.append((label, limit, e, (time.perf_counter() - t) * 1e3))
    ref_ids, row_off, q = rows
    want = None
    for label, limit, e, _ in engines:                   # warm-up: k-mer words, first uploads; results checked
        got = e.run_rows(ref_ids, row_off, q)
        if want is None:
            want = got
        elif not np.array_equal(got, want):
            raise SystemExit(f"{name} {label}: results differ from the in-core run")
    stats = {label: [] for label, _, _, _ in engines}
    for _ in range(rounds):
        for label, limit, e, _ in engines:
            t = time.perf_counter()
            e.run_rows(ref_ids, row_off, q)
            wall = time.perf_counter() - t
            stats[label].append((wall, e.timing(), e.residency()))
    pairs = int(row_off[-1])
    base = None
    for label, limit, e, set_ms in engines:
        walls = sorted(s[0] for s in stats[label])
        wall = walls[len(walls) // 2]
        tm = [s[1] for s in stats[label]]
        rs = [s[2] for s in stats[label]]
        rate = pairs / wall
        base = base or rate
        line = dict(workload=name, mode=label, genomes=len(seqs), rows=len(ref_ids), pairs=pairs, limit=limit,
                    blocks=rs[-1]["blocks"], tiles=rs[-1]["tiles"], uploads_per_run=rs[-1]["block_uploads"],
                    upload_ms=round(float(np.median([r["upload_ms"] for r in rs])), 2),
                    pairs_ms=round(float(np.median([t["pairs_ms"] for t in tm])), 2),
                    index_ms=round(float(np.median([t["index_ms"] for t in tm])), 2),
                    cand_ms=round(float(np.median([t["cand_ms"] for t in tm])), 2),
                    wall_ms=round(wall * 1e3, 1), wall_ms_all=[round(w * 1e3, 1) for w in walls],
                    pairs_per_s=round(rate), overhead_pct=round(100 * (base / rate - 1), 2),
                    peak_resident_bytes=rs[-1]["peak_resident_bytes"], host_bytes=rs[-1]["host_bytes"],
                    set_genomes_ms=round(set_ms, 1))
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
            out.flush()
    for _, _, e, _ in engines:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--dense-genomes", type=int, default=10000)
    ap.add_argument("--dense-rows", type=int, default=2000)
    ap.add_argument("--related-genomes", type=int, default=20000)
    ap.add_argument("--fam", type=int, default=50)
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None

    names, seqs = SG.make_set_cached(args.dense_genomes, 2, lmin=36000, lmax=44000)
    seqs, names, _ = reordered(seqs, names)
    ref_ids, row_off = L.dense_rows(len(seqs), range(args.dense_rows))
    run_workload("dense", seqs, (ref_ids, row_off, None), args.rounds, out)
    del seqs

    n, fam = args.related_genomes, args.fam
    names, seqs = SG.make_set_cached(n, 1, lmin=36000, lmax=44000, fam=fam, dmax=0.15)
    seqs, names, order = reordered(seqs, names)
    fam_of = np.array(order) // fam
    members = {}
    for g, f in enumerate(fam_of.tolist()):
        members.setdefault(f, []).append(g)
    qs = [[x for x in members[int(fam_of[r])] if x != r] for r in range(n)]
    row_off = np.zeros(n + 1, np.uint64)
    row_off[1:] = np.cumsum([len(x) for x in qs])
    q = np.array([x for r in qs for x in r], np.uint32)
    run_workload("related", seqs, (np.arange(n, dtype=np.uint32), row_off, q), args.rounds, out)


if __name__ == "__main__":
    main()
