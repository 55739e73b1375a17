#!/usr/bin/env python3
"""GPU box: the device k-mer prefilter (lzani_prefilter) on two workloads, one JSON line.
  bench     the 10,000 x ~40 kbp set of bench.py (families of 10), k = 21, every k-mer
  family    the 20,000-genome set of tools/related_bench.py (families of 50), k = 21, every k-mer and every fifth; and the
            bar of the stage: prefilter (every fifth k-mer) + the filtered run_rows it yields against the dense run_rows of
            the same set, wall time, same process
Per run: the four stage times of lzani_get_prefilter_info (HIP events), postings per second over their sum, and the
bytes the stage's passes move per posting (counted below from the run's own sizes) against the 8 TB/s HBM roofline.
Every figure is the median of --repeats runs after one warm-up run.
  --streamed  instead of the two workloads: the 2,000 x 36-44 kbp set (families of 50), k = 21, every fifth k-mer, through
              both entry points -- lzani_prefilter on the set held in-core, and lzani_prefilter_codes streaming it from host
              memory (--slice-bytes N, or --slices K for the smallest size that gives at most K slices; default: one
              slice) -- with both info structs and the device memory each path holds for genomes; --passes P forces the
              k-mer passes of both (LZANI_PREFILTER_PASSES) and the line carries passes, key_sweeps, hist_ms and
              workspace_bytes of lzani_get_prefilter_pass_info; --counting auto|dense|sparse chooses the accumulator of both
              (lzani_set_prefilter_counting; the line then carries lzani_get_prefilter_sparse_info and count_ms + compact_ms
              of every run) and --tile-rows R forces the height of the dense matrix tile (LZANI_PREFILTER_TILE_ROWS)
  --cross N_REF [N_REF ...]  instead of the two workloads: the same 2,000-genome set, k = 21, every fifth k-mer, through the
              all-pairs form (lzani_prefilter) and, for every n_ref given, the cross form (lzani_prefilter_cross: the first
              n_ref genomes as references against the rest) in one process: count_ms, compact_ms (every run and the
              median), matrix_bytes, tiles, entries and the atomic adds of both forms; the cross result is checked against
              the all-pairs result restricted to the cross pairs
  --max-seqs N  instead of the two workloads: the same 2,000-genome set, k = 21, every fifth k-mer, through lzani_prefilter and
              behind it lzani_prefilter_limit with N: lzani_get_prefilter_limit_info of every run (limit_ms every run and the
              median) beside the prefilter's stage times, the limited result checked against lzani_prefilter_limit_host on the
              unlimited fetch, and the pair-kernel time (lzani_get_timing) of the filtered rows without and with the limit
Usage: tools/prefilter_bench.py [--out profiles/prefilter_bench.json] [--repeats 3] [--small] [--no-dense]
       tools/prefilter_bench.py --streamed [--slice-bytes N | --slices K] [--passes P] [--counting sparse] [--tile-rows R]
                                [--out profiles/prefilter_stream_bench.json]
       tools/prefilter_bench.py --cross N_REF [N_REF ...] [--out profiles/prefilter_cross_bench.json]
       tools/prefilter_bench.py --max-seqs N [--out profiles/prefilter_limit_bench.json]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("lz-ani_amd", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np
import lzani_ctypes as L
import synth_genomes as SG

HBM_BYTES_PER_S = 8e12
K = 21


def stage_bytes(info, n, updates):
    """HBM bytes of the stage's passes, from its own counts: P kept windows, D distinct k-mers, M postings, `updates`
    atomic adds.  Keys: three passes over the packed texts (both strands, 2 bit a base: left out) writing 8 B twice and
    looking each window up in the dictionary (log2 D probes of 8 B, most of them cached: counted in full).  A radix
    pass reads a key twice and writes it once (24 B); the dictionary and the postings each read the sorted keys twice
    and write the survivors.  Counting reads a posting's run once per posting ahead of it (4 B of the atomic add each,
    8 B read) and the matrix is cleared and read once above the diagonal."""
    P, D, M = info["positions"], info["distinct_kmers"], info["postings"]
    lgD = max(1, math.ceil(math.log2(max(D, 2))))
    passes = math.ceil(2 * info["k"] / 8) + math.ceil(lgD / 8)
    keys = P * (8 + 8 + 8 * lgD)
    sort = P * 24 * passes + P * 16 * 2 + 8 * (D + M) + 4 * D
    count = 8 * M * info["tiles"] + 12 * updates + 4 * n * n
    compact = 4 * n * n // 2 + 8 * info["entries"]
    return dict(keys=keys, sort=sort, count=count, compact=compact)


def measure(eng, n, smax, min_shared, min_ratio, repeats):
    eng.prefilter(K, smax, 1, 0.0)                                  # warm-up; with these thresholds: sum of shared = atomic adds
    updates = int(eng.prefilter_fetch()[3].astype(np.int64).sum())
    runs, walls = [], []
    for _ in range(repeats):
        t = time.perf_counter()
        eng.prefilter(K, smax, min_shared, min_ratio)
        walls.append(time.perf_counter() - t)
        runs.append(eng.prefilter_info())
    info = dict(runs[0])
    for key in ("keys_ms", "sort_ms", "count_ms", "compact_ms"):
        info[key] = float(np.median([r[key] for r in runs]))
    dev_ms = info["keys_ms"] + info["sort_ms"] + info["count_ms"] + info["compact_ms"]
    b = stage_bytes(info, n, updates)
    total_b = sum(b.values())
    info.update(device_ms=dev_ms, wall_ms=float(np.median(walls)) * 1e3, atomic_adds=updates,
                postings_per_s=info["postings"] / (dev_ms * 1e-3) if dev_ms else None,
                bytes_per_posting=total_b / max(info["postings"], 1), bytes_by_stage=b,
                achieved_bytes_per_s=total_b / (dev_ms * 1e-3) if dev_ms else None,
                share_of_hbm_roofline=total_b / (dev_ms * 1e-3) / HBM_BYTES_PER_S if dev_ms else None)
    return info


STAGES = ("keys_ms", "sort_ms", "count_ms", "compact_ms")


def streamed(a):
    """The same set through lzani_prefilter (in-core) and lzani_prefilter_codes (streamed): medians of the stage times."""
    n, fam, min_shared, min_ratio = (200, 50, 5, 0.003) if a.small else (2000, 50, 5, 0.003)
    _, seqs = SG.make_set(n, 5, fam=fam, dmax=0.10)
    lens = [len(s) for s in seqs]
    total = sum(lens)
    smax = L.sample_max_of(0.2)
    sb = a.slice_bytes or total
    if a.slices:
        sb = next(x for x in range(-(-total // a.slices) // 4096 * 4096, total + 4096, 4096) if x >= max(lens) and L.plan_slices(lens, x)[0] <= a.slices)
    if a.passes:
        os.environ["LZANI_PREFILTER_PASSES"] = str(a.passes)
    if a.tile_rows:
        os.environ["LZANI_PREFILTER_TILE_ROWS"] = str(a.tile_rows)
    res = dict(tool="prefilter_bench --streamed", k=K, fraction=0.2, genomes=n, bases=total, repeats=a.repeats, slice_bytes=sb,
               forced_passes=a.passes, counting=a.counting, tile_rows=a.tile_rows, matrix_bytes=4 * n * min(n, a.tile_rows or n))

    def run_info(eng):
        return dict(eng.prefilter_info(), **eng.prefilter_pass_info(), sparse=eng.prefilter_sparse_info())

    def per_run(runs):
        return dict(count_plus_compact_ms_runs=[r["count_ms"] + r["compact_ms"] for r in runs], count_ms_runs=[r["count_ms"] for r in runs],
                    compact_ms_runs=[r["compact_ms"] for r in runs])

    def median_of(runs, keys):
        out = dict(runs[0])
        for key in keys:
            out[key] = float(np.median([r[key] for r in runs]))
        return out

    eng = L.Engine()
    eng.set_genomes(seqs)
    eng.prefilter(K, smax, min_shared, min_ratio)                   # the dense result is what every form must give
    want = eng.prefilter_fetch()
    eng.set_prefilter_counting(a.counting)
    eng.prefilter(K, smax, min_shared, min_ratio)                   # warm-up in the form measured
    same_resident = all(np.array_equal(x, y) for x, y in zip(eng.prefilter_fetch(), want))
    runs, walls = [], []
    for _ in range(a.repeats):
        t = time.perf_counter()
        eng.prefilter(K, smax, min_shared, min_ratio)
        walls.append(time.perf_counter() - t)
        runs.append(run_info(eng))
    res["resident"] = dict(median_of(runs, STAGES + ("hist_ms",)), wall_ms=float(np.median(walls)) * 1e3, walls_ms=[w * 1e3 for w in walls],
                           keys_ms_runs=[r["keys_ms"] for r in runs], bytes_genomes=eng.layout()["bytes_genomes"], equal_to_dense=bool(same_resident),
                           **per_run(runs))
    eng.close()
    print("resident:", json.dumps(res["resident"]), flush=True)

    eng = L.Engine()
    eng.set_prefilter_counting(a.counting)
    eng.prefilter_codes(seqs, K, smax, min_shared, min_ratio, slice_bytes=sb)
    got = eng.prefilter_fetch()
    same = same_resident and all(np.array_equal(x, y) for x, y in zip(got, want))
    runs, sruns, walls = [], [], []
    for _ in range(a.repeats):
        t = time.perf_counter()
        eng.prefilter_codes(seqs, K, smax, min_shared, min_ratio, slice_bytes=sb)
        walls.append(time.perf_counter() - t)
        runs.append(run_info(eng))
        sruns.append(eng.prefilter_stream_info())
    eng.close()
    res["streamed"] = dict(median_of(runs, STAGES + ("hist_ms",)), wall_ms=float(np.median(walls)) * 1e3, walls_ms=[w * 1e3 for w in walls],
                           keys_ms_runs=[r["keys_ms"] for r in runs], stream=median_of(sruns, ("upload_ms",)), equal_to_resident=bool(same), **per_run(runs))
    print("streamed:", json.dumps(res["streamed"]), flush=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    if not same:
        sys.exit("the prefilter's results differ: streamed from resident, or the form measured from the dense one")


def cross(a):
    """The all-pairs form and the cross form at every n_ref of --cross on one set, in one process."""
    n, fam, min_shared, min_ratio = (200, 50, 5, 0.003) if a.small else (2000, 50, 5, 0.003)
    _, seqs = SG.make_set(n, 5, fam=fam, dmax=0.10)
    smax = L.sample_max_of(0.2)
    res = dict(tool="prefilter_bench --cross", k=K, fraction=0.2, genomes=n, bases=sum(len(s) for s in seqs), repeats=a.repeats,
               min_shared=min_shared, min_ratio=min_ratio)
    eng = L.Engine()
    eng.set_genomes(seqs)

    def runs_of(call, adds_call):
        adds_call()                                                 # warm-up; thresholds (1, 0): the sum of shared = the atomic adds
        adds = int(eng.prefilter_fetch()[3].astype(np.int64).sum())
        runs = []
        for _ in range(a.repeats):
            call()
            runs.append(eng.prefilter_info())
        out = {key: runs[0][key] for key in ("tiles", "entries", "postings")}
        for key in ("count_ms", "compact_ms"):
            out[key] = float(np.median([r[key] for r in runs]))
            out[key + "_runs"] = [r[key] for r in runs]
        out["count_plus_compact_ms_runs"] = [r["count_ms"] + r["compact_ms"] for r in runs]
        out["atomic_adds"] = adds
        return out

    res["all_pairs"] = runs_of(lambda: eng.prefilter(K, smax, min_shared, min_ratio), lambda: eng.prefilter(K, smax, 1, 0.0))
    res["all_pairs"]["matrix_bytes"] = 4 * n * -(-n // res["all_pairs"]["tiles"]) if res["all_pairs"]["tiles"] else 0
    want = eng.prefilter_fetch()
    a_of = np.repeat(np.arange(n), np.diff(want[1]).astype(np.int64))
    print("all pairs:", json.dumps(res["all_pairs"]), flush=True)
    res["cross"], same = [], True
    for n_ref in a.cross:
        c = runs_of(lambda: eng.prefilter_cross(K, n_ref, smax, min_shared, min_ratio), lambda: eng.prefilter_cross(K, n_ref, smax, 1, 0.0))
        c.update(eng.prefilter_cross_info())
        got = eng.prefilter_fetch()
        ok = (a_of < n_ref) & (want[2] >= n_ref)
        c["equal_to_restricted_all_pairs"] = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2][ok]) and np.array_equal(got[3], want[3][ok]) and
                                                  np.array_equal(np.diff(got[1]).astype(np.int64), np.bincount(a_of[ok], minlength=n)))
        same = same and c["equal_to_restricted_all_pairs"]
        res["cross"].append(c)
        print("cross:", json.dumps(c), flush=True)
    eng.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    if not same:
        sys.exit("the cross prefilter's result differs from the restricted all-pairs result")


def filtered_rows(n, row_off, ids):
    """Both directions of every kept pair as the rows run_rows takes: (ref_ids, row_off, query_ids)."""
    ref_ids = np.arange(n, dtype=np.uint32)
    a_of = np.repeat(ref_ids, np.diff(row_off).astype(np.int64))
    r = np.concatenate((a_of, ids)).astype(np.int64)
    q = np.concatenate((ids, a_of)).astype(np.int64)
    order = np.lexsort((q, r))
    f_off = np.zeros(n + 1, dtype=np.uint64)
    f_off[1:] = np.cumsum(np.bincount(r, minlength=n))
    return ref_ids, f_off, q[order].astype(np.uint32)


def limit(a):
    """lzani_prefilter and behind it lzani_prefilter_limit on one set, and what the limit saves the pair kernel."""
    n, fam, min_shared, min_ratio = (200, 50, 5, 0.003) if a.small else (2000, 50, 5, 0.003)
    _, seqs = SG.make_set(n, 5, fam=fam, dmax=0.10)
    smax = L.sample_max_of(0.2)
    N = a.max_seqs
    res = dict(tool="prefilter_bench --max-seqs", k=K, fraction=0.2, genomes=n, family=fam, bases=sum(len(s) for s in seqs), repeats=a.repeats,
               min_shared=min_shared, min_ratio=min_ratio, max_seqs=N)
    eng = L.Engine()
    eng.set_genomes(seqs)
    eng.prefilter(K, smax, min_shared, min_ratio)                   # warm-up, and the unlimited result
    unl = eng.prefilter_fetch()
    eng.prefilter_limit(N)
    got = eng.prefilter_fetch()
    keep = L.prefilter_limit_host(n, 0, *unl, N).astype(bool)
    a_of = np.repeat(np.arange(n), np.diff(unl[1]).astype(np.int64))
    same = bool(np.array_equal(got[0], unl[0]) and np.array_equal(got[2], unl[2][keep]) and np.array_equal(got[3], unl[3][keep]) and
                np.array_equal(np.diff(got[1]).astype(np.int64), np.bincount(a_of[keep], minlength=n)))
    runs, lruns = [], []
    for _ in range(a.repeats):
        eng.prefilter(K, smax, min_shared, min_ratio)
        runs.append(eng.prefilter_info())
        eng.prefilter_limit(N)
        lruns.append(eng.prefilter_limit_info())
    res["prefilter"] = {key: float(np.median([r[key] for r in runs])) for key in STAGES}
    res["prefilter"].update(entries=runs[0]["entries"], postings=runs[0]["postings"], compact_ms_runs=[r["compact_ms"] for r in runs])
    res["limit"] = dict(lruns[0], limit_ms=float(np.median([r["limit_ms"] for r in lruns])), limit_ms_runs=[r["limit_ms"] for r in lruns],
                        equal_to_host_rule=same)
    print("limit:", json.dumps(res["limit"]), flush=True)
    # the pair kernel over the filtered rows, without and with the limit
    rows = {"unlimited": filtered_rows(n, unl[1], unl[2]), "limited": filtered_rows(n, got[1], got[2])}
    eng.run_rows(rows["limited"][0][:fam], rows["limited"][1][:fam + 1], rows["limited"][2][:int(rows["limited"][1][fam])])     # warm-up (one family)
    for tag, (ref_ids, f_off, q_ids) in rows.items():
        pr = []
        for _ in range(a.repeats):
            eng.run_rows(ref_ids, f_off, q_ids)
            pr.append(eng.timing()["pairs_ms"])
        res["rows_" + tag] = dict(directed_pairs=int(len(q_ids)), pairs_ms=float(np.median(pr)), pairs_ms_runs=pr)
    res["pairs_ms_saved"] = res["rows_unlimited"]["pairs_ms"] - res["rows_limited"]["pairs_ms"]
    eng.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    if not same:
        sys.exit("the limited result differs from lzani_prefilter_limit_host on the unlimited fetch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a tenth of both sets (rehearsal)")
    ap.add_argument("--no-dense", action="store_true", help="skip the dense run of the family set")
    ap.add_argument("--streamed", action="store_true", help="lzani_prefilter against lzani_prefilter_codes on one set")
    ap.add_argument("--slice-bytes", type=int, default=0, help="--streamed: slice size (default: the whole set in one slice)")
    ap.add_argument("--passes", type=int, default=0, help="--streamed: force this many k-mer passes (LZANI_PREFILTER_PASSES)")
    ap.add_argument("--counting", choices=("auto", "dense", "sparse"), default="auto", help="--streamed: the accumulator of the count stage (lzani_set_prefilter_counting)")
    ap.add_argument("--tile-rows", type=int, default=0, help="--streamed: force the height of the dense matrix tile (LZANI_PREFILTER_TILE_ROWS)")
    ap.add_argument("--slices", type=int, default=0, help="--streamed: the smallest slice size (in 4 KiB steps) that gives at most this many slices")
    ap.add_argument("--cross", type=int, nargs="+", default=None, metavar="N_REF",
                    help="the cross form (the first N_REF genomes against the rest) beside the all-pairs form on one set")
    ap.add_argument("--max-seqs", type=int, default=0, metavar="N", help="lzani_prefilter_limit with N behind the prefilter, and the pair-kernel time of the rows it saves")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "prefilter_limit_bench.json" if a.max_seqs else "prefilter_cross_bench.json" if a.cross else "prefilter_stream_bench.json" if a.streamed else "prefilter_bench.json")
    if a.max_seqs:
        return limit(a)
    if a.cross:
        return cross(a)
    if a.streamed:
        return streamed(a)
    n_bench, n_fam, fam = (1000, 2000, 50) if a.small else (10000, 20000, 50)
    res = dict(tool="prefilter_bench", k=K, repeats=a.repeats, hbm_roofline_bytes_per_s=HBM_BYTES_PER_S)

    _, seqs = SG.make_set_cached(n_bench, 2)
    eng = L.Engine()
    eng.set_genomes(seqs)
    res["bench_set"] = dict(genomes=n_bench, fraction_1=measure(eng, n_bench, L.SAMPLE_ALL, 1, 0.0, a.repeats))
    eng.close()
    print("bench set:", json.dumps(res["bench_set"]), flush=True)

    _, seqs = SG.make_set(n_fam, 1, fam=fam)
    eng = L.Engine()
    eng.set_genomes(seqs)
    # thresholds of the family runs: 5 shared sampled 21-mers and 0.3 % of the smaller set -- far above what unrelated
    # random genomes share by chance, far below what members of one family share
    fs = dict(genomes=n_fam, family=fam, min_shared=5, min_ratio=0.003)
    fs["fraction_1"] = measure(eng, n_fam, L.SAMPLE_ALL, 5, 0.003, a.repeats)
    fs["fraction_0.2"] = measure(eng, n_fam, L.sample_max_of(0.2), 5, 0.003, a.repeats)
    print("family set:", json.dumps(fs), flush=True)

    # the bar: prefilter + filtered rows against dense rows, wall time
    ref_ids = np.arange(n_fam, dtype=np.uint32)
    t = time.perf_counter()
    eng.prefilter(K, L.sample_max_of(0.2), 5, 0.003)
    _, row_off, ids, _ = eng.prefilter_fetch()
    a_of = np.repeat(ref_ids, np.diff(row_off).astype(np.int64))
    r = np.concatenate((a_of, ids)).astype(np.int64)                      # both directions of every kept pair
    q = np.concatenate((ids, a_of)).astype(np.int64)
    order = np.lexsort((q, r))
    q_ids = q[order].astype(np.uint32)
    f_off = np.zeros(n_fam + 1, dtype=np.uint64)
    f_off[1:] = np.cumsum(np.bincount(r, minlength=n_fam))
    t_pre = time.perf_counter() - t
    eng.run_rows(ref_ids[:fam], f_off[:fam + 1], q_ids[:int(f_off[fam])])     # warm-up of the filtered path (one family)
    t = time.perf_counter()
    eng.run_rows(ref_ids, f_off, q_ids)
    t_flt = time.perf_counter() - t
    same = int(((r // fam) == (q // fam)).sum())
    bar = dict(prefilter_and_rows_wall_s=t_pre, filtered_run_rows_wall_s=t_flt, filtered_pairs=int(len(q_ids)),
               same_family_pairs_kept=same, same_family_pairs=n_fam * (fam - 1), cross_family_pairs_kept=int(len(q_ids)) - same)
    if not a.no_dense:
        d_ids, d_off = L.dense_rows(n_fam)
        eng.run_rows(d_ids[:8], d_off[:9], None)                          # warm-up of the dense path
        t = time.perf_counter()
        eng.run_rows(d_ids, d_off, None)
        bar["dense_run_rows_wall_s"] = time.perf_counter() - t
        bar["dense_pairs"] = int(d_off[-1])
        bar["speedup"] = bar["dense_run_rows_wall_s"] / (t_pre + t_flt)
    eng.close()
    fs["filtered_against_dense"] = bar
    res["family_set"] = fs
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    if "speedup" in bar and bar["speedup"] <= 1:
        sys.exit("prefilter + filtered run_rows was not faster than the dense run_rows")


if __name__ == "__main__":
    main()
