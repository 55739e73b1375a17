#!/usr/bin/env python3
"""Seeded search, on the host model alone, for small genome sets whose split run has void segments.

Usage: tools/split_void_search.py CLASS FIRST_SEED N_SEEDS [JOBS]
  CLASS: generic | wide | defaults | long  (the split kernels' defp 0, 0, 1, 2; tests/util.py: split_repair_case)

Every seed gives one case (2-4 genomes of 4-9 kbp, a tuple); cases the device would not run by its split kernels of that
class at cuts every 512 positions (U.predict_kernels under U.SPLIT_REPAIR_ENV) are skipped.  The model
(U.model_split_rounds: the device's rounds of segments and stitches) runs each at the device's give-up rule; a case with a
void stitch is printed as one line of tests/util.py's SPLIT_REPAIR_TABLE, after a check that its results equal the
oracle's.  The last line says how many sets were searched, how many had voids, and the voids by cause in all."""
import os
import sys
from multiprocessing import Pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("lz-ani_amd", "oracle", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np

import oracle as O
import util as U


def one(arg):
    cls, seed = arg
    prm, seqs = U.split_repair_case(cls, seed)
    d = U.SPLIT_REPAIR_DEFP[cls]
    nf = int(all((s < 4).all() for s in seqs))
    if U.predict_kernels(seqs, prm, U.SPLIT_REPAIR_ENV) != {"split nfree={} defp={} mode={}".format(nf, d, m) for m in (0, 1)}:
        return None
    assert max(len(s) for s in seqs) + prm["mrd"] < 64 * 512
    got, st = U.model_split_rounds(seqs, prm, seglen=512)
    if sum(st["voids"]) == 0:
        return seed, None, st
    assert np.array_equal(got, O.oracle_all2all(seqs, prm)), (cls, seed, "the model differs from the oracle")
    return seed, dict(cls=cls, seed=seed, nfree=nf, **st), st


def main():
    cls, first, count = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    jobs = int(sys.argv[4]) if len(sys.argv) > 4 else 4
    U.model_lib()                                   # (built once, before the workers start)
    searched = found = 0
    voids = [0] * 6
    with Pool(jobs) as pool:
        for r in pool.imap(one, [(cls, s) for s in range(first, first + count)], chunksize=8):
            if r is None:
                continue
            searched += 1
            if r[1] is not None:
                found += 1
                voids = [a + b for a, b in zip(voids, r[2]["voids"])]
                print("    " + repr(r[1]) + ",", flush=True)
    print(f"# {cls}: seeds {first}..{first + count - 1}: {searched} sets searched, {found} with voids, voids by cause {voids}")


if __name__ == "__main__":
    main()
