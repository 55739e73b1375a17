"""The null chain commits events behind tracking rounds that reach beyond the query's last msl-mer: the pairs, and the child
that counts.

end_pair(k, second) is a reference r of 3,000 random symbols and a query q of Lq = 2992 + k that share two stretches and
nothing else by design: P1, 14 symbols that end 20 + k symbols in front of the query's end, and -- if `second` -- P2, 13
symbols at [Lq - 15, Lq - 2), 1,000 symbols away in the reference (distant from P1's diagonal), both between symbols that
differ.  The round behind P1 starts at i in [Lq - 35, Lq - 15]: its 41 steps reach beyond Lq - msl, and i <= Lq - 8
leaves it to the chain (i <= iend - 41) -- IF a candidate is queued behind P1, which is P2.  Without P2 the queue is empty
there, the chain leaves with nothing and the round is DevWave::track_round's.  The reference also holds, on P1's diagonal at
the step of query position Lq - 3, the query's last three symbols followed by four A (zero bits, what the packed text holds
behind the query): the window position a step without the KM_INVALID of kms_valid_nfree_head would take for a seed candidate.
(The results do not depend on that: a seed candidate is verified symbol by symbol with the query's bound.  It makes the rule
matter to the path taken.)

The child (`python tests/seed_text_cover.py` with LZANI_LIB = the coverage library, lzani_ctypes.build_diag_library) runs each
pair with and without P2 as a dense all2all of the two genomes through the candidate-bitmap kernel, compares both with the
oracle and prints the chain's raw counters of both runs (tests/path_cover.py: CHAIN_SLOTS).  Both directions of the pair are in
the totals, and P2 is an event in both, so "P2 was committed by the chain" reads: commits + 2, events_general + 0."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = 16
ENV = {"LZANI_PM_MIN_ROWS": "1", "LZANI_SPLIT": "0", "LZANI_RTC": "0"}


def end_pair(k, second):
    import numpy as np
    import synth_genomes as SG
    st = SG.Stream(7400 + k)
    rnd = lambda n: (st.u64(n) % np.uint64(4)).astype(np.uint8)
    differ = lambda x: (int(x) + 1 + st.randint(0, 2)) % 4
    Lq = 2992 + k
    r, q = rnd(3000), rnd(Lq)
    e1 = Lq - (20 + k)
    q[e1 - 14:e1] = r[500:514]
    q[e1 - 15], q[e1] = differ(r[499]), differ(r[514])
    q[Lq - 15:Lq - 2] = r[1500:1513]
    q[Lq - 16], q[Lq - 2] = differ(r[1499]), differ(r[1513])
    at = 514 + (Lq - 3 - e1)                                  # P1's diagonal at query position Lq - 3
    r[at:at + 3] = q[Lq - 3:]
    r[at + 3:at + 7] = 0
    if not second:
        q[Lq - 15:Lq - 2] = (q[Lq - 15:Lq - 2] + 2) % 4       # no symbol of P2 is left
    return [np.ascontiguousarray(r), np.ascontiguousarray(q)]


def run_cases(out=sys.stdout):
    import numpy as np
    import lzani_ctypes as L
    import oracle as O
    import path_cover as PC
    for k, v in ENV.items():
        os.environ[k] = v
    with tempfile.TemporaryDirectory() as tmp:
        for k in range(CASES):
            line = {"k": k}
            for second in (1, 0):
                seqs = end_pair(k, second)
                log = os.path.join(tmp, "stderr.txt")
                with PC._stderr_to(log):
                    eng = L.Engine(None)
                    try:
                        eng.set_genomes(seqs)
                        got = eng.all2all()
                        rec = eng.kernel_launches()
                    finally:
                        eng.close()
                with open(log, errors="replace") as f:
                    raw = PC.parse_raw(f.read())
                key = "with" if second else "without"
                line[key] = raw["chain"]
                line[key + "_ok"] = bool(np.array_equal(got, O.oracle_all2all(seqs, None, threads=4)))
                line[key + "_kernels"] = sorted(rec)
            print(json.dumps(line), file=out, flush=True)


if __name__ == "__main__":
    import torch  # noqa: F401  -- before the engine library: torch must load its own bundled HIP runtime first (same soname)
    for _p in ("lz-ani_amd", "oracle", "tools", "tests"):
        sys.path.insert(0, os.path.join(ROOT, _p))
    run_cases()
