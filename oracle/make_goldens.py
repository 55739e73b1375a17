#!/usr/bin/env python3
"""Generate tests/golden/ref_vectors.json, tests/golden/ref_live_vectors.json, tests/golden/ref_envelope_vectors.json and
tests/golden/repeat_vectors.json with the reference build (oracle/_ref).

TEST INFRASTRUCTURE ONLY.  Run in the build container (needs /root/reference to build
oracle/_ref):   make -C oracle ref && python oracle/make_goldens.py [--live-only | --envelope-only | --repeats-only]
Every vector is (inputs named by fixture/seed, expected int triples); no reference code is stored.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in ("oracle", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402
import oracle as O  # noqa: E402
import synth_genomes as SG  # noqa: E402
import util as U  # noqa: E402

EXTRA = {"mrd0": dict(mrd=0), "ar1": dict(ar=1), "aw64_am20": dict(aw=64, am=20),
         "mqd64_mrd64": dict(mqd=64, mrd=64), "mqd0": dict(mqd=0), "reg1": dict(reg=1), "am0": dict(am=0)}


def live_vectors():
    """The reference build's answers to the CPU tests that otherwise need it live: the oracle comparison on U.live_set,
    the --out-format expansions, and (as a digest) the number formatting of U.format_real_cases."""
    import hashlib
    seqs = U.live_set()
    out = {"generator": "oracle/make_goldens.py", "source": "the reference build of oracle/_ref (CParser, CParams, refresh::real_to_pchar)",
           "all2all": {name: dict(params=prm or {}, res=O.ref_all2all(seqs, prm, threads=8).tolist()) for name, prm in U.LIVE_PARAMS.items()},
           "out_format": {fmt: O.ref_expand_output_format(fmt) for fmt in U.OUT_FORMATS + ("tani,bogus",)}}
    cases = U.format_real_cases()
    digest = hashlib.sha256()
    for v, prec in cases:
        digest.update(O.ref_format_real(v, prec).encode() + b"\n")
    out["format_real"] = {"count": len(cases), "sha256": digest.hexdigest(),
                          "digest_of": "sha256 of the formatted strings of U.format_real_cases(), each followed by a newline"}
    # the INTEGRATION.md stub that `make -C oracle ref` compiled against the reference's own headers
    import integration_stub as IS
    stub = IS.stub_source(os.path.join(ROOT, "INTEGRATION.md"))
    with open(os.path.join(HERE, "_ref", "integration_stub.cpp")) as f:
        assert f.read() == stub, "oracle/_ref/integration_stub.o is stale: make -C oracle ref"
    assert os.path.exists(os.path.join(HERE, "_ref", "integration_stub.o"))
    out["integration_stub"] = {"sha256": hashlib.sha256(stub.encode()).hexdigest(),
                               "digest_of": "INTEGRATION.md section 1 as oracle/integration_stub.py writes it, compiled against the "
                                            "reference's headers into oracle/_ref/integration_stub.o"}
    path = os.path.join(ROOT, "tests", "golden", "ref_live_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes")


def envelope_vectors():
    """The reference build's all2all for every edge tuple of U.EDGE_TUPLES it can run (msl <= U.REF_MAX_MSL: its short-seed
    table has 4^msl entries) on U.edge_set() and U.envelope_family_set() (tests/test_envelope.py, tests/test_gpu_envelope.py)."""
    sets = {"edge": U.edge_set(), "family": U.envelope_family_set()}
    out = {"generator": "oracle/make_goldens.py", "source": "the reference build of oracle/_ref (CParser)",
           "layout": "res[set][tuple] = int32[n][n][3], res[r][q] = [sym_in_matches, sym_in_literals, no_components] of "
                     "parse(query=q, ref=r); diagonal zero",
           "params": {}, "res": {k: {} for k in sets}}
    for name, prm in U.EDGE_TUPLES.items():
        if prm["msl"] > U.REF_MAX_MSL:
            continue
        out["params"][name] = prm
        for k, seqs in sets.items():
            out["res"][k][name] = O.ref_all2all(seqs, prm, threads=8).tolist()
    path = os.path.join(ROOT, "tests", "golden", "ref_envelope_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes;", len(out["params"]), "tuples")


def repeat_vectors():
    """The reference build's answers on repeat-structured inputs (tests/repeat_genomes.py, tests/repeat_ties.py): result triples
    and regions of every tie case, and the all2all of the 'small' repeat sets under the defaults and the 'generic' tuple
    (tests/test_repeats.py)."""
    import repeat_genomes as RG
    import repeat_ties as RT
    out = {"generator": "oracle/make_goldens.py", "source": "the reference build of oracle/_ref (CParser)",
           "layout": "ties[case] = {res: [sym_in_matches, sym_in_literals, no_components], regions: flat rows of [ref_start, ref_end, "
                     "seq_start, seq_end, num_matches, num_mismatches]} of parse(query=qry, ref=ref); sets[set/tuple].res = "
                     "int32[n][n][3], res[r][q] of parse(query=q, ref=r), diagonal zero",
           "ties": {}, "sets": {}, "checksums": {}}
    for c in RT.tie_cases():
        res, regs = O.ref_pair(c["ref"], c["qry"], None, want_regions=True)
        out["ties"][c["name"]] = dict(res=list(res), regions=regs.reshape(-1).tolist())
    for name in ("small", "small N"):
        seqs = RG.repeat_set(name)
        out["checksums"][name] = RG.checksum(seqs)
        for pn in ("defaults", "generic"):
            out["sets"][f"{name}/{pn}"] = dict(params=U.INST_PARAMS[pn], res=O.ref_all2all(seqs, U.INST_PARAMS[pn], threads=8).tolist())
    path = os.path.join(ROOT, "tests", "golden", "repeat_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes;", len(out["ties"]), "tie cases,", len(out["sets"]), "sets")


def main():
    assert O.lib_ref() is not None, "build oracle/_ref first (make -C oracle ref)"
    if "--repeats-only" in sys.argv[1:]:
        repeat_vectors()
        return
    if "--envelope-only" in sys.argv[1:]:
        envelope_vectors()
        return
    repeat_vectors()
    live_vectors()
    envelope_vectors()
    if "--live-only" in sys.argv[1:]:
        return
    out = {"generator": "oracle/make_goldens.py", "source": "CParser of /root/reference (LZ-ANI 1.2.3) via oracle/ref_driver.cpp",
           "layout": "res[r][q] = [sym_in_matches, sym_in_literals, no_components] of parse(query=q, ref=r); diagonal zero",
           "sets": {}}
    _, ex = U.load_example()
    _, vir = U.load_vir61()
    edge = U.edge_set()
    _, syn = SG.make_set(24, 11, lmin=6000, lmax=9000, fam=6)
    for name, prm in U.VARIANTS.items():
        out["sets"][f"example/{name}"] = dict(params=prm, res=O.ref_all2all(ex, prm, threads=8).tolist())
        out["sets"][f"edge/{name}"] = dict(params=prm, res=O.ref_all2all(edge, prm, threads=8).tolist())
        out["sets"][f"synth24/{name}"] = dict(params=prm, res=O.ref_all2all(syn, prm, threads=8).tolist())
    for name, prm in EXTRA.items():
        out["sets"][f"edge/{name}"] = dict(params=prm, res=O.ref_all2all(edge, prm, threads=8).tolist())
        out["sets"][f"synth24/{name}"] = dict(params=prm, res=O.ref_all2all(syn, prm, threads=8).tolist())
    out["sets"]["vir61/default"] = dict(params={}, res=O.ref_all2all(vir, None, threads=8).tolist())
    # per-region vectors (CParser::get_parsing) for the 12 example genomes, default parameters
    regs = {}
    for r in range(len(ex)):
        for q in range(len(ex)):
            if r != q:
                _, rg = O.ref_pair(ex[r], ex[q], None, want_regions=True)
                if len(rg):
                    regs[f"{r},{q}"] = rg.tolist()
    out["regions_example_default"] = regs
    path = os.path.join(ROOT, "tests", "golden", "ref_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes;", len(out["sets"]), "sets")


if __name__ == "__main__":
    main()
