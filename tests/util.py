"""Shared helpers of the test-suite: fixture loading, seeded edge cases, the TSV emit rule."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np

import oracle as O
import synth_genomes as SG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

VARIANTS = {
    "default": {},
    "long": dict(mal=15, msl=9, reg=60),                  # BASELINE config 4 parameters
    "mrd20_mqd60": dict(mrd=20, mqd=60),
    "aw10_am3_ar5": dict(aw=10, am=3, ar=5),
    "short": dict(mrd=10, mqd=10, mal=9, msl=5, reg=20),
}


def load_example():
    recs = O.read_multifasta(os.path.join(GOLD, "example", "multifasta.fna"))
    return [r[0] for r in recs], [r[1] for r in recs]


def load_vir61():
    """--in-dir semantics: files sorted by name, every '>' record one item (multisample default)."""
    names, seqs = [], []
    for f in sorted(glob.glob(os.path.join(GOLD, "vir61", "*.fna"))):
        for nm, s in O.read_multifasta(f):
            names.append(nm)
            seqs.append(s)
    return names, seqs


def reorder(names, seqs):
    """CSeqReservoir::reorder_items (seq_reservoir.cpp:215-251): (len - 2*no_parts) as uint32, descending,
    then name ascending (bytewise); stable."""
    key = [((len(s) - 2) & 0xFFFFFFFF) for s in seqs]
    order = sorted(range(len(seqs)), key=lambda i: (-key[i], names[i].encode()))
    return [names[i] for i in order], [seqs[i] for i in order]


def edge_set():
    """Seeded corner cases: copies, reverse complement, N runs, SNPs, tiny and empty inputs, repeats."""
    st = SG.Stream(5)
    base = (st.u64(3000) % np.uint64(4)).astype(np.uint8)
    rc = (3 - base[::-1]).astype(np.uint8)
    snp = base.copy()
    snp[::50] = (snp[::50] + 1) % 4
    nins = np.concatenate([base[:1500], np.full(50, 5, np.uint8), base[1500:]])
    mosaic = np.concatenate([base[100:900], rc[1000:2000], base[2100:2500]])
    return [base, base.copy(), rc, nins, snp, base[:1500].copy(), np.full(200, 5, np.uint8),
            base[:12].copy(), base[:5].copy(), np.zeros(0, np.uint8), np.zeros(500, np.uint8),
            np.tile(np.array([0, 1], np.uint8), 400), mosaic,
            np.concatenate([np.full(3, 5, np.uint8), base[:700], np.full(1, 5, np.uint8), base[700:1400]])]


# ---- the reference's number formatting and TSV emit rule (lz_matcher.cpp:280-579,
# ---- numeric_conversions.h:228-300), restated for the tests -------------------------------
def real_to_str(v, prec):
    if v == 0:
        return "0"
    r = repr(float(v))
    mant, _, ex = r.partition("e")
    exp10 = int(ex) if ex else 0
    if "." in mant:
        ip, fp = mant.split(".")
    else:
        ip, fp = mant, ""
    digits = (ip + fp).lstrip("0")
    exp10 -= len(fp)
    lead_stripped = len(ip + fp) - len((ip + fp).lstrip("0"))
    del lead_stripped
    t = digits.rstrip("0")
    exp10 += len(digits) - len(t)
    sig = int(t)
    nd = len(t)
    if nd > prec:
        p10 = 10 ** (nd - prec)
        sig = (sig + p10 // 2) // p10
        exp10 += nd - prec
        nd = prec
        if sig >= 10 ** prec:
            sig //= 10
            exp10 += 1
    s = str(sig)
    if exp10 == 0:
        return s
    if exp10 > 0 or -exp10 >= nd + 4:
        e = exp10
        if nd == 1:
            out = s
        else:
            out = s[0] + "." + s[1:]
            e += nd - 1
        return out + ("e-%02d" % -e if e < 0 else "e+%02d" % e)
    if -exp10 < nd:
        k = nd + exp10
        return s[:k] + "." + s[k:]
    return "0." + "0" * (-exp10 - nd) + s


def emit_tsv(names, lens, res, columns, in_percent=False):
    """store_results for dense results res[r, q] (ids already in reordered order)."""
    mult = 100.0 if in_percent else 1.0
    lines = ["\t".join(columns)]
    n = len(names)
    for a in range(n):
        for b in range(a + 1, n):
            X = res[a, b]   # parse(query=b, ref=a)
            Y = res[b, a]   # parse(query=a, ref=b)
            ids = (a, b)
            ln = (lens[b], lens[a])
            mat = (int(X[0]), int(Y[0]))
            lit = (int(X[1]), int(Y[1]))
            reg = (int(X[2]), int(Y[2]))
            tani = (mat[0] + mat[1]) / (ln[0] + ln[1])
            gani = (mat[0] / ln[0], mat[1] / ln[1])
            ani = tuple(m / (m + l) if m + l else 0.0 for m, l in zip(mat, lit))
            cov = ((mat[0] + lit[0]) / ln[0], (mat[1] + lit[1]) / ln[1])
            for i in (0, 1):
                j = 1 - i
                f = {"ridx": str(ids[i]), "qidx": str(ids[j]), "reference": names[ids[i]], "query": names[ids[j]],
                     "qcov": real_to_str(mult * cov[i], 6), "rcov": real_to_str(mult * cov[j], 6),
                     "gani": real_to_str(mult * gani[i], 6), "ani": real_to_str(mult * ani[i], 6),
                     "tani": real_to_str(mult * tani, 6), "rlen": str(ln[j]), "qlen": str(ln[i]),
                     "num_alns": str(reg[i]), "nt_match": str(mat[i]), "nt_mismatch": str(lit[i])}
                if ln[0] and ln[1]:
                    f["len_ratio"] = real_to_str(min(ln[i], ln[j]) / max(ln[i], ln[j]), 4)
                else:
                    f["len_ratio"] = "0"
                lines.append("\t".join(f[c] for c in columns))
    return "\n".join(lines) + "\n"


STANDARD = "qidx,ridx,query,reference,tani,gani,ani,qcov,num_alns,len_ratio".split(",")
OUT_FORMATS = ("standard", "lite", "complete", "lite,rlen,qlen", "nt_match,standard", "query,reference,tani", "rcov")


def format_real_cases():
    """Seeded (value, precision) cases of the TSV number formatting: edge values, ratios, percentages, random magnitudes
    and random bit patterns."""
    import random
    import struct
    rnd = random.Random(3)
    vals = [0.0, 1.0, 0.5, 1e-7, 4e-7, 0.000364, 0.98725, 0.999999, 0.9999995, 0.99999949, 9.9999995, 123456.5,
            1234567.0, 1e21, 1e22, 5e-324, 1.7976931348623157e308]
    for _ in range(20000):
        k = rnd.random()
        if k < 0.5:
            v = rnd.randint(0, 10 ** rnd.randint(1, 7)) / rnd.randint(1, 10 ** rnd.randint(1, 7))
        elif k < 0.7:
            v = 100.0 * rnd.randint(0, 50000) / rnd.randint(1, 50000)
        elif k < 0.9:
            v = rnd.random() * 10 ** rnd.randint(-12, 12)
        else:
            v = struct.unpack("d", struct.pack("Q", rnd.getrandbits(62)))[0]
        if v == v and v != float("inf"):
            vals.append(v)
    return [(v, (4, 6, 6, 6, 1, 2, 9, 15)[i % 8]) for i, v in enumerate(vals)]


def live_set():
    """The synthetic set of the live oracle-vs-reference comparison: 30 genomes in families of 5, an N run in one."""
    _, seqs = SG.make_set(30, 21, lmin=4000, lmax=12000, fam=5)
    seqs[3] = np.concatenate([seqs[3][:2000], np.full(30, 5, np.uint8), seqs[3][2000:]])
    return seqs


LIVE_PARAMS = {"default": None, "long": dict(mal=15, msl=9, reg=60), "mrd25_mqd55_aw20_am9_ar2": dict(mrd=25, mqd=55, aw=20, am=9, ar=2)}


def load_ref_live():
    """What the reference build answered on live_set, OUT_FORMATS and format_real_cases (oracle/make_goldens.py)."""
    import json
    with open(os.path.join(GOLD, "ref_live_vectors.json")) as f:
        return json.load(f)


# ---- the lane-emulating host model of the kernels (tests/model) --------------------------
_model = None


def model_lib():
    global _model
    if _model is None:
        d = os.path.join(ROOT, "tests", "model")
        so = os.path.join(d, "liblzani_model.so")
        src = os.path.join(d, "lzani_model.cpp")
        hdrs = [os.path.join(ROOT, "lz-ani_amd", "csrc", h) for h in ("lzani_core.h", "lzani_layout.h")]
        if not os.path.exists(so) or any(os.path.getmtime(x) > os.path.getmtime(so) for x in [src] + hdrs):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", so])
        _model = C.CDLL(so)
    return _model


def model_all2all(seqs, params=None):
    lib = model_lib()
    seqs, ptrs, lens = O._seq_table(seqs)
    n = len(seqs)
    out = np.zeros((n, n, 3), dtype=np.int32)
    rc = lib.model_all2all(n, ptrs, O._ptr(lens), O.params_array(params), O._ptr(out))
    if rc != 0:
        raise ValueError("model: unsupported parameters")
    return out


def model_split_all2all(seqs, params=None, seglen=1000):
    """Every pair by several segments (lzani_core.h: checkpoints, segments, stitch) through the host model: (results, stats)
    with stats = [pairs stitched, segments run again after a void stitch, segments in all, segments skipped by the hand-overs].
    The fourth is two counts in one number, on purpose (tests/model/lzani_model.cpp: "counted apart"): a stitched pair adds
    its segments that no hand-over reached, and a pair that eight repair rounds did not stitch -- it is scanned whole -- adds
    1,000,000.  So stats[3] // 1,000,000 pairs were not stitched (stats[0] + that = all pairs), and stats[3] % 1,000,000 < stats[2]
    segments were skipped: 2,000,244 on a set of 20 pairs with 18 stitched is 2 pairs and 244 segments."""
    lib = model_lib()
    seqs, ptrs, lens = O._seq_table(seqs)
    n = len(seqs)
    out = np.zeros((n, n, 3), dtype=np.int32)
    stats = np.zeros(4, dtype=np.int64)
    rc = lib.model_split_all2all(n, ptrs, O._ptr(lens), O.params_array(params), int(seglen), O._ptr(out), O._ptr(stats))
    if rc != 0:
        raise ValueError("model: unsupported parameters")
    return out, stats


SPLIT_STAT_FIELDS = ("pairs_cut", "rounds", "resumed", "given_up")      # then voids[6]: lzani_split_stats, Engine.split_stats()


def model_split_rounds(seqs, params=None, seglen=512, S=None, give_up=-1, heavy=None):
    """Every pair the way the device's split runs it (run_split + k_split_stitch: rounds of segments and stitches, a void
    segment's cut disabled and the segment before it resumed, after give_up rounds every cut disabled and segment 0 run
    fresh) through the host model: (results, stats), stats as Engine.split_stats() plus "max_resumes_of_a_pair" and
    "pairs_with_void".
    S: the cuts of every pair (default: split_plan's for this set); give_up < 0: the device's rule, 6 + S / 4;
    heavy: bool[n, n], the pairs that are cut (default: all)."""
    lib = model_lib()
    p = full_params(params)
    if S is None:
        dmax = max(len(s) for s in seqs) + p["mrd"]
        S, seglen = split_plan(len(seqs) * (len(seqs) - 1), (dmax + 320 + 1023) // 1024 * 32, dmax, {"LZANI_SPLIT": "1", "LZANI_SPLIT_SEGLEN": str(seglen)})
    seqs, ptrs, lens = O._seq_table(seqs)
    n = len(seqs)
    out = np.zeros((n, n, 3), dtype=np.int32)
    stats = np.zeros(12, dtype=np.int64)
    hv = None if heavy is None else np.ascontiguousarray(heavy, dtype=np.uint8)
    rc = lib.model_split_rounds(n, ptrs, O._ptr(lens), O.params_array(params), int(seglen), int(S), int(give_up),
                                None if hv is None else O._ptr(hv), O._ptr(out), O._ptr(stats))
    if rc == -2:
        raise RuntimeError("model: no end of rounds")
    if rc != 0:
        raise ValueError("model: unsupported parameters")
    st = {k: int(stats[i]) for i, k in enumerate(SPLIT_STAT_FIELDS)}
    st["voids"] = [int(v) for v in stats[4:10]]
    st["max_resumes_of_a_pair"] = int(stats[10])
    st["pairs_with_void"] = int(stats[11])
    return out, st


def model_pair_regions(ref, qry, params=None):
    """(result triple, regions sorted like calc_regions) through the ALN instantiation of the model."""
    lib = model_lib()
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    qry = np.ascontiguousarray(qry, dtype=np.uint8)
    res = np.zeros(3, dtype=np.int32)
    regs = np.zeros((1 << 14, 6), dtype=np.int32)
    n = C.c_uint32(0)
    rc = lib.model_pair_regions(O._ptr(ref), len(ref), O._ptr(qry), len(qry), O.params_array(params), O._ptr(res),
                                O._ptr(regs), 1 << 14, C.byref(n))
    if rc != 0:
        raise ValueError("model: unsupported parameters")
    g = regs[:n.value]
    order = sorted(range(len(g)), key=lambda k: (-(int(g[k][3]) - int(g[k][2])), int(g[k][2])))
    return tuple(int(x) for x in res), g[order]


DEFAULTS = dict(mal=11, msl=7, mrd=40, mqd=40, reg=35, aw=15, am=7, ar=3)


def fuzz_case_medium(st):
    """Like fuzz_case, at genome sizes where the tag words, the bucket table and the LDS index build are in
    use (8-70 kbp, mal <= 12): an ancestor, two mutated copies (one with an inversion or N runs), one stranger."""
    msl = st.randint(4, 9)
    mal = st.randint(max(msl, 9), 12)
    mrd = st.randint(8, 64)
    prm = dict(mal=mal, msl=msl, mrd=mrd, mqd=st.randint(4, min(mrd, 64)), reg=st.randint(10, 80), aw=st.randint(4, 40),
               am=st.randint(1, 12), ar=st.randint(1, 6))
    pick = st.one()
    if pick < 0.3:
        prm = dict(DEFAULTS)
    elif pick < 0.45:                          # the second parameter set the pair kernel folds into its code (null chain included)
        prm = dict(DEFAULTS, **VARIANTS["long"])
    L = st.randint(8000, 70000)
    base = (st.u64(L) % np.uint64(4)).astype(np.uint8)
    seqs = [base, SG.mutate(base, 0.01 + 0.12 * st.one(), st)]
    g = SG.mutate(base, 0.02 + 0.2 * st.one(), st).copy()
    if st.one() < 0.5:
        for _ in range(st.randint(1, 3)):
            a = st.randint(0, len(g) - 200)
            g[a:a + st.randint(1, 120)] = 5
    else:
        a = st.randint(0, len(g) - 3000)
        g[a:a + 2500] = (3 - g[a:a + 2500][::-1])
    seqs.append(np.ascontiguousarray(g))
    seqs.append((st.u64(st.randint(8000, 70000)) % np.uint64(4)).astype(np.uint8))
    return prm, seqs


def fuzz_params_chain(st):
    """A random parameter tuple INSIDE what the hand-written null chain is written for (chain_params_ok in
    lzani_kernels_pairs.h: mqd <= 62, 64 <= mqd + mrd <= 127, 2 <= aw <= 15, ar <= aw, msl <= 9) and inside the reference's
    own well-defined range (mqd <= mrd); never one of the two tuples compiled ahead of time."""
    while True:
        mrd = st.randint(32, 64)
        mqd = st.randint(64 - mrd, min(mrd, 62, 127 - mrd))
        msl = st.randint(4, 9)
        aw = st.randint(2, 15)
        prm = dict(mal=st.randint(max(msl, 9), 13), msl=msl, mrd=mrd, mqd=mqd, reg=st.randint(10, 80), aw=aw,
                   am=st.randint(0, aw), ar=st.randint(0, min(aw, 6)))
        if prm != DEFAULTS and prm != dict(DEFAULTS, **VARIANTS["long"]):
            return prm


def fuzz_seqs_medium(st, with_n=None):
    """The sequences of fuzz_case_medium (an ancestor, two mutated copies, a stranger; 8-70 kbp); with_n: False = no N
    anywhere (the N-free kernel instantiation), True = N runs in one copy, None = either."""
    L = st.randint(8000, 70000)
    base = (st.u64(L) % np.uint64(4)).astype(np.uint8)
    seqs = [base, SG.mutate(base, 0.01 + 0.12 * st.one(), st)]
    g = SG.mutate(base, 0.02 + 0.2 * st.one(), st).copy()
    n_runs = st.one() < 0.5 if with_n is None else with_n
    if n_runs:
        for _ in range(st.randint(1, 3)):
            a = st.randint(0, len(g) - 200)
            g[a:a + st.randint(1, 120)] = 5
    else:
        a = st.randint(0, len(g) - 3000)
        g[a:a + 2500] = (3 - g[a:a + 2500][::-1])
    seqs.append(np.ascontiguousarray(g))
    seqs.append((st.u64(st.randint(8000, 70000)) % np.uint64(4)).astype(np.uint8))
    return seqs


def fuzz_case_large(st):
    """Like fuzz_case_medium at 0.3-1.2 Mbp: directories of 2^20 buckets and more (the sort-based index build) and, from
    ~0.5 Mbp on, tag words of 8 MB (candidates by the join): an ancestor, a mutated copy, a stranger."""
    prm, _ = fuzz_case_medium(st)
    L = st.randint(300_000, 1_200_000)
    base = (st.u64(L) % np.uint64(4)).astype(np.uint8)
    g = SG.mutate(base, 0.01 + 0.1 * st.one(), st).copy()
    if st.one() < 0.5:
        a = st.randint(0, len(g) - 500)
        g[a:a + st.randint(1, 300)] = 5
    other = (st.u64(st.randint(300_000, 1_200_000)) % np.uint64(4)).astype(np.uint8)
    return prm, [base, np.ascontiguousarray(g), other]


def fuzz_case(st):
    """One random differential case: LZ parameters inside the engine's envelope with mqd <= mrd (beyond
    that the reference reads past the end of its reference text, parser.cpp:288/713, and its answer
    depends on stale heap bytes), and five short genomes: an ancestor, mutated copies, unrelated
    sequences, N runs, reverse complements, low-complexity repeats."""
    wide = st.one() < 0.2                      # long k-mers / wide seed windows: the engine's generic paths
    msl = st.randint(1, 20 if wide else 12)
    mal = st.randint(msl, min(28 if wide else 16, msl + 8))
    mrd = st.randint(0, 300 if wide else 64)
    prm = dict(mal=mal, msl=msl, mrd=mrd, mqd=st.randint(0, min(mrd, 64)), reg=st.randint(1, 80), aw=st.randint(1, 64),
               am=st.randint(0, 20), ar=st.randint(0, 12))
    base = (st.u64(st.randint(50, 1500)) % np.uint64(4)).astype(np.uint8)
    seqs = [base]
    for _ in range(4):
        if st.one() < 0.8:
            g = SG.mutate(base, 0.01 + 0.25 * st.one(), st)
        else:
            g = (st.u64(st.randint(20, 1500)) % np.uint64(4)).astype(np.uint8)
        if st.one() < 0.3:
            g = g.copy()
            a = st.randint(0, max(0, len(g) - 10))
            g[a:a + st.randint(1, 30)] = 5
        if st.one() < 0.2:
            g = (3 - g[::-1]).astype(np.uint8)
            g[g > 3] = 5
        if st.one() < 0.15:
            g = np.tile(g[:st.randint(1, 6)], 60)[:400]
        seqs.append(np.ascontiguousarray(g))
    return prm, seqs


# ---- the LZ parameter envelope at its edges ---------------------------------------------------
# Plain-Python restatements of the C predicates that decide which form of the pair path a tuple takes, written from the C
# source (not generated from it), so that the tests can predict the form and check that it ran.
FAST_MAX_K = 15                                       # per-genome k-mer words exist for mal, msl <= 15 (lzani_set_plan.h)
AOT_SETS = {"defaults": dict(DEFAULTS), "long": dict(DEFAULTS, mal=15, msl=9, reg=60)}     # folded in ahead of time (DEFP 1, 2)


def full_params(prm=None):
    return dict(DEFAULTS, **(prm or {}))


def params_supported(prm):
    """lzani_layout.h: params_supported -- the envelope of the wave formulation (LZANI_ERR_PARAMS outside)."""
    p = full_params(prm)
    return (1 <= p["msl"] <= 32 and 1 <= p["mal"] <= 32 and 0 <= p["mrd"] <= 1 << 20 and 0 <= p["mqd"] <= 64 and
            1 <= p["aw"] <= 64 and p["ar"] <= 64 and p["am"] >= 0)


def chain_params_ok(prm):
    """lzani_kernels_pairs.h: chain_params_ok -- the tuples the hand-written null chain is written for."""
    p = full_params(prm)
    return (1 <= p["mal"] <= 15 and 1 <= p["msl"] <= 9 and 0 <= p["mqd"] <= 62 and p["mrd"] >= 1 and
            64 <= p["mqd"] + p["mrd"] <= 127 and 2 <= p["aw"] <= 15 and p["ar"] <= p["aw"] and p["am"] >= 0 and
            0 <= p["reg"] < 1 << 20)


def is_fast(prm):
    p = full_params(prm)
    return p["mal"] <= FAST_MAX_K and p["msl"] <= FAST_MAX_K


def is_aot(prm):
    return full_params(prm) in AOT_SETS.values()


def index_form(seqs, prm, join=False):
    """The anchor index of this genome set without environment overrides (lzani_layout.h: index_geometry; lzani_set_plan.h:
    set_layout_of): exact tags (the stored tag identifies the k-mer), a bucket table, tag words; whether the index is built
    by sorting, the presence filter and the most slabs a batch may take.  join: the set takes the join form of candidate
    detection (ooc_model.join_lists), which has no filter."""
    p = full_params(prm)
    T = 2 * max([len(s) for s in seqs] + [0]) + 3 * p["mrd"]
    clog2 = lambda x: (int(x) - 1).bit_length()           # smallest b with 2^b >= x (x >= 1)
    kb, posbits = 2 * p["mal"], max(1, clog2(T + 1))
    dirbits = min(max(8, min(clog2(max(T, 1)), 26)), kb)
    tagbits = min(kb - dirbits, 32 - posbits)
    exact = tagbits == kb - dirbits
    bk = is_fast(p) and exact and dirbits <= 26 and tagbits + posbits <= 30
    tw = bk and tagbits <= 7
    # directories of 2^20 buckets and more are built by a radix sort of 64-bit keys: slot number, hash, position -- the slot
    # number gets what hash and position leave, 16 bits at the most, and all ones is no slot
    sort_build = is_fast(p) and dirbits >= 20 and kb + posbits <= 60
    max_slots = min(65535, (1 << min(16, 64 - kb - posbits)) - 1) if sort_build else 65535     # 65535: gridDim.y
    # presence filter (probe form with tag words): f = ceil(log2 T) + 1 bits of the hash, texts below 1,024 symbols counted as
    # 1,024, 18 bits at the most (32 KB of LDS); no filter for texts beyond 2^18 symbols: one all-ones word, mask 31
    tbits = clog2(max(T, 1024))
    fbits = min(tbits + 1, 18) if tw and not join and tbits <= 18 else 0
    return dict(exact=exact, bucket_table=bk, tag_words=tw, T=T, key_bits=kb, dir_bits=dirbits, pos_bits=posbits,
                sort_build=sort_build, max_slots=max_slots, filter_bits=fbits, filter_mask=(1 << fbits) - 1 if fbits else 31)


# One table of edge tuples, a name per row; every row keeps mqd <= mrd (see fuzz_case).  Each row changes one group of
# knobs from the defaults: the seed window and the tracking steps (mqd/mrd), the approximate extension (aw/am/ar), the
# k-mer lengths (mal/msl) and the region length (reg).
EDGE_GROUPS = {
    "mqd_mrd": {"mqd0_mrd0": dict(mqd=0, mrd=0), "mqd0_mrd64": dict(mqd=0, mrd=64),
                "mqd24_mrd40": dict(mqd=24, mrd=40),            # window of 64: the chain's lower bound
                "mqd62_mrd65": dict(mqd=62, mrd=65),            # 63 tracking steps, window of 127: the chain's upper bounds
                "mqd63_mrd64": dict(mqd=63, mrd=64),            # 64 tracking steps: outside the chain
                "mqd40_mrd88": dict(mqd=40, mrd=88), "mqd63_mrd65": dict(mqd=63, mrd=65),    # window of 128: outside the chain
                "mqd64_mrd64": dict(mqd=64, mrd=64),            # 65 tracking steps
                "mqd64_mrd1000": dict(mqd=64, mrd=1000)},       # window beyond 128: no candidate bitmaps, no split
    "aw_am_ar": {"aw1_am0_ar0": dict(aw=1, am=0, ar=0), "aw2_am0_ar2": dict(aw=2, am=0, ar=2),
                 "aw2_am1_ar0": dict(aw=2, am=1, ar=0),         # AR = max(ar, 1) in ChainP
                 "aw15_am15_ar15": dict(aw=15, am=15, ar=15),
                 "aw15_am20_ar0": dict(aw=15, am=20, ar=0),     # AM = min(am, 16) in ChainP
                 "aw16_am7_ar3": dict(aw=16, am=7, ar=3),       # outside the chain
                 "aw64_am64_ar64": dict(aw=64, am=64, ar=64), "aw64_am64_ar-3": dict(aw=64, am=64, ar=-3)},
    "mal_msl": {"mal1_msl1": dict(mal=1, msl=1), "mal15_msl1": dict(mal=15, msl=1), "mal9_msl9": dict(mal=9, msl=9),
                "mal7_msl9": dict(mal=7, msl=9),                # mal < msl
                "mal15_msl8": dict(mal=15, msl=8),              # msl 8, 9: the hashed seed-bitmap mapping
                "mal15_msl15": dict(mal=15, msl=15), "mal16_msl16": dict(mal=16, msl=16),   # the FAST limit
                "mal31_msl11": dict(mal=31, msl=11),
                "mal32_msl7": dict(mal=32, msl=7), "mal32_msl11": dict(mal=32, msl=11),     # 32-symbol k-mers (quirk Q14)
                "mal32_msl32": dict(mal=32, msl=32)},
    "reg": {"reg-1": dict(reg=-1), "reg0": dict(reg=0), "reg1": dict(reg=1),
            "reg100000": dict(reg=100000)},                     # longer than every genome
}
EDGE_TUPLES = {name: full_params(d) for g in EDGE_GROUPS.values() for name, d in g.items()}
REF_MAX_MSL = 11                  # beyond, the reference's 4^msl short-seed table is the limit (see the fuzz tests)


def edge_params(st):
    """A random tuple drawn from the edges: every group of knobs from one of its edge rows or left at the defaults."""
    p = dict(DEFAULTS)
    for rows in EDGE_GROUPS.values():
        names = sorted(rows)
        k = st.randint(0, len(names))
        if k < len(names):
            p.update(rows[names[k]])
    return p


# every bound of params_supported: (knob, value one step inside, value one step outside)
ENVELOPE_BOUNDS = [("msl", 1, 0), ("msl", 32, 33), ("mal", 1, 0), ("mal", 32, 33), ("mrd", 0, -1), ("mrd", 1 << 20, (1 << 20) + 1),
                   ("mqd", 0, -1), ("mqd", 64, 65), ("aw", 1, 0), ("aw", 64, 65), ("ar", 64, 65), ("am", 0, -1)]


def bound_pair(knob, ok, bad):
    """(tuple one step inside the bound, the same tuple one step outside), the rest at the defaults with mqd <= mrd."""
    inside = dict(DEFAULTS, **{knob: ok})
    if knob == "mrd":
        inside["mqd"] = min(inside["mqd"], ok)
    else:
        inside["mrd"] = max(inside["mrd"], inside["mqd"])
    return inside, dict(inside, **{knob: bad})


def envelope_family_set(with_n=True):
    """The family set of the envelope tests: 8 genomes of 6-9 kbp in families of 3; with_n puts N runs into three of
    them (a run at the start, one in the middle, one at the end)."""
    _, seqs = SG.make_set(8, 91, lmin=6000, lmax=9000, fam=3)
    seqs = [s.copy() for s in seqs]
    if with_n:
        seqs[1][:7] = 5
        seqs[4][3000:3000 + 40] = 5
        seqs[6][3500:3520] = 5
        seqs[6][-3:] = 5
    return seqs


# ---- the pair-kernel instantiations and the launch record ---------------------------------------
# The library names every pair-kernel instantiation its dispatch can launch (lzani_debug_kernel_name) and counts the launches
# of a context's last run per name (Engine.kernel_launches).  The table and the choice of a launch's kernel live in
# lzani_pair_dispatch.h (choose_pair_kernel), the facts it goes by are gathered in lzani_hip.hip (run_rows_impl, run_batch,
# launch_pairs).  The matrix below is written from those rules, not copied from the library's table;
# tests/test_instantiations.py checks the two against each other and against the kernel symbols of the gfx950 code object,
# tests/test_pair_dispatch.py pair_kernel_choice against choose_pair_kernel over every combination of the facts.
PAIRS_NAME = "pairs fast={} nfree={} defp={} aln={} bk={} cand={}"


def expected_kernel_names():
    """Every pair-kernel instantiation the dispatch can launch.  defp: 0 generic, 1 the defaults, 2 --mal 15 --msl 9
    --reg 60 (folded where candidates come from bitmaps or the join, and in the split); bk = the tag-word anchor queue;
    cand: 0 probe, 1 join, 2 candidate bitmaps."""
    names = [PAIRS_NAME.format(0, 0, 0, 1, 0, 0), PAIRS_NAME.format(1, 0, 0, 1, 1, 0), PAIRS_NAME.format(1, 0, 0, 1, 0, 0),  # regions
             PAIRS_NAME.format(0, 0, 0, 0, 0, 0)]                                                                            # no k-mer words
    names += [PAIRS_NAME.format(1, nf, d, 0, 1, cand) for cand in (2, 1) for nf in (0, 1) for d in (0, 1, 2)]
    names += [PAIRS_NAME.format(1, nf, d, 0, bk, 0) for bk in (1, 0) for nf in (0, 1) for d in (0, 1)]
    names += ["pairs_blk nfree={} defp={}".format(nf, d) for nf in (0, 1) for d in (0, 1)]
    names += ["split nfree={} defp={} mode={}".format(nf, d, m) for nf in (0, 1) for d in (0, 1, 2) for m in (0, 1)]
    names += ["rtc nfree={} cand={}".format(nf, cand) for nf in (0, 1) for cand in (0, 1, 2)]
    return names


KERNEL_NAME_RE = (r"^(pairs fast=[01] nfree=[01] defp=[012] aln=[01] bk=[01] cand=[012]|pairs_blk nfree=[01] defp=[01]|"
                  r"split nfree=[01] defp=[012] mode=[01]|rtc nfree=[01] cand=[012])$")


def _clog2(x):
    return (int(x) - 1).bit_length() if x > 1 else 0


WAVE_SLOTS = 256 * 8 * 4                # wave slots of the MI355X: 256 CUs, 8 blocks of 4 waves


def split_rule(n_pairs, cb_words, dmax, env=None, slots=WAVE_SLOTS):
    """Whether a dense batch of n_pairs pairs with candidate bitmaps of cb_words words is split -- its pairs scanned by
    several waves each -- restated from lzani_run_plan.h (choose_split), not a call into the library.  dmax: the longest
    genome + mrd; env: the LZANI_SPLIT* switches that are set."""
    env = env or {}
    if "LZANI_SPLIT" in env:
        on = env["LZANI_SPLIT"][:1] == "1"
    else:
        on = cb_words >= 8192 and (n_pairs * 16 <= slots or (cb_words >= 65536 and n_pairs * 8 <= slots))
    if not on or n_pairs * 2 > 0xFFFFFFFF // 64:            # (segment numbers are 32 bits)
        return False
    if int(env.get("LZANI_SPLIT_SEGLEN", 0)) > 0:
        seglen = int(env["LZANI_SPLIT_SEGLEN"])
    else:
        S = min(max(2, int(env.get("LZANI_SPLIT_S", 64))), max(2, slots // n_pairs))
        seglen = -(-dmax // S)
    seglen = max(seglen, 512)
    return -(-dmax // seglen) >= 2


def split_plan(n_pairs, cb_words, dmax, env=None, slots=WAVE_SLOTS):
    """(S, seglen) of a split batch -- the cuts of every pair and the query positions between two cuts -- restated from
    lzani_run_plan.h (choose_split) as split_rule is; (0, 0) where the batch is not split."""
    env = env or {}
    if not split_rule(n_pairs, cb_words, dmax, env, slots):
        return 0, 0
    ceil_div = lambda a, b: -(-a // b)
    S = min(max(2, int(env.get("LZANI_SPLIT_S", 64))), max(2, slots // n_pairs))
    seglen = ceil_div(dmax, S)
    if int(env.get("LZANI_SPLIT_SEGLEN", 0)) > 0:
        seglen = int(env["LZANI_SPLIT_SEGLEN"])
        S = min(64, max(2, ceil_div(dmax, seglen)))
    seglen = max(seglen, 512)
    return min(S, ceil_div(dmax, seglen)), seglen


def pair_kernel_choice(regions, fast, tw, pm, split, join, blk, nfree, dsel, rtc):
    """(the ahead-of-time name, the run-time compiled name tried first or None) of one pair launch, from the facts
    lzani_pair_dispatch.h (PairFacts) goes by -- restated, not a call into the library.  A split: its mode-0 name.
    dsel: 0 generic, 1 the defaults, 2 the long-genome tuple, which the probe forms and the block kernel run generic."""
    nf, d_probe = int(nfree), int(dsel == 1)
    if regions:
        return PAIRS_NAME.format(int(fast), 0, 0, 1, int(fast and tw), 0), None
    if not fast:
        return PAIRS_NAME.format(0, 0, 0, 0, 0, 0), None
    if pm and split:
        return "split nfree={} defp={} mode=0".format(nf, dsel), None
    cand = 2 if pm else 1 if join and tw else 0 if tw else None
    rtc_name = "rtc nfree={} cand={}".format(nf, cand) if rtc and cand is not None else None
    if cand in (2, 1):
        return PAIRS_NAME.format(1, nf, dsel, 0, 1, cand), rtc_name
    if blk:
        return "pairs_blk nfree={} defp={}".format(nf, d_probe), None
    return PAIRS_NAME.format(1, nf, d_probe, 0, int(tw), 0), rtc_name


def predict_kernels(seqs, prm, env=None, form="all2all", pairs_per_row=None, n_rows=None, rtc_ready=False):
    """The names a run launches (lzani_hip.hip: run_rows_impl), from the genome set, the tuple, the environment (the
    LZANI_* switches that are set) and the call: form "all2all" (dense rows), "dup_lists" (query lists that name a
    query twice in a row: never candidate bitmaps), "regions" (lzani_run_rows_regions).  rtc_ready: the run-time
    compiled kernel of the tuple is available (compiled or in the disk cache).  One batch, memory to spare, a block
    kernel whose LDS filter fits."""
    env = env or {}
    on = lambda k: env.get(k, "")[:1] == "1"
    off = lambda k: env.get(k, "")[:1] == "0"
    p = full_params(prm)
    n = len(seqs)
    g = index_form(seqs, p)
    fast = is_fast(p)
    bk = g["bucket_table"] and not on("LZANI_NO_BUCKETS")
    tw = bk and g["tag_words"] and not on("LZANI_NO_TAGWORDS")
    window = p["mqd"] + p["mrd"] <= 128
    join_mode = (tw and 4 * (1 << g["dir_bits"]) >= int(env.get("LZANI_JOIN_MIN_BYTES", 8 << 20)) and window and
                 _clog2(n + 1) + g["key_bits"] + g["pos_bits"] <= 64 and not on("LZANI_NO_JOIN"))
    nf = int(all((s < 4).all() for s in seqs))
    d_fold = 1 if p == AOT_SETS["defaults"] else 2 if p == AOT_SETS["long"] else 0     # bitmaps, join, split
    if form == "regions" or not fast:
        return {pair_kernel_choice(form == "regions", fast, tw, False, False, False, False, nf, d_fold, False)[0]}
    n_rows = n if n_rows is None else n_rows
    pairs_per_row = n - 1 if pairs_per_row is None else pairs_per_row
    n_pairs = n_rows * pairs_per_row
    min_rows = max(1, int(env["LZANI_PM_MIN_ROWS"])) if "LZANI_PM_MIN_ROWS" in env else 2 if join_mode else 32 if tw else 8
    assert form in ("all2all", "dup_lists") or (form == "lists" and (off("LZANI_PM") or not bk)), form
    pm = form == "all2all" and bk and window and g["key_bits"] <= 30 and n >= 2 and n_rows >= min_rows and not off("LZANI_PM")
    use_join = join_mode and not pm
    Lmax = max(len(s) for s in seqs)
    split = False
    if pm:
        cb_words = (Lmax + p["mrd"] + 320 + 1023) // 1024 * 32
        split = split_rule(n_pairs, cb_words, Lmax + p["mrd"], env)
    fl = tw and not join_mode and _clog2(max(g["T"], 1024)) <= int(env.get("LZANI_FILTER_MAX_BITS", 18)) and not on("LZANI_NO_FILTER")
    blk = (not pm and tw and not join_mode and fl and pairs_per_row >= 128 and
           (on("LZANI_BLOCK_KERNEL") if "LZANI_BLOCK_KERNEL" in env else form == "all2all"))
    rtc = rtc_ready and not off("LZANI_RTC") and d_fold == 0
    aot, rtc_name = pair_kernel_choice(False, fast, tw, pm, split, use_join, blk, nf, d_fold, rtc)
    if aot.startswith("split "):
        return {aot, aot.replace("mode=0", "mode=1")}              # (a split batch runs both modes)
    return {rtc_name or aot}


# The cells of tests/test_gpu_instantiations.py: one per name of the table (two per run-time compiled kernel: a tuple
# inside the null chain's envelope with mal 13, one outside).  A cell = a genome set, a tuple, the LZANI_* switches that
# force the form, and a call: "all2all", "lists" (a few queries per reference), "dup_lists" (rows of >= 128 pairs, every
# query many times), "regions".
INST_PARAMS = {"defaults": dict(DEFAULTS), "long": dict(DEFAULTS, mal=15, msl=9, reg=60),
               "generic": full_params(dict(mrd=50, mqd=30, reg=40, aw=12, am=5, ar=2)),
               "slow": full_params(dict(mal=20, msl=9, reg=40)),                    # no k-mer words
               "rtc_chain": full_params(dict(mal=13, msl=9, reg=40)),               # null chain, stretch chain of the join form
               "rtc_plain": full_params(dict(msl=10, mqd=20, mrd=70, aw=20, am=9, ar=2, reg=40))}
_INST_FORM_ENV = {"bitmaps": {"LZANI_PM_MIN_ROWS": "1", "LZANI_SPLIT": "0"}, "join": {"LZANI_JOIN_MIN_BYTES": "1", "LZANI_PM": "0"},
                  "probe": {"LZANI_PM": "0"}, "block": {"LZANI_PM": "0", "LZANI_BLOCK_KERNEL": "1"},
                  "split": {"LZANI_PM_MIN_ROWS": "1", "LZANI_SPLIT": "1", "LZANI_SPLIT_SEGLEN": "1500", "LZANI_SPLIT_ALL": "1"}}


def _inst_cells():
    cells = []

    def add(name, setname, prm, env, form, tag=""):
        rtc = name.startswith("rtc ")
        env = dict(env, **({"LZANI_RTC_MIN_PAIRS": "0"} if rtc else {"LZANI_RTC": "0"}))
        cells.append(dict(id=name.replace(" ", "_").replace("=", "") + tag, name=name, set=setname, prm=prm, env=env, form=form))

    nsuf = {0: " N", 1: ""}
    add(PAIRS_NAME.format(0, 0, 0, 1, 0, 0), "small N", "slow", {}, "regions")
    add(PAIRS_NAME.format(1, 0, 0, 1, 1, 0), "small N", "defaults", {}, "regions")
    add(PAIRS_NAME.format(1, 0, 0, 1, 0, 0), "small N", "generic", {"LZANI_NO_TAGWORDS": "1"}, "regions")
    add(PAIRS_NAME.format(0, 0, 0, 0, 0, 0), "small N", "slow", {}, "lists")
    for nf in (0, 1):
        for d, prm in ((0, "generic"), (1, "defaults"), (2, "long")):
            add(PAIRS_NAME.format(1, nf, d, 0, 1, 2), ("split" if d == 2 else "small") + nsuf[nf], prm, _INST_FORM_ENV["bitmaps"], "all2all")
            add(PAIRS_NAME.format(1, nf, d, 0, 1, 1), ("long" if d == 2 else "small") + nsuf[nf], prm, _INST_FORM_ENV["join"],
                "lists" if d == 0 else "all2all")
            add("split nfree={} defp={} mode=0".format(nf, d), "split" + nsuf[nf], prm, _INST_FORM_ENV["split"], "all2all")
        for d, prm in ((0, "generic"), (1, "defaults")):
            add(PAIRS_NAME.format(1, nf, d, 0, 1, 0), "small" + nsuf[nf], prm, _INST_FORM_ENV["probe"], "lists" if nf == d else "all2all")
            add(PAIRS_NAME.format(1, nf, d, 0, 0, 0), "small" + nsuf[nf], prm,
                dict(_INST_FORM_ENV["probe"], **({"LZANI_NO_TAGWORDS": "1"} if nf == 0 else {"LZANI_NO_BUCKETS": "1"})), "all2all")
            add("pairs_blk nfree={} defp={}".format(nf, d), "small" + nsuf[nf], prm, _INST_FORM_ENV["block"], "dup_lists")
        for cand, form in ((0, "probe"), (1, "join"), (2, "bitmaps")):
            for prm in ("rtc_chain", "rtc_plain"):
                setname = ("mid" if prm == "rtc_chain" and cand < 2 else "small") + nsuf[nf]
                add("rtc nfree={} cand={}".format(nf, cand), setname, prm, _INST_FORM_ENV[form], "all2all", "_" + prm)
    return cells


INST_CELLS = _inst_cells()


def kernel_names_of_cell(cell):
    """What the cell must launch: its name; a split cell both modes of its k_split."""
    if cell["name"].startswith("split "):
        return {cell["name"][:-1] + "0", cell["name"][:-1] + "1"}
    return {cell["name"]}


def _put_n_runs(seqs):
    """N runs at the start (genome 1), in the middle (4) and at the end (6, with one in the middle); 7 shares a family with 6:
    a related pair with N on both sides.  The rest stay N-free: pairs of N-free genomes in a run of an NFREE=false kernel."""
    seqs = [s.copy() for s in seqs]
    seqs[1][:9] = 5
    seqs[4][len(seqs[4]) // 2:len(seqs[4]) // 2 + 40] = 5
    seqs[6][-5:] = 5
    seqs[6][1200:1217] = 5
    seqs[7][2000:2001] = 5
    return seqs


_INST_SETS = {}


def instantiation_set(name):
    """Genome sets of the cells: related pairs (families at 0.5-15 % divergence), unrelated pairs, one genome of 300 bp;
    ' N' = with N runs (_put_n_runs).  small: 9 genomes of 8.5-10 kbp (tag words at mal 11 from ~8.2 kbp on); split: 8 of
    17-25 kbp; mid: + one of 140 kbp and a relative (tag words at mal 13); long: + one of 2.2 Mbp and a relative (tag
    words at mal 15)."""
    if name not in _INST_SETS:
        base, with_n = name.split(" ")[0], name.endswith(" N")
        st = SG.Stream(4242)
        short = (st.u64(300) % np.uint64(4)).astype(np.uint8)
        if base == "split":
            seqs = SG.make_set(8, 4301, lmin=17000, lmax=25000, fam=4, dmin=0.005, dmax=0.15)[1]
        else:
            seqs = SG.make_set(9, 4302, lmin=8500, lmax=10000, fam=3, dmin=0.005, dmax=0.15)[1]
        if with_n:
            seqs = _put_n_runs(seqs)
        if base in ("mid", "long"):
            L = 140_000 if base == "mid" else 2_200_000
            big = (st.u64(L) % np.uint64(4)).astype(np.uint8)
            seqs = [big, SG.mutate(big, 0.02, st)] + seqs[:8]
            if with_n:
                seqs[0] = seqs[0].copy()
                seqs[0][L // 3:L // 3 + 100] = 5
        _INST_SETS[name] = [np.ascontiguousarray(s) for s in seqs] + [short]
    return _INST_SETS[name]


def instantiation_rows(cell, n):
    """(ref_ids, row_off, query_ids or None) of the cell's call (query_ids None: dense rows)."""
    ref_ids = np.arange(n, dtype=np.uint32)
    if cell["form"] in ("all2all", "regions"):
        return ref_ids, np.arange(n + 1, dtype=np.uint64) * np.uint64(n - 1), None
    if cell["form"] == "lists":
        lists = [[(r + d) % n for d in (1, 2, 4)] for r in range(n)]
    else:
        lists = [[q for q in range(n) if q != r] * (128 // (n - 1) + 1) for r in range(n)]
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    return ref_ids, off, np.array([q for x in lists for q in x], np.uint32)


# ---- the split's repair loop: void segments, resumes, the give-up round -----------------------------------------
# tools/split_void_search.py looks through seeded small sets for ones whose split run (cuts every 512 positions) has void
# segments on the host model; tests/test_split_repair.py and tests/test_gpu_split_repair.py run its finds, listed in
# SPLIT_REPAIR_TABLE as (class, seed) with the model's counts at the device's give-up rule.
SPLIT_REPAIR_ENV = {"LZANI_RTC": "0", "LZANI_PM_MIN_ROWS": "1", "LZANI_SPLIT": "1", "LZANI_SPLIT_SEGLEN": "512", "LZANI_SPLIT_ALL": "1"}
SPLIT_REPAIR_CLASSES = ("generic", "defaults", "long", "wide")
SPLIT_REPAIR_DEFP = {"generic": 0, "wide": 0, "defaults": 1, "long": 2}        # the split kernels' defp


def split_repair_case(cls, seed):
    """(tuple, genomes) of one seeded case of the search: 2-4 genomes of 4-9 kbp, one family (an ancestor and mutated copies
    at 8-28 % divergence; the generic and wide classes from 1 % on), in two cases out of five with an N run in one genome.
    generic: a random tuple with mal, msl <= 15 and mqd <= mrd <= 64 that is neither of the two folded ahead of time; wide:
    the same from fuzz_case's wider ranges (msl from 1, aw up to 64, am up to 20, ar up to 12, mrd and mqd from 0)."""
    st = SG.Stream(0x5EED00000000 + 1000003 * SPLIT_REPAIR_CLASSES.index(cls) + seed)
    n = st.randint(2, 4)
    with_n = st.one() < 0.4
    if cls == "wide":
        while True:
            msl = st.randint(1, 12)
            mrd = st.randint(0, 64)
            prm = dict(mal=st.randint(msl, min(15, msl + 8)), msl=msl, mrd=mrd, mqd=st.randint(0, min(mrd, 64)), reg=st.randint(1, 80),
                       aw=st.randint(1, 64), am=st.randint(0, 20), ar=st.randint(0, 12))
            if prm not in AOT_SETS.values():
                break
        dmin = 0.01
    elif cls == "generic":
        while True:
            msl = st.randint(3, 12)
            mrd = st.randint(8, 64)
            prm = dict(mal=st.randint(max(msl, 6), 15), msl=msl, mrd=mrd, mqd=st.randint(4, min(mrd, 64)), reg=st.randint(10, 80),
                       aw=st.randint(4, 40), am=st.randint(1, 12), ar=st.randint(1, 6))
            if prm not in AOT_SETS.values():
                break
        dmin = 0.01
    else:
        prm = dict(AOT_SETS[cls])
        dmin = 0.08
    seqs = SG.make_set(n, 7919 * seed + 13, lmin=4000, lmax=9000, fam=n, dmin=dmin, dmax=0.28)[1]
    if with_n:
        g = st.randint(0, n - 1)
        a = st.randint(0, len(seqs[g]) - 100)
        seqs[g] = seqs[g].copy()
        seqs[g][a:a + st.randint(1, 60)] = 5
    return prm, [np.ascontiguousarray(s) for s in seqs]


# What the search found (tools/split_void_search.py; the classes' seeds 0 .. 19,999, defaults 0 .. 9,999, long 0 .. 59,999):
# per entry the model's counts at the device's give-up rule.  wide 85 and 675 run out of rounds by that rule: one pair each
# is given up.
SPLIT_REPAIR_TABLE = [
    dict(cls='wide', seed=85, nfree=1, pairs_cut=12, rounds=11, resumed=21, given_up=1, voids=[12, 3, 0, 0, 7, 0], max_resumes_of_a_pair=9),
    dict(cls='wide', seed=145, nfree=0, pairs_cut=6, rounds=2, resumed=2, given_up=0, voids=[1, 1, 0, 0, 0, 0], max_resumes_of_a_pair=1),
    dict(cls='wide', seed=675, nfree=0, pairs_cut=6, rounds=12, resumed=13, given_up=1, voids=[12, 1, 0, 0, 1, 0], max_resumes_of_a_pair=10),
    dict(cls='wide', seed=974, nfree=0, pairs_cut=2, rounds=2, resumed=1, given_up=0, voids=[0, 0, 1, 0, 0, 0], max_resumes_of_a_pair=1),
    dict(cls='wide', seed=1698, nfree=0, pairs_cut=2, rounds=3, resumed=3, given_up=0, voids=[3, 0, 0, 0, 0, 0], max_resumes_of_a_pair=2),
    dict(cls='wide', seed=2423, nfree=0, pairs_cut=12, rounds=2, resumed=5, given_up=0, voids=[0, 0, 0, 4, 1, 0], max_resumes_of_a_pair=1),
    dict(cls='wide', seed=2937, nfree=1, pairs_cut=12, rounds=2, resumed=3, given_up=0, voids=[0, 1, 2, 0, 0, 0], max_resumes_of_a_pair=1),
    dict(cls='generic', seed=46, nfree=1, pairs_cut=12, rounds=5, resumed=18, given_up=0, voids=[0, 0, 0, 0, 18, 0], max_resumes_of_a_pair=4),
    dict(cls='generic', seed=274, nfree=1, pairs_cut=12, rounds=4, resumed=8, given_up=0, voids=[0, 8, 0, 0, 0, 0], max_resumes_of_a_pair=3),
    dict(cls='generic', seed=770, nfree=0, pairs_cut=12, rounds=5, resumed=13, given_up=0, voids=[0, 13, 0, 0, 0, 0], max_resumes_of_a_pair=4),
    dict(cls='generic', seed=976, nfree=0, pairs_cut=12, rounds=7, resumed=18, given_up=0, voids=[0, 0, 0, 0, 18, 0], max_resumes_of_a_pair=6),
    dict(cls='generic', seed=16419, nfree=1, pairs_cut=12, rounds=3, resumed=8, given_up=0, voids=[2, 5, 0, 1, 0, 0], max_resumes_of_a_pair=2),
    dict(cls='generic', seed=18986, nfree=0, pairs_cut=2, rounds=2, resumed=1, given_up=0, voids=[0, 0, 1, 0, 0, 0], max_resumes_of_a_pair=1),
    dict(cls='defaults', seed=2134, nfree=0, pairs_cut=6, rounds=2, resumed=1, given_up=0, voids=[0, 1, 0, 0, 0, 0], max_resumes_of_a_pair=1),
    dict(cls='defaults', seed=2144, nfree=1, pairs_cut=12, rounds=2, resumed=1, given_up=0, voids=[0, 1, 0, 0, 0, 0], max_resumes_of_a_pair=1),
    dict(cls='defaults', seed=2272, nfree=1, pairs_cut=12, rounds=2, resumed=1, given_up=0, voids=[0, 1, 0, 0, 0, 0], max_resumes_of_a_pair=1),
    dict(cls='defaults', seed=2398, nfree=0, pairs_cut=6, rounds=2, resumed=1, given_up=0, voids=[0, 1, 0, 0, 0, 0], max_resumes_of_a_pair=1),
    dict(cls='defaults', seed=2562, nfree=1, pairs_cut=2, rounds=2, resumed=1, given_up=0, voids=[0, 1, 0, 0, 0, 0], max_resumes_of_a_pair=1),
    dict(cls='defaults', seed=3005, nfree=0, pairs_cut=6, rounds=2, resumed=1, given_up=0, voids=[0, 1, 0, 0, 0, 0], max_resumes_of_a_pair=1),
    dict(cls='long', seed=1343, nfree=1, pairs_cut=2, rounds=2, resumed=1, given_up=0, voids=[0, 1, 0, 0, 0, 0], max_resumes_of_a_pair=1),
    dict(cls='long', seed=1675, nfree=0, pairs_cut=12, rounds=2, resumed=1, given_up=0, voids=[0, 1, 0, 0, 0, 0], max_resumes_of_a_pair=1),
    dict(cls='long', seed=2439, nfree=0, pairs_cut=6, rounds=2, resumed=1, given_up=0, voids=[0, 1, 0, 0, 0, 0], max_resumes_of_a_pair=1),
    dict(cls='long', seed=3108, nfree=1, pairs_cut=6, rounds=2, resumed=2, given_up=0, voids=[0, 2, 0, 0, 0, 0], max_resumes_of_a_pair=1),
]
SPLIT_REPAIR_IDS = ["{}_{}".format(e["cls"], e["seed"]) for e in SPLIT_REPAIR_TABLE]
# entries of four genomes whose voids all lie in the rows of one half of the references (two batches of two rows)
SPLIT_REPAIR_ONE_BATCH = [("wide", 85), ("wide", 2937), ("defaults", 2144), ("long", 1675)]
_split_repair_cache = {}


def split_repair_base(cls, seed):
    """(tuple, genomes, the oracle's results) of a case of the search, made once."""
    key = (cls, seed)
    if key not in _split_repair_cache:
        prm, seqs = split_repair_case(cls, seed)
        _split_repair_cache[key] = (prm, seqs, O.oracle_all2all(seqs, prm, threads=4))
    return _split_repair_cache[key]


def split_repair_model(cls, seed, give_up=-1):
    """(results, stats) of the model's split run of a case at cuts every 512 positions, made once per give-up rule."""
    key = (cls, seed, give_up)
    if key not in _split_repair_cache:
        prm, seqs, _ = split_repair_base(cls, seed)
        _split_repair_cache[key] = model_split_rounds(seqs, prm, seglen=512, give_up=give_up)
    return _split_repair_cache[key]


def split_partial_case(form):
    """A defaults case of the search with a stranger appended (shorter than the longest genome: the cuts and the index
    geometry stay), for a run that cuts some pairs only: (tuple, genomes, candidate counts int[n, n], threshold, switches).
    A pair is cut where its candidates -- the set bits of its bitmap, by the exact statement (index_model.plain_bitmap: the
    matrix of the defaults' 11-mers is exact) -- reach the threshold.  form "thr": LZANI_SPLIT_THR, between the stranger's
    pairs and the family's; form "all0": LZANI_SPLIT_ALL=0, whose threshold is the words of a pair's bitmap (a candidate at
    one position in 32) whatever LZANI_SPLIT_THR says, which parts the family's pairs."""
    import index_model as IM
    key = ("partial", form)
    if key not in _split_repair_cache:
        prm, seqs, _ = split_repair_base("defaults", 2144)
        st = SG.Stream(977)
        seqs = list(seqs) + [(st.u64(min(len(s) for s in seqs) - 100) % np.uint64(4)).astype(np.uint8)]
        n = len(seqs)
        words = IM.cand_words(max(len(s) for s in seqs), prm["mrd"])
        cnt = np.array([[int(IM.popcounts(IM.plain_bitmap(seqs[r], seqs[q], prm["mrd"], prm["mal"], words))) if r != q else 0
                         for q in range(n)] for r in range(n)])
        env = dict(SPLIT_REPAIR_ENV)
        del env["LZANI_SPLIT_ALL"]
        if form == "thr":
            thr = 20
            env["LZANI_SPLIT_THR"] = str(thr)
        else:
            thr = words
            env.update(LZANI_SPLIT_ALL="0", LZANI_SPLIT_THR="20")
        _split_repair_cache[key] = (prm, seqs, cnt, thr, env)
    return _split_repair_cache[key]
