"""The output filter in numpy (float64): which lines of an unordered pair pass the minima, and the kept records of a CSR
call.  Written from the definitions (the reference's CLZMatcher::store_results, lz_matcher.cpp:437-462), not from the
product's header: X = result of (ref a, query b), Y = result of (ref b, query a) for a < b, la / lb the reported lengths;
    tani = (X.m + Y.m) / (la + lb)                    the sums in 32-bit integers (int32 the matches, uint32 the lengths)
    line 0 (query b): gani = X.m / lb, ani = X.m / (X.m + X.l) or 0 where X.m + X.l == 0, qcov = (X.m + X.l) / lb,
                      rcov = (Y.m + Y.l) / la
    line 1 (query a): the same with X and Y, la and lb exchanged
a line passes unless one of its five values is < its minimum (NaN and inf are below nothing); the pair is kept iff a line
passes.  Records come in the order of the leading entries (a < b) of the CSR; a leading entry whose mate (ref b, query a)
is not in the call is unpaired: dropped and counted."""
import numpy as np

FIELDS = ("tani", "gani", "ani", "qcov", "rcov")
KEPT_DTYPE = np.dtype([("a", np.uint32), ("b", np.uint32), ("x", np.int32, (3,)), ("y", np.int32, (3,)), ("lines", np.uint32)])


def _i32(v):
    return np.asarray(v, dtype=np.int64).astype(np.int32)


def ratios(x, y, la, lb):
    """The five values of both lines: dict name -> float64[..., 2] (index 0: the line of query b).  x, y: int[..., 3]."""
    x, y = _i32(x), _i32(y)
    la, lb = np.asarray(la, dtype=np.uint32), np.asarray(lb, dtype=np.uint32)
    with np.errstate(all="ignore"):
        m = np.stack((x[..., 0], y[..., 0]), axis=-1)                            # own matches of line 0 / line 1
        al = np.stack((x[..., 0] + x[..., 1], y[..., 0] + y[..., 1]), axis=-1)   # int32 sums (wrap like the hardware's)
        qlen = np.stack((lb, la), axis=-1).astype(np.float64)
        tani1 = (x[..., 0] + y[..., 0]).astype(np.float64) / (la + lb).astype(np.float64)
        alf, mf = al.astype(np.float64), m.astype(np.float64)
        ani = np.where(al != 0, mf / np.where(al != 0, alf, 1.0), 0.0)
        return dict(tani=np.stack((tani1, tani1), axis=-1), gani=mf / qlen, ani=ani, qcov=alf / qlen,
                    rcov=alf[..., ::-1] / qlen[..., ::-1])


def lines(flt, x, y, la, lb):
    """uint32[...]: bit 0 the line of query b passes, bit 1 the line of query a.  flt: dict name -> minimum (missing: 0)."""
    r = ratios(x, y, la, lb)
    ok = np.ones(r["tani"].shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        for k in FIELDS:
            ok &= ~(r[k] < np.float64(flt.get(k, 0.0)))
    return (ok[..., 0].astype(np.uint32) | (ok[..., 1].astype(np.uint32) << np.uint32(1))).astype(np.uint32)


def entries_of(n, ref_ids, row_off, query_ids):
    """(ref, query) of every directed entry of the CSR; dense rows (query_ids None) list every id but their own, ascending."""
    ref_ids = np.asarray(ref_ids, dtype=np.int64)
    row_off = np.asarray(row_off, dtype=np.int64)
    ref = np.repeat(ref_ids, np.diff(row_off))
    if query_ids is not None:
        return ref, np.asarray(query_ids, dtype=np.int64)
    j = np.arange(len(ref), dtype=np.int64) - np.repeat(row_off[:-1], np.diff(row_off))
    return ref, j + (j >= ref)


def kept(flt, n, report_len, ref_ids, row_off, query_ids, results):
    """(records KEPT_DTYPE in the order of the leading entries, unpaired, leading, lines of every paired leading entry,
    the entry indexes of those)."""
    ref, qry = entries_of(n, ref_ids, row_off, query_ids)
    res = _i32(results).reshape(-1, 3)
    at = {(int(r), int(q)): e for e, (r, q) in enumerate(zip(ref, qry))}         # (distinct ref_ids, ascending lists: no key twice)
    assert len(at) == len(ref)
    lead = np.flatnonzero(qry > ref)
    mate = np.array([at.get((int(qry[e]), int(ref[e])), -1) for e in lead], dtype=np.int64)
    unpaired = int((mate < 0).sum())
    lead, mate = lead[mate >= 0], mate[mate >= 0]
    rl = np.asarray(report_len, dtype=np.uint32)
    ln = lines(flt, res[lead], res[mate], rl[ref[lead]], rl[qry[lead]]) if len(lead) else np.zeros(0, np.uint32)
    keep = ln != 0
    rec = np.zeros(int(keep.sum()), dtype=KEPT_DTYPE)
    rec["a"], rec["b"] = ref[lead][keep], qry[lead][keep]
    rec["x"], rec["y"], rec["lines"] = res[lead][keep], res[mate][keep], ln[keep]
    return rec, unpaired, int((qry > ref).sum()), ln, lead
