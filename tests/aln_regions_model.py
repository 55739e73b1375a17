"""The alignment-region stage in numpy: which directed entries keep their regions in the file of --out-alignment, and the
order of the regions that stay.  Written from the definitions (the reference's CLZMatcher::store_alignment, lz_matcher.cpp:
102-169), not from the product's header.  Entry e of the call's CSR is the directed pair (ref a, query b); over its regions
    mat = sum of num_matches, lit = sum of num_mismatches                    32-bit integer sums
    gani = mat / len[b],  ani = mat / (mat + lit) or 0 where mat + lit == 0,  qcov = (mat + lit) / len[b]
with a filter the entry is dropped iff gani, ani or qcov is < its minimum (NaN and inf are below nothing); without one no
entry is dropped; entries without a region are neither.  The regions that stay come by ascending e, inside an entry the
longer seq_end - seq_start first, then the smaller seq_start, ties in input order (np.lexsort is stable)."""
import numpy as np

import out_filter_model as M

REGION_DTYPE = np.dtype([("pair", np.uint64), ("ref_start", np.int32), ("ref_end", np.int32), ("seq_start", np.int32),
                         ("seq_end", np.int32), ("num_matches", np.int32), ("num_mismatches", np.int32)])
FIELDS = ("gani", "ani", "qcov")                        # the minima the alignment's rule reads


def sums(entries, regions):
    """(mat int32[entries], lit int32[entries], regions per entry)"""
    p = regions["pair"].astype(np.int64)
    mat = np.zeros(entries, dtype=np.int64)
    lit = np.zeros(entries, dtype=np.int64)
    np.add.at(mat, p, regions["num_matches"].astype(np.int64))
    np.add.at(lit, p, regions["num_mismatches"].astype(np.int64))
    return mat.astype(np.int32), lit.astype(np.int32), np.bincount(p, minlength=entries)


def ratios(mat, lit, length):
    """dict name -> float64[...] of the three values"""
    mat, lit = np.asarray(mat, dtype=np.int32), np.asarray(lit, dtype=np.int32)
    with np.errstate(all="ignore"):
        al = (mat + lit).astype(np.int32)               # (wraps like the hardware's)
        lf, mf, alf = np.asarray(length, dtype=np.uint32).astype(np.float64), mat.astype(np.float64), al.astype(np.float64)
        return dict(gani=mf / lf, ani=np.where(al != 0, mf / np.where(al != 0, alf, 1.0), 0.0), qcov=alf / lf)


def order(n, aln_len, ref_ids, row_off, query_ids, regions, flt=None):
    """(the regions that stay in the result's order, info: entries, found, kept, entries_with_regions, entries_dropped,
    the bool[entries] of the entries that stay, the ratios of every entry)"""
    regions = np.asarray(regions, dtype=REGION_DTYPE)
    entries = int(np.asarray(row_off)[-1]) if len(row_off) else 0
    _, qry = M.entries_of(n, ref_ids, row_off, query_ids)
    mat, lit, cnt = sums(entries, regions)
    r = ratios(mat, lit, np.asarray(aln_len, dtype=np.uint32)[qry] if entries else np.zeros(0, np.uint32))
    dropped = np.zeros(entries, dtype=bool)
    if flt is not None:
        with np.errstate(invalid="ignore"):
            for k in FIELDS:
                dropped |= r[k] < np.float64(flt.get(k, 0.0))
    stays = (cnt > 0) & ~dropped
    keep = regions[stays[regions["pair"].astype(np.int64)]] if len(regions) else regions
    length = keep["seq_end"].astype(np.int64) - keep["seq_start"].astype(np.int64)
    out = keep[np.lexsort((keep["seq_start"], -length, keep["pair"]))]
    info = dict(entries=entries, found=len(regions), kept=len(out), entries_with_regions=int((cnt > 0).sum()),
                entries_dropped=int(((cnt > 0) & dropped).sum()))
    return out, info, stays, r


def bits(v):
    return int(v).bit_length()


def sort_passes(entries, kept):
    """the radix passes (8 bits each) of the three sorts: by seq_start, by maxlen - length, by the entry -- each over the bits
    the field's largest value among the regions that stay has (the entry: entries - 1)"""
    if not len(kept):
        return 0
    length = kept["seq_end"].astype(np.int64) - kept["seq_start"].astype(np.int64)
    return sum((bits(v) + 7) // 8 for v in (kept["seq_start"].max(), length.max(), entries - 1))


def lists(rows):
    """[(ref, [queries])] -> ref_ids, row_off, query_ids"""
    ref = np.array([r for r, _ in rows], dtype=np.uint32)
    off = np.cumsum([0] + [len(q) for _, q in rows]).astype(np.uint64)
    return ref, off, np.array([x for _, qs in rows for x in qs], dtype=np.uint32)


def dense(n, rows=None):
    """ref_ids, row_off, None of dense rows"""
    ref = np.arange(n, dtype=np.uint32) if rows is None else np.asarray(rows, dtype=np.uint32)
    return ref, np.arange(len(ref) + 1, dtype=np.uint64) * np.uint64(max(n - 1, 0)), None


def random_rows(rng, n, kind):
    """dense: a random subset of the rows in random order; lists: rows in random order, ascending lists, some of them empty"""
    order = rng.permutation(n)[:int(rng.integers(1, n + 1))]
    if kind == "dense":
        return dense(n, order)
    rows = []
    for r in order:
        others = np.array([x for x in range(n) if x != r])
        k = 0 if rng.random() < 0.2 else int(rng.integers(1, n))
        rows.append((int(r), np.sort(rng.choice(others, k, replace=False)).tolist()))
    return lists(rows)


def random_regions(rng, entries, count, maxv, owners=None, ties=0.1):
    """count made-up regions: starts below maxv, lengths 1 .. maxv, among the entries `owners` (default: a random 70 % of
    them, so that some own none); a share `ties` repeats the entry, start and end of another record with counts of its own"""
    r = np.zeros(count, dtype=REGION_DTYPE)
    if not entries or not count:
        return r[:0]
    if owners is None:
        owners = np.flatnonzero(rng.random(entries) < 0.7)
        if not len(owners):
            owners = np.array([int(rng.integers(0, entries))])
    r["pair"] = rng.choice(np.asarray(owners), count)
    r["seq_start"] = rng.integers(0, maxv, count)
    length = rng.integers(1, maxv + 1, count)
    r["seq_end"] = r["seq_start"] + length
    tie = np.flatnonzero(rng.random(count) < ties)
    src = rng.integers(0, count, len(tie))
    for k in ("pair", "seq_start", "seq_end"):
        r[k][tie] = r[k][src]
    length = r["seq_end"] - r["seq_start"]
    r["num_matches"] = (rng.random(count) * (length + 1)).astype(np.int32)
    r["num_mismatches"] = (rng.random(count) * (length - r["num_matches"] + 1)).astype(np.int32)
    r["ref_start"] = rng.integers(0, 1 << 20, count)
    r["ref_end"] = r["ref_start"] + length
    return r


def random_call(seed, n=None, kind=None, count=None, maxv=None):
    """(n, aln_len, ref_ids, row_off, query_ids, regions) of one made-up call"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(3, 13)) if n is None else n
    kind = ("dense", "lists")[int(rng.integers(0, 2))] if kind is None else kind
    maxv = int((200, 60000, 1 << 22)[int(rng.integers(0, 3))]) if maxv is None else maxv
    ref, off, q = random_rows(rng, n, kind)
    count = int(rng.integers(8, 400)) if count is None else count
    regs = random_regions(rng, int(off[-1]), count, maxv)
    aln_len = rng.integers(1, 6 * maxv, n).astype(np.uint32)
    aln_len[rng.random(n) < 0.05] = 0
    return n, aln_len, ref, off, q, regs


def median_filters(n, aln_len, ref, off, q, regs):
    """for gani, ani and qcov: a filter at the median of the value over the call's entries that own a region (a value of the
    data itself, finite ones only); None where fewer than four entries have a finite value"""
    _, _, stays, r = order(n, aln_len, ref, off, q, regs)
    out = {}
    for k in FIELDS:
        v = np.sort(r[k][stays & np.isfinite(r[k])])
        out[k] = {k: float(v[len(v) // 2])} if len(v) >= 4 else None
    return out


def aln_line(qname, rname, reg, ref_len, mrd):
    """One line of the alignment file (store_alignment, lz_matcher.cpp:140-166), without its newline: pident in the TSV's
    number format with six digits, positions from 1, a region of the reverse strand in forward coordinates."""
    import util as U
    length = int(reg["seq_end"]) - int(reg["seq_start"])
    pident = U.real_to_str(100.0 * int(reg["num_matches"]) / length, 6)
    rs, re_ = int(reg["ref_start"]), int(reg["ref_end"])
    if rs < ref_len:
        r0, r1 = 1 + rs, re_
    else:
        corr = 2 * ref_len + 2 * mrd + 1
        r0, r1 = corr - (1 + rs), corr - re_
    return "\t".join([qname, rname, pident, str(length), str(1 + int(reg["seq_start"])), str(int(reg["seq_end"])), str(r0), str(r1),
                      str(int(reg["num_matches"])), str(int(reg["num_mismatches"]))])
