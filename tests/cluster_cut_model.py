"""The cut of a cluster level in numpy (float64), over tests/out_filter_model.py, and the edges of a level, over the weight
of tests/cluster_model.py.  Written from the definitions of the level (include/lzani.h, "cluster levels"), not from the
product's code.  For one kept record (a < b, X, Y, lines) with the reported lengths la, lb:
    the five values of line 0 (query b) and line 1 (query a) are the output filter's; a value passes unless it is < its
        minimum (NaN and inf are below nothing)
    len_ratio = min(la, lb) / max(la, lb), one float64 division, where both lengths are nonzero, else 0; both lines pass
        unless len_ratio < its minimum
    num_alns of line 0 is X.no_components, of line 1 Y.no_components; a line passes iff the maximum is 0 or
        num_alns <= the maximum (in 64-bit integers)
    cut_lines = lines & (pass0 | pass1 << 1); the record is an edge iff cut_lines != 0, weighted over the lines that stay
A cut is a dict: minima by name (tani, gani, ani, qcov, rcov, len_ratio), num_alns the maximum; what is missing is 0."""
import numpy as np

import cluster_model as CM
import out_filter_model as M

FIELDS = M.FIELDS + ("len_ratio", "num_alns")


def len_ratio(la, lb):
    la, lb = np.asarray(la, dtype=np.uint32), np.asarray(lb, dtype=np.uint32)
    lo, hi = np.minimum(la, lb).astype(np.float64), np.maximum(la, lb).astype(np.float64)
    both = (la != 0) & (lb != 0)
    return np.where(both, lo / np.where(both, hi, 1.0), 0.0)


def cut_lines(cut, x, y, lines, la, lb):
    """uint32[...]: the lines of `lines` that stay under the cut.  x, y: int[..., 3]."""
    assert set(cut) <= set(FIELDS), cut
    x64, y64 = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    five = M.lines({k: cut.get(k, 0.0) for k in M.FIELDS}, x, y, la, lb)
    with np.errstate(invalid="ignore"):
        ratio_ok = ~(len_ratio(la, lb) < np.float64(cut.get("len_ratio", 0.0)))
    most = int(cut.get("num_alns", 0))
    alns = np.stack((x64[..., 2], y64[..., 2]), axis=-1)
    alns_ok = np.ones(alns.shape, dtype=bool) if most == 0 else alns <= most
    ok = alns_ok & ratio_ok[..., None]
    passes = ok[..., 0].astype(np.uint32) | (ok[..., 1].astype(np.uint32) << np.uint32(1))
    return (np.asarray(lines, dtype=np.uint32) & five & passes).astype(np.uint32)


def level(cut, measure, rec, lens):
    """The level of the KEPT_DTYPE records `rec` under `cut`: (a, b, w of the edges in record order, lines_in, lines_out)."""
    lens = np.asarray(lens, dtype=np.uint32)
    la, lb = lens[rec["a"]], lens[rec["b"]]
    stay = cut_lines(cut, rec["x"], rec["y"], rec["lines"], la, lb) if len(rec) else np.zeros(0, np.uint32)
    keep = stay != 0
    w = CM.weight(measure, rec["x"][keep], rec["y"][keep], stay[keep], la[keep], lb[keep]) if keep.any() else np.zeros(0)
    bits = lambda v: int(((v & 1) + ((v >> 1) & 1)).sum())
    return rec["a"][keep], rec["b"][keep], np.asarray(w, dtype=np.float64), bits(rec["lines"]), bits(stay)
