"""Sparse counting of the k-mer prefilter (include/lzani.h: "Sparse counting") as Python statements: the distinct pairs of
every row, and the tile rule of the pair table -- all rows first, half the height after every overflow, no growing back."""
import numpy as np


def row_pairs(shared, n_ref=0):
    """row_pairs[r] of a shared matrix (PM.shared_matrix): the partners b > r with shared[r, b] >= 1, in the cross form
    (n_ref > 0) the partners b >= n_ref of the n_ref reference rows."""
    s = np.asarray(shared)
    n = s.shape[0]
    if n_ref:
        return np.array([int((s[a, n_ref:] > 0).sum()) for a in range(n_ref)], dtype=np.uint64)
    return np.array([int((s[a, a + 1:] > 0).sum()) for a in range(n)], dtype=np.uint64)


def plan(pairs, slots):
    """(tile_r0[T + 1], attempts), or None where a single row holds more than slots / 2 pairs.  An attempt on the rows
    r0 .. r0 + h is finished iff they hold at most slots / 2 pairs; else h = max(1, h // 2) and r0 is tried again."""
    pairs = [int(x) for x in pairs]
    n = len(pairs)
    r0, h, attempts, tile_r0 = 0, n, 0, [0]
    while r0 < n:
        attempts += 1
        r1 = min(n, r0 + h)
        if sum(pairs[r0:r1]) > slots // 2:
            if h == 1:
                return None
            h = max(1, h // 2)
            continue
        r0 = r1
        tile_r0.append(r0)
    return tile_r0, attempts
