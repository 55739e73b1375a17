"""Plain-Python statements of the out-of-core rules (lz-ani_amd/csrc/lzani_set_plan.h, lzani_tile_plan.h): the genome-table footprint of a
genome, the block plan (lzani_plan_blocks) and the tile schedule of a run (its ordered steps; what lzani_get_residency counts)."""
import numpy as np

import util as U


def _clog2(x):
    return (int(x) - 1).bit_length()


def join_lists(lens, prm):
    """lzani_set_plan.h set_layout_of, without environment overrides: the join form of candidate detection."""
    p = U.full_params(prm)
    f = U.index_form([range(int(L)) for L in lens], p)
    tw = f["tag_words"]
    return bool(tw and 4 * (1 << f["dir_bits"]) >= 8 << 20 and p["mqd"] + p["mrd"] <= 128 and
                _clog2(len(lens) + 1) + f["key_bits"] + f["pos_bits"] <= 64)


def genome_bytes(L, prm, join):
    """Packed text 16 B + N mask 8 B per 64-symbol word, k-mer words 2 x 4 B per text position (mal, msl <= 15), and the
    join lists (8 B per forward position + 20 B) where they apply."""
    p = U.full_params(prm)
    w = (2 * int(L) + 3 * p["mrd"] + 63) // 64 + 2
    return w * 24 + (w * 512 if U.is_fast(p) else 0) + (8 * int(L) + 20 if join else 0)


def min_limit(lens, prm, join=None):
    j = join_lists(lens, prm) if join is None else join
    return 2 * max(genome_bytes(L, prm, j) for L in lens)


def plan_blocks(lens, prm, limit, join=None):
    """block_of[g], or None where the limit is below the minimum (twice the largest genome's footprint).  join: whether
    join lists apply, where an environment override decides it (default: the rule of join_lists)."""
    j = join_lists(lens, prm) if join is None else join
    fp = [genome_bytes(L, prm, j) for L in lens]
    if limit == 0:
        return np.zeros(len(lens), np.uint32)
    if max(fp) > limit // 2:
        return None
    out, b, cur = [], 0, 0
    for g, f in enumerate(fp):
        if g > 0 and cur + f > limit // 2 and cur > 0:
            b, cur = b + 1, 0
        out.append(b)
        cur += f
    return np.array(out, np.uint32)


def block_bytes(lens, prm, block_of, join=None):
    j = join_lists(lens, prm) if join is None else join
    nb = int(block_of.max()) + 1
    out = [0] * nb
    for L, b in zip(lens, block_of):
        out[int(b)] += genome_bytes(L, prm, j)
    return out


def limit_for_blocks(lens, prm, blocks, join=None):
    """The smallest limit (twice a contiguous run's footprint) whose plan has exactly `blocks` blocks, or None."""
    j = join_lists(lens, prm) if join is None else join
    fp = [genome_bytes(L, prm, j) for L in lens]
    sums = sorted({sum(fp[a:b]) for a in range(len(fp)) for b in range(a + 1, len(fp) + 1)})
    for s in sums:
        bo = plan_blocks(lens, prm, 2 * s, j)
        if bo is not None and int(bo.max()) + 1 == blocks:
            return 2 * s
    return None


def steps(block_of, ref_ids, row_off, query_ids, state=(None, None)):
    """The ordered steps of one run from the halves' state (block in A, block in B), as lzani_tile_plan.h's plan_tile_steps
    makes them: reference blocks ascending, those that have rows with pairs; block i to A ("keep" if A holds it, "trade" if B
    holds it and the halves trade places, else "upload"); its query blocks i, then the one B holds, then the others
    ascending, each with whether B uploads it.  Returns ([(i, what A does, [(j, B uploads), ...]), ...], state)."""
    block_of = np.asarray(block_of)
    n, nb = len(block_of), int(block_of.max()) + 1
    size = np.bincount(block_of, minlength=nb)
    rows_of = [[] for _ in range(nb)]
    for k, r in enumerate(ref_ids):
        if row_off[k + 1] > row_off[k]:
            rows_of[int(block_of[r])].append(k)
    a, b = state
    out = []
    for i in range(nb):
        if not rows_of[i]:
            continue
        js = set()
        for k in rows_of[i]:
            r = int(ref_ids[k])
            if query_ids is None:
                js.update(x for x in range(nb) if size[x] > (1 if x == block_of[r] else 0))
            else:
                js.update(int(block_of[q]) for q in query_ids[int(row_off[k]):int(row_off[k + 1])])
        what = "keep"
        if a != i:
            if b == i:
                a, b, what = b, a, "trade"
            else:
                a, what = i, "upload"
        order = ([i] if i in js else []) + ([b] if b is not None and b != i and b in js else [])
        order += sorted(j for j in js if j != i and j != b)
        qs = []
        for j in order:
            up = j != i and b != j
            if up:
                b = j
            qs.append((j, up))
        out.append((i, what, qs))
    return out, (a, b)


def schedule(block_of, ref_ids, row_off, query_ids, state=(None, None)):
    """Tiles and block uploads of one run from the halves' state (block in A, block in B): what steps() lists, counted.
    Returns (tiles, uploads, state)."""
    st, state = steps(block_of, ref_ids, row_off, query_ids, state)
    tiles = sum(len(qs) for _, _, qs in st)
    uploads = sum(what == "upload" for _, what, _ in st) + sum(up for _, _, qs in st for _, up in qs)
    return tiles, int(uploads), state
