"""Host statements, in numpy, of what the device builds ahead of the pair kernel: k-mer words, the anchor index of a
reference slot (directory, entries, bucket table, tag words), its presence filter, and the candidate bitmap of a pair.
Everything is derived from the raw symbol codes; nothing here reads a device structure.  test_index_model.py pins the k-mer
port to lzani_core.h through the model library; tests/test_gpu_candidates.py compares the device's slabs and bitmaps
with these statements."""
import numpy as np

BK_EMPTY, BK_OVERFLOW, TW_OVERFLOW = 0xFFFFFFFF, 0xFFFFFFFE, 0x808080FF      # lzani_core.h
IDX_SORT_MAX = 32
PM_TILE = 1024                                                                # lzani_kernels_cand.h


def lowmask(n):
    return (1 << n) - 1 if n > 0 else 0


def ref_text(codes, mrd):
    """The reference text of a genome, one symbol per byte, 4 = N: fwd | N^2mrd | RC | N^mrd (k_pack, ref_text_len)."""
    c = np.minimum(np.asarray(codes, dtype=np.uint8), 4)
    rc = np.where(c[::-1] < 4, 3 - c[::-1], 4).astype(np.uint8)
    pad = np.full(2 * mrd, 4, np.uint8)
    return np.concatenate([c, pad, rc, np.full(mrd, 4, np.uint8)])


def kmer_keys(text, k):
    """(valid bool[T], key uint64[T]) of the k-mer at every text position (kmer_at): valid iff it fits the text and
    holds no N; the first symbol in the low two bits; at k = 32 a k-mer whose first symbol is G or T is absent."""
    T = len(text)
    isn = np.concatenate([[0], np.cumsum(text >= 4)])
    valid = np.zeros(T, bool)
    key = np.zeros(T, np.uint64)
    m = T - k + 1
    if m <= 0:
        return valid, key
    valid[:m] = (isn[k:k + m] - isn[:m]) == 0
    s = np.where(text < 4, text, 0).astype(np.uint64)
    acc = np.zeros(m, np.uint64)
    for j in range(k):
        acc |= s[j:j + m] << np.uint64(2 * j)
    key[:m] = acc
    if k >= 32:
        valid &= (key & np.uint64(2)) == 0
    key[~valid] = 0
    return valid, key


def mix_key(key, kb):
    """The bijective mixer on kb key bits (lzani_core.h mix_key), both branches."""
    x = np.asarray(key, dtype=np.uint64).copy()
    sh = np.uint64((kb + 1) >> 1)
    if kb <= 32:
        m = np.uint64(lowmask(kb))
        for c, last in ((0x9E3779B1, False), (0x85EBCA6B, False), (0xC2B2AE35, True)):
            x = ((x & np.uint64(0xFFFFFFFF)) * np.uint64(c)) & m           # 32-bit product, then the mask
            if not last:
                x ^= x >> sh
        return x
    m = np.uint64(lowmask(kb))
    with np.errstate(over="ignore"):
        for c, last in ((0x9E3779B97F4A7C15, False), (0xD6E8FEB86659FD93, False), (0xC2B2AE3D27D4EB4F, True)):
            x = (x * np.uint64(c)) & m
            if not last:
                x ^= x >> sh
    return x


def kmer_hashes(codes, mrd, mal):
    """(valid, mixed hash) of the mal-mer at every position of the genome's reference text: the k-mer words of k_kmers."""
    valid, key = kmer_keys(ref_text(codes, mrd), mal)
    h = mix_key(key, 2 * mal)
    h[~valid] = 0
    return valid, h


# ---- anchor index of one slot -------------------------------------------------------------------------------------

def index_entries(codes, mrd, mal, geo):
    """(bucket, entry) of every mal-mer of the text, sorted by (bucket, entry): the canonical index.
    geo: key_bits, dir_bits, pos_bits, tag_mask."""
    valid, h = kmer_hashes(codes, mrd, mal)
    p = np.nonzero(valid)[0].astype(np.uint64)
    h = h[valid]
    tb = geo["key_bits"] - geo["dir_bits"]
    bucket = (h >> np.uint64(tb)).astype(np.int64)
    tag = h & np.uint64(lowmask(tb) & geo["tag_mask"])
    entry = ((tag << np.uint64(geo["pos_bits"])) | p).astype(np.uint32)
    order = np.lexsort((entry, bucket))
    return bucket[order], entry[order]


def check_index_slot(codes, mrd, mal, geo, dirz, ent, bk=None, tw=None, fl=None, fmask=None, what=""):
    """The device's slot against the statement:
      dirz   exclusive prefix of the bucket counts, total at dirz[nb]                                 (exact)
      ent    every entry in its bucket; ascending inside buckets of <= IDX_SORT_MAX entries           (exact there,
             larger buckets as multisets)
      bk     per bucket its first four entries, BK_EMPTY padded, word 3 BK_OVERFLOW beyond four      (exact)
      tw     a byte 0x80 | tag per entry of bk, TW_OVERFLOW beyond four, 0 for an empty bucket       (exact)
      fl     bit (v & fmask) for every k-mer word v of the text                                       (exact)"""
    nb = 1 << geo["dir_bits"]
    bucket, want = index_entries(codes, mrd, mal, geo)
    cnt = np.bincount(bucket, minlength=nb)
    want_dirz = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    bad = np.nonzero(dirz[:nb + 1] != want_dirz)[0]
    assert len(bad) == 0, f"{what}: directory differs at {len(bad)} buckets, first {bad[:4].tolist()}: " \
                          f"{dirz[bad[:4]].tolist()} != {want_dirz[bad[:4]].tolist()}"
    n = len(want)
    got = np.asarray(ent[:n], dtype=np.uint32)
    small = cnt[bucket] <= IDX_SORT_MAX
    bad = np.nonzero(small & (got != want))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} entries of sorted buckets differ, first at {bad[:4].tolist()}: " \
                          f"{got[bad[:4]].tolist()} != {want[bad[:4]].tolist()}"
    big = np.lexsort((got, bucket))
    assert np.array_equal(got[big], want), f"{what}: the large buckets do not hold their entries"
    if bk is not None:
        # the first four entries of a bucket in the slot's own entry order (large buckets stay in fill order)
        s = want_dirz[:-1].astype(np.int64)
        want_bk = np.full((nb, 4), BK_EMPTY, np.uint32)
        want_tw = np.zeros(nb, np.uint32)
        pb = geo["pos_bits"]
        for j in range(4):
            has = cnt > j
            e = got[np.minimum(s + j, max(n - 1, 0))] if n else np.zeros(nb, np.uint32)
            want_bk[has, j] = e[has]
            want_tw[has] |= ((0x80 | (e[has].astype(np.uint64) >> np.uint64(pb))) << np.uint64(8 * j)).astype(np.uint32)
        want_bk[cnt > 4, 3] = BK_OVERFLOW
        want_tw[cnt > 4] = TW_OVERFLOW
        gb = np.asarray(bk[:4 * nb], dtype=np.uint32).reshape(nb, 4)
        bad = np.nonzero((gb != want_bk).any(axis=1))[0]
        assert len(bad) == 0, f"{what}: bucket table differs at {len(bad)} buckets, first {bad[:4].tolist()}: " \
                              f"{gb[bad[:2]].tolist()} != {want_bk[bad[:2]].tolist()} (counts {cnt[bad[:2]].tolist()})"
        if tw is not None:
            bad = np.nonzero(tw[:nb] != want_tw)[0]
            assert len(bad) == 0, f"{what}: tag words differ at {len(bad)} buckets, first {bad[:4].tolist()}: " \
                                  f"{[hex(x) for x in tw[bad[:4]]]} != {[hex(x) for x in want_tw[bad[:4]]]}"
    if fl is not None:
        valid, h = kmer_hashes(codes, mrd, mal)
        bits = np.zeros(len(fl) * 32, bool)
        bits[(h[valid] & np.uint64(fmask)).astype(np.int64)] = True
        want_fl = np.packbits(bits, bitorder="little").view(np.uint32)
        bad = np.nonzero(fl != want_fl)[0]
        assert len(bad) == 0, f"{what}: presence filter differs in {len(bad)} words, first {bad[:4].tolist()}"


# ---- candidate bitmaps --------------------------------------------------------------------------------------------

def cand_words(L, mrd):
    """The words of a pair's bitmap k_pm_cand writes for a query of length L: whole tiles of 1,024 positions over
    [0, L + mrd + 320) (the pair kernel reads up to five words beyond its scan position)."""
    return (L + mrd + 320 + PM_TILE - 1) // PM_TILE * (PM_TILE // 32)


def expected_bitmaps(seqs, mrd, mal, rshift, pm_bits, pair_ref, pair_qry, words):
    """uint32[n_pairs, words]: bit p of pair (r, q) set iff p < L_q + mrd, q's mal-mer at p is valid and its matrix row
    (h >> rshift) & (2^pm_bits - 1) is the row of some valid mal-mer of r's text.  Pairs are taken query by query."""
    mmask = np.uint64(lowmask(pm_bits))
    words_of = {}
    rows_of = {}
    is_ref = set(pair_ref.tolist())
    for g in np.unique(np.concatenate([pair_ref, pair_qry])):
        valid, h = kmer_hashes(seqs[g], mrd, mal)
        words_of[int(g)] = (valid, h)
        if int(g) in is_ref:
            rows_of[int(g)] = np.unique((h[valid] >> np.uint64(rshift)) & mmask)
    refs = np.unique(pair_ref)
    allrows = np.unique(np.concatenate([rows_of[int(r)] for r in refs]))
    col = {int(r): j for j, r in enumerate(refs)}
    member = np.zeros((len(allrows), (len(refs) + 7) // 8), np.uint8)        # bit j: row of reference refs[j]
    for r in refs:
        j = col[int(r)]
        member[np.searchsorted(allrows, rows_of[int(r)]), j >> 3] |= np.uint8(1 << (j & 7))
    out = np.zeros((len(pair_ref), words), np.uint32)
    order = np.argsort(pair_qry, kind="stable")
    bounds = np.searchsorted(pair_qry[order], np.unique(pair_qry), side="left").tolist() + [len(order)]
    for a, b in zip(bounds[:-1], bounds[1:]):
        idx = order[a:b]
        q = int(pair_qry[idx[0]])
        D = min(len(seqs[q]) + mrd, words * 32)
        valid, h = words_of[q]
        v, hq = valid[:D], h[:D]
        row = (hq >> np.uint64(rshift)) & mmask
        u = np.minimum(np.searchsorted(allrows, row), len(allrows) - 1)
        hit = v & (allrows[u] == row)
        m = np.unpackbits(member[u], axis=1, bitorder="little")[:, :len(refs)].astype(bool) & hit[:, None]
        cols = np.array([col[int(r)] for r in pair_ref[idx]])
        bits = np.zeros((len(idx), words * 32), bool)
        bits[:, :D] = m[:, cols].T
        out[idx] = np.packbits(bits, axis=1, bitorder="little").view(np.uint32)
    return out


def plain_bitmap(ref_codes, qry_codes, mrd, mal, words):
    """The exact-matrix form without the hash: bit p set iff q's mal-mer at p occurs in r's text (forward or RC)."""
    rv, rk = kmer_keys(ref_text(ref_codes, mrd), mal)
    qv, qk = kmer_keys(ref_text(qry_codes, mrd), mal)
    D = len(qry_codes) + mrd
    bits = np.zeros(words * 32, bool)
    bits[:D] = qv[:D] & np.isin(qk[:D], rk[rv])
    return np.packbits(bits, bitorder="little").view(np.uint32)


def popcounts(words):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1).sum(axis=-1)
