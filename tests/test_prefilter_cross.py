"""CPU: the cross form of the k-mer prefilter -- its numpy statement (tests/prefilter_cross_model.py) against a direct
double loop, the row builder cross_rows against a direct statement, and the two entry points of the C-ABI without a GPU."""
import ctypes as C

import numpy as np
import pytest

import lzani_ctypes as L
import prefilter_cross_model as XM
import prefilter_model as PM
import synth_genomes as SG


def _tiny_set():
    r = lambda seed, n: (SG.splitmix64(seed, np.arange(n, dtype=np.uint64)) % np.uint64(4)).astype(np.uint8)
    base = r(1, 90)
    seqs = [base, np.concatenate((base[:50], r(2, 40))), r(3, 70), (3 - base[::-1]).astype(np.uint8), np.concatenate((r(4, 30), base[40:])),
            np.full(40, 5, dtype=np.uint8), r(5, 6), np.concatenate((r(2, 40), r(3, 70)[:35]))]
    return seqs


@pytest.mark.parametrize("k", [8, 12])
def test_restriction_equals_a_double_loop(k):
    seqs = _tiny_set()
    n = len(seqs)
    sets = [set(PM.kmer_set(s, k).tolist()) for s in seqs]
    seen = 0
    for min_shared, min_ratio in ((1, 0.0), (3, 0.2)):
        for n_ref in range(1, n):
            off, ids, sh = [0], [], []
            for a in range(n):
                for b in range(a + 1, n):
                    s = len(sets[a] & sets[b])
                    if a < n_ref <= b and s >= max(min_shared, 1) and s / min(len(sets[a]), len(sets[b])) >= min_ratio:
                        ids.append(b)
                        sh.append(s)
                off.append(len(ids))
            got = XM.prefilter_cross(seqs, k, n_ref, PM.SAMPLE_ALL, min_shared, min_ratio)
            assert got[0].tolist() == [len(x) for x in sets]
            assert got[1].dtype == np.uint64 and got[1].tolist() == off and got[2].tolist() == ids and got[3].tolist() == sh
            assert off[n_ref:] == [len(ids)] * (n - n_ref + 1)                     # the rows from n_ref on are empty
            seen += len(ids)
    assert seen > 0


def _rows_of(ref_ids, row_off, query_ids):
    return {int(r): query_ids[int(row_off[i]):int(row_off[i + 1])].tolist() for i, r in enumerate(ref_ids)}


def test_cross_rows_dense():
    for n, n_ref in ((5, 2), (2, 1), (7, 6), (7, 1)):
        ref_ids, row_off, query_ids = L.cross_rows(n, n_ref)
        assert ref_ids.dtype == np.uint32 and row_off.dtype == np.uint64 and query_ids.dtype == np.uint32
        assert ref_ids.tolist() == list(range(n))
        want = {a: list(range(n_ref, n)) if a < n_ref else list(range(n_ref)) for a in range(n)}
        assert _rows_of(ref_ids, row_off, query_ids) == want
        assert int(row_off[-1]) == len(query_ids) == 2 * n_ref * (n - n_ref)


def test_cross_rows_from_kept_pairs():
    n, n_ref = 7, 3
    pairs = [(0, 4), (0, 6), (2, 3), (2, 4)]                                        # row 1 and the queries 5 have no partner
    pair_off = np.array([0, 2, 2, 4, 4, 4, 4, 4], dtype=np.uint64)
    pair_ids = np.array([b for _, b in pairs], dtype=np.uint32)
    ref_ids, row_off, query_ids = L.cross_rows(n, n_ref, pair_off, pair_ids)
    want = {}
    for a, b in pairs:
        want.setdefault(a, []).append(b)
        want.setdefault(b, []).append(a)
    assert ref_ids.tolist() == sorted(want) == [0, 2, 3, 4, 6]
    assert _rows_of(ref_ids, row_off, query_ids) == {g: sorted(v) for g, v in want.items()}
    empty = L.cross_rows(n, n_ref, np.zeros(n + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    assert len(empty[0]) == 0 and empty[1].tolist() == [0] and len(empty[2]) == 0


def test_entry_points_exported_and_fail_cleanly_without_a_context():
    L.build_library()
    lib = L.load_library()
    for name in ("lzani_prefilter_cross", "lzani_prefilter_codes_cross", "lzani_get_prefilter_cross_info"):
        assert name in L.EXPORTS and getattr(lib, name) is not None
    cnt = C.c_uint64(7)
    assert lib.lzani_prefilter_cross(None, 16, C.c_uint64(PM.SAMPLE_ALL), 1, 0.0, 1, C.byref(cnt)) == -1            # LZANI_ERR_ARG
    seq = np.zeros(40, dtype=np.uint8)
    ptrs = (C.c_void_p * 2)(seq.ctypes.data, seq.ctypes.data)
    lens = np.array([40, 40], dtype=np.uint32)
    assert lib.lzani_prefilter_codes_cross(None, 2, ptrs, lens.ctypes.data_as(C.c_void_p), 16, C.c_uint64(PM.SAMPLE_ALL), 1, 0.0,
                                           C.c_uint64(0), 1, C.byref(cnt)) == -1
    info = L.PrefilterCrossInfo()
    assert lib.lzani_get_prefilter_cross_info(None, C.byref(info)) == -1
    assert cnt.value == 7 and C.sizeof(L.PrefilterCrossInfo) == 24
