"""CPU: the numpy statements of tests/index_model.py -- reference text, k-mer validity, the mixer's 32- and 64-bit
branches -- against lzani_core.h itself, through the model library (model_kmers)."""
import ctypes as C

import numpy as np
import pytest

import index_model as IM
import oracle as O
import synth_genomes as SG
import util as U


def _genomes():
    st = SG.Stream(4242)
    g = [(st.u64(3000) % np.uint64(4)).astype(np.uint8)]
    x = (st.u64(2500) % np.uint64(4)).astype(np.uint8)
    x[100:160] = 5                                         # a run of N
    x[(st.u64(40) % np.uint64(2500)).astype(np.int64)] = 4  # scattered N
    g.append(x)
    g.append(np.zeros(700, np.uint8))                       # poly-A
    g.append(np.tile(np.array([0, 1, 2, 3, 3, 1], np.uint8), 150))
    g.append(np.array([2, 3, 3], np.uint8))                 # shorter than most k
    return g


@pytest.mark.parametrize("name", ["defaults", "mal1_msl1", "mal9_msl9", "mal15_msl8", "mal16_msl16", "mal31_msl11",
                                  "mal32_msl7", "mqd0_mrd0", "mqd0_mrd64"])
def test_kmer_words_match_core(name):
    prm = U.full_params(None) if name == "defaults" else U.EDGE_TUPLES[name]
    lib = U.model_lib()
    for codes in _genomes():
        T = 2 * len(codes) + 3 * prm["mrd"]
        assert len(IM.ref_text(codes, prm["mrd"])) == T
        for k in sorted({prm["mal"], prm["msl"], 32}):
            valid = np.zeros(T, np.uint8)
            h = np.zeros(T, np.uint64)
            s = np.ascontiguousarray(codes)
            assert lib.model_kmers(O._ptr(s), C.c_uint32(len(s)), O.params_array(prm), C.c_int32(k), O._ptr(valid), O._ptr(h)) == 0
            v, key = IM.kmer_keys(IM.ref_text(codes, prm["mrd"]), k)
            assert np.array_equal(v, valid.astype(bool)), (name, k, len(codes))
            got = IM.mix_key(key, 2 * k)
            got[~v] = 0
            assert np.array_equal(got, h), (name, k, len(codes))


def test_mixer_is_a_bijection_on_small_key_spaces():
    for kb in (2, 8, 14, 18):
        h = IM.mix_key(np.arange(1 << kb, dtype=np.uint64), kb)
        assert len(np.unique(h)) == 1 << kb and int(h.max()) < 1 << kb
