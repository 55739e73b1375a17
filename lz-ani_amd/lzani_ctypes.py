"""ctypes binding of the C-ABI in include/lzani.h (liblzani_hip.so).

Used by the test-suite, bench.py and __graft_entry__.py.  It is deliberately thin: the product
is the shared library; this module only marshals numpy arrays into the plain pointers and sizes
the ABI takes.  There is no CPU fallback: if the HIP library is missing or a call fails, it raises.

Interface mirror: `Engine` plays the role of the reference's CParser + the worker loop of
CLZMatcher::do_matching (/root/reference/src/parser.h:237-253, lz_matcher.cpp:172-277):
construct with the LZ parameters, hand over the sequences, run rows of (reference, queries).
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.environ.get("LZANI_LIB") or os.path.join(HERE, "liblzani_hip.so")   # LZANI_LIB: diagnostic builds
SRC = os.path.join(HERE, "csrc", "lzani_hip.hip")

PARAM_ORDER = ("mal", "msl", "mrd", "mqd", "reg", "aw", "am", "ar")
DEFAULT_PARAMS = dict(mal=11, msl=7, mrd=40, mqd=40, reg=35, aw=15, am=7, ar=3)

ERRORS = {-1: "LZANI_ERR_ARG", -2: "LZANI_ERR_PARAMS", -3: "LZANI_ERR_DEVICE",
          -4: "LZANI_ERR_STATE", -5: "LZANI_ERR_NOMEM"}

EXPORTS = ("lzani_default_params", "lzani_create", "lzani_destroy", "lzani_last_error",
           "lzani_set_genomes", "lzani_run_rows", "lzani_run_rows_device", "lzani_get_timing",
           "lzani_debug_get_index", "lzani_run_rows_regions", "lzani_get_layout",
           "lzani_row_costs", "lzani_partition_rows", "lzani_comm_unique_id", "lzani_comm_init", "lzani_comm_allgather",
           "lzani_comm_gatherv", "lzani_group_create", "lzani_group_destroy", "lzani_group_last_error",
           "lzani_group_set_genomes", "lzani_group_run_rows", "lzani_group_get_timing", "lzani_plan_gather", "lzani_get_rtc_info", "lzani_debug_rtc_compile",
           "lzani_debug_sort_segments", "lzani_debug_kernel_launches", "lzani_debug_kernel_name", "lzani_debug_split_stats",
           "lzani_set_genome_memory", "lzani_plan_blocks", "lzani_get_residency", "lzani_group_set_genome_memory",
           "lzani_group_get_residency", "lzani_debug_index_slab", "lzani_debug_run_candidates",
           "lzani_prefilter", "lzani_prefilter_fetch", "lzani_get_prefilter_info",
           "lzani_prefilter_codes", "lzani_plan_slices", "lzani_get_prefilter_stream_info",
           "lzani_get_prefilter_pass_info", "lzani_prefilter_pass_plan", "lzani_plan_passes",
           "lzani_prefilter_cross", "lzani_prefilter_codes_cross", "lzani_get_prefilter_cross_info",
           "lzani_set_prefilter_counting", "lzani_get_prefilter_sparse_info", "lzani_plan_sparse_tiles",
           "lzani_prefilter_limit", "lzani_get_prefilter_limit_info", "lzani_prefilter_limit_host", "lzani_debug_prefilter_set",
           "lzani_out_filter_lines", "lzani_run_rows_kept", "lzani_kept_fetch", "lzani_filter_results_device",
           "lzani_debug_filter_results", "lzani_get_kept_info", "lzani_group_run_rows_kept", "lzani_group_kept_fetch",
           "lzani_group_get_kept_info",
           "lzani_cluster_weight", "lzani_cluster_host", "lzani_cluster_begin", "lzani_cluster_add_kept",
           "lzani_debug_cluster_add_edges", "lzani_cluster_run", "lzani_cluster_fetch", "lzani_get_cluster_info",
           "lzani_group_cluster_begin", "lzani_group_cluster_add_kept", "lzani_group_cluster_run", "lzani_group_cluster_fetch",
           "lzani_group_get_cluster_info", "lzani_get_cluster_cover_info", "lzani_group_get_cluster_cover_info",
           "lzani_get_cluster_link_info", "lzani_group_get_cluster_link_info", "lzani_cluster_leiden_host",
           "lzani_debug_cluster_leiden_host_cap", "lzani_set_cluster_leiden", "lzani_group_set_cluster_leiden",
           "lzani_get_cluster_leiden_info", "lzani_group_get_cluster_leiden_info", "lzani_debug_alloc_fault",
           "lzani_cluster_cut_lines", "lzani_cluster_store_begin", "lzani_cluster_store_add_kept", "lzani_cluster_level",
           "lzani_get_cluster_store_info", "lzani_get_cluster_level_info", "lzani_debug_cluster_store_add", "lzani_debug_cluster_edges",
           "lzani_group_cluster_store_begin", "lzani_group_cluster_store_add_kept", "lzani_group_cluster_level",
           "lzani_group_get_cluster_store_info", "lzani_group_get_cluster_level_info",
           "lzani_set_region_capacity", "lzani_run_rows_aligned", "lzani_regions_fetch", "lzani_get_regions_info",
           "lzani_debug_order_regions", "lzani_regions_host")


class LzaniError(RuntimeError):
    pass


class Timing(C.Structure):
    _fields_ = [("index_ms", C.c_double), ("pairs_ms", C.c_double), ("pair_launches", C.c_uint32),
                ("index_launches", C.c_uint32), ("pairs", C.c_uint64), ("cand_ms", C.c_double), ("kmers_ms", C.c_double),
                ("cand_launches", C.c_uint32), ("reserved_", C.c_uint32)]


class LayoutInfo(C.Structure):
    _fields_ = [("key_bits", C.c_int32), ("dir_bits", C.c_int32), ("pos_bits", C.c_int32), ("tag_mask", C.c_uint32),
                ("kmer_words", C.c_int32), ("bucket_table", C.c_int32), ("tag_words", C.c_int32), ("n_free", C.c_int32),
                ("slots", C.c_uint32), ("batches_last_run", C.c_uint32), ("bytes_per_slot", C.c_uint64),
                ("bytes_genomes", C.c_uint64), ("join_lists", C.c_int32), ("block_launches", C.c_int32),
                ("bitmap_launches", C.c_int32), ("rtc_launches", C.c_int32),
                ("lpt_launches", C.c_int32), ("matrix_from_index", C.c_int32), ("split_launches", C.c_int32), ("reserved_", C.c_int32),
                ("split_segments", C.c_uint64)]


class RtcInfo(C.Structure):
    _fields_ = [("folded_ahead_of_time", C.c_int32), ("null_chain", C.c_int32), ("kernels_built", C.c_int32),
                ("kernels_from_cache", C.c_int32), ("kernels_failed", C.c_int32), ("reserved_", C.c_int32), ("build_ms", C.c_double)]


class SplitStats(C.Structure):
    _fields_ = [("pairs_cut", C.c_uint64), ("rounds", C.c_uint64), ("resumed", C.c_uint64), ("given_up", C.c_uint64),
                ("voids", C.c_uint64 * 6)]


class SlabInfo(C.Structure):
    _fields_ = [("key_bits", C.c_int32), ("dir_bits", C.c_int32), ("pos_bits", C.c_int32), ("tag_mask", C.c_uint32),
                ("filter_mask", C.c_uint32), ("build", C.c_int32), ("dir_stride", C.c_uint64), ("ent_stride", C.c_uint64),
                ("bk_stride", C.c_uint64), ("tw_stride", C.c_uint64), ("fl_stride", C.c_uint64)]


INDEX_BUILDS = ("lds", "atomics", "sort")          # LZANI_INDEX_BUILD_*


class CandPlan(C.Structure):
    _fields_ = [("pm", C.c_int32), ("pm_bits", C.c_int32), ("rshift", C.c_int32), ("pm_group", C.c_uint32),
                ("cb_words", C.c_uint64), ("batches", C.c_uint32), ("from_index_launches", C.c_uint32),
                ("cand_launches", C.c_uint32), ("counted_batches", C.c_uint32)]


class ResidencyInfo(C.Structure):
    _fields_ = [("limit", C.c_uint64), ("blocks", C.c_uint32), ("tiles", C.c_uint32), ("block_uploads", C.c_uint64),
                ("peak_resident_bytes", C.c_uint64), ("host_bytes", C.c_uint64), ("upload_ms", C.c_double)]


class PrefilterInfo(C.Structure):
    _fields_ = [("k", C.c_int32), ("tiles", C.c_uint32), ("positions", C.c_uint64), ("distinct_kmers", C.c_uint64),
                ("postings", C.c_uint64), ("entries", C.c_uint64), ("keys_ms", C.c_double), ("sort_ms", C.c_double),
                ("count_ms", C.c_double), ("compact_ms", C.c_double)]


class PrefilterStreamInfo(C.Structure):
    _fields_ = [("slices", C.c_uint32), ("slice_uploads", C.c_uint32), ("staged_bytes", C.c_uint64), ("stage_bytes", C.c_uint64),
                ("upload_ms", C.c_double)]


class PrefilterPassInfo(C.Structure):
    _fields_ = [("passes", C.c_uint32), ("key_sweeps", C.c_uint32), ("cap", C.c_uint64), ("largest_pass", C.c_uint64),
                ("workspace_bytes", C.c_uint64), ("hist_ms", C.c_double)]


class PrefilterCrossInfo(C.Structure):
    _fields_ = [("n_ref", C.c_uint32), ("n_query", C.c_uint32), ("tile_rows", C.c_uint32), ("reserved_", C.c_uint32),
                ("matrix_bytes", C.c_uint64)]


class PrefilterSparseInfo(C.Structure):
    _fields_ = [("sparse", C.c_uint32), ("attempts", C.c_uint32), ("pass_runs", C.c_uint32), ("reserved_", C.c_uint32),
                ("slots", C.c_uint64), ("table_bytes", C.c_uint64), ("pairs_seen", C.c_uint64), ("max_fill", C.c_uint64)]


class PrefilterLimitInfo(C.Structure):
    _fields_ = [("max_per_genome", C.c_uint32), ("limiting", C.c_uint32), ("entries_in", C.c_uint64), ("entries_out", C.c_uint64),
                ("genomes_cut", C.c_uint64), ("workspace_bytes", C.c_uint64), ("limit_ms", C.c_double)]


class OutFilter(C.Structure):
    _fields_ = [("min_tani", C.c_double), ("min_gani", C.c_double), ("min_ani", C.c_double), ("min_qcov", C.c_double),
                ("min_rcov", C.c_double)]


class Result(C.Structure):
    _fields_ = [("sym_in_matches", C.c_int32), ("sym_in_literals", C.c_int32), ("no_components", C.c_int32)]


class KeptPair(C.Structure):
    _fields_ = [("a", C.c_uint32), ("b", C.c_uint32), ("x", Result), ("y", Result), ("lines", C.c_uint32)]


class KeptInfo(C.Structure):
    _fields_ = [("entries", C.c_uint64), ("leading", C.c_uint64), ("unpaired", C.c_uint64), ("kept_pairs", C.c_uint64),
                ("kept_lines", C.c_uint64), ("bytes_to_host", C.c_uint64), ("filter_ms", C.c_double)]


# lzani_kept_pair as a numpy record: x = parse(query b, ref a), y = parse(query a, ref b), three int32 each
KEPT_DTYPE = np.dtype([("a", np.uint32), ("b", np.uint32), ("x", np.int32, (3,)), ("y", np.int32, (3,)), ("lines", np.uint32)])
assert KEPT_DTYPE.itemsize == C.sizeof(KeptPair) == 36
FILTER_FIELDS = ("tani", "gani", "ani", "qcov", "rcov")


def out_filter(flt=None, **minima):
    """An OutFilter from a dict / keywords of minima by column name (tani, gani, ani, qcov, rcov; the others 0)."""
    m = dict(flt or {}, **minima)
    assert set(m) <= set(FILTER_FIELDS), m
    return OutFilter(*[float(m.get(k, 0.0)) for k in FILTER_FIELDS])


def out_filter_lines(flt, x, y, len_a, len_b):
    """lzani_out_filter_lines (no GPU needed): the `lines` of the pair a < b with x = result of (ref a, query b) and
    y = result of (ref b, query a); 0xFFFFFFFF where a minimum is NaN."""
    lib = load_library()
    f = flt if isinstance(flt, OutFilter) else out_filter(flt)
    rx, ry = Result(*[int(v) for v in x]), Result(*[int(v) for v in y])
    return int(lib.lzani_out_filter_lines(C.byref(f), C.byref(rx), C.byref(ry), C.c_uint32(int(len_a)), C.c_uint32(int(len_b))))


def _kept_info(o):
    return {k: getattr(o, k) for k, _ in KeptInfo._fields_}


class RegionsInfo(C.Structure):
    _fields_ = [("entries", C.c_uint64), ("found", C.c_uint64), ("kept", C.c_uint64), ("entries_with_regions", C.c_uint64),
                ("entries_dropped", C.c_uint64), ("capacity", C.c_uint64), ("runs", C.c_uint64), ("sort_passes", C.c_uint64),
                ("workspace_bytes", C.c_uint64), ("bytes_to_host", C.c_uint64), ("sums_ms", C.c_double), ("sort_ms", C.c_double),
                ("write_ms", C.c_double)]


# lzani_region as a numpy record
REGION_DTYPE = np.dtype([("pair", np.uint64), ("ref_start", np.int32), ("ref_end", np.int32), ("seq_start", np.int32),
                         ("seq_end", np.int32), ("num_matches", np.int32), ("num_mismatches", np.int32)])
assert REGION_DTYPE.itemsize == 32


def _regions_info(o):
    return {k: getattr(o, k) for k, _ in RegionsInfo._fields_}


def _filter_or_null(flt):
    """None: a NULL filter; an OutFilter or a dict by column name: that filter."""
    if flt is None:
        return None
    return flt if isinstance(flt, OutFilter) else out_filter(flt)


def regions_host(n, aln_len, ref_ids, row_off, query_ids, regions, flt=None):
    """lzani_regions_host (no GPU needed): (the regions of the entries that stay, in file order, REGION_DTYPE; info dict) of
    made-up REGION_DTYPE regions of n genomes under the alignment filter `flt` (None: no entry is dropped)."""
    lib = load_library()
    ref_ids = np.ascontiguousarray(ref_ids, dtype=np.uint32)
    row_off = np.ascontiguousarray(row_off, dtype=np.uint64)
    q = None if query_ids is None else np.ascontiguousarray(query_ids, dtype=np.uint32)
    al = np.ascontiguousarray(aln_len, dtype=np.uint32)
    r = np.ascontiguousarray(regions, dtype=REGION_DTYPE)
    f = _filter_or_null(flt)
    out = np.zeros(len(r), dtype=REGION_DTYPE)
    cnt, info = C.c_uint64(0), RegionsInfo()
    rc = lib.lzani_regions_host(int(n), _ptr(al), len(ref_ids), _ptr(ref_ids), _ptr(row_off), _ptr(q), _ptr(r) if len(r) else None, C.c_uint64(len(r)),
                                C.byref(f) if f is not None else None, _ptr(out) if len(r) else None, C.byref(cnt), C.byref(info))
    if rc != 0:
        raise LzaniError(f"lzani_regions_host: {ERRORS.get(rc, rc)}")
    return out[:cnt.value].copy(), _regions_info(info)


class ClusterInfo(C.Structure):
    _fields_ = [("n", C.c_uint32), ("algo", C.c_int32), ("measure", C.c_int32), ("rounds", C.c_uint32), ("edges", C.c_uint64),
                ("clusters", C.c_uint64), ("singletons", C.c_uint64), ("largest", C.c_uint64), ("edge_bytes", C.c_uint64),
                ("add_ms", C.c_double), ("run_ms", C.c_double)]


class ClusterCoverInfo(C.Structure):
    _fields_ = [("distinct_edges", C.c_uint64), ("duplicate_edges", C.c_uint64), ("workspace_bytes", C.c_uint64),
                ("dedup_ms", C.c_double), ("rounds_ms", C.c_double)]


class ClusterLinkInfo(C.Structure):
    _fields_ = [("distinct_edges", C.c_uint64), ("duplicate_edges", C.c_uint64), ("merges", C.c_uint64), ("table_slots", C.c_uint64),
                ("workspace_bytes", C.c_uint64), ("dedup_ms", C.c_double), ("rounds_ms", C.c_double)]


class ClusterLeidenInfo(C.Structure):
    _fields_ = [("iterations", C.c_uint64), ("levels", C.c_uint64), ("move_rounds", C.c_uint64), ("refine_rounds", C.c_uint64),
                ("moves", C.c_uint64), ("merges", C.c_uint64), ("quality", C.c_int64), ("resolution_q", C.c_uint64),
                ("distinct_edges", C.c_uint64), ("duplicate_edges", C.c_uint64), ("table_slots", C.c_uint64), ("workspace_bytes", C.c_uint64),
                ("dedup_ms", C.c_double), ("rounds_ms", C.c_double)]


class ClusterCut(C.Structure):
    _fields_ = [("min_tani", C.c_double), ("min_gani", C.c_double), ("min_ani", C.c_double), ("min_qcov", C.c_double),
                ("min_rcov", C.c_double), ("min_len_ratio", C.c_double), ("max_num_alns", C.c_uint32), ("reserved_", C.c_uint32)]


class ClusterStoreInfo(C.Structure):
    _fields_ = [("n", C.c_uint32), ("records", C.c_uint64), ("record_bytes", C.c_uint64), ("add_ms", C.c_double)]


class ClusterLevelInfo(C.Structure):
    _fields_ = [("records_in", C.c_uint64), ("edges_out", C.c_uint64), ("lines_in", C.c_uint64), ("lines_out", C.c_uint64),
                ("level_ms", C.c_double)]


assert C.sizeof(ClusterCut) == 56
CUT_FIELDS = FILTER_FIELDS + ("len_ratio", "num_alns")


def cluster_cut(cut=None, reserved=0, **limits):
    """A ClusterCut from a dict / keywords by column name: minima of tani, gani, ani, qcov, rcov and len_ratio, and num_alns,
    the maximum of a line's num_alns (0: none); what is not named is 0.  reserved: the reserved word (tests)."""
    m = dict(cut or {}, **limits)
    assert set(m) <= set(CUT_FIELDS), m
    return ClusterCut(*[float(m.get(k, 0.0)) for k in FILTER_FIELDS], float(m.get("len_ratio", 0.0)), int(m.get("num_alns", 0)), int(reserved))


def cluster_cut_lines(cut, x, y, lines, len_a, len_b):
    """lzani_cluster_cut_lines (no GPU needed): the lines of the kept record (x, y, lines) of the pair a < b that stay under
    the cut; 0xFFFFFFFF where a minimum is NaN or the reserved word is not 0."""
    lib = load_library()
    f = cut if isinstance(cut, ClusterCut) else cluster_cut(cut)
    rx, ry = Result(*[int(v) for v in x]), Result(*[int(v) for v in y])
    return int(lib.lzani_cluster_cut_lines(C.byref(f), C.byref(rx), C.byref(ry), C.c_uint32(int(lines)), C.c_uint32(int(len_a)),
                                           C.c_uint32(int(len_b))))


# lzani_cluster_edge as a numpy record: a < b (either order is taken), w >= 0
EDGE_DTYPE = np.dtype([("a", np.uint32), ("b", np.uint32), ("w", np.float64)])
assert EDGE_DTYPE.itemsize == 16
CLUSTER_ALGOS = {"single": 0, "greedy-first": 1, "greedy-best": 2, "set-cover": 4,     # LZANI_CLUSTER_SINGLE ... (3 and 5 are no algorithms)
                 "complete-linkage": 6, "leiden-cpm": 8}                  # (7 is none either; "leiden" alone is no name)
CLUSTER_MEASURES = {"tani": 0, "gani": 1, "ani": 2}                       # LZANI_CLUSTER_TANI ...


def _algo(a):
    return CLUSTER_ALGOS[a] if isinstance(a, str) else int(a)


def _measure(m):
    return CLUSTER_MEASURES[m] if isinstance(m, str) else int(m)


def _cluster_info(o):
    return {k: getattr(o, k) for k, _ in ClusterInfo._fields_}


def cluster_edges(a, b, w):
    """An EDGE_DTYPE array from three sequences."""
    e = np.zeros(len(a), dtype=EDGE_DTYPE)
    e["a"], e["b"], e["w"] = a, b, w
    return e


def cluster_weight(measure, x, y, lines, len_a, len_b):
    """lzani_cluster_weight (no GPU needed): the weight of the pair a < b with x = result of (ref a, query b), y = result of
    (ref b, query a) and the output filter's `lines`; NaN for an unknown measure."""
    lib = load_library()
    rx, ry = Result(*[int(v) for v in x]), Result(*[int(v) for v in y])
    return float(lib.lzani_cluster_weight(_measure(measure), C.byref(rx), C.byref(ry), C.c_uint32(int(lines)), C.c_uint32(int(len_a)),
                                          C.c_uint32(int(len_b))))


def cluster_host(n, edges, algo):
    """lzani_cluster_host (no GPU needed): (rep_of uint32[n], cluster_of uint32[n], clusters) of EDGE_DTYPE edges."""
    lib = load_library()
    e = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
    rep, cl = np.zeros(int(n), dtype=np.uint32), np.zeros(int(n), dtype=np.uint32)
    k = C.c_uint32(0)
    rc = lib.lzani_cluster_host(C.c_uint32(int(n)), _ptr(e) if len(e) else None, C.c_uint64(len(e)), _algo(algo), _ptr(rep) if n else None,
                                _ptr(cl) if n else None, C.byref(k))
    if rc != 0:
        raise LzaniError(f"lzani_cluster_host: {ERRORS.get(rc, rc)}")
    return rep, cl, int(k.value)


def cluster_leiden_host(n, edges, resolution=0.7, iterations=2, cap=None):
    """lzani_cluster_leiden_host (no GPU needed): (rep_of uint32[n], cluster_of uint32[n], info dict) of EDGE_DTYPE edges.
    cap = (cap_mul, cap_add): the test hook with a phase's cap of rounds at cap_mul * n_level + cap_add."""
    lib = load_library()
    e = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
    rep, cl = np.zeros(int(n), dtype=np.uint32), np.zeros(int(n), dtype=np.uint32)
    o = ClusterLeidenInfo()
    head = (C.c_uint32(int(n)), _ptr(e) if len(e) else None, C.c_uint64(len(e)), C.c_double(float(resolution)), C.c_int(int(iterations)))
    tail = (_ptr(rep) if n else None, _ptr(cl) if n else None, C.byref(o))
    if cap is None:
        rc = lib.lzani_cluster_leiden_host(*head, *tail)
    else:
        rc = lib.lzani_debug_cluster_leiden_host_cap(*head, C.c_uint64(int(cap[0])), C.c_uint64(int(cap[1])), *tail)
    if rc != 0:
        raise LzaniError(f"lzani_cluster_leiden_host: {ERRORS.get(rc, rc)}")
    return rep, cl, {k: getattr(o, k) for k, _ in ClusterLeidenInfo._fields_}


PF_COUNTING = {"auto": 0, "dense": 1, "sparse": 2}   # LZANI_PF_COUNTING_*
PREFILTER_BINS = 4096                               # bins of the prefilter's k-mer passes
SAMPLE_ALL = 0xFFFFFFFFFFFFFFFF                     # lzani_prefilter's sample_max that keeps every k-mer


def sample_max_of(fraction):
    """sample_max of a sampling fraction in (0, 1]: floor(fraction * 2^64), saturated."""
    from fractions import Fraction
    return min(SAMPLE_ALL, int(Fraction(float(fraction)) * (1 << 64)))


DIAG_LIB_PATH = os.path.join(ROOT, "build", "diag", "liblzani_cover.so")
DIAG_DEFINES = ("-DLZANI_PATH_STATS", "-DLZANI_CHAIN_STATS")


def _build(out, defines, force):
    csrc = os.path.join(HERE, "csrc")                       # every header and source there: a new one cannot be forgotten
    deps = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hip"))] + [os.path.join(ROOT, "include", "lzani.h")]
    if not force and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
           "-Wno-unused-value", *defines, "-I" + os.path.join(HERE, "csrc"), "-I" + os.path.join(ROOT, "include"),      # (-I: the .incbin of lzani_rtc.h)
           "-o", out, SRC, os.path.join(HERE, "csrc", "lzani_sort.hip"), "-lrccl", "-lhiprtc"]
    subprocess.check_call(cmd)
    return out


def build_library(force=False):
    """hipcc cross-compiles for gfx950 without a GPU present."""
    return _build(LIB_PATH, (), force)


def build_diag_library(force=False):
    """The coverage library of tests/test_gpu_path_cover.py: build_library's recipe plus the two counter defines (the pair
    kernel's exits by reason, printed as raw totals per run: report_diagnostics), build/diag/liblzani_cover.so; run with
    LZANI_LIB pointing at it.  The same staleness rule."""
    return _build(DIAG_LIB_PATH, DIAG_DEFINES, force)


_lib = None


def load_library():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LzaniError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(there is no CPU fallback for the HIP path)")
        lib = C.CDLL(LIB_PATH)
        lib.lzani_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        lib.lzani_destroy.argtypes = [C.c_void_p]
        lib.lzani_destroy.restype = None
        lib.lzani_last_error.argtypes = [C.c_void_p]
        lib.lzani_last_error.restype = C.c_char_p
        lib.lzani_set_genomes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.lzani_run_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.lzani_run_rows_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.lzani_get_timing.argtypes = [C.c_void_p, C.c_void_p]
        lib.lzani_get_layout.argtypes = [C.c_void_p, C.c_void_p]
        lib.lzani_get_rtc_info.argtypes = [C.c_void_p, C.c_void_p]
        lib.lzani_debug_rtc_compile.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_uint64]
        lib.lzani_debug_rtc_compile.restype = C.c_int64
        lib.lzani_debug_kernel_launches.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        lib.lzani_debug_kernel_name.argtypes = [C.c_uint32]
        lib.lzani_debug_kernel_name.restype = C.c_char_p
        lib.lzani_debug_split_stats.argtypes = [C.c_void_p, C.c_void_p]
        lib.lzani_run_rows_regions.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_uint64, C.c_void_p]
        lib.lzani_debug_get_index.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
        lib.lzani_debug_index_slab.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7
        lib.lzani_debug_run_candidates.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.lzani_debug_sort_segments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_int]
        lib.lzani_row_costs.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.lzani_partition_rows.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.lzani_comm_unique_id.argtypes = [C.c_void_p]
        lib.lzani_comm_init.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.lzani_comm_allgather.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        lib.lzani_comm_gatherv.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        lib.lzani_group_create.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p)]
        lib.lzani_group_destroy.argtypes = [C.c_void_p]
        lib.lzani_group_destroy.restype = None
        lib.lzani_group_last_error.argtypes = [C.c_void_p]
        lib.lzani_group_last_error.restype = C.c_char_p
        lib.lzani_group_set_genomes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.lzani_group_run_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.lzani_group_get_timing.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.lzani_plan_gather.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 5
        lib.lzani_set_genome_memory.argtypes = [C.c_void_p, C.c_uint64]
        lib.lzani_group_set_genome_memory.argtypes = [C.c_void_p, C.c_uint64]
        lib.lzani_plan_blocks.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        lib.lzani_get_residency.argtypes = [C.c_void_p, C.c_void_p]
        lib.lzani_group_get_residency.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        lib.lzani_prefilter.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint32, C.c_double, C.c_void_p]
        lib.lzani_prefilter_fetch.argtypes = [C.c_void_p] + [C.c_void_p] * 4
        lib.lzani_get_prefilter_info.argtypes = [C.c_void_p, C.c_void_p]
        lib.lzani_prefilter_codes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_uint32, C.c_double,
                                              C.c_uint64, C.c_void_p]
        lib.lzani_plan_slices.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
        lib.lzani_get_prefilter_stream_info.argtypes = [C.c_void_p, C.c_void_p]
        lib.lzani_get_prefilter_pass_info.argtypes = [C.c_void_p, C.c_void_p]
        lib.lzani_prefilter_pass_plan.argtypes = [C.c_void_p, C.c_void_p]
        lib.lzani_plan_passes.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
        lib.lzani_prefilter_cross.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint32, C.c_double, C.c_uint32, C.c_void_p]
        lib.lzani_prefilter_codes_cross.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_uint32, C.c_double,
                                                    C.c_uint64, C.c_uint32, C.c_void_p]
        lib.lzani_get_prefilter_cross_info.argtypes = [C.c_void_p, C.c_void_p]
        lib.lzani_set_prefilter_counting.argtypes = [C.c_void_p, C.c_int]
        lib.lzani_get_prefilter_sparse_info.argtypes = [C.c_void_p, C.c_void_p]
        lib.lzani_plan_sparse_tiles.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        lib.lzani_prefilter_limit.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        lib.lzani_get_prefilter_limit_info.argtypes = [C.c_void_p, C.c_void_p]
        lib.lzani_prefilter_limit_host.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p]
        lib.lzani_debug_prefilter_set.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4
        lib.lzani_out_filter_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        lib.lzani_out_filter_lines.restype = C.c_uint32
        lib.lzani_run_rows_kept.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
        lib.lzani_kept_fetch.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        lib.lzani_filter_results_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
        lib.lzani_debug_filter_results.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
        lib.lzani_get_kept_info.argtypes = [C.c_void_p, C.c_void_p]
        lib.lzani_set_region_capacity.argtypes = [C.c_void_p, C.c_uint64]
        lib.lzani_run_rows_aligned.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 10
        lib.lzani_regions_fetch.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        lib.lzani_get_regions_info.argtypes = [C.c_void_p, C.c_void_p]
        lib.lzani_debug_order_regions.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint64, C.c_void_p, C.c_void_p]
        lib.lzani_regions_host.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint64] + [C.c_void_p] * 4
        lib.lzani_group_run_rows_kept.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
        lib.lzani_group_kept_fetch.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        lib.lzani_group_get_kept_info.argtypes = [C.c_void_p, C.c_void_p]
        lib.lzani_cluster_weight.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
        lib.lzani_cluster_weight.restype = C.c_double
        lib.lzani_cluster_host.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        for pre in ("lzani_", "lzani_group_"):
            getattr(lib, pre + "cluster_begin").argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int]
            getattr(lib, pre + "cluster_add_kept").argtypes = [C.c_void_p, C.c_void_p]
            getattr(lib, pre + "cluster_run").argtypes = [C.c_void_p, C.c_int, C.c_void_p]
            getattr(lib, pre + "cluster_fetch").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            getattr(lib, pre + "get_cluster_info").argtypes = [C.c_void_p, C.c_void_p]
            getattr(lib, pre + "get_cluster_cover_info").argtypes = [C.c_void_p, C.c_void_p]
            getattr(lib, pre + "get_cluster_link_info").argtypes = [C.c_void_p, C.c_void_p]
            getattr(lib, pre + "get_cluster_leiden_info").argtypes = [C.c_void_p, C.c_void_p]
            getattr(lib, pre + "set_cluster_leiden").argtypes = [C.c_void_p, C.c_double, C.c_int]
        lib.lzani_cluster_leiden_host.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.lzani_debug_cluster_leiden_host_cap.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_double, C.c_int, C.c_uint64, C.c_uint64,
                                                            C.c_void_p, C.c_void_p, C.c_void_p]
        lib.lzani_debug_cluster_add_edges.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        lib.lzani_debug_alloc_fault.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
        lib.lzani_cluster_cut_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
        lib.lzani_cluster_cut_lines.restype = C.c_uint32
        for pre in ("lzani_", "lzani_group_"):
            getattr(lib, pre + "cluster_store_begin").argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
            getattr(lib, pre + "cluster_store_add_kept").argtypes = [C.c_void_p, C.c_void_p]
            getattr(lib, pre + "cluster_level").argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
            getattr(lib, pre + "get_cluster_store_info").argtypes = [C.c_void_p, C.c_void_p]
            getattr(lib, pre + "get_cluster_level_info").argtypes = [C.c_void_p, C.c_void_p]
        lib.lzani_debug_cluster_store_add.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        lib.lzani_debug_cluster_edges.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        _lib = lib
    return _lib


ALLOC_FAULT_ALL = 1 << 63                           # lzani_debug_alloc_fault's count for "every attempt from `first` on"


def alloc_fault(first=0, count=1):
    """lzani_debug_alloc_fault (test hook, process-wide, no GPU needed): the first-th device or pinned allocation attempt
    from now fails, and the count - 1 behind it; first = 0 disarms.  Returns the attempts counted since the previous call."""
    lib = load_library()
    seen = C.c_uint64(0)
    rc = lib.lzani_debug_alloc_fault(C.c_uint64(int(first)), C.c_uint64(int(count)), C.byref(seen))
    if rc != 0:
        raise LzaniError(f"lzani_debug_alloc_fault: {ERRORS.get(rc, rc)}")
    return int(seen.value)


class AllocFault:
    """`with AllocFault(first, count) as f:` arms the fault for the block and always disarms on the way out; f.seen is then
    the number of attempts the block made."""

    def __init__(self, first=0, count=1):
        self.first, self.count, self.seen = int(first), int(count), None

    def __enter__(self):
        alloc_fault(self.first, self.count)
        return self

    def __exit__(self, *exc):
        self.seen = alloc_fault(0)
        return False


def params_array(params=None):
    p = dict(DEFAULT_PARAMS)
    if params:
        p.update(params)
    return (C.c_int32 * 8)(*[int(p[k]) for k in PARAM_ORDER]), p


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def dense_rows(n, rows=None):
    """CSR description of dense all2all rows (query_ids = None): ref_ids, row_off."""
    ref_ids = np.arange(n, dtype=np.uint32) if rows is None else np.asarray(rows, dtype=np.uint32)
    row_off = np.arange(len(ref_ids) + 1, dtype=np.uint64) * np.uint64(max(n - 1, 0))
    return ref_ids, row_off


def cross_rows(n, n_ref, pair_off=None, pair_ids=None):
    """The directed rows run_rows takes for the cross pairs of the references 0 .. n_ref - 1 and the queries n_ref .. n - 1,
    in both directions: (ref_ids, row_off, query_ids).  Without a CSR: every reference with all queries ascending, then
    every query with all references ascending.  With the CSR of kept pairs a < n_ref <= b (pair_off[n + 1], pair_ids, as
    prefilter_fetch gives it): one row per genome that has a partner, in id order, its partners ascending."""
    n, n_ref = int(n), int(n_ref)
    if pair_off is None:
        a = np.repeat(np.arange(n_ref, dtype=np.int64), n - n_ref)
        b = np.tile(np.arange(n_ref, n, dtype=np.int64), n_ref)
    else:
        a = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(pair_off).astype(np.int64)))
        b = np.asarray(pair_ids, dtype=np.int64)
    rows = np.concatenate((a, b))                           # row a lists b, row b lists a
    cols = np.concatenate((b, a))
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    cnt = np.bincount(rows, minlength=n)
    ref_ids = np.flatnonzero(cnt).astype(np.uint32)
    row_off = np.concatenate(([0], np.cumsum(cnt[cnt > 0]))).astype(np.uint64)
    return ref_ids, row_off, cols.astype(np.uint32)


def row_costs(ref_ids, row_off, query_ids, lens):
    """cost(row) = sum of query lengths + LZANI_ROW_COST_REF_WEIGHT * reference length (lzani_row_costs; no GPU needed)."""
    lib = load_library()
    ref_ids = np.ascontiguousarray(ref_ids, dtype=np.uint32)
    row_off = np.ascontiguousarray(row_off, dtype=np.uint64)
    q = None if query_ids is None else np.ascontiguousarray(query_ids, dtype=np.uint32)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    cost = np.zeros(len(ref_ids), dtype=np.uint64)
    rc = lib.lzani_row_costs(len(ref_ids), _ptr(ref_ids), _ptr(row_off), _ptr(q), len(lens), _ptr(lens), _ptr(cost))
    if rc != 0:
        raise LzaniError(f"lzani_row_costs: {ERRORS.get(rc, rc)}")
    return cost


def plan_gather(row_off, part_of_row, n_parts):
    """Shard bookkeeping of lzani_group_run_rows (lzani_plan_gather; no GPU needed): shard_base[n_parts + 1] and the
    scatter table src / dst / cnt / row_of_entry, one entry per row, shard by shard."""
    lib = load_library()
    row_off = np.ascontiguousarray(row_off, dtype=np.uint64)
    part = np.ascontiguousarray(part_of_row, dtype=np.uint32)
    n = len(part)
    base = np.zeros(n_parts + 1, dtype=np.uint64)
    src, dst, cnt = (np.zeros(n, dtype=np.uint64) for _ in range(3))
    row = np.zeros(n, dtype=np.uint32)
    rc = lib.lzani_plan_gather(n, _ptr(row_off), _ptr(part), n_parts, _ptr(base), _ptr(src), _ptr(dst), _ptr(cnt), _ptr(row))
    if rc != 0:
        raise LzaniError(f"lzani_plan_gather: {ERRORS.get(rc, rc)}")
    return base, src, dst, cnt, row


def partition_rows(n_rows, n_parts, row_cost=None):
    """Shard index of every row (lzani_partition_rows: cyclic without costs, greedy LPT with; no GPU needed)."""
    lib = load_library()
    cost = None if row_cost is None else np.ascontiguousarray(row_cost, dtype=np.uint64)
    part = np.zeros(n_rows, dtype=np.uint32)
    rc = lib.lzani_partition_rows(n_rows, _ptr(cost), n_parts, _ptr(part))
    if rc != 0:
        raise LzaniError(f"lzani_partition_rows: {ERRORS.get(rc, rc)}")
    return part


def plan_blocks(lens, params=None, limit=0):
    """Block plan of an out-of-core genome set (lzani_plan_blocks; no GPU needed): (number of blocks, block_of[n])."""
    lib = load_library()
    arr, _ = params_array(params)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    block_of = np.zeros(len(lens), dtype=np.uint32)
    nb = lib.lzani_plan_blocks(len(lens), _ptr(lens), arr, C.c_uint64(int(limit)), _ptr(block_of))
    if nb < 0:
        raise LzaniError(f"lzani_plan_blocks: {ERRORS.get(nb, nb)}")
    return nb, block_of


def plan_passes(hist, cap, forced=0):
    """Pass plan of the prefilter (lzani_plan_passes; no GPU needed): bin_lo[P + 1] from the windows per bin, the windows a
    pass may hold and a forced number of passes (0: automatic)."""
    lib = load_library()
    hist = np.ascontiguousarray(hist, dtype=np.uint64)
    if len(hist) != PREFILTER_BINS:
        raise LzaniError(f"lzani_plan_passes: the histogram has {PREFILTER_BINS} bins")
    bin_lo = np.zeros(PREFILTER_BINS + 1, dtype=np.uint32)
    np_ = lib.lzani_plan_passes(_ptr(hist), C.c_uint64(int(cap)), C.c_uint32(int(forced)), _ptr(bin_lo))
    if np_ < 0:
        raise LzaniError(f"lzani_plan_passes: {ERRORS.get(np_, np_)}")
    return bin_lo[:np_ + 1].copy()


def plan_sparse_tiles(row_pairs, slots):
    """Tiles of sparse counting (lzani_plan_sparse_tiles; no GPU needed): (tile_r0[T + 1], attempts) from the distinct pairs
    of every row and the slots of the pair table."""
    lib = load_library()
    row_pairs = np.ascontiguousarray(row_pairs, dtype=np.uint64)
    tile_r0 = np.zeros(len(row_pairs) + 1, dtype=np.uint32)
    attempts = C.c_uint32(0)
    nt = lib.lzani_plan_sparse_tiles(len(row_pairs), _ptr(row_pairs) if len(row_pairs) else None, C.c_uint64(int(slots)), _ptr(tile_r0), C.byref(attempts))
    if nt < 0:
        raise LzaniError(f"lzani_plan_sparse_tiles: {ERRORS.get(nt, nt)}")
    return tile_r0[:nt + 1].copy(), attempts.value


def _csr_arrays(kmers_of, row_off, ids, shared):
    return (np.ascontiguousarray(kmers_of, dtype=np.uint32), np.ascontiguousarray(row_off, dtype=np.uint64),
            np.ascontiguousarray(ids, dtype=np.uint32), np.ascontiguousarray(shared, dtype=np.uint32))


def prefilter_limit_host(n, n_ref, kmers_of, row_off, ids, shared, max_per_genome):
    """The limit rule of the prefilter (lzani_prefilter_limit_host; no GPU needed): keep uint8[e], 1 where the CSR entry
    survives with at most max_per_genome pairs per limiting genome; n_ref 0 = all-pairs."""
    lib = load_library()
    kmers_of, row_off, ids, shared = _csr_arrays(kmers_of, row_off, ids, shared)
    keep = np.zeros(len(ids), dtype=np.uint8)
    rc = lib.lzani_prefilter_limit_host(int(n), int(n_ref), _ptr(kmers_of), _ptr(row_off), _ptr(ids), _ptr(shared),
                                        C.c_uint32(int(max_per_genome)), _ptr(keep))
    if rc != 0:
        raise LzaniError(f"lzani_prefilter_limit_host: {ERRORS.get(rc, rc)}")
    return keep


def plan_slices(lens, slice_bytes):
    """Slice plan of the streamed prefilter (lzani_plan_slices; no GPU needed): (number of slices, slice_of[n])."""
    lib = load_library()
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    slice_of = np.zeros(len(lens), dtype=np.uint32)
    ns = lib.lzani_plan_slices(len(lens), _ptr(lens), C.c_uint64(int(slice_bytes)), _ptr(slice_of))
    if ns < 0:
        raise LzaniError(f"lzani_plan_slices: {ERRORS.get(ns, ns)}")
    return ns, slice_of


def _residency(o):
    return {k: getattr(o, k) for k, _ in ResidencyInfo._fields_}


def rtc_compile(params=None, nfree=True, cand=2, arch="gfx950"):
    """Compile-only check of the run-time compiled pair kernel (no GPU needed): (code object bytes or negative code, log)."""
    lib = load_library()
    arr, _ = params_array(params)
    log = C.create_string_buffer(1 << 16)
    n = lib.lzani_debug_rtc_compile(arr, int(bool(nfree)), int(cand), arch.encode(), log, len(log))
    return int(n), log.value.decode(errors="replace")


def kernel_names():
    """Names of the launch record's entries, by id (lzani_debug_kernel_name; no GPU needed)."""
    lib = load_library()
    names = []
    while True:
        n = lib.lzani_debug_kernel_name(len(names))
        if n is None:
            return names
        names.append(n.decode())


def comm_unique_id():
    lib = load_library()
    buf = (C.c_uint8 * 128)()
    rc = lib.lzani_comm_unique_id(buf)
    if rc != 0:
        raise LzaniError(f"lzani_comm_unique_id: {ERRORS.get(rc, rc)}")
    return bytes(buf)


class _ClusterCalls:
    """The cluster stage of an Engine (pre = "lzani_") or a Group (pre = "lzani_group_": the first device's context)."""

    def cluster_begin(self, n=None, report_len=None, measure="tani"):
        """An empty edge set for n genomes (default: the genome set's) with their reported lengths (default: its own)."""
        n = int(self.n if n is None else n)
        rl = None if report_len is None else np.ascontiguousarray(report_len, dtype=np.uint32)
        assert rl is None or len(rl) == n
        self._check(getattr(self.lib, self._pre + "cluster_begin")(self.h, n, _ptr(rl), _measure(measure)), self._pre + "cluster_begin")
        self._cluster_n = n

    def cluster_add_kept(self):
        """Appends the edges of the current kept result; returns the number of edge records there are now."""
        tot = C.c_uint64(0)
        self._check(getattr(self.lib, self._pre + "cluster_add_kept")(self.h, C.byref(tot)), self._pre + "cluster_add_kept")
        return int(tot.value)

    def cluster_run(self, algo):
        """Runs "single", "greedy-first", "greedy-best", "set-cover", "complete-linkage" or "leiden-cpm" on the edges there are; returns the number
        of clusters."""
        k = C.c_uint64(0)
        self._check(getattr(self.lib, self._pre + "cluster_run")(self.h, _algo(algo), C.byref(k)), self._pre + "cluster_run")
        return int(k.value)

    def cluster_fetch(self):
        """(rep_of uint32[n], cluster_of uint32[n]) of the last run."""
        n = getattr(self, "_cluster_n", 0)
        rep, cl = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        self._check(getattr(self.lib, self._pre + "cluster_fetch")(self.h, _ptr(rep), _ptr(cl)), self._pre + "cluster_fetch")
        return rep[:n], cl[:n]

    def cluster_info(self):
        """n, algo, measure, rounds, edges, clusters, singletons, largest, edge_bytes, add_ms, run_ms."""
        o = ClusterInfo()
        self._check(getattr(self.lib, self._pre + "get_cluster_info")(self.h, C.byref(o)), self._pre + "get_cluster_info")
        return _cluster_info(o)

    def cluster_cover_info(self):
        """distinct_edges, duplicate_edges, workspace_bytes, dedup_ms, rounds_ms of the last run, a "set-cover" one."""
        o = ClusterCoverInfo()
        self._check(getattr(self.lib, self._pre + "get_cluster_cover_info")(self.h, C.byref(o)), self._pre + "get_cluster_cover_info")
        return {k: getattr(o, k) for k, _ in ClusterCoverInfo._fields_}

    def cluster_link_info(self):
        """distinct_edges, duplicate_edges, merges, table_slots, workspace_bytes, dedup_ms, rounds_ms of the last run, a
        "complete-linkage" one."""
        o = ClusterLinkInfo()
        self._check(getattr(self.lib, self._pre + "get_cluster_link_info")(self.h, C.byref(o)), self._pre + "get_cluster_link_info")
        return {k: getattr(o, k) for k, _ in ClusterLinkInfo._fields_}

    def set_cluster_leiden(self, resolution=0.7, iterations=2):
        """The parameters of the later "leiden-cpm" runs: resolution in [0, 1], iterations in 1..16."""
        self._check(getattr(self.lib, self._pre + "set_cluster_leiden")(self.h, C.c_double(float(resolution)), C.c_int(int(iterations))),
                    self._pre + "set_cluster_leiden")

    def cluster_leiden_info(self):
        """iterations, levels, move_rounds, refine_rounds, moves, merges, quality, resolution_q, distinct_edges, duplicate_edges,
        table_slots, workspace_bytes, dedup_ms, rounds_ms of the last run, which was one of "leiden-cpm"."""
        o = ClusterLeidenInfo()
        self._check(getattr(self.lib, self._pre + "get_cluster_leiden_info")(self.h, C.byref(o)), self._pre + "get_cluster_leiden_info")
        return {k: getattr(o, k) for k, _ in ClusterLeidenInfo._fields_}

    def cluster_store_begin(self, n=None, report_len=None):
        """An empty record store for n genomes (default: the genome set's) with their reported lengths (default: its own)."""
        n = int(self.n if n is None else n)
        rl = None if report_len is None else np.ascontiguousarray(report_len, dtype=np.uint32)
        assert rl is None or len(rl) == n
        self._check(getattr(self.lib, self._pre + "cluster_store_begin")(self.h, n, _ptr(rl)), self._pre + "cluster_store_begin")
        self._store_n = n

    def cluster_store_add_kept(self):
        """Appends the records of the current kept result to the store; returns the number of records there are now."""
        tot = C.c_uint64(0)
        self._check(getattr(self.lib, self._pre + "cluster_store_add_kept")(self.h, C.byref(tot)), self._pre + "cluster_store_add_kept")
        return int(tot.value)

    def cluster_level(self, measure="tani", cut=None):
        """A begun cluster state whose edges are the store's records under `cut` (a ClusterCut, or a dict by column name);
        returns the number of edges."""
        f = cut if isinstance(cut, ClusterCut) else cluster_cut(cut)
        e = C.c_uint64(0)
        self._check(getattr(self.lib, self._pre + "cluster_level")(self.h, _measure(measure), C.byref(f), C.byref(e)), self._pre + "cluster_level")
        self._cluster_n = getattr(self, "_store_n", 0)
        return int(e.value)

    def cluster_store_info(self):
        """n, records, record_bytes, add_ms."""
        o = ClusterStoreInfo()
        self._check(getattr(self.lib, self._pre + "get_cluster_store_info")(self.h, C.byref(o)), self._pre + "get_cluster_store_info")
        return {k: getattr(o, k) for k, _ in ClusterStoreInfo._fields_}

    def cluster_level_info(self):
        """records_in, edges_out, lines_in, lines_out, level_ms of the level that made the current cluster state."""
        o = ClusterLevelInfo()
        self._check(getattr(self.lib, self._pre + "get_cluster_level_info")(self.h, C.byref(o)), self._pre + "get_cluster_level_info")
        return {k: getattr(o, k) for k, _ in ClusterLevelInfo._fields_}


class Group(_ClusterCalls):
    """lzani_group_*: one process, several GPUs (what `lz-ani --gpus n` uses)."""
    _pre = "lzani_group_"

    def __init__(self, params=None, devices=(0,)):
        self.lib = load_library()
        arr, self.params = params_array(params)
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        rc = self.lib.lzani_group_create(arr, len(devices), devs, C.byref(h))
        if rc != 0:
            raise LzaniError(f"lzani_group_create failed: {ERRORS.get(rc, rc)}")
        self.h = h
        self.n_dev = len(devices)

    def close(self):
        if getattr(self, "h", None):
            self.lib.lzani_group_destroy(self.h)
            self.h = None

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.lzani_group_last_error(self.h)
            raise LzaniError(f"{what}: {ERRORS.get(rc, rc)}: {msg.decode() if msg else ''}")

    def set_genomes(self, seqs):
        seqs = [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
        ptrs = (C.c_void_p * len(seqs))(*[s.ctypes.data for s in seqs])
        lens = np.array([len(s) for s in seqs], dtype=np.uint32)
        self._check(self.lib.lzani_group_set_genomes(self.h, len(seqs), ptrs, _ptr(lens)), "lzani_group_set_genomes")
        self.n = len(seqs)

    def run_rows(self, ref_ids, row_off, query_ids=None):
        ref_ids = np.ascontiguousarray(ref_ids, dtype=np.uint32)
        row_off = np.ascontiguousarray(row_off, dtype=np.uint64)
        q = None if query_ids is None else np.ascontiguousarray(query_ids, dtype=np.uint32)
        n_pairs = int(row_off[-1]) if len(row_off) else 0
        out = np.zeros((n_pairs, 3), dtype=np.int32)
        self._check(self.lib.lzani_group_run_rows(self.h, len(ref_ids), _ptr(ref_ids), _ptr(row_off), _ptr(q), _ptr(out)),
                    "lzani_group_run_rows")
        return out

    def run_rows_kept(self, ref_ids, row_off, query_ids=None, flt=None, report_len=None):
        """lzani_group_run_rows_kept and the fetch of all records: a KEPT_DTYPE array; kept_info() has the counters."""
        ref_ids = np.ascontiguousarray(ref_ids, dtype=np.uint32)
        row_off = np.ascontiguousarray(row_off, dtype=np.uint64)
        q = None if query_ids is None else np.ascontiguousarray(query_ids, dtype=np.uint32)
        rl = None if report_len is None else np.ascontiguousarray(report_len, dtype=np.uint32)
        f = flt if isinstance(flt, OutFilter) else out_filter(flt)
        cnt = C.c_uint64(0)
        self._check(self.lib.lzani_group_run_rows_kept(self.h, len(ref_ids), _ptr(ref_ids), _ptr(row_off), _ptr(q), C.byref(f), _ptr(rl),
                                                       C.byref(cnt)), "lzani_group_run_rows_kept")
        return self.kept_fetch(0, int(cnt.value))

    def kept_fetch(self, first, count):
        out = np.zeros(int(count), dtype=KEPT_DTYPE)
        self._check(self.lib.lzani_group_kept_fetch(self.h, C.c_uint64(int(first)), C.c_uint64(int(count)), _ptr(out) if count else None),
                    "lzani_group_kept_fetch")
        return out

    def kept_info(self):
        o = KeptInfo()
        self._check(self.lib.lzani_group_get_kept_info(self.h, C.byref(o)), "lzani_group_get_kept_info")
        return _kept_info(o)

    def set_genome_memory(self, nbytes):
        """Genome-memory limit of every device context, applied at the next set_genomes (0: automatic)."""
        self._check(self.lib.lzani_group_set_genome_memory(self.h, C.c_uint64(int(nbytes))), "lzani_group_set_genome_memory")

    def residency(self, device_index=0):
        o = ResidencyInfo()
        self._check(self.lib.lzani_group_get_residency(self.h, device_index, C.byref(o)), "lzani_group_get_residency")
        return _residency(o)

    def timing(self, device_index=0):
        t = Timing()
        g = C.c_double(0)
        self._check(self.lib.lzani_group_get_timing(self.h, device_index, C.byref(t), C.byref(g)), "lzani_group_get_timing")
        return dict(index_ms=t.index_ms, pairs_ms=t.pairs_ms, pair_launches=t.pair_launches, pairs=t.pairs, gather_ms=g.value,
                    cand_ms=t.cand_ms, kmers_ms=t.kmers_ms)


class Engine(_ClusterCalls):
    _pre = "lzani_"

    def debug_cluster_add_edges(self, edges):
        """Test hook: appends made-up EDGE_DTYPE edges from host memory."""
        e = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
        self._check(self.lib.lzani_debug_cluster_add_edges(self.h, _ptr(e) if len(e) else None, C.c_uint64(len(e))), "lzani_debug_cluster_add_edges")

    def debug_cluster_store_add(self, records):
        """Test hook: appends made-up KEPT_DTYPE records from host memory to the record store."""
        r = np.ascontiguousarray(records, dtype=KEPT_DTYPE)
        self._check(self.lib.lzani_debug_cluster_store_add(self.h, _ptr(r) if len(r) else None, C.c_uint64(len(r))), "lzani_debug_cluster_store_add")

    def debug_cluster_edges(self, first=0, count=None):
        """Test hook: edges first .. first + count - 1 (default: to the end) of the current cluster state, EDGE_DTYPE."""
        if count is None:
            count = self.cluster_info()["edges"] - int(first)
        out = np.zeros(int(count), dtype=EDGE_DTYPE)
        self._check(self.lib.lzani_debug_cluster_edges(self.h, C.c_uint64(int(first)), C.c_uint64(int(count)), _ptr(out) if count else None),
                    "lzani_debug_cluster_edges")
        return out

    def __init__(self, params=None, device=0):
        self.lib = load_library()
        arr, self.params = params_array(params)
        h = C.c_void_p()
        rc = self.lib.lzani_create(arr, int(device), C.byref(h))
        if rc != 0:
            raise LzaniError(f"lzani_create failed: {ERRORS.get(rc, rc)}")
        self.h = h
        self.n = 0
        self.pf_n = 0
        self.lens = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.lzani_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.lzani_last_error(self.h)
            raise LzaniError(f"{what}: {ERRORS.get(rc, rc)}: {msg.decode() if msg else ''}")

    def set_genomes(self, seqs):
        seqs = [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
        ptrs = (C.c_void_p * len(seqs))(*[s.ctypes.data for s in seqs])
        lens = np.array([len(s) for s in seqs], dtype=np.uint32)
        self._check(self.lib.lzani_set_genomes(self.h, len(seqs), ptrs, _ptr(lens)), "lzani_set_genomes")
        self.n = len(seqs)
        self.lens = lens

    def set_genome_memory(self, nbytes):
        """Genome-memory limit (bytes of genome tables), applied at the next set_genomes; 0 = automatic.  A set beyond
        it stays on the host and runs in tiles of (reference block, query block)."""
        self._check(self.lib.lzani_set_genome_memory(self.h, C.c_uint64(int(nbytes))), "lzani_set_genome_memory")

    def residency(self):
        """lzani_get_residency: limit, blocks, tiles and block_uploads of the last run, peak_resident_bytes, host_bytes, upload_ms."""
        o = ResidencyInfo()
        self._check(self.lib.lzani_get_residency(self.h, C.byref(o)), "lzani_get_residency")
        return _residency(o)

    def prefilter(self, k, sample_max=SAMPLE_ALL, min_shared=1, min_ratio=0.0):
        """lzani_prefilter on the resident set: the shared canonical k-mer counts of all genome pairs, and the pairs a < b
        with shared >= max(min_shared, 1) and shared / min(|K(a)|, |K(b)|) >= min_ratio.  Returns the number of kept pairs;
        prefilter_fetch() brings them."""
        cnt = C.c_uint64(0)
        self._check(self.lib.lzani_prefilter(self.h, int(k), C.c_uint64(int(sample_max)), C.c_uint32(int(min_shared)),
                                             C.c_double(float(min_ratio)), C.byref(cnt)), "lzani_prefilter")
        self.pf_n = self.n
        return int(cnt.value)

    def prefilter_codes(self, seqs, k, sample_max=SAMPLE_ALL, min_shared=1, min_ratio=0.0, slice_bytes=0):
        """lzani_prefilter_codes: the prefilter of `seqs` streamed from host memory through a staging buffer of slice_bytes
        (0: automatic); the context's own genome set, if any, is neither needed nor touched.  Returns the number of kept
        pairs; prefilter_fetch() brings them, prefilter_stream_info() the slice counters."""
        seqs = [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
        ptrs = (C.c_void_p * max(len(seqs), 1))(*[s.ctypes.data for s in seqs])
        lens = np.array([len(s) for s in seqs], dtype=np.uint32)
        cnt = C.c_uint64(0)
        self._check(self.lib.lzani_prefilter_codes(self.h, len(seqs), ptrs, _ptr(lens), int(k), C.c_uint64(int(sample_max)),
                                                   C.c_uint32(int(min_shared)), C.c_double(float(min_ratio)),
                                                   C.c_uint64(int(slice_bytes)), C.byref(cnt)), "lzani_prefilter_codes")
        self.pf_n = len(seqs)
        return int(cnt.value)

    def prefilter_cross(self, k, n_ref, sample_max=SAMPLE_ALL, min_shared=1, min_ratio=0.0):
        """lzani_prefilter_cross on the resident set: the prefilter restricted to the pairs a < n_ref <= b (references
        0 .. n_ref - 1 against queries n_ref .. n - 1).  Returns the number of kept pairs; prefilter_fetch() brings them,
        prefilter_cross_info() the shape of the count matrix."""
        cnt = C.c_uint64(0)
        self.pf_n = self.n
        self._check(self.lib.lzani_prefilter_cross(self.h, int(k), C.c_uint64(int(sample_max)), C.c_uint32(int(min_shared)),
                                                   C.c_double(float(min_ratio)), C.c_uint32(int(n_ref)), C.byref(cnt)), "lzani_prefilter_cross")
        return int(cnt.value)

    def prefilter_codes_cross(self, seqs, k, n_ref, sample_max=SAMPLE_ALL, min_shared=1, min_ratio=0.0, slice_bytes=0):
        """lzani_prefilter_codes_cross: prefilter_cross of `seqs` streamed from host memory, as prefilter_codes streams them."""
        seqs = [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
        ptrs = (C.c_void_p * max(len(seqs), 1))(*[s.ctypes.data for s in seqs])
        lens = np.array([len(s) for s in seqs], dtype=np.uint32)
        cnt = C.c_uint64(0)
        self.pf_n = len(seqs)
        self._check(self.lib.lzani_prefilter_codes_cross(self.h, len(seqs), ptrs, _ptr(lens), int(k), C.c_uint64(int(sample_max)),
                                                         C.c_uint32(int(min_shared)), C.c_double(float(min_ratio)),
                                                         C.c_uint64(int(slice_bytes)), C.c_uint32(int(n_ref)), C.byref(cnt)),
                    "lzani_prefilter_codes_cross")
        return int(cnt.value)

    def set_prefilter_counting(self, mode):
        """lzani_set_prefilter_counting: "auto", "dense" or "sparse" (or the LZANI_PF_COUNTING_* number) for the later prefilter calls."""
        self._check(self.lib.lzani_set_prefilter_counting(self.h, int(PF_COUNTING.get(mode, mode))), "lzani_set_prefilter_counting")

    def prefilter_limit(self, max_per_genome):
        """lzani_prefilter_limit: the current prefilter result cut to every limiting genome's max_per_genome best pairs.
        Returns the number of pairs that survive; prefilter_fetch() brings them, prefilter_limit_info() the counters."""
        cnt = C.c_uint64(0)
        self._check(self.lib.lzani_prefilter_limit(self.h, C.c_uint32(int(max_per_genome)), C.byref(cnt)), "lzani_prefilter_limit")
        return int(cnt.value)

    def prefilter_limit_info(self):
        o = PrefilterLimitInfo()
        self._check(self.lib.lzani_get_prefilter_limit_info(self.h, C.byref(o)), "lzani_get_prefilter_limit_info")
        return {k: getattr(o, k) for k, _ in PrefilterLimitInfo._fields_}

    def debug_prefilter_set(self, n, n_ref, kmers_of, row_off, ids, shared):
        """lzani_debug_prefilter_set: a made-up prefilter result in place of the context's (n_ref 0 = all-pairs)."""
        kmers_of, row_off, ids, shared = _csr_arrays(kmers_of, row_off, ids, shared)
        self._check(self.lib.lzani_debug_prefilter_set(self.h, int(n), int(n_ref), _ptr(kmers_of), _ptr(row_off), _ptr(ids), _ptr(shared)),
                    "lzani_debug_prefilter_set")
        self.pf_n = int(n)

    def prefilter_sparse_info(self):
        o = PrefilterSparseInfo()
        self._check(self.lib.lzani_get_prefilter_sparse_info(self.h, C.byref(o)), "lzani_get_prefilter_sparse_info")
        return {k: getattr(o, k) for k, _ in PrefilterSparseInfo._fields_ if k != "reserved_"}

    def prefilter_cross_info(self):
        o = PrefilterCrossInfo()
        self._check(self.lib.lzani_get_prefilter_cross_info(self.h, C.byref(o)), "lzani_get_prefilter_cross_info")
        return {k: getattr(o, k) for k, _ in PrefilterCrossInfo._fields_ if k != "reserved_"}

    def prefilter_stream_info(self):
        o = PrefilterStreamInfo()
        self._check(self.lib.lzani_get_prefilter_stream_info(self.h, C.byref(o)), "lzani_get_prefilter_stream_info")
        return {k: getattr(o, k) for k, _ in PrefilterStreamInfo._fields_}

    def prefilter_pass_info(self):
        o = PrefilterPassInfo()
        self._check(self.lib.lzani_get_prefilter_pass_info(self.h, C.byref(o)), "lzani_get_prefilter_pass_info")
        return {k: getattr(o, k) for k, _ in PrefilterPassInfo._fields_}

    def prefilter_pass_plan(self):
        """bin_lo[passes + 1] of the last prefilter: pass p held the bins bin_lo[p] .. bin_lo[p + 1]."""
        bin_lo = np.zeros(PREFILTER_BINS + 1, dtype=np.uint32)
        np_ = self.lib.lzani_prefilter_pass_plan(self.h, _ptr(bin_lo))
        self._check(min(np_, 0), "lzani_prefilter_pass_plan")
        return bin_lo[:np_ + 1].copy()

    def prefilter_info(self):
        o = PrefilterInfo()
        self._check(self.lib.lzani_get_prefilter_info(self.h, C.byref(o)), "lzani_get_prefilter_info")
        return {k: getattr(o, k) for k, _ in PrefilterInfo._fields_}

    def prefilter_fetch(self):
        """(kmers_of uint32[n], row_off uint64[n + 1], ids uint32[e], shared uint32[e]): CSR of the kept pairs a < b."""
        n = self.pf_n                                   # the n of the prefilter that made the result
        kmers_of = np.zeros(n, dtype=np.uint32)
        row_off = np.zeros(n + 1, dtype=np.uint64)
        self._check(self.lib.lzani_prefilter_fetch(self.h, _ptr(kmers_of), _ptr(row_off), None, None), "lzani_prefilter_fetch")
        e = int(row_off[-1])
        ids = np.zeros(e, dtype=np.uint32)
        shared = np.zeros(e, dtype=np.uint32)
        self._check(self.lib.lzani_prefilter_fetch(self.h, None, None, _ptr(ids), _ptr(shared)), "lzani_prefilter_fetch")
        return kmers_of, row_off, ids, shared

    def run_rows(self, ref_ids, row_off, query_ids=None):
        ref_ids = np.ascontiguousarray(ref_ids, dtype=np.uint32)
        row_off = np.ascontiguousarray(row_off, dtype=np.uint64)
        q = None if query_ids is None else np.ascontiguousarray(query_ids, dtype=np.uint32)
        n_pairs = int(row_off[-1]) if len(row_off) else 0
        out = np.zeros((n_pairs, 3), dtype=np.int32)
        self._check(self.lib.lzani_run_rows(self.h, len(ref_ids), _ptr(ref_ids), _ptr(row_off), _ptr(q), _ptr(out)),
                    "lzani_run_rows")
        return out

    def run_rows_kept(self, ref_ids, row_off, query_ids=None, flt=None, report_len=None, fetch=True):
        """lzani_run_rows_kept: the rows run, their results stay on the device, and the output filter keeps the pairs a < b of
        which a line passes the minima `flt` (an OutFilter, or a dict by column name).  Returns the records (KEPT_DTYPE), all
        fetched at once, or with fetch=False their number; kept_fetch() / kept_info() read the result."""
        ref_ids = np.ascontiguousarray(ref_ids, dtype=np.uint32)
        row_off = np.ascontiguousarray(row_off, dtype=np.uint64)
        q = None if query_ids is None else np.ascontiguousarray(query_ids, dtype=np.uint32)
        rl = None if report_len is None else np.ascontiguousarray(report_len, dtype=np.uint32)
        f = flt if isinstance(flt, OutFilter) else out_filter(flt)
        cnt = C.c_uint64(0)
        self._check(self.lib.lzani_run_rows_kept(self.h, len(ref_ids), _ptr(ref_ids), _ptr(row_off), _ptr(q), C.byref(f), _ptr(rl),
                                                 C.byref(cnt)), "lzani_run_rows_kept")
        return self.kept_fetch(0, int(cnt.value)) if fetch else int(cnt.value)

    def filter_results(self, n, report_len, ref_ids, row_off, query_ids, results, flt, fetch=True):
        """The output filter's stage alone on made-up or earlier results of n genomes: `results` is an int32[entries, 3] array
        (lzani_debug_filter_results uploads it) or an int, the raw device pointer of such a buffer
        (lzani_filter_results_device).  Returns like run_rows_kept."""
        ref_ids = np.ascontiguousarray(ref_ids, dtype=np.uint32)
        row_off = np.ascontiguousarray(row_off, dtype=np.uint64)
        q = None if query_ids is None else np.ascontiguousarray(query_ids, dtype=np.uint32)
        rl = np.ascontiguousarray(report_len, dtype=np.uint32)
        f = flt if isinstance(flt, OutFilter) else out_filter(flt)
        cnt = C.c_uint64(0)
        if isinstance(results, (int, np.integer)):
            self._check(self.lib.lzani_filter_results_device(self.h, int(n), _ptr(rl), len(ref_ids), _ptr(ref_ids), _ptr(row_off), _ptr(q),
                                                             C.c_void_p(int(results)), C.byref(f), C.byref(cnt)), "lzani_filter_results_device")
        else:
            res = np.ascontiguousarray(results, dtype=np.int32).reshape(-1, 3)
            self._check(self.lib.lzani_debug_filter_results(self.h, int(n), _ptr(rl), len(ref_ids), _ptr(ref_ids), _ptr(row_off), _ptr(q),
                                                            _ptr(res) if len(res) else None, C.byref(f), C.byref(cnt)), "lzani_debug_filter_results")
        return self.kept_fetch(0, int(cnt.value)) if fetch else int(cnt.value)

    def kept_fetch(self, first, count):
        """lzani_kept_fetch: records first .. first + count - 1 of the kept result (KEPT_DTYPE)."""
        out = np.zeros(int(count), dtype=KEPT_DTYPE)
        self._check(self.lib.lzani_kept_fetch(self.h, C.c_uint64(int(first)), C.c_uint64(int(count)), _ptr(out) if count else None),
                    "lzani_kept_fetch")
        return out

    def kept_info(self):
        """lzani_get_kept_info: entries, leading, unpaired, kept_pairs, kept_lines, bytes_to_host, filter_ms."""
        o = KeptInfo()
        self._check(self.lib.lzani_get_kept_info(self.h, C.byref(o)), "lzani_get_kept_info")
        return _kept_info(o)

    def set_region_capacity(self, regions):
        """lzani_set_region_capacity: the first capacity of the later run_rows_aligned calls, in regions; 0 = automatic."""
        self._check(self.lib.lzani_set_region_capacity(self.h, C.c_uint64(int(regions))), "lzani_set_region_capacity")

    def run_rows_aligned(self, ref_ids, row_off, query_ids=None, kept_flt=None, report_len=None, aln_flt=None, aln_len=None, results=True):
        """lzani_run_rows_aligned: one run with the region sink on the device, then the output filter's stage (kept_flt: an
        OutFilter or a dict, None: none) and the region stage (aln_flt likewise, None: no entry is dropped).  Returns
        (results int32[entries, 3] or None, the number of kept pairs, the number of regions that stay); kept_fetch() and
        regions_fetch() read the two results."""
        ref_ids = np.ascontiguousarray(ref_ids, dtype=np.uint32)
        row_off = np.ascontiguousarray(row_off, dtype=np.uint64)
        q = None if query_ids is None else np.ascontiguousarray(query_ids, dtype=np.uint32)
        rl = None if report_len is None else np.ascontiguousarray(report_len, dtype=np.uint32)
        al = None if aln_len is None else np.ascontiguousarray(aln_len, dtype=np.uint32)
        kf, af = _filter_or_null(kept_flt), _filter_or_null(aln_flt)
        out = np.zeros((int(row_off[-1]) if len(row_off) else 0, 3), dtype=np.int32) if results else None
        nk, nr = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.lzani_run_rows_aligned(self.h, len(ref_ids), _ptr(ref_ids), _ptr(row_off), _ptr(q), _ptr(out) if results and len(out) else None,
                                                    C.byref(kf) if kf is not None else None, _ptr(rl), C.byref(af) if af is not None else None, _ptr(al),
                                                    C.byref(nk), C.byref(nr)), "lzani_run_rows_aligned")
        return out, int(nk.value), int(nr.value)

    def order_regions(self, n, aln_len, ref_ids, row_off, query_ids, regions, flt=None, fetch=True):
        """lzani_debug_order_regions: the region stage alone on made-up REGION_DTYPE regions of n genomes (uploaded here).
        Returns the regions that stay, all fetched at once, or with fetch=False their number."""
        ref_ids = np.ascontiguousarray(ref_ids, dtype=np.uint32)
        row_off = np.ascontiguousarray(row_off, dtype=np.uint64)
        q = None if query_ids is None else np.ascontiguousarray(query_ids, dtype=np.uint32)
        al = np.ascontiguousarray(aln_len, dtype=np.uint32)
        r = np.ascontiguousarray(regions, dtype=REGION_DTYPE)
        f = _filter_or_null(flt)
        cnt = C.c_uint64(0)
        self._check(self.lib.lzani_debug_order_regions(self.h, int(n), _ptr(al), len(ref_ids), _ptr(ref_ids), _ptr(row_off), _ptr(q),
                                                       _ptr(r) if len(r) else None, C.c_uint64(len(r)), C.byref(f) if f is not None else None,
                                                       C.byref(cnt)), "lzani_debug_order_regions")
        return self.regions_fetch(0, int(cnt.value)) if fetch else int(cnt.value)

    def regions_fetch(self, first, count):
        """lzani_regions_fetch: records first .. first + count - 1 of the regions result (REGION_DTYPE)."""
        out = np.zeros(int(count), dtype=REGION_DTYPE)
        self._check(self.lib.lzani_regions_fetch(self.h, C.c_uint64(int(first)), C.c_uint64(int(count)), _ptr(out) if count else None),
                    "lzani_regions_fetch")
        return out

    def regions_info(self):
        """lzani_get_regions_info: entries, found, kept, entries_with_regions, entries_dropped, capacity, runs, sort_passes,
        workspace_bytes, bytes_to_host, sums_ms, sort_ms, write_ms."""
        o = RegionsInfo()
        self._check(self.lib.lzani_get_regions_info(self.h, C.byref(o)), "lzani_get_regions_info")
        return _regions_info(o)

    def run_rows_device(self, ref_ids, row_off, query_ids, d_out_ptr):
        """Results stay on the GPU at raw device pointer d_out_ptr (3 int32 per pair)."""
        ref_ids = np.ascontiguousarray(ref_ids, dtype=np.uint32)
        row_off = np.ascontiguousarray(row_off, dtype=np.uint64)
        q = None if query_ids is None else np.ascontiguousarray(query_ids, dtype=np.uint32)
        self._check(self.lib.lzani_run_rows_device(self.h, len(ref_ids), _ptr(ref_ids), _ptr(row_off), _ptr(q),
                                                   C.c_void_p(int(d_out_ptr))), "lzani_run_rows_device")

    REGION_DTYPE = np.dtype([("pair", np.uint64), ("ref_start", np.int32), ("ref_end", np.int32), ("seq_start", np.int32),
                             ("seq_end", np.int32), ("num_matches", np.int32), ("num_mismatches", np.int32)])

    def run_rows_regions(self, ref_ids, row_off, query_ids=None, capacity=1 << 16):
        """(results int32[n_pairs, 3], regions structured array sorted by (pair, length desc, seq_start))."""
        ref_ids = np.ascontiguousarray(ref_ids, dtype=np.uint32)
        row_off = np.ascontiguousarray(row_off, dtype=np.uint64)
        q = None if query_ids is None else np.ascontiguousarray(query_ids, dtype=np.uint32)
        n_pairs = int(row_off[-1]) if len(row_off) else 0
        while True:
            out = np.zeros((n_pairs, 3), dtype=np.int32)
            regs = np.zeros(capacity, dtype=self.REGION_DTYPE)
            cnt = C.c_uint64(0)
            self._check(self.lib.lzani_run_rows_regions(self.h, len(ref_ids), _ptr(ref_ids), _ptr(row_off), _ptr(q), _ptr(out),
                                                        _ptr(regs), capacity, C.byref(cnt)), "lzani_run_rows_regions")
            if cnt.value <= capacity:
                break
            capacity = int(cnt.value)
        regs = regs[:cnt.value]
        order = np.lexsort((regs["seq_start"], -(regs["seq_end"] - regs["seq_start"]), regs["pair"]))
        return out, regs[order]

    def all2all(self):
        """int32[n, n, 3]: out[r, q] = parse(query=q, ref=r), diagonal zero."""
        n = self.n
        ref_ids, row_off = dense_rows(n)
        flat = self.run_rows(ref_ids, row_off, None)
        out = np.zeros((n, n, 3), dtype=np.int32)
        out[~np.eye(n, dtype=bool)] = flat
        return out

    def comm_init(self, n_ranks, rank, unique_id):
        """RCCL communicator of this context (one process per GPU); unique_id = comm_unique_id() of rank 0."""
        buf = (C.c_uint8 * 128)(*unique_id)
        self._check(self.lib.lzani_comm_init(self.h, n_ranks, rank, buf), "lzani_comm_init")

    def comm_allgather(self, d_send_ptr, d_recv_ptr, n_results):
        self._check(self.lib.lzani_comm_allgather(self.h, C.c_void_p(int(d_send_ptr)), C.c_void_p(int(d_recv_ptr)), n_results),
                    "lzani_comm_allgather")

    def comm_gatherv(self, d_send_ptr, d_recv_ptr, counts, root=0):
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        self._check(self.lib.lzani_comm_gatherv(self.h, C.c_void_p(int(d_send_ptr)), C.c_void_p(int(d_recv_ptr or 0)),
                                                _ptr(counts), root), "lzani_comm_gatherv")

    def timing(self):
        t = Timing()
        self._check(self.lib.lzani_get_timing(self.h, C.byref(t)), "lzani_get_timing")
        return dict(index_ms=t.index_ms, pairs_ms=t.pairs_ms, pair_launches=t.pair_launches,
                    index_launches=t.index_launches, pairs=t.pairs, cand_ms=t.cand_ms, kmers_ms=t.kmers_ms,
                    cand_launches=t.cand_launches)

    def layout(self):
        o = LayoutInfo()
        self._check(self.lib.lzani_get_layout(self.h, C.byref(o)), "lzani_get_layout")
        return {k: getattr(o, k) for k, _ in LayoutInfo._fields_}

    def rtc_info(self):
        o = RtcInfo()
        self._check(self.lib.lzani_get_rtc_info(self.h, C.byref(o)), "lzani_get_rtc_info")
        return {k: getattr(o, k) for k, _ in RtcInfo._fields_ if k != "reserved_"}

    def kernel_launches(self):
        """Launches of the last run per pair-kernel instantiation: {name: count}, nonzero entries only."""
        names = kernel_names()
        counts = np.zeros(len(names), dtype=np.uint64)
        n = self.lib.lzani_debug_kernel_launches(self.h, _ptr(counts), len(counts))
        if n < 0:
            self._check(n, "lzani_debug_kernel_launches")
        assert n == len(names), (n, len(names))
        return {names[i]: int(counts[i]) for i in range(len(names)) if counts[i]}

    def split_stats(self):
        """lzani_debug_split_stats: the split path's repair loop in the last run -- pairs_cut, rounds (the most of a batch),
        resumed, given_up and voids (a list by cause 0..5)."""
        o = SplitStats()
        self._check(self.lib.lzani_debug_split_stats(self.h, C.byref(o)), "lzani_debug_split_stats")
        return dict(pairs_cut=int(o.pairs_cut), rounds=int(o.rounds), resumed=int(o.resumed), given_up=int(o.given_up),
                    voids=[int(v) for v in o.voids])

    def debug_sort_segments(self, keys, seg_len, n_seg, begin_bit, end_bit):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        assert keys.size == seg_len * n_seg
        out = np.zeros_like(keys)
        self._check(self.lib.lzani_debug_sort_segments(self.h, _ptr(keys), _ptr(out), C.c_uint64(seg_len), C.c_uint32(n_seg),
                                                       C.c_int(begin_bit), C.c_int(end_bit)), "debug_sort_segments")
        return out

    def debug_index(self, gid):
        mrd = self.params["mrd"]
        T = 2 * int(self.lens[gid]) + 3 * mrd
        wn = (T + 63) // 64 + 2
        geom = np.zeros(4, dtype=np.uint32)
        self._check(self.lib.lzani_debug_get_index(self.h, gid, None, None, None, None, None, _ptr(geom)), "debug")
        nm = np.zeros(wn, dtype=np.uint64)
        t2 = np.zeros(2 * wn, dtype=np.uint64)
        dirz = np.zeros((1 << int(geom[1])) + 1, dtype=np.uint32)
        ent = np.zeros(T + 1, dtype=np.uint32)
        n_ent = C.c_uint32(0)
        self._check(self.lib.lzani_debug_get_index(self.h, gid, _ptr(t2), _ptr(nm), _ptr(dirz), _ptr(ent),
                                                   C.byref(n_ent), _ptr(geom)), "debug")
        return dict(t2=t2, nm=nm, dirz=dirz, ent=ent[:n_ent.value].copy(), geom=geom)

    def debug_index_slab(self, ref_ids, with_filter=True, with_tw=True):
        """The index slabs of one batch of reference ids (lzani_debug_index_slab): a dict of the geometry, the build that ran
        ("lds", "atomics", "sort") and per-slot arrays [rows, stride] of dirz, ent, bk, tw, fl (None where not built) and
        status (LDS build: nonzero = the slot fell back to the global-atomics kernels)."""
        ref_ids = np.ascontiguousarray(ref_ids, dtype=np.uint32)
        rows = len(ref_ids)
        info = SlabInfo()
        self._check(self.lib.lzani_debug_index_slab(self.h, rows, _ptr(ref_ids), int(with_filter), int(with_tw), C.byref(info),
                                                    None, None, None, None, None, None), "lzani_debug_index_slab")
        bufs = {k: np.zeros((rows, getattr(info, k + "_stride")), dtype=np.uint32) for k in ("dir", "ent", "bk", "tw", "fl")}
        status = np.zeros(rows, dtype=np.uint32)
        self._check(self.lib.lzani_debug_index_slab(self.h, rows, _ptr(ref_ids), int(with_filter), int(with_tw), C.byref(info),
                                                    *[_ptr(bufs[k]) for k in ("dir", "ent", "bk", "tw", "fl")], _ptr(status)),
                    "lzani_debug_index_slab")
        out = {k: getattr(info, k) for k, _ in SlabInfo._fields_}
        out["build"] = INDEX_BUILDS[info.build]
        out.update(dirz=bufs["dir"], ent=bufs["ent"], status=status)
        for k in ("bk", "tw", "fl"):
            out[k] = bufs[k] if getattr(info, k + "_stride") else None
        return out

    def debug_run_candidates(self, ref_ids, row_off, query_ids=None, words=None):
        """lzani_run_rows plus every pair's candidate bitmap (first `words` 32-bit words; default: enough for the longest
        genome) and candidate count (0xFFFFFFFF where its batch did not count): (results int32[n_pairs, 3],
        cbits uint32[n_pairs, words], pcount uint32[n_pairs], plan dict)."""
        ref_ids = np.ascontiguousarray(ref_ids, dtype=np.uint32)
        row_off = np.ascontiguousarray(row_off, dtype=np.uint64)
        q = None if query_ids is None else np.ascontiguousarray(query_ids, dtype=np.uint32)
        n_pairs = int(row_off[-1]) if len(row_off) else 0
        if words is None:
            words = (int(self.lens.max()) + self.params["mrd"] + 320 + 1023) // 1024 * 32
        out = np.zeros((n_pairs, 3), dtype=np.int32)
        cbits = np.zeros((n_pairs, words), dtype=np.uint32)
        pcount = np.zeros(n_pairs, dtype=np.uint32)
        plan = CandPlan()
        self._check(self.lib.lzani_debug_run_candidates(self.h, len(ref_ids), _ptr(ref_ids), _ptr(row_off), _ptr(q), _ptr(out),
                                                        C.c_uint64(words), _ptr(cbits), _ptr(pcount), C.byref(plan)),
                    "lzani_debug_run_candidates")
        return out, cbits, pcount, {k: getattr(plan, k) for k, _ in CandPlan._fields_}
