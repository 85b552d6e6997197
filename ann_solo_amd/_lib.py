"""ctypes loader for libannsolo_mi.so (the C ABI of include/annsolo_mi.h).

The product path has no CPU fallback: if the shared library is missing or no HIP
device is present, every compute call raises ``AnnSoloMiError``.
"""
import ctypes as C
import os
import subprocess
from ctypes import byref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ASL_LIB_PATH: load another build of the same library (same-box A/B measurements)
LIB_PATH = os.environ.get('ASL_LIB_PATH') or os.path.join(_HERE, 'libannsolo_mi.so')
_lib = None

c_f32p = C.POINTER(C.c_float)
c_f64p = C.POINTER(C.c_double)
c_i32p = C.POINTER(C.c_int32)
c_i64p = C.POINTER(C.c_int64)
c_u8p = C.POINTER(C.c_uint8)
c_u32p = C.POINTER(C.c_uint32)


TK_MAX_K = 2048      # largest nprobe / single-pass k of the LDS top-k (csrc/ivf_kernels.hpp)
TK_MAX_K_PASSES = 16384   # largest k of a search (bounded passes beyond TK_MAX_K)
SCORE_HIST_BINS = 128     # include/annsolo_mi.h: ASL_SCORE_HIST_BINS


class AnnSoloMiError(RuntimeError):
    code = None     # the negative ASL_ERR_* value where the error came from the library (``check``)


class AslPeaks(C.Structure):
    _fields_ = [('n', C.c_int32), ('offsets', C.c_void_p), ('mz', C.c_void_p),
                ('intensity', C.c_void_p), ('charge', C.c_void_p),
                ('precursor_mz', C.c_void_p), ('precursor_charge', C.c_void_p),
                ('n_peaks', C.c_int64)]


class AslSearchParams(C.Structure):
    _fields_ = [('min_bound', C.c_double), ('bin_size', C.c_double),
                ('hash_seed', C.c_uint32), ('k', C.c_int32), ('nprobe', C.c_int32),
                ('charge', C.c_int32), ('precursor_tol', C.c_double),
                ('precursor_mode', C.c_int32), ('fragment_mz_tolerance', C.c_double),
                ('allow_shift', C.c_int32), ('use_ann', C.c_int32),
                # [nq, 2] float64 (lo, hi), host or device: read with precursor_mode 2 (ASL_TOL_INTERVAL) only
                ('precursor_window', C.c_void_p)]


class AslProcessParams(C.Structure):
    _fields_ = [('min_mz', C.c_double), ('max_mz', C.c_double), ('remove_precursor', C.c_int32),
                ('remove_precursor_tolerance', C.c_double), ('min_intensity', C.c_double),
                ('max_peaks', C.c_int32), ('scaling', C.c_int32), ('min_peaks', C.c_int32),
                ('min_mz_range', C.c_double), ('round_mz', C.c_int32), ('resolution', C.c_int32)]


class AslIndexInfo(C.Structure):
    _fields_ = [('d', C.c_int32), ('nlist', C.c_int32), ('kind', C.c_int32),
                ('pq_m', C.c_int32), ('pq_ksub', C.c_int32), ('pq_dsub', C.c_int32),
                ('ntotal', C.c_int64), ('nlocal', C.c_int64), ('trained', C.c_int32),
                ('shard_rank', C.c_int32), ('shard_world', C.c_int32)]


EXPORTS = [
    'asl_last_error', 'asl_version', 'asl_get_num_gpus', 'asl_set_device', 'asl_set_stream',
    'asl_synchronize', 'asl_set_pipeline', 'asl_set_scan_postfilter', 'asl_set_window_pair_budget', 'asl_get_dim', 'asl_hash_idx', 'asl_encode_batch', 'asl_index_create',
    'asl_index_free', 'asl_index_train', 'asl_index_add', 'asl_index_add_preassigned', 'asl_index_search',
    'asl_index_reset', 'asl_index_ntotal', 'asl_index_is_trained', 'asl_index_save',
    'asl_index_load', 'asl_index_set_niter', 'asl_index_info', 'asl_index_get_centroids',
    'asl_index_get_codebooks', 'asl_index_set_trained', 'asl_index_get_lists',
    'asl_index_shard', 'asl_index_shard_map', 'asl_topk_merge', 'asl_index_coarse',
    'asl_index_pq_lut', 'asl_rescore_batch', 'asl_library_create', 'asl_library_free',
    'asl_library_size', 'asl_search_batch', 'asl_window_candidates', 'asl_profile_enable',
    'asl_profile_reset', 'asl_profile_get', 'asl_profile_scanned_vectors',
    'asl_rescore_knn', 'asl_lpt_owner', 'asl_index_supports_keys', 'asl_index_search_sharded', 'asl_index_postings_work', 'asl_index_set_refine', 'asl_index_get_refine', 'asl_index_refine', 'asl_index_set_scan_variant', 'asl_index_codes_mmajor', 'asl_index_search_preassigned', 'asl_process_batch',
    'asl_ssm_features_batch', 'asl_ssm_cosine_batch', 'asl_index_set_unordered', 'asl_topk_merge_keys',
    'asl_index_set_flat_storage', 'asl_index_get_flat_storage', 'asl_index_flat_layout',
    'asl_keys_split', 'asl_keys_merge_heads', 'asl_keys_extras', 'asl_keys_merge_final',
    'asl_keys_rescan_list', 'asl_shard_k', 'asl_index_search_gated', 'asl_index_search_entries',
    'asl_encode_entries_batch', 'asl_index_search_sharded_ex',
    'asl_index_set_window_key', 'asl_index_search_window', 'asl_index_set_window_scan',
    'asl_rescore_batch_topn', 'asl_search_batch_topn', 'asl_rescore_knn_topn',
    'asl_index_rank',
    'asl_index_set_by_residual', 'asl_index_get_by_residual',
    'asl_library_set_groups', 'asl_rescore_batch_topn_distinct', 'asl_search_batch_topn_distinct',
    'asl_rescore_knn_topn_distinct',
    'asl_profile_rescore_counts',
    'asl_library_set_selection', 'asl_index_set_selector', 'asl_index_search_selected',
    'asl_rescore_batch_topn_hist', 'asl_search_batch_topn_hist', 'asl_rescore_knn_topn_hist',
    'asl_decoy_batch',
    'asl_localize_batch', 'asl_deplete_batch',
    'asl_l2svm_fit', 'asl_linear_scores',
    'asl_forest_bin', 'asl_forest_fit', 'asl_forest_predict', 'asl_set_forest_workspace',
    'asl_tdc_qvalues',
    'asl_ssm_groups',
    'asl_mgf_measure', 'asl_mgf_fill', 'asl_mgf_sort', 'asl_mgf_number',
    'asl_mgf_sort_charged', 'asl_sptxt_measure', 'asl_sptxt_fill', 'asl_sptxt_fragment_charge',
    'asl_mzml_measure', 'asl_mzml_fill', 'asl_mzml_inflate',
    'asl_mzxml_measure', 'asl_mzxml_fill', 'asl_mzxml_duration', 'asl_mzxml_pairs',
]

SVM_MAX_DIM = 63          # include/annsolo_mi.h: ASL_SVM_MAX_DIM
SVM_MAX_PROBLEMS = 32     # ASL_SVM_MAX_PROBLEMS


class AslL2SvmParams(C.Structure):
    _fields_ = [('C', C.c_double), ('gtol_abs', C.c_double), ('gtol_rel', C.c_double),
                ('max_newton', C.c_int32)]


FOREST_MAX_BINS = 256     # ASL_FOREST_MAX_BINS
FOREST_MAX_DEPTH = 12     # ASL_FOREST_MAX_DEPTH
FOREST_MAX_TREES = 1024   # ASL_FOREST_MAX_TREES
FOREST_NODES = 8191       # ASL_FOREST_NODES
FOREST_ROW = 64           # ASL_FOREST_ROW


class AslForestParams(C.Structure):
    _fields_ = [('trees', C.c_int32), ('max_depth', C.c_int32), ('seed', C.c_uint32)]


class AslForestModel(C.Structure):
    _fields_ = [('trees', C.c_int32), ('max_depth', C.c_int32), ('col', C.c_void_p), ('bin', C.c_void_p),
                ('n0', C.c_void_p), ('n1', C.c_void_p), ('value', C.c_void_p)]


def build(force: bool = False) -> str:
    """Compile libannsolo_mi.so for gfx950 with hipcc (cross-compiles without a GPU).
    ``force`` (or ASL_FORCE_REBUILD=1) recompiles every translation unit; otherwise only what is
    older than its sources. Every run appends one line to ``csrc/build/build.log`` naming the
    objects that were recompiled."""
    import time
    src = os.path.join(_HERE, 'csrc')
    force = force or os.environ.get('ASL_FORCE_REBUILD', '') not in ('', '0')
    stale = force or not os.path.exists(LIB_PATH)
    if not stale:
        t = os.path.getmtime(LIB_PATH)
        deps = [os.path.join(src, f) for f in os.listdir(src)
                if f.endswith(('.hip', '.hpp'))]
        deps.append(os.path.join(_HERE, '..', 'include', 'annsolo_mi.h'))
        stale = any(os.path.getmtime(p) > t for p in deps)
    rebuilt = []
    if stale:
        if not os.path.exists('/opt/rocm/bin/hipcc'):
            raise AnnSoloMiError('hipcc not found and libannsolo_mi.so is stale/missing')
        obj_dir = os.path.join(src, 'build')
        before = {f: os.path.getmtime(os.path.join(obj_dir, f))
                  for f in (os.listdir(obj_dir) if os.path.isdir(obj_dir) else []) if f.endswith('.o')}
        cmd = ['make', '-C', src, '-j8'] + (['-B'] if force else [])
        subprocess.check_call(cmd)
        for f in sorted(os.listdir(obj_dir)):
            if f.endswith('.o') and os.path.getmtime(os.path.join(obj_dir, f)) > before.get(f, 0.0):
                rebuilt.append(f)
    try:
        os.makedirs(os.path.join(src, 'build'), exist_ok=True)
        with open(os.path.join(src, 'build', 'build.log'), 'a') as f:
            f.write('%s force=%d recompiled=%d [%s] -> %s\n' % (
                time.strftime('%Y-%m-%dT%H:%M:%S'), int(force), len(rebuilt), ' '.join(rebuilt),
                os.path.basename(LIB_PATH)))
    except OSError:
        pass
    print('[build] libannsolo_mi.so: %d translation units recompiled for gfx950%s'
          % (len(rebuilt), (' (' + ' '.join(rebuilt) + ')') if rebuilt else ' (up to date)'))
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AnnSoloMiError(
                f'{LIB_PATH} is missing: build it with __graft_entry__.build() '
                '(there is no CPU fallback)')
        # torch first: it ships a HIP runtime of its own, and in a process where this library was loaded
        # and touched the device before torch was imported, torch finds no GPU afterwards ("No HIP GPUs
        # are available"); with torch imported first both work (tests/test_gpu_index.py)
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        L.asl_last_error.restype = C.c_char_p
        L.asl_version.restype = C.c_char_p
        L.asl_hash_idx.restype = C.c_int32
        L.asl_hash_idx.argtypes = [C.c_int64, C.c_int32, C.c_uint32]
        L.asl_get_dim.argtypes = [C.c_double, C.c_double, C.c_double, c_i64p, c_f64p, c_f64p]
        L.asl_encode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.c_double, C.c_double, C.c_int32, C.c_uint32, C.c_int,
                                       C.c_void_p]
        L.asl_index_create.restype = C.c_void_p
        L.asl_index_create.argtypes = [C.c_int32] * 5
        L.asl_index_free.argtypes = [C.c_void_p]
        L.asl_index_free.restype = None
        L.asl_index_train.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64]
        L.asl_index_add.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.asl_index_add_preassigned.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.asl_index_search.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                       C.c_int32, C.c_void_p, C.c_void_p]
        L.asl_index_search_preassigned.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                                   C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p]
        L.asl_process_batch.argtypes = [C.POINTER(AslPeaks), C.POINTER(AslProcessParams),
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.asl_ssm_features_batch.argtypes = [C.POINTER(AslPeaks), C.POINTER(AslPeaks), C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_int32, C.c_double,
                                             C.c_double, C.c_double, C.c_int32, C.c_void_p]
        L.asl_ssm_cosine_batch.argtypes = [C.POINTER(AslPeaks), C.POINTER(AslPeaks), C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.asl_index_search_sharded.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                               C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.asl_index_search_sharded_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                                  C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                                  C.c_int32, C.c_int32, C.c_int64]
        L.asl_index_set_refine.argtypes = [C.c_void_p, C.c_int32]
        L.asl_index_refine.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                       C.c_int32, C.c_void_p, C.c_void_p]
        L.asl_index_reset.argtypes = [C.c_void_p]
        L.asl_index_ntotal.argtypes = [C.c_void_p]
        L.asl_index_ntotal.restype = C.c_int64
        L.asl_index_is_trained.argtypes = [C.c_void_p]
        L.asl_index_save.argtypes = [C.c_void_p, C.c_char_p]
        L.asl_index_load.argtypes = [C.c_char_p]
        L.asl_index_load.restype = C.c_void_p
        L.asl_index_set_niter.argtypes = [C.c_void_p, C.c_int32]
        L.asl_index_set_scan_variant.argtypes = [C.c_void_p, C.c_int32]
        if hasattr(L, 'asl_index_codes_mmajor'):      # (an older library given by ASL_LIB_PATH has none)
            L.asl_index_codes_mmajor.argtypes = [C.c_void_p]
        L.asl_index_set_window_key.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.asl_index_search_window.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                              C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                              C.c_void_p]
        L.asl_index_set_window_scan.argtypes = [C.c_void_p, C.c_int32]
        L.asl_index_rank.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p]
        L.asl_index_set_flat_storage.argtypes = [C.c_void_p, C.c_int32]
        L.asl_index_flat_layout.argtypes = [C.c_void_p]
        L.asl_index_get_flat_storage.argtypes = [C.c_void_p]
        L.asl_keys_split.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.asl_keys_merge_heads.argtypes = [C.c_int32] * 4 + [C.c_void_p] * 4
        L.asl_keys_rescan_list.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]
        L.asl_keys_extras.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int32]
        L.asl_keys_merge_final.argtypes = [C.c_int32] * 4 + [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                             C.c_void_p, C.c_void_p, C.c_void_p]
        L.asl_shard_k.argtypes = [C.c_int32, C.c_int32]
        L.asl_shard_k.restype = C.c_int32
        L.asl_index_supports_keys.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.asl_index_search_gated.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.asl_index_search_entries.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.asl_encode_entries_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                               C.c_double, C.c_double, C.c_int32, C.c_uint32, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_void_p]
        L.asl_index_postings_work.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, c_i64p, c_i64p]
        L.asl_index_get_refine.argtypes = [C.c_void_p]
        L.asl_index_get_refine.restype = C.c_int32
        L.asl_index_set_unordered.argtypes = [C.c_void_p, C.c_int32]
        L.asl_topk_merge_keys.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int32]
        L.asl_index_info.argtypes = [C.c_void_p, C.POINTER(AslIndexInfo)]
        L.asl_index_get_centroids.argtypes = [C.c_void_p, C.c_void_p]
        L.asl_index_get_codebooks.argtypes = [C.c_void_p, C.c_void_p]
        L.asl_index_set_trained.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.asl_index_get_lists.argtypes = [C.c_void_p] * 5
        L.asl_index_shard.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.asl_index_shard_map.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.asl_topk_merge.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]
        L.asl_index_coarse.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                       C.c_void_p, C.c_void_p]
        L.asl_index_pq_lut.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.asl_rescore_batch.argtypes = [C.POINTER(AslPeaks), C.POINTER(AslPeaks), C.c_void_p,
                                        C.c_void_p, C.c_double, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        L.asl_library_create.restype = C.c_void_p
        L.asl_library_create.argtypes = [C.POINTER(AslPeaks), C.c_void_p, C.c_void_p]
        L.asl_library_free.argtypes = [C.c_void_p]
        L.asl_library_free.restype = None
        L.asl_library_size.argtypes = [C.c_void_p]
        L.asl_library_size.restype = C.c_int64
        L.asl_search_batch.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(AslPeaks),
                                       C.POINTER(AslSearchParams), C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.c_void_p]
        L.asl_rescore_knn.argtypes = [C.c_void_p, C.POINTER(AslPeaks),
                                      C.POINTER(AslSearchParams), C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        L.asl_rescore_batch_topn.argtypes = [C.POINTER(AslPeaks), C.POINTER(AslPeaks), C.c_void_p,
                                             C.c_void_p, C.c_double, C.c_int, C.c_int32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        L.asl_search_batch_topn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(AslPeaks),
                                            C.POINTER(AslSearchParams), C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                            C.c_void_p]
        L.asl_rescore_knn_topn.argtypes = [C.c_void_p, C.POINTER(AslPeaks),
                                           C.POINTER(AslSearchParams), C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_int32]
        # (an ASL_LIB_PATH build from before these exports still loads, for A/B runs of the calls it
        # has; calling a missing one raises AttributeError)
        if hasattr(L, 'asl_library_set_groups'):
            L.asl_library_set_groups.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
            L.asl_rescore_batch_topn_distinct.argtypes = [C.POINTER(AslPeaks), C.POINTER(AslPeaks), C.c_void_p,
                                                          C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int32,
                                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
            L.asl_search_batch_topn_distinct.argtypes = L.asl_search_batch_topn.argtypes
            L.asl_rescore_knn_topn_distinct.argtypes = L.asl_rescore_knn_topn.argtypes
        if hasattr(L, 'asl_library_set_selection'):
            L.asl_library_set_selection.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
            L.asl_index_set_selector.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
            L.asl_index_search_selected.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                                    C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                                    C.c_void_p]
        if hasattr(L, 'asl_search_batch_topn_hist'):
            L.asl_rescore_batch_topn_hist.argtypes = [C.POINTER(AslPeaks), C.POINTER(AslPeaks), C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int32,
                                                      C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_int32, C.c_void_p]
            L.asl_search_batch_topn_hist.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(AslPeaks),
                                                     C.POINTER(AslSearchParams), C.c_int32, C.c_int32, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                     C.c_void_p, C.c_void_p]
            L.asl_rescore_knn_topn_hist.argtypes = [C.c_void_p, C.POINTER(AslPeaks),
                                                    C.POINTER(AslSearchParams), C.c_void_p, C.c_int32, C.c_int32,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_int32, C.c_void_p]
        if hasattr(L, 'asl_decoy_batch'):
            L.asl_decoy_batch.argtypes = [C.POINTER(AslPeaks)] + [C.c_void_p] * 6 + [C.c_double, C.c_int32] + \
                [C.c_void_p] * 8
        if hasattr(L, 'asl_localize_batch'):
            L.asl_localize_batch.argtypes = [C.POINTER(AslPeaks)] + [C.c_void_p] * 6 + [C.c_double, C.c_int32] + \
                [C.c_void_p] * 9
        if hasattr(L, 'asl_deplete_batch'):
            L.asl_deplete_batch.argtypes = [C.POINTER(AslPeaks), C.POINTER(AslPeaks), C.c_void_p, C.c_double, C.c_int,
                                            C.c_int32, C.c_double, C.c_int32] + [C.c_void_p] * 6
        if hasattr(L, 'asl_l2svm_fit'):
            L.asl_l2svm_fit.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                        C.POINTER(AslL2SvmParams)] + [C.c_void_p] * 4
            L.asl_linear_scores.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        if hasattr(L, 'asl_forest_fit'):
            L.asl_forest_bin.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
            L.asl_forest_fit.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.c_void_p, C.POINTER(AslForestParams), C.POINTER(AslForestModel)]
            L.asl_forest_predict.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(AslForestModel), C.c_int32,
                                             C.c_int32, C.c_void_p]
            L.asl_set_forest_workspace.argtypes = [C.c_int64]
            L.asl_set_forest_workspace.restype = C.c_int64
        if hasattr(L, 'asl_tdc_qvalues'):
            L.asl_tdc_qvalues.argtypes = [C.c_void_p] * 4 + [C.c_int64, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]
        if hasattr(L, 'asl_ssm_groups'):
            L.asl_ssm_groups.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, c_i64p, c_i64p, C.c_void_p,
                                         C.c_void_p]
        if hasattr(L, 'asl_mgf_measure'):
            L.asl_mgf_measure.argtypes = [C.c_void_p, C.c_int64, C.c_int32, c_i64p]
            L.asl_mgf_fill.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 10
            L.asl_mgf_sort.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, c_i64p]
            L.asl_mgf_number.argtypes = [C.c_char_p, C.c_int32, c_f64p]
        if hasattr(L, 'asl_sptxt_measure'):
            L.asl_mgf_sort_charged.argtypes = [C.c_void_p] * 4 + [C.c_int32, C.c_int64, c_i64p]
            L.asl_sptxt_measure.argtypes = [C.c_void_p, C.c_int64, C.c_int32, c_i64p]
            L.asl_sptxt_fill.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 7
            L.asl_sptxt_fragment_charge.argtypes = [C.c_char_p, C.c_int32]
        if hasattr(L, 'asl_mzml_measure'):
            L.asl_mzml_measure.argtypes = [C.c_void_p, C.c_int64, C.c_int32, c_i64p]
            L.asl_mzml_fill.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 14
            L.asl_mzml_inflate.argtypes = [C.c_char_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, c_i64p]
        if hasattr(L, 'asl_mzxml_measure'):
            L.asl_mzxml_measure.argtypes = [C.c_void_p, C.c_int64, C.c_int32, c_i64p]
            L.asl_mzxml_fill.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 14
            L.asl_mzxml_duration.argtypes = [C.c_char_p, C.c_int32, c_f64p]
            L.asl_mzxml_pairs.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        if hasattr(L, 'asl_index_set_by_residual'):
            L.asl_index_set_by_residual.argtypes = [C.c_void_p, C.c_int32]
            L.asl_index_get_by_residual.argtypes = [C.c_void_p]
        L.asl_lpt_owner.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        L.asl_window_candidates.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                            C.c_double, C.c_int32, C.c_void_p, C.c_void_p]
        L.asl_set_stream.argtypes = [C.c_void_p]
        L.asl_set_window_pair_budget.argtypes = [C.c_int64]
        L.asl_set_window_pair_budget.restype = C.c_int64
        L.asl_profile_get.argtypes = [C.c_char_p, c_f64p, c_i64p]
        L.asl_profile_scanned_vectors.restype = C.c_int64
        if hasattr(L, 'asl_profile_rescore_counts'):
            L.asl_profile_rescore_counts.argtypes = [c_i64p, c_i64p, c_i64p]
        _lib = L
    return _lib


def check(rc: int):
    if rc != 0:
        msg = lib().asl_last_error()
        err = AnnSoloMiError(f'libannsolo_mi error {rc}: {msg.decode() if msg else ""}')
        err.code = int(rc)
        raise err


def ptr(a):
    """Raw address of a numpy array or torch tensor (host or device), or None."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        if not a.flags['C_CONTIGUOUS']:
            raise ValueError('array must be C-contiguous')
        return a.ctypes.data
    if hasattr(a, 'data_ptr'):
        if not a.is_contiguous():
            raise ValueError('tensor must be contiguous')
        if a.is_cuda:
            _require_default_stream(a.device)
        return a.data_ptr()
    raise TypeError(type(a))


_DEFAULT_RAW = {}


def _default_raw_stream(idx: int) -> int:
    import torch
    if idx not in _DEFAULT_RAW:
        _DEFAULT_RAW[idx] = int(torch.cuda.default_stream(idx).cuda_stream)
    return _DEFAULT_RAW[idx]


def _require_default_stream(device):
    """The library issues its kernels on the null stream (and, in pipeline mode, on streams of
    its own that it orders against the null stream). That is ordered with PyTorch only while
    PyTorch's CURRENT stream is its default stream: under ``torch.cuda.stream(s)`` with a
    non-blocking ``s`` the tensors handed over here could still be written, or be read back
    before the library has finished. Every device tensor crosses ``ptr()``, so the check lives
    here and such a call fails instead of racing."""
    import torch
    # (every device tensor of every call passes here: the raw-handle query is a C call of well
    # under a microsecond; the stream objects of the public API cost ~10 us a pair)
    try:
        idx = device.index if device.index is not None else torch.cuda.current_device()
        ok = torch._C._cuda_getCurrentRawStream(idx) == _default_raw_stream(idx)
    except AttributeError:      # a PyTorch without the private hook
        ok = torch.cuda.current_stream(device) == torch.cuda.default_stream(device)
    if not ok:
        raise AnnSoloMiError(
            'libannsolo_mi issues its work on the default HIP stream: call it with '
            "PyTorch's default stream current (not inside torch.cuda.stream(...)), or "
            'synchronise the side stream and switch back first')


def peaks_struct(p) -> AslPeaks:
    """AslPeaks view of a PackedSpectra (torch) or a tuple of numpy arrays."""
    if hasattr(p, 'offsets') and hasattr(p, 'precursor_charge'):
        arrs = (p.offsets, p.mz, p.intensity, p.charge, p.precursor_mz, p.precursor_charge)
        n = p.n
    else:
        arrs = p
        n = len(p[0]) - 1
    # a pack's peak arrays are exactly sized (offsets[n] == len(mz)): telling the library spares
    # it the read-back of offsets[n] from the device (a stream synchronisation per call)
    mz = arrs[1]
    n_peaks = int(mz.numel()) if hasattr(mz, 'numel') else int(len(mz))
    return AslPeaks(n, *[ptr(a) for a in arrs], n_peaks)


def _as_f64(a, ndim: int, what: str):
    """``a`` as C-contiguous float64, numpy (host) or torch (wherever it lives)."""
    if hasattr(a, 'data_ptr'):
        import torch
        a = a.to(torch.float64).contiguous()
    else:
        a = np.ascontiguousarray(a, np.float64)
    if a.ndim != ndim:
        raise ValueError(f'{what}: {ndim} dimensions expected, got {a.ndim}')
    return a


def l2svm_fit(X, label, cw, C: float = 1.0, gtol_abs: float = 1e-9, gtol_rel: float = 0.0,
              max_newton: int = 100, wb=None):
    """``asl_l2svm_fit``: P L2-regularised squared-hinge linear SVMs over one matrix ``X [n, d]`` (float64;
    numpy or torch, host or device). ``label [P, n]`` int8 in {+1, -1, 0} (0: the row is not part of the
    problem; numpy or torch), ``cw [P, 2]`` the weights of the -1 / +1 class, ``wb [P, d + 1]`` the starting
    point (default zeros). Returns ``(wb, objective, n_newton, status)`` as numpy arrays; status 0 converged
    (``||g|| <= max(gtol_abs, gtol_rel * ||g0||)``), 1 iteration cap, 2 line search stalled."""
    X = _as_f64(X, 2, 'X')
    n, d = int(X.shape[0]), int(X.shape[1])
    if hasattr(label, 'data_ptr'):
        import torch
        label = label.to(torch.int8).contiguous()
    else:
        label = np.ascontiguousarray(label, np.int8)
    if label.ndim != 2 or int(label.shape[1]) != n:
        raise ValueError(f'label: [P, {n}] expected, got {tuple(label.shape)}')
    P = int(label.shape[0])
    cw = np.ascontiguousarray(cw, np.float64)
    if cw.shape != (P, 2):
        raise ValueError(f'cw: [{P}, 2] expected, got {cw.shape}')
    wb = np.zeros((P, d + 1), np.float64) if wb is None else np.array(wb, np.float64, order='C')
    if wb.shape != (P, d + 1):
        raise ValueError(f'wb: [{P}, {d + 1}] expected, got {wb.shape}')
    objective, n_newton, status = np.zeros(P, np.float64), np.zeros(P, np.int32), np.zeros(P, np.int32)
    params = AslL2SvmParams(float(C), float(gtol_abs), float(gtol_rel), int(max_newton))
    check(lib().asl_l2svm_fit(ptr(X) if n else None, n, d, ptr(label) if n else None, ptr(cw), P,
                              byref(params), ptr(wb), ptr(objective), ptr(n_newton), ptr(status)))
    return wb, objective, n_newton, status


def linear_scores(X, wb):
    """``asl_linear_scores``: ``out[p, i] = wb[p, :d] . X[i] + wb[p, d]``, ``[P, n]`` float64; lives where
    ``X`` lives (numpy, or a torch tensor on ``X``'s device)."""
    X = _as_f64(X, 2, 'X')
    n, d = int(X.shape[0]), int(X.shape[1])
    wb = np.ascontiguousarray(wb, np.float64)
    if wb.ndim != 2 or wb.shape[1] != d + 1:
        raise ValueError(f'wb: [P, {d + 1}] expected, got {wb.shape}')
    P = int(wb.shape[0])
    if hasattr(X, 'data_ptr'):
        import torch
        out = torch.empty((P, n), dtype=torch.float64, device=X.device)
    else:
        out = np.empty((P, n), np.float64)
    check(lib().asl_linear_scores(ptr(X) if n else None, n, d, ptr(wb), P, ptr(out) if n else None))
    return out


class ForestModel:
    """P forests as ``asl_forest_fit`` writes them: ``col`` int16, ``bin`` uint8, ``n0`` / ``n1`` uint32 and
    ``value`` float64, each ``[P, trees, FOREST_NODES]`` (numpy, or torch tensors on one device), and the depth
    they were grown to."""
    FIELDS = (('col', np.int16), ('bin', np.uint8), ('n0', np.uint32), ('n1', np.uint32), ('value', np.float64))

    def __init__(self, P: int, trees: int, max_depth: int, device=None):
        self.P, self.trees, self.max_depth = int(P), int(trees), int(max_depth)
        shape = (self.P, self.trees, FOREST_NODES)
        for name, dt in self.FIELDS:
            if device is None:
                a = np.empty(shape, dt)
            else:
                import torch
                # (the counts travel as int32 bits on the torch side: numpy() reads them back as uint32)
                a = torch.empty(shape, dtype=getattr(torch, np.dtype(dt).name.replace('uint32', 'int32')),
                                device=device)
            setattr(self, name, a)

    def struct(self) -> AslForestModel:
        return AslForestModel(self.trees, self.max_depth, *[ptr(getattr(self, name)) for name, _ in self.FIELDS])

    def numpy(self) -> dict:
        """The five arrays on the host."""
        return {name: (a.cpu().numpy().view(dt) if hasattr(a, 'cpu') else a)
                for name, dt, a in ((name, dt, getattr(self, name)) for name, dt in self.FIELDS)}


def _as_bins(bins):
    if hasattr(bins, 'data_ptr'):
        import torch
        if bins.dtype != torch.uint8:
            raise ValueError(f'bins: uint8 expected, got {bins.dtype}')
        bins = bins.contiguous()
    else:
        bins = np.asarray(bins)
        if bins.dtype != np.uint8:
            raise ValueError(f'bins: uint8 expected, got {bins.dtype}')
        bins = np.ascontiguousarray(bins)
    if bins.ndim != 2 or int(bins.shape[1]) != FOREST_ROW:
        raise ValueError(f'bins: [n, {FOREST_ROW}] expected, got {tuple(bins.shape)}')
    return bins


def forest_bin(X, edges, n_edges):
    """``asl_forest_bin``: ``X [n, d]`` float64 (numpy or torch, host or device) to ``[n, 64]`` uint8 rows, where
    ``X`` lives: byte j of a row is the number of ``edges[j, :n_edges[j]]`` (ascending; ``[d, 255]``) below
    ``X[i, j]``, bytes d .. 63 are 0."""
    X = _as_f64(X, 2, 'X')
    n, d = int(X.shape[0]), int(X.shape[1])
    edges = np.ascontiguousarray(edges, np.float64)
    n_edges = np.ascontiguousarray(n_edges, np.int32)
    if edges.shape != (d, FOREST_MAX_BINS - 1):
        raise ValueError(f'edges: [{d}, {FOREST_MAX_BINS - 1}] expected, got {edges.shape}')
    if n_edges.shape != (d,):
        raise ValueError(f'n_edges: [{d}] expected, got {n_edges.shape}')
    if hasattr(X, 'data_ptr'):
        import torch
        out = torch.empty((n, FOREST_ROW), dtype=torch.uint8, device=X.device)
    else:
        out = np.empty((n, FOREST_ROW), np.uint8)
    check(lib().asl_forest_bin(ptr(X) if n else None, n, d, ptr(edges), ptr(n_edges), ptr(out) if n else None))
    return out


def forest_fit(bins, d: int, label, cw, trees: int = 100, max_depth: int = FOREST_MAX_DEPTH, seed: int = 1,
               n_bins=None) -> ForestModel:
    """``asl_forest_fit``: P histogram forests of ``trees`` trees over one binned matrix ``bins [n, 64]`` uint8
    with ``d`` columns (numpy or torch, host or device). ``label [P, n]`` int8 in {+1, -1, 0} (0: the row is not
    part of the problem), ``cw [P, 2]`` the weights of the -1 / +1 class, ``n_bins [d]`` the columns' bin counts
    (checked against ``bins`` when given). The model lives where ``bins`` lives."""
    bins = _as_bins(bins)
    n = int(bins.shape[0])
    if hasattr(label, 'data_ptr'):
        import torch
        label = label.to(torch.int8).contiguous()
    else:
        label = np.ascontiguousarray(label, np.int8)
    if label.ndim != 2 or int(label.shape[1]) != n:
        raise ValueError(f'label: [P, {n}] expected, got {tuple(label.shape)}')
    P = int(label.shape[0])
    cw = np.ascontiguousarray(cw, np.float64)
    if cw.shape != (P, 2):
        raise ValueError(f'cw: [{P}, 2] expected, got {cw.shape}')
    if n_bins is not None:
        n_bins = np.ascontiguousarray(n_bins, np.int32)
        if n_bins.shape != (int(d),):
            raise ValueError(f'n_bins: [{int(d)}] expected, got {n_bins.shape}')
    if not 1 <= P <= SVM_MAX_PROBLEMS or not 1 <= int(trees) <= FOREST_MAX_TREES:
        raise ValueError(f'forest_fit: P = {P} (1 .. {SVM_MAX_PROBLEMS}), trees = {trees} (1 .. {FOREST_MAX_TREES})')
    model = ForestModel(P, trees, max_depth, bins.device if hasattr(bins, 'data_ptr') and bins.is_cuda else None)
    params = AslForestParams(int(trees), int(max_depth), int(seed) & 0xffffffff)
    ms = model.struct()
    check(lib().asl_forest_fit(ptr(bins) if n else None, n, int(d), ptr(label) if n else None, ptr(cw), P,
                               ptr(n_bins), byref(params), byref(ms)))
    return model


def forest_predict(bins, d: int, model: ForestModel, max_depth=None):
    """``asl_forest_predict``: ``proba [P, n]`` float64 where ``bins`` lives -- the mean over the trees of the
    value of the node where a row stops after at most ``max_depth`` levels (default: the depth grown)."""
    bins = _as_bins(bins)
    n = int(bins.shape[0])
    depth = model.max_depth if max_depth is None else int(max_depth)
    if hasattr(bins, 'data_ptr'):
        import torch
        out = torch.empty((model.P, n), dtype=torch.float64, device=bins.device)
    else:
        out = np.empty((model.P, n), np.float64)
    ms = model.struct()
    check(lib().asl_forest_predict(ptr(bins) if n else None, n, int(d), byref(ms), model.P, depth,
                                   ptr(out) if n else None))
    return out


def set_forest_workspace(nbytes: int) -> int:
    """``asl_set_forest_workspace``: the device bytes one batch of (problem, tree) pairs may take while
    ``forest_fit`` grows a level; returns the previous value. The result does not depend on it."""
    prev = lib().asl_set_forest_workspace(int(nbytes))
    if prev <= 0:
        check(int(prev))
    return int(prev)


TDC_TILE = 1024           # ASL_TDC_TILE


def _as_column(a, like, np_dtype, n: int, what: str):
    """``a`` as a contiguous ``[n]`` column of ``np_dtype`` (bool columns as 0 / 1 bytes) of the kind ``like``
    is: a torch tensor on ``like``'s device, or numpy."""
    if hasattr(like, 'data_ptr'):
        import torch
        dt = getattr(torch, np.dtype(np_dtype).name)
        a = torch.as_tensor(a, device=like.device) if not hasattr(a, 'data_ptr') else a.to(like.device)
        a = (a != 0).to(dt) if np_dtype is np.uint8 else a.to(dt)
        a = a.contiguous()
    else:
        if hasattr(a, 'cpu'):
            a = a.cpu().numpy()
        a = np.asarray(a)
        a = np.ascontiguousarray(a != 0, np.uint8) if np_dtype is np.uint8 else np.ascontiguousarray(a, np_dtype)
    if a.ndim != 1 or int(a.shape[0]) != n:
        raise ValueError(f'{what}: [{n}] expected, got {tuple(a.shape)}')
    return a


def tdc_qvalues(score, is_target, group=None, use=None, desc: bool = True, fdr=None):
    """``asl_tdc_qvalues``: q-values by target-decoy competition (``fdr.tdc_qvalues``) inside every group
    (``fdr._grouped_q``) over the rows where ``use`` is non-zero (default: all). ``score [n]`` float64 (numpy or
    torch, host or device), ``is_target [n]`` and ``use [n]`` bool or 0 / non-0, ``group [n]`` int32 ids
    (default: one group), ``desc``: a higher score is better. Returns ``q [n]`` (NaN for unused rows), or with
    ``fdr`` given ``(q, label)``: label int8, +1 used target with q <= fdr, 0 other used target and every
    unused row, -1 used decoy. The outputs live where ``score`` lives (numpy, or torch on its device)."""
    score = _as_f64(score, 1, 'score')
    n = int(score.shape[0])
    is_target = _as_column(is_target, score, np.uint8, n, 'is_target')
    group = None if group is None else _as_column(group, score, np.int32, n, 'group')
    use = None if use is None else _as_column(use, score, np.uint8, n, 'use')
    if hasattr(score, 'data_ptr'):
        import torch
        q = torch.empty(n, dtype=torch.float64, device=score.device)
        label = None if fdr is None else torch.empty(n, dtype=torch.int8, device=score.device)
    else:
        q = np.empty(n, np.float64)
        label = None if fdr is None else np.empty(n, np.int8)
    check(lib().asl_tdc_qvalues(ptr(score) if n else None, ptr(is_target) if n else None,
                                ptr(group) if n else None, ptr(use) if n else None, n, 1 if desc else 0,
                                0.0 if fdr is None else float(fdr), ptr(q) if n else None,
                                ptr(label) if n and label is not None else None))
    return q if fdr is None else (q, label)


GROUPS_MAX_SPAN = 65536   # ASL_GROUPS_MAX_SPAN
ERR_INVALID, ERR_CAPACITY = -1, -4      # ASL_ERR_INVALID, ASL_ERR_CAPACITY
MGF_TILE = 256            # ASL_MGF_TILE
MGF_MAX_PEAKS = 4096      # ASL_MGF_MAX_PEAKS
MGF_MAX_LINE = 65536      # ASL_MGF_MAX_LINE


def mgf_number(token):
    """``asl_mgf_number``: the numeral ``token`` (bytes or str) as the device converts it -- ``(0, value)``, or
    ``(1, None)`` where the device defers the token to the host's ``float()``. Host only: needs no GPU."""
    b = token.encode('utf-8') if isinstance(token, str) else bytes(token)
    out = C.c_double(0.0)
    rc = lib().asl_mgf_number(b, len(b), byref(out))
    return (0, out.value) if rc == 0 else (1, None)


def sptxt_fragment_charge(annotation) -> int:
    """``asl_sptxt_fragment_charge``: the fragment charge the device reads from the annotation field of a .sptxt
    peak line (bytes or str); 0 = unannotated. Host only: needs no GPU."""
    b = annotation.encode('utf-8') if isinstance(annotation, str) else bytes(annotation)
    return int(lib().asl_sptxt_fragment_charge(b, len(b)))


MZML_MAX_TAG = 4096       # ASL_MZML_MAX_TAG
MZML_SMALL_PEAKS = 512    # ASL_MZML_SMALL_PEAKS
MZML_INF_TEXT = {1: 'a byte that is not base64', 2: 'base64 of a length that is no multiple of 4',
                 3: 'base64 padding inside the text', 4: 'a compressed stream longer than the array allows',
                 5: 'a bad zlib header', 6: 'an invalid DEFLATE block type', 7: 'invalid stored block lengths',
                 8: 'an invalid set of code lengths', 9: 'an invalid code', 10: 'a distance too far back',
                 11: 'a truncated zlib stream', 12: 'more values than defaultArrayLength',
                 13: 'a wrong Adler-32', 14: 'fewer values than defaultArrayLength'}      # ASL_MZML_INF_*


def mzml_inflate(b64, use_zlib: bool, cap: int):
    """``asl_mzml_inflate``: the characters ``b64`` of one ``<binary>`` as the device decodes them -- base64, then
    zlib where ``use_zlib`` -- into at most ``cap`` bytes: ``(0, bytes)`` or ``(code, None)``, ``code`` a key of
    ``MZML_INF_TEXT``. Host only: needs no GPU."""
    b = b64.encode('ascii') if isinstance(b64, str) else bytes(b64)
    out = C.create_string_buffer(max(int(cap), 1))
    n_out = C.c_int64(0)
    rc = lib().asl_mzml_inflate(b, len(b), int(bool(use_zlib)), out, int(cap), byref(n_out))
    if rc < 0:
        raise ValueError('asl_mzml_inflate: an invalid argument')
    return (0, out.raw[:n_out.value]) if rc == 0 else (rc, None)


def ssm_groups(mass_diff, min_group_size: int, profile: bool = False):
    """``asl_ssm_groups``: the open level's mass-difference group labels (``fdr.ssm_groups``, the same bytes) from
    ``mass_diff [n]`` float64 (numpy or torch, host or device). Returns ``(group [n] int32, n_labels)`` --
    ``n_labels`` the number of distinct values in ``group``, -1 included when present -- or with ``profile``
    ``(group, n_labels, peak_mass [n_peaks] float64, peak_size [n_peaks] int64)``: per id handed out BEFORE ids of
    fewer than ``min_group_size`` SSMs were folded into -1, the left bin edge of its histogram peak and the SSMs
    assigned to it. The arrays live where ``mass_diff`` lives. A non-finite value or a negative
    ``min_group_size`` is ``AnnSoloMiError`` with ``code == ERR_INVALID``; nominal mass differences that span more
    than ``GROUPS_MAX_SPAN`` intervals ``code == ERR_CAPACITY``."""
    md = _as_f64(mass_diff, 1, 'mass_diff')
    n = int(md.shape[0])
    if hasattr(md, 'data_ptr'):
        import torch

        def empty(dtype):
            return torch.empty(n, dtype=getattr(torch, dtype), device=md.device)
    else:
        def empty(dtype):
            return np.empty(n, dtype)
    group = empty('int32')
    mass, size = (empty('float64'), empty('int64')) if profile else (None, None)
    n_peaks, n_labels = C.c_int64(0), C.c_int64(0)
    check(lib().asl_ssm_groups(ptr(md) if n else None, n, int(min_group_size), ptr(group) if n else None,
                               byref(n_peaks), byref(n_labels), ptr(mass) if n and profile else None,
                               ptr(size) if n and profile else None))
    if not profile:
        return group, int(n_labels.value)
    return group, int(n_labels.value), mass[:n_peaks.value], size[:n_peaks.value]


def mzxml_duration(value):
    """``asl_mzxml_duration``: the value of a ``retentionTime`` attribute (bytes or str) as the device converts it --
    ``(0, minutes)``, or ``(1, None)`` where the device defers the value to ``mzxml.duration_minutes``. Host only:
    needs no GPU."""
    b = value.encode('utf-8') if isinstance(value, str) else bytes(value)
    out = C.c_double(0.0)
    rc = lib().asl_mzxml_duration(b, len(b), byref(out))
    return (0, out.value) if rc == 0 else (1, None)


def mzxml_pairs(raw, n_peaks: int, precision: int):
    """``asl_mzxml_pairs``: the decoded ``<peaks>`` stream ``raw`` (big-endian m/z, intensity pairs of ``precision``
    bits) as the device converts it: ``(mz, intensity)``, float32 numpy arrays. Host only: needs no GPU."""
    b = bytes(raw)
    if precision not in (32, 64) or len(b) != n_peaks * 2 * (precision // 8):
        raise ValueError(f'asl_mzxml_pairs: {len(b)} bytes for {n_peaks} peaks of {precision} bits')
    mz, it = np.empty(n_peaks, np.float32), np.empty(n_peaks, np.float32)
    if lib().asl_mzxml_pairs(b, n_peaks, precision, mz.ctypes.data, it.ctypes.data) != 0:
        raise ValueError('asl_mzxml_pairs: an invalid argument')
    return mz, it
