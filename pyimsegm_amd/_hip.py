"""Thin ctypes binding of ``libimsegm_hip.so`` (C ABI declared in ``include/imsegm_hip.h``).

The library holds every compute kernel of the package (hand-written HIP for gfx950).  There is no
CPU fallback: if the shared library or a GPU is missing, the calls raise ``HipUnavailableError``.
The HIP runtime is initialised lazily, per process, on the first call that needs the device, so
importing the package before ``multiprocessing`` forks workers (the reference's only parallelism,
``imsegm/utilities/experiments.py:392-403``) is safe.
"""
import ctypes as C
import functools
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('IMSEGM_HIP_LIBRARY') or os.path.join(_HERE, 'libimsegm_hip.so')

U8, F64, F32 = 0, 1, 2
PROFILE_GROUPS = {
    'slic_assign': 0,
    'slic': 1,
    'connectivity': 2,
    'color_stats': 3,
    'graph': 4,
    'graphcut': 5,
    'gather': 6,
    'slic_preprocess': 7,
    'terms': 8,
    'texture': 9,
}


class HipUnavailableError(RuntimeError):
    """the HIP library or a HIP device is not available (no CPU fallback exists)"""


class HipError(RuntimeError):
    """a C-ABI call returned an error status"""


class HipFusedPathError(HipError):
    """``IMSEGM_E_FUSED_PATH`` of include/imsegm_hip.h: the fused back half (``imsegm_image2d_segment`` /
    ``imsegm_image2d_graph_prepare``) does not apply to this label map on this device -- nothing is wrong with the session, the
    caller takes the staged calls (graph, terms, ``cut_general_graph``, gather) instead"""


class HipFitCapsError(HipError):
    """``IMSEGM_E_FIT_CAPS`` of include/imsegm_hip.h: the table or the model is outside the caps of the device fit
    (``imsegm_kmeans_lloyd`` / ``imsegm_mixture_em``: 16 features, 8 components, 16 restarts; the ``_wide`` pair: 17 to 256
    features, 8 components, 16 restarts) -- nothing is wrong with the context, the caller fits on the host"""


class HipForestInputError(HipError):
    """``IMSEGM_E_FOREST_INPUT`` of include/imsegm_hip.h: the forest entry points refuse this table (a value that is not finite in
    float32) or this forest (more than 16 classes, 256 features or 1 024 trees, a node index out of range) -- nothing was
    written, nothing is wrong with the context, the caller evaluates the model on the host"""


class HipClusterInputError(HipError, ValueError):
    """``IMSEGM_E_CLUSTER_INPUT`` of include/imsegm_hip.h: ``imsegm_dbscan_points`` refuses what scikit-learn's DBSCAN answers with a
    ``ValueError`` (a coordinate that is not finite, ``eps`` that is not positive and finite, ``min_samples`` below 1) -- nothing
    was written, nothing is wrong with the context"""


IMSEGM_E_FUSED_PATH = -3
IMSEGM_E_FIT_CAPS = -4
IMSEGM_E_OBJECT_CAPS = -5
IMSEGM_E_FOREST_INPUT = -6
IMSEGM_E_CLUSTER_INPUT = -7


_lib = None
_lib_lock = threading.Lock()

_vp = C.c_void_p
_ip = C.POINTER(C.c_int)

class GmmParams(C.Structure):
    """``imsegm_gmm`` of include/imsegm_hip.h"""
    _fields_ = [('n_features', C.c_int), ('n_classes', C.c_int), ('scaler_mean', _vp), ('scaler_scale', _vp),
                ('prec_chol', _vp), ('mu_proj', _vp), ('log_det', _vp), ('log_weights', _vp), ('const_term', C.c_double),
                ('n_inputs', C.c_int), ('pca_components_t', _vp), ('pca_shift', _vp), ('pca_scale', _vp)]


class ForestParams(C.Structure):
    """``imsegm_forest`` of include/imsegm_hip.h"""
    _fields_ = [('n_features', C.c_int), ('n_classes', C.c_int), ('n_trees', C.c_int), ('n_nodes', C.c_int), ('n_leaves', C.c_int),
                ('scaler_mean', _vp), ('scaler_scale', _vp), ('nodes', _vp), ('tree_start', _vp), ('leaf_values', _vp)]


class TermsDebug(C.Structure):
    """``imsegm_terms_debug`` of include/imsegm_hip.h"""
    _fields_ = [('edge_capacity', C.c_int), ('n_edges', C.c_int), ('edges', _vp), ('edge_weights', _vp),
                ('edge_weights_int', _vp), ('unary', _vp), ('unary_int', _vp), ('centres', _vp), ('energy', _vp),
                ('keep_soft_on_device', C.c_int), ('segm_u8', C.c_int), ('soft_f32', C.c_int)]


#: colour spaces of ``imsegm_image2d_convert_color`` (0: back to the uploaded image)
COLOR_SPACES = {'hsv': 1, 'luv': 2, 'lab': 3, 'hed': 4, 'xyz': 5}

#: edge types of ``imsegm_image2d_segment``; 0x100 = divide by the relative centre distance (graph_cuts.py:647-650)
EDGE_TYPES = {'': 0, 'const': 0, 'spatial': 1 | 0x100, 'model': 2 | 0x100, 'model_lT': 2, 'model_l1': 3, 'model_l2': 4,
              'features': 5 | 0x100}

_SIGNATURES = {
    'imsegm_last_error': (C.c_char_p, []),
    'imsegm_host_alloc': (C.c_int, [C.c_size_t, C.POINTER(_vp)]),
    'imsegm_host_free': (None, [_vp]),
    'imsegm_device_alloc': (C.c_int, [C.c_int, C.c_size_t, C.POINTER(_vp)]),
    'imsegm_device_free': (None, [_vp]),
    'imsegm_set_device': (C.c_int, [C.c_int]),
    'imsegm_ctx_stream': (C.c_int, [_vp, C.POINTER(_vp)]),
    'imsegm_ctx_copy': (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_int]),
    'imsegm_image2d_features_color': (C.c_int, [_vp, C.c_int, _vp]),
    'imsegm_image2d_features_place': (C.c_int, [_vp, C.c_int, C.c_int]),
    'imsegm_image2d_get_features': (C.c_int, [_vp, _vp, C.c_int]),
    'imsegm_image2d_run_color': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_double, _vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.POINTER(GmmParams), C.c_int, _vp, C.c_int, C.c_double, C.c_int, _vp, _vp, _vp, _ip]),
    'imsegm_device_mem_info': (C.c_int, [C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    'imsegm_image2d_graph_prepare': (C.c_int, [_vp]),
    'imsegm_image2d_segment': (C.c_int, [_vp, C.POINTER(GmmParams), _vp, C.c_int, _vp, C.c_int, C.c_double, C.c_int, _vp, _vp, _vp,
                                         _vp, _vp, C.POINTER(TermsDebug)]),
    'imsegm_version': (C.c_int, []),
    'imsegm_device_count': (C.c_int, [_ip]),
    'imsegm_ctx_create': (C.c_int, [C.c_int, C.POINTER(_vp)]),
    'imsegm_ctx_destroy': (None, [_vp]),
    'imsegm_ctx_synchronize': (C.c_int, [_vp]),
    'imsegm_ctx_profile_enable': (C.c_int, [_vp, C.c_int]),
    'imsegm_ctx_profile_reset': (C.c_int, [_vp]),
    'imsegm_ctx_profile_get': (C.c_int, [_vp, C.c_int, C.POINTER(C.c_double), _ip]),
    'imsegm_image2d_create': (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    'imsegm_image2d_destroy': (None, [_vp]),
    'imsegm_image2d_upload': (C.c_int, [_vp, _vp, C.c_int]),
    'imsegm_image2d_slic': (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int,
                                      C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, _ip]),
    'imsegm_image2d_get_labels': (C.c_int, [_vp, _vp]),
    'imsegm_image2d_set_labels': (C.c_int, [_vp, _vp, C.c_int]),
    'imsegm_image2d_enforce_connectivity': (C.c_int, [_vp, _vp, C.c_long, C.c_long, C.c_int, _vp]),
    'imsegm_debug_conn_general_runs': (C.c_long, []),
    'imsegm_debug_conn_last': (C.c_int, [_vp]),
    'imsegm_debug_slic_sweep_runs': (C.c_int, [_vp, _vp]),
    'imsegm_debug_gc_grid_fallbacks': (C.c_long, []),
    'imsegm_debug_exclusive_scan': (C.c_int, [_vp, C.c_int, _vp, _ip]),
    'imsegm_debug_poison_context': (C.c_int, [_vp, C.c_uint32, C.POINTER(C.c_size_t)]),
    'imsegm_debug_image2d_poison': (C.c_int, [_vp, C.c_uint32, C.POINTER(C.c_size_t)]),
    'imsegm_assume_bg_on_boundary': (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, _ip]),
    'imsegm_image2d_all_finite': (C.c_int, [_vp, _ip]),
    'imsegm_image2d_lm_features': (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_double, C.c_int, _vp]),
    'imsegm_batch2d_create': (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    'imsegm_batch2d_destroy': (None, [_vp]),
    'imsegm_batch2d_run_color': (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_double, _vp, C.c_int, C.c_int, C.c_int,
                                           C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_double, C.c_int, _vp, _vp, _vp]),
    'imsegm_batch2d_device_ptr': (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    'imsegm_device_pci_bus_id': (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    'imsegm_init': (C.c_int, [C.c_int]),
    'imsegm_debug_reload_env': (None, []),
    'imsegm_image2d_label_hist': (C.c_int, [_vp, _vp, C.c_int, _vp]),
    'imsegm_image2d_get_lab': (C.c_int, [_vp, _vp]),
    'imsegm_image2d_get_nearest': (C.c_int, [_vp, _vp]),
    'imsegm_image2d_get_pre_scalars': (C.c_int, [_vp, _vp]),
    'imsegm_image2d_get_centroids': (C.c_int, [_vp, _vp, _vp, _ip]),
    'imsegm_image2d_color_stats': (C.c_int, [_vp, _vp, _vp, _vp]),
    'imsegm_image2d_graph': (C.c_int, [_vp, _vp, C.c_int, _ip, _vp, _vp]),
    'imsegm_image2d_gather': (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp]),
    'imsegm_image2d_lm_prepare': (C.c_int, [_vp, _vp, C.c_int, _vp]),
    'imsegm_image2d_lm_features_sep': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_double, C.c_int, _vp]),
    'imsegm_image2d_lm_battery': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double)]),
    'imsegm_image2d_response_stats': (C.c_int, [_vp, C.c_double, C.c_double, _vp, _vp, _vp]),
    'imsegm_image2d_response_median': (C.c_int, [_vp, C.c_double, C.c_double, _vp]),
    'imsegm_image2d_response_mean_gradient': (C.c_int, [_vp, C.c_double, C.c_double, _vp]),
    'imsegm_image2d_get_response': (C.c_int, [_vp, _vp]),
    'imsegm_image2d_device_ptr': (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    'imsegm_volume_create': (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    'imsegm_volume_upload': (C.c_int, [_vp, _vp, C.c_int, C.c_double, C.c_double]),
    'imsegm_volume_slic': (C.c_int, [_vp, C.c_int, C.c_double, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int,
                                     C.c_int, C.c_double, C.c_double, C.c_int, _ip]),
    'imsegm_volume_get_pre': (C.c_int, [_vp, _vp, _ip, C.POINTER(C.c_double)]),
    'imsegm_volume_get_centroids': (C.c_int, [_vp, _vp, _ip, _ip]),
    'imsegm_volume_label_cc': (C.c_int, [_vp, _ip]),
    'imsegm_volume_gray_stats': (C.c_int, [_vp, _vp, _vp, _vp]),
    'imsegm_volume_graph': (C.c_int, [_vp, _vp, C.c_int, _ip, _vp, _vp]),
    'imsegm_image2d_median': (C.c_int, [_vp, _vp]),
    'imsegm_image2d_mean_gradient': (C.c_int, [_vp, _vp]),
    'imsegm_image2d_convert_color': (C.c_int, [_vp, C.c_int, _vp]),
    'imsegm_image2d_get_converted': (C.c_int, [_vp, _vp]),
    'imsegm_label_hist2d': (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp]),
    'imsegm_ray_features_binary2d': (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp]),
    'imsegm_ring_hist2d': (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp]),
    'imsegm_ring_hist_proba2d': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, _vp]),
    'imsegm_ray_features_labels2d': (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int,
                                               _vp]),
    'imsegm_cut_general_graph': (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp,
                                           C.POINTER(C.c_int64)]),
    'imsegm_cut_general_graph_scaled': (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, C.c_double, C.c_int, _vp,
                                                  C.POINTER(C.c_int64)]),
    'imsegm_debug_grid_arcs': (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    'imsegm_cut_grid_graph': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.POINTER(C.c_int64)]),
    'imsegm_object_cut_pixels': (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_int, C.c_double,
                                           C.c_double, C.c_int, C.c_int, _vp, C.POINTER(C.c_int64), _vp, C.POINTER(C.c_double)]),
    'imsegm_kmeans_lloyd': (C.c_int, [_vp, _vp, C.c_long, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_double, _vp, _vp, _vp, _vp, _vp]),
    'imsegm_mixture_em': (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _vp]),
    'imsegm_bayes_mixture_em': (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, C.c_double, C.c_double, _vp, C.c_double, _vp,
                                          C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'imsegm_kmeans_lloyd_wide': (C.c_int, [_vp, _vp, C.c_long, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_double, _vp, _vp, _vp, _vp,
                                           _vp]),
    'imsegm_mixture_em_wide': (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp,
                                         _vp, _vp, _vp, _vp]),
    'imsegm_boundary_mask': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    'imsegm_distance_map': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    'imsegm_boundary_distances': (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_int, _ip]),
    'imsegm_image2d_boundary_distances': (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _ip]),
    'imsegm_boundary_mask3d': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp]),
    'imsegm_distance_map3d': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp]),
    'imsegm_boundary_distances3d': (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _ip]),
    'imsegm_volume_boundary_distances': (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _ip]),
    'imsegm_labels_overlap': (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_int, C.c_int, _vp]),
    'imsegm_ellipse_ransac': (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double, _vp, _vp, _vp, _vp,
                                        _vp]),
    'imsegm_ellipse_place': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_double, _vp]),
    'imsegm_ellipse_overlaps': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, _vp]),
    'imsegm_split_background_foreground': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    'imsegm_boundary_rays': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, _vp]),
    'imsegm_rg_open': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    'imsegm_rg_close': (None, [_vp]),
    'imsegm_rg_get': (C.c_int, [_vp, C.c_int, _vp]),
    'imsegm_rg_set_costs': (C.c_int, [_vp, _vp, _vp]),
    'imsegm_rg_shape_costs': (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    'imsegm_rg_object_shapes': (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _vp]),
    'imsegm_rg_greedy_step': (C.c_int, [_vp, _vp, C.c_int, _vp, _ip, _vp, _vp, _vp]),
    'imsegm_rg_criterion': (C.c_int, [_vp, _vp, _vp, _vp]),
    'imsegm_object_shapes': (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _ip, _vp, _vp, _vp, _vp]),
    'imsegm_annot_match': (C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp, C.c_int, C.c_int, _vp, C.POINTER(C.c_int64)]),
    'imsegm_annot_paint': (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, _vp, _vp, _vp]),
    'imsegm_cut_objects': (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp,
                                     _vp, _vp, _ip]),
    'imsegm_correct_segm': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _ip]),
    'imsegm_center_levels': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _vp]),
    'imsegm_debug_center_distances': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    'imsegm_create_annot_centers': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _ip, _vp, _vp]),
    'imsegm_watershed_markers': (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, _vp]),
    'imsegm_watershed_post_morph': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    'imsegm_watershed': (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp]),
    'imsegm_stack_median_u8': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    'imsegm_orient_stack': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    'imsegm_resize_crops': (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    'imsegm_ellipse_cut_scale': (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp,
                                           _vp, _vp, _ip]),
    'imsegm_annot_color_hist': (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, _ip, _vp, _vp]),
    'imsegm_annot_nearest_valid': (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp]),
    'imsegm_annot_quantize_nearest_pixel': (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp]),
    'imsegm_score_pairs': (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp]),
    'imsegm_forest_proba': (C.c_int, [_vp, C.POINTER(ForestParams), _vp, C.c_int, C.c_int, _vp]),
    'imsegm_image2d_forest_proba': (C.c_int, [_vp, C.POINTER(ForestParams), _vp]),
    'imsegm_dbscan_points': (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_double, C.c_int, _vp, _vp, _vp]),
}

#: every symbol ``include/imsegm_hip.h`` declares
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def load_library():
    """load ``libimsegm_hip.so`` and declare the signatures (no device is touched)"""
    global _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise HipUnavailableError(
                    'libimsegm_hip.so is not built (%s); run `python -m pyimsegm_amd.build`' % LIB_PATH)
            try:
                lib = C.CDLL(LIB_PATH)
            except OSError as ex:
                raise HipUnavailableError('cannot load %s: %s' % (LIB_PATH, ex))
            for name, (res, args) in _SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def init(hardware_queues=8):
    """Explicit, optional, once per process before the first device call (``imsegm_init``): the number of hardware queues the HIP
    runtime maps this process's streams onto (its ``GPU_MAX_HW_QUEUES``, default 4).  With one stream per image in flight plus
    the default stream, a fourth image shares a queue with another one and its kernels wait behind that image's: eight queues
    gave 6.5-6.9 instead of 5.6-5.8 Gpx/s on the 2048^2 line with four images in flight (round 3).
    Returns True when the request was recorded; False when the runtime is already up or the user has set the variable (his
    value wins).  Loading the library never touches the environment."""
    status = load_library().imsegm_init(int(hardware_queues))
    if status < 0:
        raise HipError(load_library().imsegm_last_error().decode('utf-8', 'replace'))
    if status == 0:
        # (the C library's setenv does not show in os.environ, which Python copied at start-up: keep the two in step for
        # child processes started with os.environ and for anyone who looks)
        os.environ.setdefault('GPU_MAX_HW_QUEUES', str(int(hardware_queues)))
    return status == 0


def device_pci_bus_id(device=0):
    """PCI address of a HIP device, e.g. ``'0000:c1:00.0'``"""
    buf = C.create_string_buffer(64)
    _check(load_library().imsegm_device_pci_bus_id(int(device), buf, 64))
    return buf.value.decode('ascii', 'replace').lower()


def mem_info(device=0):
    """(free, total) bytes of a device's memory right now"""
    free_b, total_b = C.c_size_t(0), C.c_size_t(0)
    _check(load_library().imsegm_device_mem_info(int(device), C.byref(free_b), C.byref(total_b)))
    return int(free_b.value), int(total_b.value)


def reload_env():
    """read the IMSEGM_* debug switches again (the library reads them once): tests flip them at run time"""
    load_library().imsegm_debug_reload_env()


def _check(status):
    if status != 0:
        message = load_library().imsegm_last_error().decode('utf-8', 'replace')
        raise {IMSEGM_E_FUSED_PATH: HipFusedPathError, IMSEGM_E_FIT_CAPS: HipFitCapsError,
               IMSEGM_E_FOREST_INPUT: HipForestInputError, IMSEGM_E_CLUSTER_INPUT: HipClusterInputError}.get(status, HipError)(message)


_device_count = {}


def device_count():
    """number of visible HIP devices (cached per process: forked children ask again)"""
    pid = os.getpid()
    if pid not in _device_count:
        n = C.c_int(0)
        load_library().imsegm_device_count(C.byref(n))
        _device_count[pid] = n.value
    return _device_count[pid]


def resolve_place(on, variable, raise_without_device):
    """Where a call with the keyword ``on=None | 'host' | 'device'`` runs: ``(place, explicit)``.  ``on=None`` reads the environment
    variable ``variable`` (unset or empty: nothing asked); any other value raises ValueError.  With nothing asked the place is
    'device' when a device is present and 'host' otherwise, and ``explicit`` is False: the caller may still have a default of its
    own.  'device' asked for without a device raises HipUnavailableError here when ``raise_without_device``; otherwise 'device' is
    handed back without a look at the devices, and the call fails where it needs one."""
    if on is None:
        on = os.environ.get(variable) or None
    if on not in (None, 'host', 'device'):
        raise ValueError("on is 'host' or 'device', not %r" % (on, ))
    if on == 'host' or (on == 'device' and not raise_without_device):
        return on, True
    try:
        present = device_count() > 0
    except HipUnavailableError:
        present = False
    if not present and on == 'device':
        raise HipUnavailableError('no HIP device is visible')
    return ('device' if present else 'host'), on is not None


def _ptr(arr):
    return None if arr is None else arr.ctypes.data_as(_vp)


class Context(object):
    """one HIP device + one stream"""

    #: sessions alive on this context (a context with sessions is never released behind their back)
    users = 0

    def __init__(self, device=0):
        #: idle sessions kept for reuse, by image shape (superpixels._open_session / _release_session)
        self.idle_sessions = {}
        lib = load_library()
        if device_count() < 1:
            raise HipUnavailableError('no HIP device is visible: the imsegm HIP path cannot run (no CPU fallback)')
        self._h = _vp()
        self.device = device
        self.pid = os.getpid()
        _check(lib.imsegm_ctx_create(device, C.byref(self._h)))

    def synchronize(self):
        _check(load_library().imsegm_ctx_synchronize(self._h))

    @property
    def stream(self):
        """the HIP stream of this context as an integer handle (for RCCL calls on the same stream)"""
        p = _vp()
        _check(load_library().imsegm_ctx_stream(self._h, C.byref(p)))
        return p.value

    def copy(self, dst_ptr, src_ptr, nbytes, synchronize=True):
        """``hipMemcpyAsync`` (any direction) on this context's stream"""
        _check(load_library().imsegm_ctx_copy(self._h, _vp(dst_ptr), _vp(src_ptr), int(nbytes), int(bool(synchronize))))

    def profile_enable(self, enable=True):
        _check(load_library().imsegm_ctx_profile_enable(self._h, int(enable)))

    def profile_reset(self):
        _check(load_library().imsegm_ctx_profile_reset(self._h))

    def profile_get(self, group):
        ms, n = C.c_double(0), C.c_int(0)
        _check(load_library().imsegm_ctx_profile_get(self._h, PROFILE_GROUPS[group], C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def poison(self, word):
        """diagnostic (``imsegm_debug_poison_context``): fill the context's device scratch with the 32-bit ``word`` over its whole
        capacity and forget the resident table of a mixture fit -- a new context whose buffers hold ``word``; returns the bytes filled"""
        nbytes = C.c_size_t(0)
        _check(load_library().imsegm_debug_poison_context(self._h, int(word) & 0xffffffff, C.byref(nbytes)))
        return int(nbytes.value)

    def close_idle_sessions(self):
        """give the device memory of the sessions kept for reuse back (a volume session owns ~70 bytes per voxel)"""
        for sess in list(self.idle_sessions.values()):
            sess.close()
        self.idle_sessions.clear()

    def close(self):
        self.close_idle_sessions()
        if self._h and self.pid == os.getpid():
            load_library().imsegm_ctx_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}
_default_ctx_lock = threading.RLock()


def _reap_contexts_locked(pid):
    alive = {t.ident for t in threading.enumerate()}
    dead = [k for k in _default_ctx if k[0] == pid and k[1] not in alive
            and _default_ctx[k].users == len(_default_ctx[k].idle_sessions)]
    for old in dead:
        _default_ctx.pop(old).close()
    return len(dead)


def reap_contexts():
    """close the contexts of this process's threads that have ended, with the sessions they kept for reuse (a gray-volume session
    holds ~75 bytes of device memory per voxel): done whenever a new thread asks for its context, and here on request -- after a
    pool of worker threads has gone and before the calling thread needs the memory itself.  Returns the number closed."""
    with _default_ctx_lock:
        return _reap_contexts_locked(os.getpid())


def default_context():
    """per-process, per-thread, per-device lazily created context (re-created in forked children).

    A context owns one HIP stream and its pinned staging buffers, so worker threads that keep several
    images in flight on one GPU (``pipelines.NB_WORKERS``) each get their own."""
    key = (os.getpid(), threading.get_ident(), os.environ.get('IMSEGM_HIP_DEVICE', os.environ.get('LOCAL_RANK', '0')))
    # the whole lookup runs under the lock: thread identifiers are recycled, and a new thread must not pick up the
    # context of a dead thread with the same identifier while another new thread is giving that context back
    with _default_ctx_lock:
        ctx = _default_ctx.get(key)
        if ctx is None:
            # a new thread asks for its context: first give back those of threads that have ended (and the
            # sessions they kept for reuse)
            _reap_contexts_locked(key[0])
            device = int(key[2])
            n = device_count()
            if n > 0:
                device %= n
            ctx = Context(device)
            _default_ctx[key] = ctx
    return ctx


class _PinnedBlock(object):
    """a page-locked host allocation; goes back to the free list of its size class when the last numpy view dies"""
    __slots__ = ('ptr', 'size', 'pid', '__weakref__')

    def __init__(self, ptr, size):
        self.ptr, self.size, self.pid = ptr, size, os.getpid()

    def __del__(self):
        try:
            if self.pid != os.getpid():
                return
            with _pinned_lock:
                cache = _pinned_free.setdefault(self.size, [])
                if len(cache) < (_PINNED_KEEP if self.size < _PINNED_BIG else _PINNED_KEEP_BIG):
                    cache.append(self.ptr)
                    return
            load_library().imsegm_host_free(self.ptr)
        except Exception:
            pass


_pinned_free = {}
_pinned_lock = threading.RLock()
_PINNED_KEEP = 16      # blocks kept per size class for reuse (hipHostMalloc costs far more than the copy it speeds up)
_PINNED_BIG, _PINNED_KEEP_BIG = 256 << 20, 3      # ... of 256 MB and more (the 4.3 GB class map of a 64 x 4096 x 4096 volume): three


def pinned_empty(shape, dtype):
    """``numpy.empty(shape, dtype)`` in page-locked host memory: uploads from / downloads into such an array run as
    asynchronous DMA (``Image2D.upload``, ``Image2D.segment``).  The memory returns to a small per-size free list when
    the array (and every view of it) is garbage collected."""
    dtype = np.dtype(dtype)
    shape = tuple(int(v) for v in np.atleast_1d(shape))
    nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    size = max(4096, (nbytes + 4095) & ~4095)
    ptr = None
    with _pinned_lock:
        cache = _pinned_free.get(size)
        if cache:
            ptr = cache.pop()
    if ptr is None:
        if device_count() < 1:
            raise HipUnavailableError('no HIP device is visible: page-locked memory is not available')
        p = _vp()
        _check(load_library().imsegm_host_alloc(size, C.byref(p)))
        ptr = p.value
    block = _PinnedBlock(ptr, size)
    buf = (C.c_char * size).from_address(ptr)
    buf._block = block                                    # the ctypes buffer (base of the array) keeps the block alive
    return np.frombuffer(buf, dtype=dtype, count=nbytes // dtype.itemsize).reshape(shape)


def kmeans_lloyd(table, seeds, max_iter=300, tol=0., want_labels=True, ctx=None):
    """``imsegm_kmeans_lloyd``: Lloyd iterations of all restarts at once from the centres ``seeds`` (R x C x F) on ``table``
    (n x F float64), which stays on the device of ``ctx`` for :func:`mixture_em`.  ``tol`` is absolute (scikit-learn's
    ``tol * mean(var(table, axis=0))``).  Returns a dict: labels (R x n int32, or None when not wanted -- they stay on the device
    either way), centres, inertia, n_iter, empty (R flags: a cluster lost all its rows, the restart stopped there).
    Raises :class:`HipFitCapsError` outside F <= 16, C <= 8, R <= 16."""
    return _kmeans_lloyd('imsegm_kmeans_lloyd', table, seeds, max_iter, tol, want_labels, ctx)


def _kmeans_lloyd(entry, table, seeds, max_iter, tol, want_labels, ctx):
    """the narrow or the wide Lloyd entry point of the library"""
    ctx = ctx or default_context()
    table = np.ascontiguousarray(table, dtype=np.float64)
    seeds = np.ascontiguousarray(seeds, dtype=np.float64)
    if table.ndim != 2 or seeds.ndim != 3 or seeds.shape[2] != table.shape[1]:
        raise ValueError('table is n x F, seeds are R x C x F')
    n_restarts, n_clusters, _ = seeds.shape
    labels = np.empty((n_restarts, len(table)), dtype=np.int32) if want_labels else None
    centres, inertia = np.empty_like(seeds), np.empty(n_restarts)
    n_iter, empty = np.zeros(n_restarts, dtype=np.int32), np.zeros(n_restarts, dtype=np.int32)
    _check(getattr(load_library(), entry)(ctx._h, _ptr(table), len(table), table.shape[1], _ptr(seeds), n_restarts, n_clusters,
                                           int(max_iter), float(tol), _ptr(labels), _ptr(centres), _ptr(inertia), _ptr(n_iter),
                                           _ptr(empty)))
    return dict(labels=labels, centres=centres, inertia=inertia, n_iter=n_iter, empty=empty.astype(bool))


def kmeans_lloyd_wide(table, seeds, max_iter=300, tol=0., want_labels=True, ctx=None):
    """``imsegm_kmeans_lloyd_wide``: :func:`kmeans_lloyd` for tables of 17 to 256 features (csrc/mixture_fit_wide.hip); the table
    stays on the device of ``ctx`` for :func:`mixture_em_wide`.  Same arguments, same dict.
    Raises :class:`HipFitCapsError` outside 17 <= F <= 256, C <= 8, R <= 16 -- also for F <= 16, which :func:`kmeans_lloyd` fits."""
    return _kmeans_lloyd('imsegm_kmeans_lloyd_wide', table, seeds, max_iter, tol, want_labels, ctx)


def mixture_em(n_restarts, n_components, n_features, labels=None, start=None, reg_covar=1e-6, tol=1e-3, max_iter=100, ctx=None):
    """``imsegm_mixture_em``: EM for full covariances, all restarts at once, on the table the last :func:`kmeans_lloyd` of ``ctx``
    uploaded.  Start: ``start`` = (weights R x C, means R x C x F, precisions_cholesky R x C x F x F), or one-hot responsibilities
    from ``labels`` (R x n int32), or -- both None -- from the labels that call left on the device.  Returns a dict: weights,
    means, covariances, precisions_cholesky, lower_bound, n_iter, converged, not_pd (R flags: a covariance was not positive
    definite, the restart stopped there)."""
    return _mixture_em('imsegm_mixture_em', 16, n_restarts, n_components, n_features, labels, start, reg_covar, tol, max_iter, ctx)


def _mixture_em(entry, max_features, n_restarts, n_components, n_features, labels, start, reg_covar, tol, max_iter, ctx):
    """the narrow or the wide EM entry point of the library"""
    ctx = ctx or default_context()
    R, K, F = int(n_restarts), int(n_components), int(n_features)
    if labels is not None:
        labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(R, -1)
    w0 = m0 = p0 = None
    if start is not None:
        w0, m0, p0 = (np.ascontiguousarray(v, dtype=np.float64) for v in start)
        if w0.shape != (R, K) or m0.shape != (R, K, F) or p0.shape != (R, K, F, F):
            raise ValueError('start parameters are (R x C, R x C x F, R x C x F x F)')
    safe = (min(R, 16), min(K, 8), min(F, max_features))          # (beyond the caps the call writes nothing)
    weights, means = np.zeros(safe[:2]), np.zeros(safe)
    cov, prec = np.zeros(safe + (safe[2], )), np.zeros(safe + (safe[2], ))
    bound = np.zeros(safe[0])
    n_iter, converged, not_pd = (np.zeros(safe[0], dtype=np.int32) for _ in range(3))
    _check(getattr(load_library(), entry)(ctx._h, R, K, _ptr(labels), _ptr(w0), _ptr(m0), _ptr(p0), float(reg_covar), float(tol),
                                           int(max_iter), _ptr(weights), _ptr(means), _ptr(cov), _ptr(prec), _ptr(bound), _ptr(n_iter),
                                           _ptr(converged), _ptr(not_pd)))
    return dict(weights=weights, means=means, covariances=cov, precisions_cholesky=prec, lower_bound=bound, n_iter=n_iter,
                converged=converged.astype(bool), not_pd=not_pd.astype(bool))


#: ``weight_concentration_prior_type`` of scikit-learn's BayesianGaussianMixture -> ``prior_type`` of ``imsegm_bayes_mixture_em``
BAYES_PRIOR_TYPES = {'dirichlet_process': 0, 'dirichlet_distribution': 1}


def bayes_mixture_em(n_restarts, n_components, n_features, prior_type, weight_concentration_prior, mean_precision_prior, mean_prior,
                     degrees_of_freedom_prior, covariance_prior, labels=None, reg_covar=1e-6, tol=1e-3, max_iter=100, ctx=None):
    """``imsegm_bayes_mixture_em``: the variational fit of ``BayesianGaussianMixture(covariance_type='full')``, all restarts at
    once, on the table the last :func:`kmeans_lloyd` of ``ctx`` uploaded.  Start: one-hot responsibilities from ``labels`` (R x n
    int32) or -- None -- from the labels that call left on the device.  ``prior_type`` is scikit-learn's name (a key of
    ``BAYES_PRIOR_TYPES``); the priors are the estimator's checked ones (``weight_concentration_prior_`` ...).  Returns a dict:
    weight_concentration (R x 2 x C: rows a, b of the process; row 0 of the distribution), mean_precision, means,
    degrees_of_freedom, covariances, precisions_cholesky, lower_bound, n_iter, converged, not_pd (R flags: a covariance was not
    positive definite, the restart stopped there).  Raises :class:`HipFitCapsError` outside F <= 16, C <= 8, R <= 16."""
    ctx = ctx or default_context()
    R, K, F = int(n_restarts), int(n_components), int(n_features)
    if labels is not None:
        labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(R, -1)
    mean_prior = np.ascontiguousarray(mean_prior, dtype=np.float64)
    covariance_prior = np.ascontiguousarray(covariance_prior, dtype=np.float64)
    if mean_prior.shape != (F, ) or covariance_prior.shape != (F, F):
        raise ValueError('the mean prior is F, the covariance prior F x F')
    safe = (min(R, 16), min(K, 8), min(F, 16))          # (beyond the caps the call writes nothing)
    concentration, precision, dof = np.zeros((safe[0], 2, safe[1])), np.zeros(safe[:2]), np.zeros(safe[:2])
    means, cov, prec = np.zeros(safe), np.zeros(safe + (safe[2], )), np.zeros(safe + (safe[2], ))
    bound = np.zeros(safe[0])
    n_iter, converged, not_pd = (np.zeros(safe[0], dtype=np.int32) for _ in range(3))
    _check(load_library().imsegm_bayes_mixture_em(
        ctx._h, R, K, _ptr(labels), BAYES_PRIOR_TYPES[prior_type], float(weight_concentration_prior), float(mean_precision_prior),
        _ptr(mean_prior), float(degrees_of_freedom_prior), _ptr(covariance_prior), float(reg_covar), float(tol), int(max_iter),
        _ptr(concentration), _ptr(precision), _ptr(means), _ptr(dof), _ptr(cov), _ptr(prec), _ptr(bound), _ptr(n_iter),
        _ptr(converged), _ptr(not_pd)))
    return dict(weight_concentration=concentration, mean_precision=precision, means=means, degrees_of_freedom=dof, covariances=cov,
                precisions_cholesky=prec, lower_bound=bound, n_iter=n_iter, converged=converged.astype(bool),
                not_pd=not_pd.astype(bool))


def mixture_em_wide(n_restarts, n_components, n_features, labels=None, start=None, reg_covar=1e-6, tol=1e-3, max_iter=100, ctx=None):
    """``imsegm_mixture_em_wide``: :func:`mixture_em` on the table the last :func:`kmeans_lloyd_wide` of ``ctx`` uploaded (17 to
    256 features).  Same arguments, same dict; of ``start``'s precision factors the upper triangle is read.  When a covariance
    is not positive definite the restart keeps the parameters, the covariances and the lower bound of its last completed
    iteration (nothing of the failed one is written)."""
    return _mixture_em('imsegm_mixture_em_wide', 256, n_restarts, n_components, n_features, labels, start, reg_covar, tol, max_iter, ctx)


class DeviceGmm(object):
    """the constants of a fitted ``Pipeline([StandardScaler,] [PCA,] mixture)`` -- the mixture a ``GaussianMixture`` or a
    ``BayesianGaussianMixture`` with ``covariance_type='full'`` -- that the device needs for ``predict_proba``: what scikit-learn
    computes once per model (``means_ @ precisions_cholesky_``, the log-determinants, ``log(weights_)``), formed with the very
    numpy expressions of ``sklearn/mixture/_gaussian_mixture.py`` (``_estimate_log_gaussian_prob``, ``_compute_log_det_cholesky``).

    PCA (``sklearn/decomposition/_base.py`` ``_BasePCA._transform``): ``components_.T`` (``pca_components_t``), the centring
    term ``mean_ @ components_.T`` (``pca_shift``) and, with ``whiten``, the clipped ``sqrt(explained_variance_)``
    (``pca_scale``).  ``n_inputs`` is the width of the table the model reads, ``n_features`` the dimension of the mixture.

    Bayesian mixture (``sklearn/mixture/_bayesian_mixture.py`` ``_estimate_log_prob`` / ``_estimate_log_weights``): per
    component it adds ``-0.5 F log(nu) + 0.5 (F log 2 + sum_i digamma(0.5 (nu - i)) - F / kappa)`` to the log-density -- kept
    as ``bayes_log_prob_const`` and folded into ``log_det`` -- and takes the digamma form of the log-weights."""

    def __init__(self, model):
        from sklearn.decomposition import PCA
        from sklearn.mixture import BayesianGaussianMixture, GaussianMixture
        from sklearn.pipeline import Pipeline
        from sklearn.preprocessing import StandardScaler
        steps = [st for _, st in model.steps] if isinstance(model, Pipeline) else [model]
        gmm = steps[-1]
        if type(gmm) not in (GaussianMixture, BayesianGaussianMixture) or gmm.covariance_type != 'full' \
                or not hasattr(gmm, 'precisions_cholesky_'):
            raise TypeError('not a fitted full-covariance GaussianMixture / BayesianGaussianMixture')
        front = steps[:-1]
        scaler = front.pop(0) if front and type(front[0]) is StandardScaler else None
        pca = front.pop(0) if front and type(front[0]) is PCA else None
        if front:
            raise TypeError('only an optional StandardScaler and an optional PCA, in that order, in front of the mixture are '
                            'evaluated on the device')
        n_comp, n_feat = gmm.means_.shape
        n_in = int(pca.components_.shape[1]) if pca is not None else int(n_feat)
        if pca is not None and pca.components_.shape[0] != n_feat:
            raise TypeError('the PCA does not produce the columns the mixture was fitted on')
        if n_in > 256 or n_comp > 16:
            raise TypeError('device class model: at most 256 features and 16 classes')
        self.n_features, self.n_classes, self.n_inputs = int(n_feat), int(n_comp), n_in
        self.classes = getattr(model, 'classes_', None)
        par = GmmParams()
        par.n_features, par.n_classes = self.n_features, self.n_classes
        par.n_inputs = n_in if pca is not None else 0
        self.scaler_mean = self.scaler_scale = None
        if scaler is not None:
            if scaler.with_mean:
                self.scaler_mean = np.ascontiguousarray(scaler.mean_, dtype=np.float64)
            if scaler.with_std:
                self.scaler_scale = np.ascontiguousarray(scaler.scale_, dtype=np.float64)
        self.pca_components_t = self.pca_shift = self.pca_scale = None
        if pca is not None:
            components = np.asarray(pca.components_, dtype=np.float64)
            self.pca_components_t = np.ascontiguousarray(components.T)
            mean = np.zeros(n_in) if pca.mean_ is None else np.asarray(pca.mean_, dtype=np.float64)
            self.pca_shift = np.ascontiguousarray((np.reshape(mean, (1, -1)) @ components.T)[0])
            if pca.whiten:
                scale = np.sqrt(np.asarray(pca.explained_variance_, dtype=np.float64))
                min_scale = np.finfo(scale.dtype).eps
                scale[scale < min_scale] = min_scale
                self.pca_scale = np.ascontiguousarray(scale)
        chol = np.ascontiguousarray(gmm.precisions_cholesky_, dtype=np.float64)
        self.prec_chol = chol
        self.mu_proj = np.ascontiguousarray([np.dot(mu, pc) for mu, pc in zip(gmm.means_, chol)], dtype=np.float64)
        log_det = np.sum(np.log(chol.reshape(n_comp, -1)[:, ::n_feat + 1]), 1)
        self.bayes_log_prob_const = None
        if type(gmm) is BayesianGaussianMixture:
            from scipy.special import digamma
            log_lambda = n_feat * np.log(2.0) + np.sum(
                digamma(0.5 * (gmm.degrees_of_freedom_ - np.arange(0, n_feat)[:, np.newaxis])), 0)
            self.bayes_log_prob_const = -0.5 * n_feat * np.log(gmm.degrees_of_freedom_) \
                + 0.5 * (log_lambda - n_feat / gmm.mean_precision_)
            log_det = log_det + self.bayes_log_prob_const
            log_weights = gmm._estimate_log_weights()
        else:
            log_weights = np.log(gmm.weights_)
        self.log_det = np.ascontiguousarray(log_det, dtype=np.float64)
        self.log_weights = np.ascontiguousarray(log_weights, dtype=np.float64)
        self.const_term = float(n_feat * np.log(2 * np.pi))
        for name in ('scaler_mean', 'scaler_scale', 'prec_chol', 'mu_proj', 'log_det', 'log_weights', 'pca_components_t',
                     'pca_shift', 'pca_scale'):
            setattr(par, name, _ptr(getattr(self, name)))
        par.const_term = self.const_term
        self.params = par


#: a node of a packed tree (``imsegm_forest_node``): the float32 threshold rounded DOWN from scikit-learn's float64 one, and a word
#: -- not negative: ``feature | right child << 8`` (the left child is the next node), negative: a leaf, ``~word`` its row of the
#: leaf table
FOREST_NODE = np.dtype([('threshold', '<f4'), ('word', '<i4')])
FOREST_MAX_CLASSES, FOREST_MAX_FEATURES, FOREST_MAX_TREES, FOREST_MAX_TREE_NODES = 16, 256, 1024, 1 << 23
#: rows a workgroup of the walk takes at a time, and the largest tree it stages in LDS (the tests take their sizes from here)
FOREST_ROWS, FOREST_LDS_NODES = 256, 4096


def forest_threshold(threshold64):
    """the largest float32 that is <= each float64 threshold: ``float32(x) <= threshold64`` is ``float32(x) <= forest_threshold(...)``"""
    threshold64 = np.asarray(threshold64, dtype=np.float64)
    with np.errstate(over='ignore'):
        rounded = threshold64.astype(np.float32)
    above = rounded.astype(np.float64) > threshold64
    rounded[above] = np.nextafter(rounded[above], np.float32(-np.inf))
    return rounded


def _forest_steps(model):
    """(scaler or None, classifier) of a model the forest entry points take, or the reason why they do not, as a string"""
    from sklearn.ensemble import ExtraTreesClassifier, RandomForestClassifier
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import StandardScaler
    from sklearn.tree import DecisionTreeClassifier
    steps = [st for _, st in model.steps] if isinstance(model, Pipeline) else [model]
    clf = steps[-1]
    front = steps[:-1]
    scaler = front.pop(0) if front and type(front[0]) is StandardScaler else None
    if front:
        return 'only an optional StandardScaler in front of the classifier is evaluated on the device'
    if type(clf) not in (RandomForestClassifier, ExtraTreesClassifier, DecisionTreeClassifier):
        return '%s is not a random forest, extra trees or a decision tree' % type(clf).__name__
    if not hasattr(clf, 'tree_' if type(clf) is DecisionTreeClassifier else 'estimators_'):
        return 'the classifier is not fitted'
    if clf.n_outputs_ != 1:
        return 'the classifier has more than one output'
    trees = [clf] if type(clf) is DecisionTreeClassifier else list(clf.estimators_)
    if not 1 <= len(trees) <= FOREST_MAX_TREES:
        return 'the device takes 1 .. %d trees' % FOREST_MAX_TREES
    if len(clf.classes_) > FOREST_MAX_CLASSES or clf.n_features_in_ > FOREST_MAX_FEATURES:
        return 'the device takes at most %d classes and %d features' % (FOREST_MAX_CLASSES, FOREST_MAX_FEATURES)
    if max(tree.tree_.node_count for tree in trees) > FOREST_MAX_TREE_NODES:
        return 'a tree has more than 2^23 nodes'
    return scaler, clf


def _leaf_rows(tree, rows):
    """what ``DecisionTreeClassifier.predict_proba`` of the installed scikit-learn returns in the leaves ``rows`` of ``tree``: the
    stored class fractions as they are (1.3 and later); before that the stored class weights divided by their sum"""
    import sklearn
    values = np.array(tree.tree_.value[rows, 0, :tree.n_classes_], dtype=np.float64)
    if tuple(int(part) for part in sklearn.__version__.split('.')[:2]) < (1, 3):
        normalizer = values.sum(axis=1)[:, np.newaxis]
        normalizer[normalizer == 0.0] = 1.0
        values /= normalizer
    return values


class DeviceForest(object):
    """the arrays of a fitted ``Pipeline([StandardScaler,] clf)`` -- ``clf`` a ``RandomForestClassifier``, ``ExtraTreesClassifier``
    or ``DecisionTreeClassifier`` with one output -- that the device needs for ``predict_proba`` (``imsegm_forest`` of
    include/imsegm_hip.h), all plain numpy: ``nodes`` (:data:`FOREST_NODE`, tree after tree, every tree in preorder so that the
    left child is the next node), ``tree_start`` (int32, T + 1), ``leaf_values`` (float64, leaves x C, what the tree's own
    ``predict_proba`` returns there), ``scaler_mean`` / ``scaler_scale`` or None, and ``threshold64``, scikit-learn's thresholds in
    the order of ``nodes`` (for the tests of the rounding).  ``DeviceForest(model)`` is None for a model the device does not take
    (:func:`forest_refusal` says why); :meth:`from_arrays` builds one by hand."""

    def __new__(cls, model=None):
        self = object.__new__(cls)
        if model is None:
            return self
        parts = _forest_steps(model)
        if isinstance(parts, str):
            return None
        self._pack(*parts)
        return self

    def __init__(self, model=None):
        pass

    @classmethod
    def from_arrays(cls, nodes, tree_start, leaf_values, n_features, scaler_mean=None, scaler_scale=None, classes=None):
        self = cls()
        self.nodes = np.ascontiguousarray(nodes, dtype=FOREST_NODE)
        self.tree_start = np.ascontiguousarray(tree_start, dtype=np.int32)
        self.leaf_values = np.ascontiguousarray(leaf_values, dtype=np.float64)
        if self.nodes.ndim != 1 or self.tree_start.ndim != 1 or len(self.tree_start) < 2 or self.leaf_values.ndim != 2:
            raise ValueError('nodes [N], tree_start [T + 1] and leaf_values [L, C] are expected')
        self.n_features, self.n_classes, self.n_trees = int(n_features), int(self.leaf_values.shape[1]), len(self.tree_start) - 1
        self.scaler_mean = None if scaler_mean is None else np.ascontiguousarray(scaler_mean, dtype=np.float64)
        self.scaler_scale = None if scaler_scale is None else np.ascontiguousarray(scaler_scale, dtype=np.float64)
        for vector in (self.scaler_mean, self.scaler_scale):
            if vector is not None and vector.shape != (self.n_features, ):
                raise ValueError('a scaler vector holds one value per feature')
        self.classes = None if classes is None else np.asarray(classes)
        self.threshold64 = self.nodes['threshold'].astype(np.float64)
        return self

    def _pack(self, scaler, clf):
        trees = [clf] if hasattr(clf, 'tree_') else list(clf.estimators_)
        nodes, thresholds, values, starts, n_leaves = [], [], [], [0], 0
        for tree in trees:
            inner = tree.tree_
            left, right, feature = inner.children_left.tolist(), inner.children_right.tolist(), inner.feature
            # preorder: a node, its left subtree, its right subtree (scikit-learn's depth-first builder lays its trees out so; its
            # best-first builder, max_leaf_nodes, does not)
            order, stack = [], [0]
            while stack:
                node = stack.pop()
                order.append(node)
                if left[node] >= 0:
                    stack.append(right[node])
                    stack.append(left[node])
            order = np.array(order, dtype=np.int64)
            place = np.empty(len(order), dtype=np.int64)
            place[order] = np.arange(len(order))
            is_leaf = inner.children_left[order] < 0
            packed = np.zeros(len(order), dtype=FOREST_NODE)
            threshold64 = np.where(is_leaf, 0.0, inner.threshold[order])
            packed['threshold'] = forest_threshold(threshold64)
            word = feature[order].astype(np.int64) | (place[inner.children_right[order]] << 8)
            word[is_leaf] = ~(n_leaves + np.arange(int(is_leaf.sum()), dtype=np.int64))
            packed['word'] = word.astype(np.int32)
            nodes.append(packed)
            thresholds.append(threshold64)
            values.append(_leaf_rows(tree, order[is_leaf]))
            n_leaves += int(is_leaf.sum())
            starts.append(starts[-1] + len(order))
        self.nodes = np.concatenate(nodes)
        self.threshold64 = np.concatenate(thresholds)
        self.tree_start = np.array(starts, dtype=np.int32)
        self.leaf_values = np.ascontiguousarray(np.concatenate(values, axis=0))
        self.n_features, self.n_classes, self.n_trees = int(clf.n_features_in_), len(clf.classes_), len(trees)
        self.scaler_mean = self.scaler_scale = None
        if scaler is not None:
            if scaler.with_mean:
                self.scaler_mean = np.ascontiguousarray(scaler.mean_, dtype=np.float64)
            if scaler.with_std:
                self.scaler_scale = np.ascontiguousarray(scaler.scale_, dtype=np.float64)
        self.classes = np.asarray(clf.classes_)

    def params(self):
        """the ``imsegm_forest`` of the arrays as they are now (it points into them: keep the forest alive over the call)"""
        par = ForestParams()
        par.n_features, par.n_classes, par.n_trees = self.n_features, self.n_classes, self.n_trees
        par.n_nodes, par.n_leaves = len(self.nodes), len(self.leaf_values)
        for name in ('scaler_mean', 'scaler_scale', 'nodes', 'tree_start', 'leaf_values'):
            setattr(par, name, _ptr(getattr(self, name)))
        return par


def forest_refusal(model):
    """why ``DeviceForest(model)`` is None, or None when it is not"""
    parts = _forest_steps(model)
    return parts if isinstance(parts, str) else None


def forest_proba(forest, table, out=None, ctx=None):
    """``imsegm_forest_proba``: the probabilities (n x C float64) of a :class:`DeviceForest` on a host table (n x F float64).
    Raises :class:`HipForestInputError`, with ``out`` untouched, for a table or a forest the device refuses."""
    ctx = ctx or default_context()
    table = np.ascontiguousarray(table, dtype=np.float64)
    if table.ndim != 2:
        raise ValueError('the table is n x F')
    if out is None:
        out = np.empty((len(table), forest.n_classes), dtype=np.float64)
    elif out.shape != (len(table), forest.n_classes) or out.dtype != np.float64 or not out.flags.c_contiguous:
        raise ValueError('out must be a C-contiguous float64 array of n x C')
    _check(load_library().imsegm_forest_proba(ctx._h, C.byref(forest.params()), _ptr(table), len(table), table.shape[1], _ptr(out)))
    return out


@functools.lru_cache(maxsize=64)
def gaussian_taps(sigma, truncate=4.0):
    """half of the kernel of ``scipy.ndimage.gaussian_filter1d(sigma)`` (taps[0] = centre), computed
    with the very numpy expressions of ``scipy.ndimage._filters._gaussian_kernel1d``; None: no blur
    (cached: the result must be treated as read-only)"""
    sigma = float(sigma)
    if not sigma > 0:
        return None
    radius = int(truncate * sigma + 0.5)
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x**2)
    phi_x = phi_x / phi_x.sum()
    return np.ascontiguousarray(phi_x[::-1][radius:], dtype=np.float64)


_DTYPES = {np.dtype(np.uint8): U8, np.dtype(np.float64): F64, np.dtype(np.float32): F32}


class Image2D(object):
    """device-resident pipeline state of one H x W colour image"""

    def __init__(self, height, width, ctx=None):
        self.ctx = ctx or default_context()
        self.shape = (int(height), int(width))
        self._h = _vp()
        self.n_labels = 0
        _check(load_library().imsegm_image2d_create(self.ctx._h, self.shape[0], self.shape[1], C.byref(self._h)))
        self.ctx.users += 1

    def close(self):
        if self._h and self.ctx is not None:
            self.ctx.users -= 1
            if self.ctx._h and self.ctx.pid == os.getpid():
                load_library().imsegm_image2d_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, image):
        """H x W x 3 image; uint8 / float32 / float64 go up as they are, anything else as float64"""
        image = np.asarray(image)
        if image.ndim != 3 or image.shape[2] != 3 or image.shape[:2] != self.shape:
            raise ValueError('expected an image of shape %r + (3,), got %r' % (self.shape, image.shape))
        if image.dtype not in _DTYPES:
            image = image.astype(np.float64)
        image = np.ascontiguousarray(image)
        _check(load_library().imsegm_image2d_upload(self._h, _ptr(image), _DTYPES[image.dtype]))
        self._uploaded = image          # a page-locked source is read asynchronously: keep it alive until the next sync
        return self

    def poison(self, word):
        """diagnostic (``imsegm_debug_image2d_poison``): fill every device buffer of the session with the 32-bit ``word`` over its
        whole capacity and forget the image, the label map and everything derived from them -- a new session whose buffers hold
        ``word``; returns the bytes filled"""
        nbytes = C.c_size_t(0)
        _check(load_library().imsegm_debug_image2d_poison(self._h, int(word) & 0xffffffff, C.byref(nbytes)))
        self.n_labels = 0
        self._uploaded = None
        return int(nbytes.value)

    def run_color(self, image, n_segments, compactness, gmm, pairwise, edge_type='model', feature_flags=(True, True, True),
                  sigma=1., normalize=2, max_iter=10, start_label=0, slic_zero=False, edge_cost=1., use_graphcut=True,
                  classes=None, want_soft=False, pinned=True):
        """upload + SLIC + colour features + class model + graph cut + gathers of one uint8 / float64 colour image in
        one C call (``imsegm_image2d_run_color``); returns (segm int32 H x W, soft or None)"""
        image = np.ascontiguousarray(image)
        if image.shape != self.shape + (3, ) or image.dtype not in _DTYPES:
            raise ValueError('expected an image of shape %r + (3,) and dtype uint8 / float32 / float64' % (self.shape, ))
        code = EDGE_TYPES.get(edge_type)
        if code is None:
            raise ValueError('edge type %r is not evaluated on the device' % (edge_type, ))
        pairwise = np.ascontiguousarray(pairwise, dtype=np.float64)
        nc = gmm.n_classes
        if pairwise.shape != (nc, nc):
            raise ValueError('pairwise cost must be %d x %d' % (nc, nc))
        cl = None if classes is None else np.ascontiguousarray(classes, dtype=np.int32)
        taps = gaussian_taps(sigma)
        r = -1 if taps is None else len(taps) - 1
        alloc = pinned_empty if pinned else np.empty
        segm = alloc(self.shape, np.int32)
        soft = alloc(self.shape + (nc, ), np.float64) if want_soft else None
        mask = (1 if feature_flags[0] else 0) | (2 if feature_flags[1] else 0) | (4 if feature_flags[2] else 0)
        n_out = C.c_int(0)
        _check(load_library().imsegm_image2d_run_color(
            self._h, _ptr(image), _DTYPES[image.dtype], int(normalize), int(n_segments), float(compactness), _ptr(taps), r,
            int(max_iter), int(start_label), int(bool(slic_zero)), mask, C.byref(gmm.params), nc, _ptr(pairwise), code,
            float(edge_cost), int(bool(use_graphcut)), _ptr(cl), _ptr(segm), _ptr(soft), C.byref(n_out)))
        self.n_labels = n_out.value
        self._uploaded = image
        return segm, soft

    def median(self):
        """per-label median of the uploaded image / volume on the current labels: K x 3 (K for a volume)"""
        out = np.empty((self.n_labels, 3) if len(self.shape) == 2 else (self.n_labels, ), dtype=np.float64)
        _check(load_library().imsegm_image2d_median(self._h, _ptr(out)))
        return out

    def mean_gradient(self):
        """per-label mean of ``np.sum(np.gradient(slice), axis=0)`` (stored in the image's dtype): K x 3 (K for a volume)"""
        out = np.empty((self.n_labels, 3) if len(self.shape) == 2 else (self.n_labels, ), dtype=np.float64)
        _check(load_library().imsegm_image2d_mean_gradient(self._h, _ptr(out)))
        return out

    def convert_color(self, space, matrix=None):
        """convert the uploaded RGB image to a colour space on the device (``imsegm_image2d_convert_color``; no synchronisation)
        and make the result what :meth:`color_stats`, :meth:`features_color`, :meth:`median` and :meth:`mean_gradient` read,
        until ``convert_color(0)`` or the next upload.  ``space``: a name of :data:`COLOR_SPACES` or its code; ``matrix``: the
        3 x 3 stain matrix of 'hed' (``data_io._HED_FROM_RGB``)"""
        code = COLOR_SPACES[space] if isinstance(space, str) else int(space)
        mat = None if matrix is None else np.ascontiguousarray(matrix, dtype=np.float64)
        if mat is not None and mat.shape != (3, 3):
            raise ValueError('the stain matrix must be 3 x 3')
        _check(load_library().imsegm_image2d_convert_color(self._h, code, _ptr(mat)))
        return self

    def converted(self):
        """the image of the last :meth:`convert_color` on the host: H x W x 3 float64"""
        out = np.empty(tuple(self.shape[-2:]) + (3, ), dtype=np.float64)
        _check(load_library().imsegm_image2d_get_converted(self._h, _ptr(out)))
        return out

    def features_color(self, mean=True, std=True, energy=True, to_host=True):
        """resident feature table (columns mean | std | energy, 3 each) of the uploaded image on the current labels;
        returns it as K x F float64 when ``to_host``"""
        mask = (1 if mean else 0) | (2 if std else 0) | (4 if energy else 0)
        nflags = bool(mean) + bool(std) + bool(energy)
        out = np.empty((self.n_labels, 3 * nflags), dtype=np.float64) if to_host else None
        _check(load_library().imsegm_image2d_features_color(self._h, mask, _ptr(out)))
        return out

    def forest_proba(self, forest, to_host=False):
        """``imsegm_image2d_forest_proba``: the probabilities of a :class:`DeviceForest` on the resident feature table, left on the
        device for the next :meth:`segment` with neither ``gmm`` nor ``proba``.  Without ``to_host`` nothing waits and None is
        returned (a table the forest refuses then shows as :class:`HipForestInputError` of that ``segment``); with it, K x C float64."""
        out = np.empty((self.n_labels, forest.n_classes), dtype=np.float64) if to_host else None
        _check(load_library().imsegm_image2d_forest_proba(self._h, C.byref(forest.params()), _ptr(out)))
        return out

    def graph_prepare(self):
        """enqueue the graph of the resident label map (neighbour pairs, centres, edges, arcs) ahead of :meth:`segment`, without
        a synchronisation (``imsegm_image2d_graph_prepare``): it depends on the label map alone, so it can run while the host fits
        the class model.  Raises :class:`HipFusedPathError` when the fused back half does not apply."""
        _check(load_library().imsegm_image2d_graph_prepare(self._h))

    def segment(self, pairwise, edge_type='model', edge_cost=1., gmm=None, proba=None, use_graphcut=True, classes=None,
                want_segm=True, want_soft=False, want_graph_labels=False, want_proba=False, debug=False, pinned=True,
                keep_soft_on_device=False, segm_dtype=None, soft_dtype=None, segm_out=None):
        """fused back half of the pipeline on the resident label map (``imsegm_image2d_segment``): class probabilities
        (``gmm``: :class:`DeviceGmm` on the resident features, else ``proba`` K x C from the host), unary / edge terms,
        alpha-expansion, ``classes[graph_labels][slic]`` and ``proba[slic]``; one synchronisation.

        ``segm_out``: the caller's own C-contiguous array for the class map (shape and dtype of 'segm'), e.g. one whose pages have been
        touched while the device worked -- a download into untouched pageable memory runs at half the rate of the link.

        :return dict: 'segm' (H x W int32), 'soft' (H x W x C), 'graph_labels' (K), 'proba' (K x C) as requested, plus
            with ``debug`` the graph-cut terms ('edges', 'edge_weights', 'edge_weights_int', 'unary', 'unary_int',
            'centres', 'energy').  With ``debug`` the whole call runs a second time when the label map has more edges than
            the debug arrays were sized for (3 K + 64, volumes 16 K + 64: a map that is no planar partition), with arrays of
            the size the first run reported; without ``debug`` it is always one call"""
        code = EDGE_TYPES.get(edge_type)
        if code is None:
            raise ValueError('edge type %r is not evaluated on the device' % (edge_type, ))
        pairwise = np.ascontiguousarray(pairwise, dtype=np.float64)
        nc = pairwise.shape[0]
        if pairwise.shape != (nc, nc):
            raise ValueError('pairwise cost must be square')
        k = self.n_labels
        pr = None
        if gmm is None and proba is None:
            pass            # (the probabilities :meth:`forest_proba` left on this label map and table, or the library's error)
        elif gmm is None:
            pr = np.ascontiguousarray(proba, dtype=np.float64)
            if pr.ndim != 2 or pr.shape[0] < k or pr.shape[1] != nc:
                raise ValueError('proba %r does not fit %d superpixels x %d classes' % (pr.shape, k, nc))
            pr = np.ascontiguousarray(pr[:k])
        elif gmm.n_classes != nc:
            raise ValueError('class model has %d classes, pairwise cost %d' % (gmm.n_classes, nc))
        cl = None if classes is None else np.ascontiguousarray(classes, dtype=np.int32)
        if cl is not None and cl.shape != (nc, ):
            raise ValueError('classes must hold one value per class')
        alloc = pinned_empty if pinned else np.empty
        out = {}
        # narrow result formats (explicit opt-in, not the reference's dtypes): uint8 class map, float32 soft segmentation
        segm_u8 = segm_dtype is not None and np.dtype(segm_dtype) == np.uint8
        soft_f32 = soft_dtype is not None and np.dtype(soft_dtype) == np.float32
        if segm_dtype is not None and not segm_u8 and np.dtype(segm_dtype) != np.int32:
            raise ValueError('the class map leaves the device as int32 (the reference) or uint8')
        if soft_dtype is not None and not soft_f32 and np.dtype(soft_dtype) != np.float64:
            raise ValueError('the soft segmentation leaves the device as float64 (the reference) or float32')
        if segm_u8 and (nc > 256 or (cl is not None and (cl.min() < 0 or cl.max() > 255))):
            raise ValueError('uint8 class map: class values must lie in 0..255')
        if want_segm:
            want_dtype = np.dtype(np.uint8 if segm_u8 else np.int32)
            if segm_out is not None:
                if not isinstance(segm_out, np.ndarray) or segm_out.shape != tuple(self.shape) or segm_out.dtype != want_dtype \
                        or not segm_out.flags.c_contiguous or not segm_out.flags.writeable:
                    raise ValueError('segm_out must be a writeable C-contiguous %s array of shape %r' % (want_dtype, tuple(self.shape)))
                out['segm'] = segm_out
            else:
                out['segm'] = alloc(self.shape, want_dtype)
        if want_soft:
            out['soft'] = alloc(self.shape + (nc, ), np.float32 if soft_f32 else np.float64)
        if want_graph_labels or debug:
            out['graph_labels'] = np.empty(k, dtype=np.int32)
        if want_proba or debug:
            out['proba'] = np.empty((k, nc), dtype=np.float64)
        dbg = None
        if debug or keep_soft_on_device or segm_u8 or soft_f32:
            dbg = TermsDebug()
            dbg.keep_soft_on_device = int(bool(keep_soft_on_device))
            dbg.segm_u8, dbg.soft_f32 = int(segm_u8), int(soft_f32)
        if debug:
            ndim = len(self.shape)
            out.update(unary=np.empty((k, nc)), unary_int=np.empty((k, nc), np.int32), centres=np.empty((k, ndim)),
                       energy=np.zeros(1, np.int64))
            for name in ('unary', 'unary_int', 'centres', 'energy'):
                setattr(dbg, name, _ptr(out[name]))
        cap = (16 if len(self.shape) == 3 else 3) * k + 64
        while True:
            if debug:
                out.update(edges=np.empty((cap, 2), np.int32), edge_weights=np.empty(cap), edge_weights_int=np.empty(cap, np.int32))
                dbg.edge_capacity = cap
                for name in ('edges', 'edge_weights', 'edge_weights_int'):
                    setattr(dbg, name, _ptr(out[name]))
            _check(load_library().imsegm_image2d_segment(
                self._h, C.byref(gmm.params) if gmm is not None else None, _ptr(pr), nc, _ptr(pairwise), code, float(edge_cost),
                int(bool(use_graphcut)), _ptr(cl), _ptr(out.get('segm')), _ptr(out.get('soft')), _ptr(out.get('graph_labels')),
                _ptr(out.get('proba')), C.byref(dbg) if dbg is not None else None))
            # (a label map that is no planar partition has more edges than the debug arrays were sized for: once more, as graph())
            if not debug or dbg.n_edges <= cap:
                break
            cap = dbg.n_edges
        if debug:
            ne = dbg.n_edges
            for name in ('edges', 'edge_weights', 'edge_weights_int'):
                out[name] = out[name][:ne]
            out['energy'] = int(out['energy'][0])
        return out

    def slic(self, n_segments, compactness, sigma=1., normalize=2, max_iter=10, enforce_connectivity=True,
             min_size_factor=0.5, max_size_factor=3., start_label=0, max_candidates=0, slic_zero=False):
        taps = gaussian_taps(sigma)
        r = -1 if taps is None else len(taps) - 1
        n_out = C.c_int(0)
        _check(load_library().imsegm_image2d_slic(
            self._h, int(normalize), int(n_segments), float(compactness), _ptr(taps), r, _ptr(taps), r, _ptr(taps), r,
            int(max_iter), int(bool(enforce_connectivity)), float(min_size_factor), float(max_size_factor),
            int(start_label), int(max_candidates), int(bool(slic_zero)), C.byref(n_out)))
        self.n_labels = n_out.value
        return self.n_labels

    def get_labels(self):
        out = np.empty(self.shape, dtype=np.int64)
        _check(load_library().imsegm_image2d_get_labels(self._h, _ptr(out)))
        return out

    def get_labels_int32(self):
        """the resident label map as it lives in HBM (int32), without the int64 widening of :meth:`get_labels`"""
        out = np.empty(self.shape, dtype=np.int32)
        src = _device_array(self, 0, self.shape, '<i4').__cuda_array_interface__['data'][0]
        self.ctx.copy(out.ctypes.data, src, out.nbytes, synchronize=True)
        return out

    def enforce_connectivity(self, labels, min_size, max_size, start_label=0):
        """``_enforce_label_connectivity_cython`` of scikit-image 0.18 on a given label map; returns the int64 map"""
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if labels.shape != self.shape:
            raise ValueError('label map %r does not match image %r' % (labels.shape, self.shape))
        n_out = C.c_int(0)
        _check(load_library().imsegm_image2d_enforce_connectivity(self._h, _ptr(labels), int(min_size), int(max_size),
                                                                  int(start_label), C.byref(n_out)))
        self.n_labels = n_out.value
        return self.get_labels()

    def set_labels(self, labels, n_labels=None):
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if labels.shape != self.shape:
            raise ValueError('label map %r does not match image %r' % (labels.shape, self.shape))
        if labels.size and labels.min() < 0:
            raise ValueError('labels must be non-negative')
        if n_labels is None:
            n_labels = int(labels.max()) + 1
        elif labels.size and int(labels.max()) >= n_labels:
            # (the per-label tables of the kernels have n_labels rows: a larger label would write past them)
            raise ValueError('label %d is out of range for n_labels = %d' % (int(labels.max()), n_labels))
        _check(load_library().imsegm_image2d_set_labels(self._h, _ptr(labels), int(n_labels)))
        self.n_labels = int(n_labels)
        return self

    def label_hist(self, annot, nb_annot=None):
        """counts[k, a] = pixels with resident label k and annotation a (int64 [n_labels, nb_annot])"""
        annot = np.ascontiguousarray(annot, dtype=np.int32)
        if annot.shape != self.shape:
            raise ValueError('annotation %r does not match the session %r' % (annot.shape, self.shape))
        if nb_annot is None:
            nb_annot = int(annot.max()) + 1 if annot.size else 1
        out = np.empty((self.n_labels, int(nb_annot)), dtype=np.int64)
        _check(load_library().imsegm_image2d_label_hist(self._h, _ptr(annot), int(nb_annot), _ptr(out)))
        return out

    def boundary_distances(self, segm_ref):
        """``imsegm_image2d_boundary_distances``: the thick boundary of ``segm_ref`` (points int32 n x 2, row-major) and its
        distances (float64 n) to the thick boundary of the resident label map; only ``segm_ref`` is uploaded"""
        segm_ref = np.ascontiguousarray(segm_ref, dtype=np.int32)
        if segm_ref.shape != self.shape:
            raise ValueError('reference map %r does not match the session %r' % (segm_ref.shape, self.shape))
        lib = load_library()
        return _boundary_distances(lambda *out: lib.imsegm_image2d_boundary_distances(self._h, _ptr(segm_ref), *out), self.shape)

    def get_lab(self):
        out = np.empty((3,) + self.shape, dtype=np.float64)
        _check(load_library().imsegm_image2d_get_lab(self._h, _ptr(out)))
        return out

    def get_pre_scalars(self):
        """(min, max, premax) of the last :meth:`slic` as the device holds them: the extremes of the uploaded image and the
        largest |value| of the pre-processed planes"""
        out = np.empty(3, dtype=np.float64)
        _check(load_library().imsegm_image2d_get_pre_scalars(self._h, _ptr(out)))
        return float(out[0]), float(out[1]), float(out[2])

    def get_nearest(self):
        out = np.empty(self.shape, dtype=np.int32)
        _check(load_library().imsegm_image2d_get_nearest(self._h, _ptr(out)))
        return out

    def get_centroids(self):
        """the centroid table of the last :meth:`slic` as its last centroid update left it -- no update follows the last sweep, so
        after ``max_iter`` sweeps this is the table that went into sweep ``max_iter``: (K x 5 float64 rows of (cy, cx, cL, ca, cb),
        K x 4 int32 search windows (y0, y1, x0, x1)); a centroid that lost its last pixel has an empty (all zero) window"""
        lib = load_library()
        count = C.c_int(0)
        _check(lib.imsegm_image2d_get_centroids(self._h, None, None, C.byref(count)))
        rows = np.empty((count.value, 5), dtype=np.float64)
        windows = np.empty((count.value, 4), dtype=np.int32)
        _check(lib.imsegm_image2d_get_centroids(self._h, _ptr(rows), _ptr(windows), C.byref(count)))
        return rows, windows

    def color_stats(self, mean=True, energy=True, var=True):
        k = self.n_labels
        m = np.empty((k, 3), dtype=np.float64) if mean else None
        e = np.empty((k, 3), dtype=np.float64) if energy else None
        v = np.empty((k, 3), dtype=np.float64) if var else None
        _check(load_library().imsegm_image2d_color_stats(self._h, _ptr(m), _ptr(e), _ptr(v)))
        return m, e, v

    # -- Leung-Malik texture responses ------------------------------------------------------------
    def lm_prepare(self, sigma=150.):
        """planes = image - gaussian_filter(image.astype(float), sigma)   (descriptors.py:1078)"""
        taps = gaussian_taps(sigma)
        radius = len(taps) - 1
        full = np.concatenate([taps[:0:-1], taps])
        mix = np.zeros((3, 3))
        for c_out in range(3):          # the same filter along the 3-element channel axis, 'reflect'
            for j in range(-radius, radius + 1):
                i = (c_out + j) % 6
                mix[c_out, i if i < 3 else 5 - i] += full[j + radius]
        _check(load_library().imsegm_image2d_lm_prepare(self._h, _ptr(taps), radius, _ptr(np.ascontiguousarray(mix))))
        return self

    def lm_battery(self, battery, clip):
        """response of one filter battery (k x S x S convolution kernels) -> L2 norm over the channels"""
        battery = np.asarray(battery, dtype=np.float64)
        nk, side = battery.shape[0], battery.shape[1]
        if battery.ndim != 3 or battery.shape[2] != side or side % 2 != 1:
            raise ValueError('wrong battery dim %r' % (battery.shape, ))
        pad = {1: 1, 2: 2, 3: 4, 4: 4, 5: 8, 6: 8, 7: 8, 8: 8}.get(nk)
        if pad is None:
            raise ValueError('at most 8 kernels per battery')
        if pad != nk:                    # repeat the last kernel: the maximum is unchanged
            battery = np.concatenate([battery, np.repeat(battery[-1:], pad - nk, axis=0)], axis=0)
        # true convolution == correlation with the flipped kernel; layout [kx][ky][kernel]
        weights = np.ascontiguousarray(battery[:, ::-1, ::-1].transpose(2, 1, 0))
        ssq = C.c_double(0)
        _check(load_library().imsegm_image2d_lm_battery(self._h, _ptr(weights), pad, side // 2, float(clip), C.byref(ssq)))
        return float(np.sqrt(ssq.value))

    @staticmethod
    def _battery_weights(battery):
        """(weights [kx][ky][kernel] of the flipped kernels, kernels after padding to 1 / 2 / 4 / 8, radius)"""
        battery = np.asarray(battery, dtype=np.float64)
        nk, side = battery.shape[0], battery.shape[1]
        if battery.ndim != 3 or battery.shape[2] != side or side % 2 != 1:
            raise ValueError('wrong battery dim %r' % (battery.shape, ))
        pad = {1: 1, 2: 2, 3: 4, 4: 4, 5: 8, 6: 8, 7: 8, 8: 8}.get(nk)
        if pad is None:
            raise ValueError('at most 8 kernels per battery')
        if pad != nk:                    # repeat the last kernel: the maximum is unchanged
            battery = np.concatenate([battery, np.repeat(battery[-1:], pad - nk, axis=0)], axis=0)
        # true convolution == correlation with the flipped kernel; layout [kx][ky][kernel]
        return np.ascontiguousarray(battery[:, ::-1, ::-1].transpose(2, 1, 0)), pad, side // 2

    #: kernels whose singular values fall below this share of the largest after RANK components are evaluated as separable passes
    SEPARABLE_TOLERANCE, SEPARABLE_MAX_RANK = 1e-13, 2

    #: two dense kernels count as mirror images of each other when they differ by less than this share of their maximum
    MIRROR_TOLERANCE = 1e-12

    @classmethod
    def _mirror_pairs(cls, dense):
        """the dense (flipped) kernels as pairs (a, b, m) with ``dense[b] == m * dense[a][:, ::-1]`` (m = +-1) to MIRROR_TOLERANCE,
        or None when they do not all pair up -- the orientations theta and pi - theta of a Leung-Malik battery do"""
        left = list(range(len(dense)))
        pairs = []
        while left:
            a = left.pop(0)
            mirrored = dense[a][:, ::-1]
            bound = cls.MIRROR_TOLERANCE * np.abs(dense[a]).max()
            for b in left:
                hit = [m for m in (1., -1.) if np.abs(dense[b] - m * mirrored).max() <= bound]
                if hit:
                    pairs.append((a, b, hit[0]))
                    left.remove(b)
                    break
            else:
                return None
        return pairs

    @classmethod
    def _quad_table(cls, dense, pairs, radius):
        """the table of ``k_conv_battery_quad`` (csrc/texture.hip): [x = 0..r][t = 0..r][WS of the pairs | WD of the pairs], WS / WD =
        half the sum / difference of the first kernel of a pair at (row t, column r + x) and (row t, column r - x), the row of
        the kernel centre halved once more; then the mirror signs"""
        r = radius
        table = np.zeros((r + 1, r + 1, 2 * len(pairs)))
        for k, (a, _, _) in enumerate(pairs):
            right, left = dense[a][:r + 1, r:], dense[a][:r + 1, r::-1]           # [t][x]: columns r + x | r - x
            table[:, :, k] = ((right + left) / 2).T
            table[:, :, len(pairs) + k] = ((right - left) / 2).T
        table[:, r, :] /= 2
        return np.concatenate([table.ravel(), [m for _, _, m in pairs]])

    @classmethod
    def _split_battery(cls, battery, separable=True, symmetric=True, mirror=True):
        """one battery (k x S x S convolution kernels) as the device takes it: (dense weights [kx][ky][kernel] of the flipped
        kernels that stay dense, their number after padding to 0 / 1 / 2 / 4 / 6 / 8, separable taps, groups, rank, radius, parity).
        A kernel of numerical rank <= SEPARABLE_MAX_RANK (numpy SVD of the flipped kernel) becomes `rank` pairs of (x taps, y
        taps); at most two kernels per battery go that way (the 0 and 90 degree orientations of an edge / bar battery).
        parity: +-1 the dense kernels are all even / odd under the point reflection; +-2 (``mirror``, side 33) they are mirror
        images of each other in pairs as well -- the dense weights are then the quad table (:meth:`_quad_table`) in a block of
        the usual size."""
        battery = np.asarray(battery, dtype=np.float64)
        nk, side = battery.shape[0], battery.shape[1]
        if battery.ndim != 3 or battery.shape[2] != side or side % 2 != 1:
            raise ValueError('wrong battery dim %r' % (battery.shape, ))
        if nk > 8:
            raise ValueError('at most 8 kernels per battery')
        flipped = battery[:, ::-1, ::-1]
        dense, factors = [], []
        for kernel in flipped:
            parts = None
            if separable and len(factors) < 2:
                u, sv, vt = np.linalg.svd(kernel)
                rank = int(np.sum(sv > cls.SEPARABLE_TOLERANCE * sv[0])) if sv[0] > 0 else 0
                if 1 <= rank <= cls.SEPARABLE_MAX_RANK:
                    parts = [(vt[i], sv[i] * u[:, i]) for i in range(rank)]          # (taps along x, taps along y)
            if parts is None:
                dense.append(kernel)
            else:
                factors.append(parts)
        rank = max([len(p) for p in factors] or [0])
        taps = np.zeros((len(factors), rank, 2, side))
        for g, parts in enumerate(factors):
            for i, (tx, ty) in enumerate(parts):
                taps[g, i, 0], taps[g, i, 1] = tx, ty
        # point symmetry of the kernels that stay dense: all even (K[-p] == K[p]) -> +1, all odd -> -1, bit for bit; else 0
        parity = 0
        if dense and symmetric:
            if all(np.array_equal(k[::-1, ::-1], k) for k in dense):
                parity = 1
            elif all(np.array_equal(k[::-1, ::-1], -k) for k in dense):
                parity = -1
        if parity and mirror and side == 33 and len(dense) in (2, 4, 6, 8):
            pairs = cls._mirror_pairs(dense)
            if pairs is not None:
                weights = np.zeros(side * side * len(dense))
                table = cls._quad_table(dense, pairs, side // 2)
                weights[:table.size] = table
                return weights, len(dense), taps, len(factors), rank, side // 2, 2 * parity
        pad = {0: 0, 1: 1, 2: 2, 3: 4, 4: 4, 5: 6, 6: 6, 7: 8, 8: 8}[len(dense)]
        if pad != len(dense):            # repeat the last kernel: the maximum is unchanged
            dense = dense + [dense[-1]] * (pad - len(dense))
        weights = np.ascontiguousarray(np.asarray(dense).transpose(2, 1, 0)) if dense else np.zeros(0)
        return weights, pad, taps, len(factors), rank, side // 2, parity

    #: the last banks handed to :meth:`lm_features`, split and packed (the factorisation is 60 SVDs per bank)
    _packed_banks = []

    @classmethod
    def _pack_bank(cls, batteries, separable, mirror=True):
        """the arguments of ``imsegm_image2d_lm_features_sep`` for a list of batteries; remembered per list of battery ARRAYS (the
        bank of the descriptors is built once per process) with their sums as a guard against arrays changed in place"""
        batteries = [np.asarray(b, dtype=np.float64) for b in batteries]
        sums = [float(b.sum()) for b in batteries]
        flag_now = (separable, mirror)
        for held, flag, held_sums, packed in cls._packed_banks:
            if flag == flag_now and len(held) == len(batteries) and all(a is b for a, b in zip(held, batteries)) and held_sums == sums:
                return packed
        parts = [cls._split_battery(b, separable, separable, mirror and separable) for b in batteries]
        radius = parts[0][5]
        if any(p[5] != radius for p in parts):
            raise ValueError('the batteries of one call have one kernel size')
        weights = np.concatenate([p[0].ravel() for p in parts])
        taps = np.concatenate([p[2].ravel() for p in parts])
        packed = dict(weights=weights if weights.size else None, taps=taps if taps.size else None, radius=radius, count=len(parts),
                      kernels=np.array([p[1] for p in parts], dtype=np.int32), groups=np.array([p[3] for p in parts], dtype=np.int32),
                      ranks=np.array([p[4] for p in parts], dtype=np.int32), parity=np.array([p[6] for p in parts], dtype=np.int32))
        cls._packed_banks.insert(0, (batteries, flag_now, sums, packed))
        del cls._packed_banks[4:]
        return packed

    def lm_features(self, batteries, clip, mean=True, std=True, energy=True, separable=True, to_host=True, mirror=True):
        """``imsegm_image2d_lm_features_sep``: K x (3 * flags * len(batteries)) statistics of all batteries in one call;
        ``separable=False``: every kernel as a dense S x S sum (``imsegm_image2d_lm_features``); ``to_host=False``: the table
        stays on the device (for :meth:`segment` with a device class model, :meth:`get_features`) and nothing is waited for;
        ``mirror=False``: the dense kernels of a battery one by one (point symmetry only), not as mirror pairs"""
        bank = self._pack_bank(batteries, bool(separable), bool(mirror))
        mask = (1 if mean else 0) | (2 if std else 0) | (4 if energy else 0)
        out = np.empty((self.n_labels, 3 * bin(mask).count('1') * bank['count']), dtype=np.float64) if to_host else None
        _check(load_library().imsegm_image2d_lm_features_sep(
            self._h, _ptr(bank['weights']), _ptr(bank['kernels']), _ptr(bank['parity']), _ptr(bank['taps']), _ptr(bank['groups']),
            _ptr(bank['ranks']), bank['count'], bank['radius'], float(clip), mask, _ptr(out)))
        return out

    def features_place(self, total_columns, column):
        """``imsegm_image2d_features_place``: the next :meth:`features_color` / :meth:`lm_features` (``to_host=False``) writes its
        columns at ``column`` of a resident table ``total_columns`` wide"""
        _check(load_library().imsegm_image2d_features_place(self._h, int(total_columns), int(column)))
        return self

    def get_features(self, columns):
        """the resident K x ``columns`` feature table (``imsegm_image2d_get_features``)"""
        out = np.empty((self.n_labels, int(columns)), dtype=np.float64)
        _check(load_library().imsegm_image2d_get_features(self._h, _ptr(out), int(columns)))
        return out

    def put_features(self, table):
        """make ``table`` (C-contiguous float64, ``n_labels`` x F with 3 <= F <= 256) the resident feature table: the colour means
        placed into an F-wide table allocate it and mark it valid, then all K x F values are overwritten through
        ``imsegm_image2d_device_ptr(which = 3)``.  A descriptor group is three columns wide, so a table of one or two columns
        cannot be placed (``imsegm_image2d_features_place``).  Needs an uploaded image / volume and a label map."""
        if not isinstance(table, np.ndarray) or table.dtype != np.float64 or table.ndim != 2 or not table.flags.c_contiguous:
            raise ValueError('put_features: a C-contiguous float64 K x F array is required')
        k, f = table.shape
        if k != self.n_labels or k < 1:
            raise ValueError('put_features: %d rows for %d labels' % (k, self.n_labels))
        if f < 3 or f > 256:
            raise ValueError('put_features: 3 .. 256 columns (a descriptor group is three columns wide), got %d' % f)
        self.features_place(f, 0)
        self.features_color(True, False, False, to_host=False)
        ptr = _vp()
        _check(load_library().imsegm_image2d_device_ptr(self._h, 3, C.byref(ptr)))
        self.ctx.copy(ptr.value, table.ctypes.data, table.nbytes, synchronize=True)
        return self

    def response_stats(self, mul, div, mean=True, energy=True, var=True):
        k = self.n_labels
        m = np.empty((k, 3), dtype=np.float64) if mean else None
        e = np.empty((k, 3), dtype=np.float64) if energy else None
        v = np.empty((k, 3), dtype=np.float64) if var else None
        _check(load_library().imsegm_image2d_response_stats(self._h, float(mul), float(div), _ptr(m), _ptr(e), _ptr(v)))
        return m, e, v

    def response_median(self, mul, div):
        """per-label median of the normalised response (response * mul) / div: K x 3 (NaN for a label without pixels)"""
        out = np.empty((self.n_labels, 3), dtype=np.float64)
        _check(load_library().imsegm_image2d_response_median(self._h, float(mul), float(div), _ptr(out)))
        return out

    def response_mean_gradient(self, mul, div):
        """per-label mean of ``np.sum(np.gradient(plane), axis=0)`` of the normalised response, per channel: K x 3"""
        out = np.empty((self.n_labels, 3), dtype=np.float64)
        _check(load_library().imsegm_image2d_response_mean_gradient(self._h, float(mul), float(div), _ptr(out)))
        return out

    def get_response(self):
        out = np.empty((3, ) + self.shape, dtype=np.float64)
        _check(load_library().imsegm_image2d_get_response(self._h, _ptr(out)))
        return out

    def graph(self):
        """(edges int32 E x 2 ordered by (b, a); centres K x 2; present flags K)"""
        k = self.n_labels
        cap = max(64, 4 * k)
        centres = np.empty((k, 2), dtype=np.float64)
        present = np.empty(k, dtype=np.uint8)
        while True:
            edges = np.empty((cap, 2), dtype=np.int32)
            ne = C.c_int(0)
            _check(load_library().imsegm_image2d_graph(self._h, _ptr(edges), cap, C.byref(ne), _ptr(centres),
                                                       _ptr(present)))
            if ne.value <= cap:
                return edges[:ne.value], centres, present.astype(bool)
            cap = ne.value

    def all_finite(self):
        """no NaN / inf among the uploaded pixels (``imsegm_image2d_all_finite``)"""
        ok = C.c_int(0)
        _check(load_library().imsegm_image2d_all_finite(self._h, C.byref(ok)))
        return bool(ok.value)

    def gather(self, graph_labels=None, proba=None, to_host=True, segm_out=None):
        """``graph_labels[slic]`` (int32 H x W) and ``proba[slic]`` (float64 H x W x C); ``segm_out``: the caller's own
        C-contiguous int32 array of the session's shape for the first"""
        segm = soft = None
        gl = pr = None
        nc = 0
        if graph_labels is not None:
            gl = np.ascontiguousarray(graph_labels, dtype=np.int32)
            if gl.shape[0] < self.n_labels:
                raise ValueError('label LUT shorter than the number of superpixels')
            segm = np.empty(self.shape, dtype=np.int32) if to_host else None
            if to_host and segm_out is not None:
                if not isinstance(segm_out, np.ndarray) or segm_out.shape != tuple(self.shape) or segm_out.dtype != np.int32 \
                        or not segm_out.flags.c_contiguous or not segm_out.flags.writeable:
                    raise ValueError('segm_out must be a writeable C-contiguous int32 array of shape %r' % (tuple(self.shape), ))
                segm = segm_out
        if proba is not None:
            pr = np.ascontiguousarray(proba, dtype=np.float64)
            if pr.ndim != 2 or pr.shape[0] < self.n_labels:
                raise ValueError('proba LUT shorter than the number of superpixels')
            nc = pr.shape[1]
            soft = np.empty(self.shape + (nc,), dtype=np.float64) if to_host else None
        _check(load_library().imsegm_image2d_gather(self._h, _ptr(gl), _ptr(pr), nc, _ptr(segm), _ptr(soft)))
        return segm, soft


def img_as_float_map(dtype):
    """``skimage.util.img_as_float`` (util/dtype.py) as an affine map ``(v + offset) * scale``"""
    dtype = np.dtype(dtype)
    if dtype.kind in 'fb':
        return 0., 1.
    if dtype.kind == 'u':
        return 0., 1. / np.iinfo(dtype).max
    if dtype.kind == 'i':
        info = np.iinfo(dtype)
        return 0.5, 2. / (float(info.max) - float(info.min))
    raise ValueError('unsupported dtype %r' % dtype)


class Volume3D(Image2D):
    """device-resident state of one D x H x W gray volume (supervoxel path)"""

    def __init__(self, depth, height, width, ctx=None):
        self.ctx = ctx or default_context()
        self.shape = (int(depth), int(height), int(width))
        self._h = _vp()
        self.n_labels = 0
        _check(load_library().imsegm_volume_create(self.ctx._h, self.shape[0], self.shape[1], self.shape[2],
                                                   C.byref(self._h)))
        self.ctx.users += 1

    def upload(self, volume):
        """D x H x W volume; uint8 / float32 / float64 go up as they are, anything else as float64
        (exact for integers up to 53 bits); SLIC sees ``img_as_float`` of the source dtype"""
        volume = np.asarray(volume)
        if volume.shape != self.shape:
            raise ValueError('expected a volume of shape %r, got %r' % (self.shape, volume.shape))
        off, scale = img_as_float_map(volume.dtype)
        if volume.dtype not in _DTYPES:
            volume = volume.astype(np.float64)
        volume = np.ascontiguousarray(volume)
        _check(load_library().imsegm_volume_upload(self._h, _ptr(volume), _DTYPES[volume.dtype], off, scale))
        self.dtype = volume.dtype
        return self

    def slic(self, n_segments, compactness, sigma=1., spacing=(1., 1., 1.), max_iter=10, enforce_connectivity=True,
             min_size_factor=0.5, max_size_factor=3., start_label=0):
        # scikit-image 0.18 keeps spacing and sigma in the dtype of the image: float32 for a float32 volume (which then
        # runs in float32 on the device too), float64 for everything else
        fdt = np.float32 if getattr(self, 'dtype', None) == np.float32 else np.float64
        spacing = np.ascontiguousarray(spacing, dtype=fdt)
        if spacing.shape != (3, ):
            raise ValueError('spacing must have 3 elements (z, y, x)')
        taps = [gaussian_taps(float(s)) for s in np.array([sigma, sigma, sigma], dtype=fdt) / spacing]
        spacing = np.ascontiguousarray(spacing, dtype=np.float64)
        args = []
        for t in taps:
            args += [_ptr(t), -1 if t is None else len(t) - 1]
        n_out = C.c_int(0)
        _check(load_library().imsegm_volume_slic(
            self._h, int(n_segments), float(compactness), *args, _ptr(spacing), int(max_iter),
            int(bool(enforce_connectivity)), float(min_size_factor), float(max_size_factor), int(start_label),
            C.byref(n_out)))
        self.n_labels = n_out.value
        return self.n_labels

    def get_pre_scalar(self):
        """(inspection for the parity tests) (plane, premax) of the last ``slic``: the pre-processed D x H x W plane in the type the
        SLIC kernels read it -- float32 for a float32 volume, float64 for every other -- and the device's max |value| of a float64
        plane (None for a float32 one)"""
        lib = load_library()
        code, premax = C.c_int(-1), C.c_double(0.)
        _check(lib.imsegm_volume_get_pre(self._h, None, C.byref(code), None))
        out = np.empty(self.shape, dtype=np.float32 if code.value == F32 else np.float64)
        _check(lib.imsegm_volume_get_pre(self._h, _ptr(out), C.byref(code), C.byref(premax)))
        return out, (None if code.value == F32 else premax.value)

    def get_pre(self):
        """(inspection for the parity tests) the pre-processed plane of the last ``slic`` (see ``get_pre_scalar``)"""
        return self.get_pre_scalar()[0]

    def get_centroids(self):
        """(inspection for the parity tests) K x 4 centroid table (z, y, x, value) of the last ``slic``, float32 for a float32
        volume and float64 otherwise: what the last centroid update left (no update follows the last sweep)"""
        lib = load_library()
        code, count = C.c_int(-1), C.c_int(0)
        _check(lib.imsegm_volume_get_centroids(self._h, None, C.byref(code), C.byref(count)))
        out = np.empty((count.value, 4), dtype=np.float32 if code.value == F32 else np.float64)
        _check(lib.imsegm_volume_get_centroids(self._h, _ptr(out), C.byref(code), C.byref(count)))
        return out

    def label_cc(self):
        """``skimage.measure.label`` of the current label map, in place; returns max label + 1"""
        n_out = C.c_int(0)
        _check(load_library().imsegm_volume_label_cc(self._h, C.byref(n_out)))
        self.n_labels = n_out.value
        return self.n_labels

    def gray_stats(self, mean=True, energy=True, var=True):
        k = self.n_labels
        m = np.empty(k, dtype=np.float64) if mean else None
        e = np.empty(k, dtype=np.float64) if energy else None
        v = np.empty(k, dtype=np.float64) if var else None
        _check(load_library().imsegm_volume_gray_stats(self._h, _ptr(m), _ptr(e), _ptr(v)))
        return m, e, v

    def graph(self):
        """(edges int32 E x 2 ordered by (b, a); centres K x 3 (z, y, x); present flags K)"""
        k = self.n_labels
        cap = max(64, 8 * k)
        centres = np.empty((k, 3), dtype=np.float64)
        present = np.empty(k, dtype=np.uint8)
        while True:
            edges = np.empty((cap, 2), dtype=np.int32)
            ne = C.c_int(0)
            _check(load_library().imsegm_volume_graph(self._h, _ptr(edges), cap, C.byref(ne), _ptr(centres),
                                                      _ptr(present)))
            if ne.value <= cap:
                return edges[:ne.value], centres, present.astype(bool)
            cap = ne.value

    def boundary_distances(self, segm_ref):
        """``imsegm_volume_boundary_distances``: the thick boundary of ``segm_ref`` (points int32 n x 3, raster order) and its
        distances (float64 n) to the thick boundary of the resident label map; only ``segm_ref`` is uploaded"""
        segm_ref = np.ascontiguousarray(segm_ref, dtype=np.int32)
        if segm_ref.shape != self.shape:
            raise ValueError('reference map %r does not match the session %r' % (segm_ref.shape, self.shape))
        lib = load_library()
        return _boundary_distances(lambda *out: lib.imsegm_volume_boundary_distances(self._h, _ptr(segm_ref), *out), self.shape)

    def _unsupported(self, *args, **kwargs):
        raise HipError('not available for volumes')

    get_lab = color_stats = run_color = _unsupported

    # -- Leung-Malik responses of the slices (descriptors.py:969-1038: every slice is filtered as a 2-D image) --------
    def lm_prepare(self, sigma=150.):
        """planes = volume - gaussian_filter(slice, sigma) per slice   (image_subtract_gauss_smooth, descriptors.py:981-994)"""
        taps = gaussian_taps(sigma)
        _check(load_library().imsegm_image2d_lm_prepare(self._h, _ptr(taps), len(taps) - 1, None))
        return self

    def response_stats(self, mul, div, mean=True, energy=True, var=True):
        k = self.n_labels
        m = np.empty(k, dtype=np.float64) if mean else None
        e = np.empty(k, dtype=np.float64) if energy else None
        v = np.empty(k, dtype=np.float64) if var else None
        _check(load_library().imsegm_image2d_response_stats(self._h, float(mul), float(div), _ptr(m), _ptr(e), _ptr(v)))
        return m, e, v

    def response_median(self, mul, div):
        """per-supervoxel median of the normalised response (response * mul) / div: K (NaN for a label without voxels)"""
        out = np.empty(self.n_labels, dtype=np.float64)
        _check(load_library().imsegm_image2d_response_median(self._h, float(mul), float(div), _ptr(out)))
        return out

    def response_mean_gradient(self, mul, div):
        """per-supervoxel mean of ``np.sum(np.gradient(slice), axis=0)`` of the normalised response (never along z): K"""
        out = np.empty(self.n_labels, dtype=np.float64)
        _check(load_library().imsegm_image2d_response_mean_gradient(self._h, float(mul), float(div), _ptr(out)))
        return out

    def get_response(self):
        out = np.empty(self.shape, dtype=np.float64)
        _check(load_library().imsegm_image2d_get_response(self._h, _ptr(out)))
        return out


class Batch2D(object):
    """up to ``max_images`` colour images of ONE size through the whole pipeline in one chain of launches
    (``imsegm_batch2d_*``, csrc/batch.hip: image = blockIdx.z): what the reference does by mapping ``segment_image_model``
    over a process pool (``run_segm_slic_model_graphcut.py:505-514``)"""

    def __init__(self, max_images, height, width, ctx=None):
        self.ctx = ctx or default_context()
        self.shape = (int(height), int(width))
        self.max_images = int(max_images)
        self._h = _vp()
        self.n_labels = []
        self.n_images = 0
        _check(load_library().imsegm_batch2d_create(self.ctx._h, self.max_images, self.shape[0], self.shape[1], C.byref(self._h)))
        self.ctx.users += 1

    def close(self):
        if self._h and self.ctx is not None:
            self.ctx.users -= 1
            if self.ctx._h and self.ctx.pid == os.getpid():
                load_library().imsegm_batch2d_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run_color(self, images, n_segments, compactness, gmm, pairwise, edge_type='model', feature_flags=(True, True, True),
                  sigma=1., normalize=2, max_iter=10, start_label=0, edge_cost=1., use_graphcut=True, classes=None, to_host=True,
                  pinned=True, out=None):
        """``Image2D.run_color`` for a list of images of this batch's size and one dtype (uint8 / float32 / float64):
        returns the list of segmentations (int32 H x W; ``out``: arrays to write them into) or, with ``to_host=False``,
        leaves them on the device (:meth:`segm_device_array`)"""
        images = [np.ascontiguousarray(im) for im in images]
        if not 0 < len(images) <= self.max_images:
            raise ValueError('between 1 and %d images per batch' % self.max_images)
        dtype = images[0].dtype
        if dtype not in _DTYPES or any(im.shape != self.shape + (3, ) or im.dtype != dtype for im in images):
            raise ValueError('expected images of shape %r + (3,) and one dtype of uint8 / float32 / float64' % (self.shape, ))
        code = EDGE_TYPES.get(edge_type)
        if code is None:
            raise ValueError('edge type %r is not evaluated on the device' % (edge_type, ))
        pairwise = np.ascontiguousarray(pairwise, dtype=np.float64)
        nc = gmm.n_classes
        if pairwise.shape != (nc, nc):
            raise ValueError('pairwise cost must be %d x %d' % (nc, nc))
        cl = None if classes is None else np.ascontiguousarray(classes, dtype=np.int32)
        taps = gaussian_taps(sigma)
        r = -1 if taps is None else len(taps) - 1
        n = len(images)
        src = (_vp * n)(*[im.ctypes.data for im in images])
        segm, dst = None, None
        if to_host:
            if out is not None:
                segm = list(out)
                if len(segm) != n or any(a.shape != self.shape or a.dtype != np.int32 or not a.flags['C_CONTIGUOUS'] for a in segm):
                    raise ValueError('out: one C-contiguous int32 array of the image size per image')
            else:
                alloc = pinned_empty if pinned else np.empty
                segm = [alloc(self.shape, np.int32) for _ in range(n)]
            dst = (_vp * n)(*[a.ctypes.data for a in segm])
        mask = (1 if feature_flags[0] else 0) | (2 if feature_flags[1] else 0) | (4 if feature_flags[2] else 0)
        counts = (C.c_int * n)()
        _check(load_library().imsegm_batch2d_run_color(
            self._h, n, src, _DTYPES[dtype], int(normalize), int(n_segments), float(compactness), _ptr(taps), r, int(max_iter),
            int(start_label), mask, C.byref(gmm.params), nc, _ptr(pairwise), code, float(edge_cost), int(bool(use_graphcut)), _ptr(cl),
            dst, counts))
        self.n_labels = list(counts)
        self.n_images = n
        self._feature_columns = 3 * bin(mask).count('1')
        self._uploaded = images         # page-locked sources are read asynchronously (the call ends with a synchronisation)
        return segm

    def _device_array(self, image, which):
        ptr = _vp()
        _check(load_library().imsegm_batch2d_device_ptr(self._h, int(image), which, C.byref(ptr)))
        return DeviceArray(ptr.value, self.shape, '<i4', self)

    def segm_device_array(self, image):
        """the segmentation of image ``image`` of the last batch (int32 H x W) as a device array"""
        return self._device_array(image, 1)

    def labels_device_array(self, image):
        """the superpixel map of image ``image`` of the last batch (int32 H x W) as a device array"""
        return self._device_array(image, 0)

    def get_features(self, image):
        """feature table of image ``image`` of the last batch on the host (float64 n_labels x F, columns mean | std | energy as
        ``feature_flags`` asked for)"""
        ptr = _vp()
        _check(load_library().imsegm_batch2d_device_ptr(self._h, int(image), 2, C.byref(ptr)))
        out = np.empty((self.n_labels[image], self._feature_columns), dtype=np.float64)
        if out.size:
            self.ctx.copy(out.ctypes.data, ptr.value, out.nbytes, synchronize=True)
        return out

    def _get_f64(self, image, which, shape):
        ptr = _vp()
        _check(load_library().imsegm_batch2d_device_ptr(self._h, int(image), which, C.byref(ptr)))
        out = np.empty(shape, dtype=np.float64)
        self.ctx.copy(out.ctypes.data, ptr.value, out.nbytes, synchronize=True)
        return out

    def get_lab(self, image):
        """the pre-processed planes of image ``image`` of the last batch on the host (float64 3 x H x W), as :meth:`Image2D.get_lab`"""
        return self._get_f64(image, 3, (3, ) + self.shape)

    def get_pre_scalars(self, image):
        """(min, max, premax) of image ``image`` of the last batch, as :meth:`Image2D.get_pre_scalars`"""
        return tuple(float(v) for v in self._get_f64(image, 4, (3, )))

    def get_labels(self, image):
        """superpixel map of image ``image`` of the last batch on the host (int64, the dtype scikit-image leaks)"""
        arr = self.labels_device_array(image)
        out = np.empty(self.shape, dtype=np.int32)
        self.ctx.copy(out.ctypes.data, arr.__cuda_array_interface__['data'][0], out.nbytes, synchronize=True)
        return out.astype(np.int64)


class DeviceArray(object):
    """a result buffer in HBM, exposed through ``__cuda_array_interface__`` (zero-copy hand-over to
    ``torch.as_tensor(..., device='cuda')`` / RCCL on the same HIP runtime)"""

    def __init__(self, ptr, shape, typestr, owner):
        self.owner = owner          # keeps the session alive
        self.__cuda_array_interface__ = {'shape': tuple(shape), 'typestr': typestr, 'data': (int(ptr), False),
                                         'version': 2, 'strides': None}


#: names of the counters of csrc/connectivity.hip (CNT_*) by index
CONN_COUNTERS = {'over': 0, 'small': 1, 'cursor': 2, 'kept': 3, 'fallback': 4, 'big': 5, 'little': 6, 'lroot': 8, 'flag': 9,
                 'fb': 10, 'fb2': 11}


def conn_last():
    """which kernels finished the last single-map connectivity pass of this process (imsegm_debug_conn_last): a dict with
    ``tile`` (counters of the tile attempt by name, None when none was made), ``general`` (counters of the general path's tail,
    None when it did not run) and ``oversize_rounds``; for tests"""
    raw = np.zeros(28, np.int32)
    _check(load_library().imsegm_debug_conn_last(_ptr(raw)))
    tile = {k: int(raw[4 + i]) for k, i in CONN_COUNTERS.items()} if raw[0] else None
    general = {k: int(raw[20 + i]) for k, i in CONN_COUNTERS.items() if i < 8} if raw[1] else None
    return {'tile': tile, 'general': general, 'oversize_rounds': int(raw[2])}


def gc_grid_fallbacks():
    """grid-wide graph cuts of this process that gave up waiting for a workgroup and were redone by the single workgroup"""
    return int(load_library().imsegm_debug_gc_grid_fallbacks())


def exclusive_scan(values):
    """(exclusive prefix sums, total) of int32 `values` by the library's one-workgroup scan (csrc/scan.hip); for tests"""
    values = np.ascontiguousarray(values, dtype=np.int32)
    out, total = np.empty_like(values), C.c_int(0)
    _check(load_library().imsegm_debug_exclusive_scan(values.ctypes.data, values.size, out.ctypes.data, C.byref(total)))
    return out, total.value


def slic_sweep_runs():
    """(2-D SLIC runs whose sweeps after the first ran in the one persistent launch, runs of those that were handed back to the
    per-sweep launches) of this process"""
    a, b = C.c_long(0), C.c_long(0)
    _check(load_library().imsegm_debug_slic_sweep_runs(C.byref(a), C.byref(b)))
    return a.value, b.value


def assign_sweeps_per_launch(max_iter=10):
    """sweeps one launch of the dominant SLIC kernel covered in the runs so far: max_iter - 1 when the persistent kernel took
    them all, 1 with the per-sweep launches (bench.py: algorithmic bytes per launch)"""
    persistent, fallback = slic_sweep_runs()
    return max_iter - 1 if (persistent > 0 and fallback == 0) else 1


def _device_array(sess, which, shape, typestr):
    ptr = _vp()
    _check(load_library().imsegm_image2d_device_ptr(sess._h, which, C.byref(ptr)))
    sess.ctx.synchronize()
    return DeviceArray(ptr.value, shape, typestr, sess)


def segm_device_array(sess):
    """the gathered segmentation (``graph_labels[slic]``, int32 H x W) as a device array"""
    return _device_array(sess, 1, sess.shape, '<i4')


def cut_general_graph(edges, edge_weights, unary_cost, pairwise_cost, n_iter=-1, algorithm='expansion',
                      return_energy=False, ctx=None):
    """drop-in for ``gco.cut_general_graph`` (gco-wrapper), expansion algorithm, on the GPU"""
    if algorithm != 'expansion':
        raise NotImplementedError('only algorithm="expansion" is implemented on the HIP path')
    ctx = ctx or default_context()
    edges = np.ascontiguousarray(np.asarray(edges).reshape(-1, 2), dtype=np.int32)
    ew = np.ascontiguousarray(edge_weights, dtype=np.float64)
    un = np.ascontiguousarray(unary_cost, dtype=np.float64)
    pw = np.ascontiguousarray(pairwise_cost, dtype=np.float64)
    if un.ndim != 2 or pw.shape != (un.shape[1], un.shape[1]) or len(ew) != len(edges):
        raise ValueError('shape mismatch among edges %r, weights %r, unary %r, pairwise %r' %
                         (edges.shape, ew.shape, un.shape, pw.shape))
    labels = np.empty(un.shape[0], dtype=np.int32)
    energy = C.c_int64(0)
    _check(load_library().imsegm_cut_general_graph(ctx._h, _ptr(edges), len(edges), _ptr(ew), _ptr(un), un.shape[0],
                                                   un.shape[1], _ptr(pw), int(n_iter), _ptr(labels), C.byref(energy)))
    return (labels, energy.value) if return_energy else labels


def cut_general_graph_scaled(edges, edge_weights, unary_cost, pairwise_cost, weight_max, n_iter=-1, return_energy=False, ctx=None):
    """:func:`cut_general_graph` whose scaling maximum of ``|edge_weights|`` also covers ``weight_max``: for a caller that has
    dropped edges joining a site with itself, whose weights pyGCO still sees when it scales (``imsegm_cut_general_graph_scaled``)"""
    ctx = ctx or default_context()
    edges = np.ascontiguousarray(np.asarray(edges).reshape(-1, 2), dtype=np.int32)
    ew = np.ascontiguousarray(edge_weights, dtype=np.float64)
    un = np.ascontiguousarray(unary_cost, dtype=np.float64)
    pw = np.ascontiguousarray(pairwise_cost, dtype=np.float64)
    if un.ndim != 2 or pw.shape != (un.shape[1], un.shape[1]) or len(ew) != len(edges):
        raise ValueError('shape mismatch among edges %r, weights %r, unary %r, pairwise %r' %
                         (edges.shape, ew.shape, un.shape, pw.shape))
    labels = np.empty(un.shape[0], dtype=np.int32)
    energy = C.c_int64(0)
    _check(load_library().imsegm_cut_general_graph_scaled(ctx._h, _ptr(edges), len(edges), _ptr(ew), _ptr(un), un.shape[0],
                                                          un.shape[1], _ptr(pw), float(weight_max), int(n_iter), _ptr(labels),
                                                          C.byref(energy)))
    return (labels, energy.value) if return_energy else labels


def cut_grid_graph(unary_cost, pairwise_cost, cost_v, cost_h, n_iter=-1, algorithm='expansion', return_energy=False, ctx=None):
    """drop-in for ``gco.cut_grid_graph`` (gco-wrapper, reference ``region_growing.py:248``): 4-connected pixel grid with
    vertical / horizontal edge costs ``cost_v`` (H-1 x W) / ``cost_h`` (H x W-1).  The float costs go to the device as they are
    (``imsegm_cut_grid_graph``): pyGCO's conversion to integers and the arcs of the grid -- pygco hands GCO the vertical edges
    followed by the horizontal ones of the general graph -- are computed there.  Returns int32 labels of the H*W sites.  With a
    ``ctx`` that is not a :class:`Context` (a stand-in, no device behind it) the graph goes through ``cut_general_graph``."""
    if algorithm != 'expansion':
        raise NotImplementedError('only algorithm="expansion" is implemented on the HIP path')
    unary_cost = np.ascontiguousarray(unary_cost, dtype=np.float64)
    if unary_cost.ndim != 3:
        raise ValueError('unary_cost must be height x width x labels')
    height, width, n_labels = unary_cost.shape
    cost_v, cost_h = np.ascontiguousarray(cost_v, dtype=np.float64), np.ascontiguousarray(cost_h, dtype=np.float64)
    if cost_v.shape != (height - 1, width) or cost_h.shape != (height, width - 1):
        raise ValueError('cost_v / cost_h do not match the grid %d x %d' % (height, width))
    pw = np.ascontiguousarray(pairwise_cost, dtype=np.float64)
    if pw.shape != (n_labels, n_labels):
        raise ValueError('shape mismatch between unary %r and pairwise %r' % (unary_cost.shape, pw.shape))
    ctx = ctx or default_context()
    if not isinstance(ctx, Context):
        # NOT a device path: `ctx` is a stand-in for the context, as the CPU dry runs of the drivers install one together with
        # their own cut in the place of cut_general_graph -- the general graph pygco builds goes through that function
        index = np.arange(height * width, dtype=np.int32).reshape(height, width)
        edges = np.concatenate([np.stack([index[:-1].ravel(), index[1:].ravel()], axis=1),
                                np.stack([index[:, :-1].ravel(), index[:, 1:].ravel()], axis=1)], axis=0)
        weights = np.concatenate([cost_v.ravel(), cost_h.ravel()])
        more = {'return_energy': True} if return_energy else {}
        return cut_general_graph(edges, weights, unary_cost.reshape(height * width, n_labels), pw, n_iter=n_iter, ctx=ctx, **more)
    labels = np.empty(height * width, dtype=np.int32)
    energy = C.c_int64(0)
    _check(load_library().imsegm_cut_grid_graph(ctx._h, _ptr(unary_cost), height, width, n_labels, _ptr(pw), _ptr(cost_v), _ptr(cost_h),
                                                int(n_iter), _ptr(labels), C.byref(energy)))
    return (labels, energy.value) if return_energy else labels


def grid_arcs(height, width, ctx=None):
    """(edges, arc_start, arc_to, arc_rev, edge_arc) of the ``height`` x ``width`` grid as the device builds them for
    :func:`cut_grid_graph` and :func:`object_cut_pixels` (``imsegm_debug_grid_arcs``; tests)"""
    ctx = ctx or default_context()
    n_sites, n_edges = height * width, (height - 1) * width + height * (width - 1)
    edges, edge_arc = np.zeros((n_edges, 2), dtype=np.int32), np.zeros((n_edges, 2), dtype=np.int32)
    arc_start, arc_to, arc_rev = np.zeros(n_sites + 1, np.int32), np.zeros(2 * n_edges, np.int32), np.zeros(2 * n_edges, np.int32)
    _check(load_library().imsegm_debug_grid_arcs(ctx._h, int(height), int(width), _ptr(edges), _ptr(arc_start), _ptr(arc_to),
                                                 _ptr(arc_rev), _ptr(edge_arc)))
    return edges, arc_start, arc_to, arc_rev, edge_arc


def object_cut_pixels(segm, centres, a_bg, a_fg, s_bg, b, coef_shape, gc_regul, seed_size, n_iter=999, debug=False, ctx=None):
    """``imsegm_object_cut_pixels``: the unary costs of ``object_segmentation_graphcut_pixels`` from the class map ``segm`` (int32
    H x W), ``centres`` (int32 n x 4: row, column of the distance; row, column of the seed) and the four tables, pyGCO's integers,
    the grid and the cut, all on the device.  Returns (labels H x W int32, energy); with ``debug`` also pyGCO's integer unary costs
    (H x W x (n + 1)) and its down-weight factor."""
    ctx = ctx or default_context()
    segm = np.ascontiguousarray(segm, dtype=np.int32)
    centres = np.ascontiguousarray(centres, dtype=np.int32).reshape(-1, 4)
    a_bg, a_fg, s_bg, b = (np.ascontiguousarray(t, dtype=np.float64).ravel() for t in (a_bg, a_fg, s_bg, b))
    if segm.ndim != 2 or not (len(a_bg) == len(a_fg) == len(s_bg)):
        raise ValueError('segm is height x width; a_bg, a_fg and s_bg have one entry per class')
    height, width = segm.shape
    labels = np.empty((height, width), dtype=np.int32)
    energy, dwf = C.c_int64(0), C.c_double(0.)
    unary_int = np.empty((height, width, len(centres) + 1), dtype=np.int32) if debug else None
    _check(load_library().imsegm_object_cut_pixels(ctx._h, _ptr(segm), height, width, _ptr(centres), len(centres), _ptr(a_bg), _ptr(a_fg),
                                                   _ptr(s_bg), len(a_bg), _ptr(b), len(b), float(coef_shape), float(gc_regul),
                                                   int(seed_size), int(n_iter), _ptr(labels), C.byref(energy), _ptr(unary_int),
                                                   C.byref(dwf) if debug else None))
    return (labels, energy.value, unary_int, dwf.value) if debug else (labels, energy.value)


def assume_bg_on_boundary(work, strips, bg_label, ctx=None):
    """``imsegm_assume_bg_on_boundary`` on a contiguous int32 label image (modified in place); returns the label that
    dominates the four border strips"""
    found = C.c_int(0)
    ctx = ctx or default_context()
    _check(load_library().imsegm_assume_bg_on_boundary(ctx._h, _ptr(work), work.shape[0], work.shape[1], _ptr(strips), int(bg_label),
                                                       C.byref(found)))
    return found.value


def label_hist2d(segm, windows, struc_elem, nb_labels, ctx=None):
    """``computeLabelHistogram2d`` for a batch of windows (``imsegm_label_hist2d``): uint32 [P, nb_labels]"""
    ctx = ctx or default_context()
    segm = np.ascontiguousarray(segm, dtype=np.int16)
    selem = np.ascontiguousarray(struc_elem, dtype=np.int16)
    windows = np.ascontiguousarray(windows, dtype=np.int32).reshape(-1, 6)
    out = np.zeros((len(windows), int(nb_labels)), dtype=np.uint32)
    _check(load_library().imsegm_label_hist2d(ctx._h, _ptr(segm), segm.shape[0], segm.shape[1], _ptr(windows), len(windows),
                                              _ptr(selem), selem.shape[0], selem.shape[1], int(nb_labels), _ptr(out)))
    return out


#: modes of ``imsegm_boundary_mask`` / ``imsegm_distance_map`` (``IMSEGM_BOUNDARY_*`` of include/imsegm_hip.h)
BOUNDARY_THICK, BOUNDARY_CONTOUR, BOUNDARY_CONTOUR_BORDER = 0, 1, 2


def boundary_mask(labels, mode, label=0, ctx=None):
    """``imsegm_boundary_mask`` on a contiguous 2-D int32 label map: uint8 H x W, 1 on the boundary"""
    ctx = ctx or default_context()
    out = np.empty(labels.shape, dtype=np.uint8)
    _check(load_library().imsegm_boundary_mask(ctx._h, _ptr(labels), labels.shape[0], labels.shape[1], int(mode), int(label), _ptr(out)))
    return out


def distance_map(labels, mode, label=0, ctx=None):
    """``imsegm_distance_map`` on a contiguous 2-D int32 label map: float64 H x W, distance to the nearest mask pixel"""
    ctx = ctx or default_context()
    out = np.empty(labels.shape, dtype=np.float64)
    _check(load_library().imsegm_distance_map(ctx._h, _ptr(labels), labels.shape[0], labels.shape[1], int(mode), int(label), _ptr(out)))
    return out


def _boundary_distances(call, shape):
    # room for every pixel: virtual memory only, the pages no point reaches are never touched.  The points go back as a view (the
    # caller converts them to int64 and lets the block go), the distances as a copy of their own so that the block is not kept.
    capacity = int(np.prod(shape, dtype=np.int64))
    points, dist, count = np.empty((capacity, len(shape)), dtype=np.int32), np.empty(capacity, dtype=np.float64), C.c_int(0)
    _check(call(_ptr(points), _ptr(dist), capacity, C.byref(count)))
    return points[:count.value], dist[:count.value].copy()


def boundary_distances(segm_ref, segm, ctx=None):
    """``imsegm_boundary_distances`` on two contiguous 2-D int32 label maps of one shape: (points int32 n x 2, dist float64 n)"""
    ctx = ctx or default_context()
    lib = load_library()
    return _boundary_distances(lambda *out: lib.imsegm_boundary_distances(ctx._h, _ptr(segm_ref), _ptr(segm), segm.shape[0],
                                                                          segm.shape[1], *out), segm.shape)


def boundary3d_fits(shape):
    """whether the volume kernels take a map of this shape (``edt3d_size_ok`` of csrc/boundary3d.hip): three positive extents,
    squared distances that fit 32 bits and at most 2^30 voxels; looks at the shape only"""
    if len(shape) != 3 or min(shape) < 1:
        return False
    depth, height, width = (int(extent) for extent in shape)
    return depth**2 + height**2 + width**2 <= 2**32 - 1 and depth * height * width <= 2**30


def boundary_mask3d(labels, ctx=None):
    """``imsegm_boundary_mask3d`` on a contiguous 3-D int32 label map: uint8 D x H x W, 1 on the thick boundary"""
    ctx = ctx or default_context()
    out = np.empty(labels.shape, dtype=np.uint8)
    _check(load_library().imsegm_boundary_mask3d(ctx._h, _ptr(labels), labels.shape[0], labels.shape[1], labels.shape[2], _ptr(out)))
    return out


def distance_map3d(labels, ctx=None):
    """``imsegm_distance_map3d`` on a contiguous 3-D int32 label map: float64 D x H x W, distance to the nearest voxel of the thick
    boundary"""
    ctx = ctx or default_context()
    out = np.empty(labels.shape, dtype=np.float64)
    _check(load_library().imsegm_distance_map3d(ctx._h, _ptr(labels), labels.shape[0], labels.shape[1], labels.shape[2], _ptr(out)))
    return out


def boundary_distances3d(segm_ref, segm, ctx=None):
    """``imsegm_boundary_distances3d`` on two contiguous 3-D int32 label maps of one shape: (points int32 n x 3, dist float64 n)"""
    ctx = ctx or default_context()
    lib = load_library()
    return _boundary_distances(lambda *out: lib.imsegm_boundary_distances3d(ctx._h, _ptr(segm_ref), _ptr(segm), segm.shape[0],
                                                                            segm.shape[1], segm.shape[2], *out), segm.shape)


def labels_overlap(seg1, seg2, n_labels1, n_labels2, ctx=None):
    """``imsegm_labels_overlap`` on two contiguous int32 label arrays of one size: int64 [n_labels1, n_labels2]"""
    ctx = ctx or default_context()
    out = np.empty((int(n_labels1), int(n_labels2)), dtype=np.int64)
    _check(load_library().imsegm_labels_overlap(ctx._h, _ptr(seg1), _ptr(seg2), seg1.size, int(n_labels1), int(n_labels2), _ptr(out)))
    return out


def ellipse_ransac(point_offsets, points, params, success, trial_egg, points_all, point_value, residual_threshold,
                   with_residuals=False, ctx=None):
    """``imsegm_ellipse_ransac``: scores the RANSAC trials of all egg candidates of an image.  ``point_offsets`` int32 [E + 1] into
    ``points`` float64 [P, 2]; ``params`` float64 [T, 5] with ``success`` uint8 [T] and ``trial_egg`` int32 [T] (not decreasing);
    ``points_all`` float64 [N, 2] with ``point_value`` float64 [N].  Returns (best int32 [E], kept int32 [E], mask uint8 [P],
    criterion float64 [T], residuals float64 [pairs] or None): see include/imsegm_hip.h."""
    ctx = ctx or default_context()
    point_offsets = np.ascontiguousarray(point_offsets, dtype=np.int32).ravel()
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    params = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 5)
    success = np.ascontiguousarray(success, dtype=np.uint8).ravel()
    trial_egg = np.ascontiguousarray(trial_egg, dtype=np.int32).ravel()
    points_all = np.ascontiguousarray(points_all, dtype=np.float64).reshape(-1, 2)
    point_value = np.ascontiguousarray(point_value, dtype=np.float64).ravel()
    n_eggs, n_trials = len(point_offsets) - 1, len(params)
    if len(success) != n_trials or len(trial_egg) != n_trials or len(point_value) != len(points_all):
        raise ValueError('ellipse_ransac: one success flag and one egg per trial, one value per centre')
    if n_eggs >= 1 and (point_offsets[0] != 0 or point_offsets[-1] != len(points)):
        raise ValueError('ellipse_ransac: the point offsets must span the point list')
    best, kept = np.empty(max(n_eggs, 0), dtype=np.int32), np.empty(max(n_eggs, 0), dtype=np.int32)
    mask, criterion = np.empty(len(points), dtype=np.uint8), np.empty(n_trials, dtype=np.float64)
    residuals = None
    if with_residuals and n_eggs >= 1 and n_trials >= 1:
        counts = np.diff(point_offsets.astype(np.int64))
        inside = (trial_egg >= 0) & (trial_egg < n_eggs)
        residuals = np.empty(int(counts[trial_egg[inside]].sum()) if inside.all() else 0, dtype=np.float64)
    _check(load_library().imsegm_ellipse_ransac(ctx._h, n_eggs, _ptr(point_offsets), _ptr(points), n_trials, _ptr(params), _ptr(success),
                                                _ptr(trial_egg), _ptr(points_all), _ptr(point_value), len(points_all),
                                                float(residual_threshold), _ptr(best), _ptr(kept), _ptr(mask), _ptr(criterion),
                                                _ptr(residuals)))
    return best, kept, mask, criterion, residuals


#: ``IMSEGM_ELLIPSE_PLACE_LABELS``: labels 0 .. 4095 own a slot of the label tables of csrc/ellipse_place.hip
ELLIPSE_PLACE_LABELS = 4096
#: what a centre coordinate or a radius of ``imsegm_ellipse_place`` / ``imsegm_ellipse_overlaps`` may be in absolute value
ELLIPSE_PLACE_MAX_COORD = 1 << 30


def _ellipse_arguments(segm, geom, sincos):
    if segm.ndim != 2 or segm.dtype != np.int32 or not segm.flags.c_contiguous:
        raise ValueError('the label map must be a C-contiguous 2-D int32 array')
    geom = np.ascontiguousarray(geom, dtype=np.int32).reshape(-1, 8)
    sincos = np.ascontiguousarray(sincos, dtype=np.float64).reshape(-1, 2)
    if len(geom) != len(sincos):
        raise ValueError('one (sin, cos) pair per ellipse')
    return geom, sincos


def ellipse_place(segm, geom, sincos, labels, thr_overlap, ctx=None):
    """``imsegm_ellipse_place``: paints the ellipses ``geom`` int32 [n, 8] (centre, radii, clipped box) / ``sincos`` float64 [n, 2]
    with ``labels`` int32 [n] into the C-contiguous int32 map ``segm`` IN PLACE, one after the other, each unless it overlaps a label
    of the map as it stands by more than ``thr_overlap``; returns placed uint8 [n]: see include/imsegm_hip.h"""
    geom, sincos = _ellipse_arguments(segm, geom, sincos)
    labels = np.ascontiguousarray(labels, dtype=np.int32).ravel()
    if len(labels) != len(geom):
        raise ValueError('one label per ellipse')
    placed = np.zeros(len(geom), dtype=np.uint8)
    if len(geom) == 0:
        return placed
    ctx = ctx or default_context()
    _check(load_library().imsegm_ellipse_place(ctx._h, _ptr(segm), segm.shape[0], segm.shape[1], len(geom), _ptr(geom), _ptr(sincos),
                                               _ptr(labels), float(thr_overlap), _ptr(placed)))
    return placed


def ellipse_overlaps(segm, geom, sincos, nb_labels, ctx=None):
    """``imsegm_ellipse_overlaps``: per ellipse the histogram of the labels 0 .. nb_labels - 1 of the C-contiguous int32 map
    ``segm`` under its mask and the size of the mask: (counts int64 [n, nb_labels], areas int64 [n])"""
    geom, sincos = _ellipse_arguments(segm, geom, sincos)
    counts, areas = np.zeros((len(geom), int(nb_labels)), dtype=np.int64), np.zeros(len(geom), dtype=np.int64)
    if len(geom) == 0:
        return counts, areas
    ctx = ctx or default_context()
    _check(load_library().imsegm_ellipse_overlaps(ctx._h, _ptr(segm), segm.shape[0], segm.shape[1], len(geom), _ptr(geom), _ptr(sincos),
                                                  int(nb_labels), _ptr(counts), _ptr(areas)))
    return counts, areas


#: ``IMSEGM_MORPH_MAX_RADIUS``: the largest disc radius of the opening kernels
MORPH_MAX_RADIUS = 64


def split_background_foreground(segm, sel_bg, sel_fg, ctx=None):
    """``imsegm_split_background_foreground`` on a 2-D class map and integer radii: (seg_bg, seg_fg) uint8 H x W"""
    ctx = ctx or default_context()
    segm = np.ascontiguousarray(segm, dtype=np.int32)
    seg_bg, seg_fg = np.empty(segm.shape, dtype=np.uint8), np.empty(segm.shape, dtype=np.uint8)
    _check(load_library().imsegm_split_background_foreground(ctx._h, _ptr(segm), segm.shape[0], segm.shape[1], int(sel_bg), int(sel_fg),
                                                             _ptr(seg_bg), _ptr(seg_fg)))
    return seg_bg, seg_fg


def boundary_rays(segm, sel_bg, sel_fg, positions, directions, with_fg=True, ctx=None):
    """``imsegm_boundary_rays``: the rays of all positions on the smoothed background mask (edge 'up') and, ``with_fg``, on the
    smoothed foreground mask (edge 'down') of a 2-D class map, the masks staying on the device: (float32 [P, A], float32 [P, A] or
    None)"""
    ctx = ctx or default_context()
    segm = np.ascontiguousarray(segm, dtype=np.int32)
    positions = np.ascontiguousarray(positions, dtype=np.int32).reshape(-1, 2)
    directions = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 2)
    rays_bg = np.empty((len(positions), len(directions)), dtype=np.float32)
    rays_fg = np.empty_like(rays_bg) if with_fg else None
    _check(load_library().imsegm_boundary_rays(ctx._h, _ptr(segm), segm.shape[0], segm.shape[1], int(sel_bg), int(sel_fg), _ptr(positions),
                                               len(positions), _ptr(directions), len(directions), _ptr(rays_bg), _ptr(rays_fg)))
    return rays_bg, rays_fg


#: ``IMSEGM_OBJECT_SHAPES_MAX_SPAN`` / ``IMSEGM_OBJECT_SHAPES_MAX_OBJECTS``
OBJECT_SHAPES_MAX_SPAN, OBJECT_SHAPES_MAX_OBJECTS = 65536, 65536


def object_shapes(segm, directions, max_objects=1024, ctx=None):
    """``imsegm_object_shapes``: the objects of a C-contiguous 2-D int32 label map in the order of ``compute_object_shapes`` with
    their moments, rounded centres of mass and raw 'down' rays, from one chain of launches: (n_objects, labels int32 [n], moments
    int64 [n, 3], centres int32 [n, 2], rays float32 [n, A]).  A map the call does not take (``IMSEGM_E_OBJECT_CAPS``) gives
    (n_objects, None, None, None, None): n_objects above ``max_objects``, or -1 for label values that span
    ``OBJECT_SHAPES_MAX_SPAN`` or more -- no error."""
    if segm.ndim != 2 or segm.dtype != np.int32 or not segm.flags.c_contiguous:
        raise ValueError('the label map must be a C-contiguous 2-D int32 array')
    directions = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 2)
    capacity = int(max_objects)
    labels, moments = np.empty(capacity, dtype=np.int32), np.empty((capacity, 3), dtype=np.int64)
    centres, rays = np.empty((capacity, 2), dtype=np.int32), np.empty((capacity, len(directions)), dtype=np.float32)
    count = C.c_int(0)
    ctx = ctx or default_context()
    status = load_library().imsegm_object_shapes(ctx._h, _ptr(segm), segm.shape[0], segm.shape[1], _ptr(directions), len(directions),
                                                 capacity, C.byref(count), _ptr(labels), _ptr(moments), _ptr(centres), _ptr(rays))
    if status == IMSEGM_E_OBJECT_CAPS:
        return count.value, None, None, None, None
    _check(status)
    n = count.value
    return n, labels[:n], moments[:n], centres[:n], rays[:n]


#: ``IMSEGM_CUT_OBJECTS_MAX_LABELS`` / ``IMSEGM_CUT_OBJECTS_MAX_CHANNELS``
CUT_OBJECTS_MAX_LABELS, CUT_OBJECTS_MAX_CHANNELS = 1024, 4
#: ``imsegm_cut_geometry_fn``
CUT_GEOMETRY_FN = C.CFUNCTYPE(C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_double),
                              C.POINTER(C.c_int32))


def _geometry_callback(geometry, raised):
    """``geometry(moments_row, (H, W), allow_rotate)`` as an ``imsegm_cut_geometry_fn``; what it raises is kept in ``raised``"""

    def hook(user, n_labels, rotate, hook_height, hook_width, moments, geometry_out, frames_out):
        try:
            for k in range(n_labels):
                g = geometry([int(moments[10 * k + i]) for i in range(10)], (hook_height, hook_width), bool(rotate))
                row = (g['shift'][0], g['shift'][1], g['matrix'][0, 0], g['matrix'][0, 1], g['matrix'][1, 0], g['matrix'][1, 1],
                       g['offset'][0], g['offset'][1])
                for i, value in enumerate(row):
                    geometry_out[8 * k + i] = float(value)
                for i, value in enumerate(tuple(g['canvas']) + tuple(g['window'])):
                    frames_out[6 * k + i] = int(value)
            return 0
        except BaseException as ex:                    # (an exception must not cross the C frames)
            raised.append(ex)
            return 1

    return CUT_GEOMETRY_FN(hook)


def cut_objects(image, segm, labels, padding, use_mask, bg_color, allow_rotate, geometry, ctx=None):
    """``imsegm_cut_objects``: the crops of all ``labels`` (strictly ascending int32) of the C-contiguous int32 map ``segm`` [H, W] out
    of the C-contiguous uint8 ``image`` [H, W, C] in one call: (crops -- a list of uint8 arrays [h, w, C] --, moments int64 [n, 10],
    boxes int32 [n, 4] on the canvases).  ``geometry(moments_row, (H, W), allow_rotate)`` returns the dict of
    ``utilities.data_io._cut_geometry``; an exception it raises (``IndexError`` for a label without a pixel) is raised here.  A label
    whose turned mask is empty raises ``IndexError`` as well.  A request outside the caps (``IMSEGM_E_OBJECT_CAPS``) gives None --
    no error."""
    if image.dtype != np.uint8 or image.ndim != 3 or not image.flags.c_contiguous or image.size == 0:
        raise ValueError('the image must be a non-empty C-contiguous uint8 array [H, W, C]')
    if segm.dtype != np.int32 or segm.shape != image.shape[:2] or not segm.flags.c_contiguous:
        raise ValueError('the label map must be a C-contiguous int32 array of the height and width of the image')
    height, width, channels = image.shape
    labels = np.ascontiguousarray(labels, dtype=np.int32).ravel()
    n = len(labels)
    bg = np.zeros(max(channels, 1), dtype=np.uint8)
    bg[...] = bg_color
    raised = []
    moments, boxes = np.zeros((n, 10), dtype=np.int64), np.zeros((n, 4), dtype=np.int32)
    offsets, packed, first_empty = np.zeros(n + 1, dtype=np.int64), _vp(), C.c_int(-1)
    ctx = ctx or default_context()
    callback = _geometry_callback(geometry, raised)    # (alive until the call returns)
    status = load_library().imsegm_cut_objects(ctx._h, _ptr(image), _ptr(segm), height, width, channels, _ptr(labels), n, int(padding),
                                               int(bool(use_mask)), _ptr(bg), int(bool(allow_rotate)), C.cast(callback, _vp),
                                               None, _ptr(moments), _ptr(boxes), _ptr(offsets), C.byref(packed), C.byref(first_empty))
    if raised:
        raise raised[0]
    if status == IMSEGM_E_OBJECT_CAPS:
        return None
    _check(status)
    if first_empty.value >= 0:
        raise IndexError('list index out of range')         # regionprops(...)[0] of the reference on the turned mask
    crops = []
    if n:
        flat = np.ctypeslib.as_array(C.cast(packed, C.POINTER(C.c_uint8)), shape=(max(int(offsets[n]), 1), ))
        for k in range(n):
            shape = (int(boxes[k, 2] - boxes[k, 0]), int(boxes[k, 3] - boxes[k, 1]), channels)
            crops.append(flat[offsets[k]:offsets[k + 1]].reshape(shape).copy())
    return crops, moments, boxes


#: ``IMSEGM_RESIZE_MAX_RADIUS``: the largest blur radius of csrc/resize.hip (a shrink by a factor of about 33)
RESIZE_MAX_RADIUS = 64
#: ``imsegm_blur_taps_fn``
BLUR_TAPS_FN = C.CFUNCTYPE(C.c_int, _vp, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double))


def _resize_outputs(n, out_shape, channels, want_u8):
    h, w = int(out_shape[0]), int(out_shape[1])
    out = None if want_u8 else np.empty((n, h, w, channels), dtype=np.float64)
    out_u8 = np.empty((n, h, w, channels), dtype=np.uint8) if want_u8 else None
    return h, w, out, out_u8


def resize_crops(crops, out_shape, radii, weights, want_u8=False, ctx=None):
    """``imsegm_resize_crops``: the C-contiguous uint8 ``crops`` [H_i, W_i, C] (a list, one channel count) resized to ``out_shape``
    with the blur taps ``radii`` int32 [n, 2] / ``weights`` float64 [n, 2, RESIZE_MAX_RADIUS + 1] of
    ``ellipse_cut_scale.blur_taps``: (float64 [n, h, w, C], None), or with ``want_u8`` (None, the exported uint8 stack); None for
    a request outside the caps (``IMSEGM_E_OBJECT_CAPS``) -- no error"""
    n = len(crops)
    channels = crops[0].shape[2]
    for crop in crops:
        if crop.dtype != np.uint8 or crop.ndim != 3 or crop.shape[2] != channels or crop.size == 0 or not crop.flags.c_contiguous:
            raise ValueError('the crops must be non-empty C-contiguous uint8 arrays [H, W, C] of one channel count')
    sizes = np.array([crop.shape[:2] for crop in crops], dtype=np.int32)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([crop.size for crop in crops], out=offsets[1:])
    packed = np.concatenate([crop.ravel() for crop in crops])
    radii = np.ascontiguousarray(radii, dtype=np.int32)
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    if radii.shape != (n, 2) or weights.shape != (n, 2, RESIZE_MAX_RADIUS + 1):
        raise ValueError('radii [n, 2] and weights [n, 2, %d] are expected' % (RESIZE_MAX_RADIUS + 1))
    h, w, out, out_u8 = _resize_outputs(n, out_shape, channels, want_u8)
    ctx = ctx or default_context()
    status = load_library().imsegm_resize_crops(ctx._h, _ptr(packed), _ptr(offsets), _ptr(sizes), n, channels, h, w, _ptr(radii),
                                                _ptr(weights), _ptr(out), _ptr(out_u8))
    if status == IMSEGM_E_OBJECT_CAPS:
        return None
    _check(status)
    return out, out_u8


def ellipse_cut_scale(image, geom, sincos, bg_color, out_shape, geometry, taps, want_u8=True, ctx=None):
    """``imsegm_ellipse_cut_scale``: every ellipse ``geom`` int32 [n, 8] / ``sincos`` float64 [n, 2] (``ellipse_fitting.
    ellipse_geometry``) cut out of the C-contiguous uint8 ``image`` [H, W, C] under its own mask, resized to ``out_shape`` and, with
    ``want_u8``, exported: uint8 (or float64) [n, h, w, C].  ``geometry`` as in :func:`cut_objects`; ``taps(sizes)`` returns the
    (radii, weights) of ``imsegm_resize_crops`` for crops of ``sizes`` [n, 2], or None for a radius above the cap.  An ellipse
    without a pixel raises ``IndexError``.  A request outside the caps (``IMSEGM_E_OBJECT_CAPS``) gives None -- no error."""
    if image.dtype != np.uint8 or image.ndim != 3 or not image.flags.c_contiguous or image.size == 0:
        raise ValueError('the image must be a non-empty C-contiguous uint8 array [H, W, C]')
    height, width, channels = image.shape
    geom = np.ascontiguousarray(geom, dtype=np.int32).reshape(-1, 8)
    sincos = np.ascontiguousarray(sincos, dtype=np.float64).reshape(-1, 2)
    if len(geom) != len(sincos):
        raise ValueError('one (sin, cos) pair per ellipse')
    n = len(geom)
    bg = np.zeros(max(channels, 1), dtype=np.uint8)
    bg[...] = bg_color
    raised = []

    def taps_hook(user, n_crops, sizes, out_h, out_w, radii_out, weights_out):
        try:
            got = taps([(sizes[2 * k], sizes[2 * k + 1]) for k in range(n_crops)])
            if got is None:
                radii_out[0] = RESIZE_MAX_RADIUS + 1           # (the entry answers IMSEGM_E_OBJECT_CAPS)
                return 0
            C.memmove(radii_out, _ptr(np.ascontiguousarray(got[0], dtype=np.int32)), n_crops * 2 * 4)
            C.memmove(weights_out, _ptr(np.ascontiguousarray(got[1], dtype=np.float64)), n_crops * 2 * (RESIZE_MAX_RADIUS + 1) * 8)
            return 0
        except BaseException as ex:                    # (an exception must not cross the C frames)
            raised.append(ex)
            return 1

    h, w, out, out_u8 = _resize_outputs(n, out_shape, channels, want_u8)
    first_empty = C.c_int(-1)
    ctx = ctx or default_context()
    geometry_cb, taps_cb = _geometry_callback(geometry, raised), BLUR_TAPS_FN(taps_hook)       # (alive until the call returns)
    status = load_library().imsegm_ellipse_cut_scale(ctx._h, _ptr(image), height, width, channels, n, _ptr(geom), _ptr(sincos), _ptr(bg),
                                                     h, w, C.cast(geometry_cb, _vp), C.cast(taps_cb, _vp), None, _ptr(out),
                                                     _ptr(out_u8), C.byref(first_empty))
    if raised:
        raise raised[0]
    if status == IMSEGM_E_OBJECT_CAPS:
        return None
    _check(status)
    if first_empty.value >= 0:
        raise IndexError('list index out of range')         # regionprops(...)[0] of the reference on the turned mask
    return out_u8 if want_u8 else out


#: ``IMSEGM_CENTER_ANNOT_MAX_LABELS`` / ``IMSEGM_CENTER_ANNOT_MAX_LEVELS``
CENTER_ANNOT_MAX_LABELS, CENTER_ANNOT_MAX_LEVELS = 1024, 8


def _egg_map(img):
    if img.ndim != 2 or img.dtype not in (np.uint8, np.int32) or not img.flags.c_contiguous or img.size == 0:
        raise ValueError('the egg map must be a non-empty C-contiguous 2-D uint8 or int32 array')
    return int(img.dtype == np.int32)


def correct_segm(img, sel_radius, min_size, ctx=None):
    """``imsegm_correct_segm`` on a C-contiguous 2-D uint8 or int32 map: (seg uint8 H x W, labels int32 H x W, number of labels), or
    None for a map outside the caps (``IMSEGM_E_OBJECT_CAPS``) -- no error"""
    is_i32 = _egg_map(img)
    seg, labels, n_labels = np.empty(img.shape, dtype=np.uint8), np.empty(img.shape, dtype=np.int32), C.c_int(0)
    ctx = ctx or default_context()
    status = load_library().imsegm_correct_segm(ctx._h, _ptr(img), is_i32, img.shape[0], img.shape[1], int(sel_radius),
                                                int(np.clip(min_size, -2 ** 31, 2 ** 31 - 1)), _ptr(seg), _ptr(labels), C.byref(n_labels))
    if status == IMSEGM_E_OBJECT_CAPS:
        return None
    _check(status)
    return seg, labels, n_labels.value


def center_levels(labels, max_label, levels, ctx=None):
    """``imsegm_center_levels`` on a 2-D integer label map whose largest value is ``max_label`` (1 .. CENTER_ANNOT_MAX_LABELS):
    (level map uint8 H x W -- None without levels --, counts int64 [max_label], centres float64 [max_label, 2] as (X, Y), rows of the
    labels 1 .. max_label), or None for a request outside the caps (``IMSEGM_E_OBJECT_CAPS``) -- no error"""
    if labels.ndim != 2 or labels.size == 0:
        raise ValueError('the label map must be a non-empty 2-D array')
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    levels = np.ascontiguousarray(levels, dtype=np.float64).ravel()
    max_label = int(max_label)
    out = np.empty(labels.shape, dtype=np.uint8) if len(levels) else None
    counts, centres = np.zeros(max_label + 1, dtype=np.int64), np.zeros((max_label + 1, 2), dtype=np.float64)
    ctx = ctx or default_context()
    status = load_library().imsegm_center_levels(ctx._h, _ptr(labels), labels.shape[0], labels.shape[1], max_label, _ptr(levels),
                                                 len(levels), _ptr(out), _ptr(counts), _ptr(centres))
    if status == IMSEGM_E_OBJECT_CAPS:
        return None
    _check(status)
    return out, counts[1:], centres[1:]


def center_distances(labels, max_label, ctx=None):
    """diagnostic (``imsegm_debug_center_distances``; tests): what ``imsegm_center_levels`` holds in front of its code pass -- (d2 uint32
    H x W, max2 uint32 [max_label], sums int64 [max_label, 3] = pixel count, row sum, column sum; rows of the labels 1 .. max_label),
    or None for a request outside the caps"""
    if labels.ndim != 2 or labels.size == 0:
        raise ValueError('the label map must be a non-empty 2-D array')
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    max_label = int(max_label)
    d2 = np.empty(labels.shape, dtype=np.uint32)
    max2, sums = np.zeros(max_label + 1, dtype=np.uint32), np.zeros((max_label + 1, 3), dtype=np.int64)
    ctx = ctx or default_context()
    status = load_library().imsegm_debug_center_distances(ctx._h, _ptr(labels), labels.shape[0], labels.shape[1], max_label, _ptr(d2),
                                                          _ptr(max2), _ptr(sums))
    if status == IMSEGM_E_OBJECT_CAPS:
        return None
    _check(status)
    return d2, max2[1:], sums[1:]


def create_annot_centers(img, sel_radius, min_size, levels, ctx=None):
    """``imsegm_create_annot_centers`` on a C-contiguous 2-D uint8 or int32 map: (level map uint8 H x W, counts int64 [n], centres
    float64 [n, 2] as (X, Y)) of the n labels, or None for a request outside the caps (``IMSEGM_E_OBJECT_CAPS``) -- no error"""
    is_i32 = _egg_map(img)
    levels = np.ascontiguousarray(levels, dtype=np.float64).ravel()
    out, n_labels = np.empty(img.shape, dtype=np.uint8), C.c_int(0)
    counts = np.zeros(CENTER_ANNOT_MAX_LABELS + 1, dtype=np.int64)
    centres = np.zeros((CENTER_ANNOT_MAX_LABELS + 1, 2), dtype=np.float64)
    ctx = ctx or default_context()
    status = load_library().imsegm_create_annot_centers(ctx._h, _ptr(img), is_i32, img.shape[0], img.shape[1], int(sel_radius),
                                                        int(np.clip(min_size, -2 ** 31, 2 ** 31 - 1)), _ptr(levels), len(levels), _ptr(out),
                                                        C.byref(n_labels), _ptr(counts), _ptr(centres))
    if status == IMSEGM_E_OBJECT_CAPS:
        return None
    _check(status)
    n = n_labels.value
    return out, counts[1:n + 1], centres[1:n + 1]


#: ``IMSEGM_WATERSHED_MAX_LABELS``
WATERSHED_MAX_LABELS = 1024


def _mask_bytes(mask):
    if mask.ndim != 2 or mask.size == 0:
        raise ValueError('the mask must be a non-empty 2-D array')
    return np.ascontiguousarray(mask != 0).view(np.uint8)


def watershed_markers(mask, seed_pixels, seed_labels, keys=None, ctx=None):
    """``imsegm_watershed_markers`` on a 2-D mask, the (pixel index, label) pairs of its markers (distinct pixels) and int32 keys of
    the mask's shape (None: minus the squared distances to the background): the flooded map int32 H x W, or None for a request
    outside the caps (``IMSEGM_E_OBJECT_CAPS``) -- no error"""
    mask = _mask_bytes(mask)
    seed_pixels = np.ascontiguousarray(seed_pixels, dtype=np.int32).ravel()
    seed_labels = np.ascontiguousarray(seed_labels, dtype=np.int32).ravel()
    if len(seed_pixels) != len(seed_labels):
        raise ValueError('one label per seed')
    if keys is not None:
        keys = np.ascontiguousarray(keys, dtype=np.int32)
        if keys.shape != mask.shape:
            raise ValueError('mask and keys differ in shape')
    out = np.empty(mask.shape, dtype=np.int32)
    ctx = ctx or default_context()
    status = load_library().imsegm_watershed_markers(ctx._h, _ptr(mask), mask.shape[0], mask.shape[1], _ptr(keys), _ptr(seed_pixels),
                                                     _ptr(seed_labels), len(seed_pixels), _ptr(out))
    if status == IMSEGM_E_OBJECT_CAPS:
        return None
    _check(status)
    return out


def watershed_post_morph(segm, radius_close, radius_open, ctx=None):
    """``imsegm_watershed_post_morph`` on a 2-D integer label map: the cleaned map int32 H x W, or None for a request outside the
    caps (``IMSEGM_E_OBJECT_CAPS``) -- no error"""
    if segm.ndim != 2 or segm.size == 0:
        raise ValueError('the label map must be a non-empty 2-D array')
    top = int(segm.max())
    if top > WATERSHED_MAX_LABELS:
        return None
    segm = np.ascontiguousarray(segm, dtype=np.int32)
    out = np.empty(segm.shape, dtype=np.int32)
    ctx = ctx or default_context()
    status = load_library().imsegm_watershed_post_morph(ctx._h, _ptr(segm), segm.shape[0], segm.shape[1], max(top, 0), int(radius_close),
                                                        int(radius_open), _ptr(out))
    if status == IMSEGM_E_OBJECT_CAPS:
        return None
    _check(status)
    return out


def watershed(seg_binary, centres, post_morph, radii=None, ctx=None):
    """``imsegm_watershed`` on the 2-D boolean map ``seg > 0`` and the centres as int32 (row, column) rows inside the map, centre
    ``i`` for label ``i + 1``: the segmentation int32 H x W, or None for a request outside the caps (``IMSEGM_E_OBJECT_CAPS``) --
    no error"""
    seg = _mask_bytes(seg_binary)
    centres = np.ascontiguousarray(centres, dtype=np.int32).reshape(-1, 2)
    n = len(centres)
    radii = None if radii is None else np.ascontiguousarray(radii, dtype=np.int32)
    out = np.empty(seg.shape, dtype=np.int32)
    ctx = ctx or default_context()
    status = load_library().imsegm_watershed(ctx._h, _ptr(seg), seg.shape[0], seg.shape[1], _ptr(centres), n, int(bool(post_morph)),
                                             _ptr(radii), _ptr(out))
    if status == IMSEGM_E_OBJECT_CAPS:
        return None
    _check(status)
    return out


#: ``IMSEGM_ORIENT_MAX_IMAGES`` / ``IMSEGM_ORIENT_SUM_WORDS``
ORIENT_MAX_IMAGES, ORIENT_SUM_WORDS = 65535, 9
#: modes of ``imsegm_orient_stack``
ORIENT_MODES = {'cc': 0, 'density': 1}


def _orient_stack(stack, channel):
    if stack.dtype != np.uint8 or stack.ndim != 4 or stack.size == 0 or not stack.flags.c_contiguous:
        raise ValueError('the stack must be a non-empty C-contiguous uint8 array [N, h, w, C]')
    if not 0 <= int(channel) < stack.shape[3]:
        raise ValueError('channel %r of %d' % (channel, stack.shape[3]))
    return stack


def stack_median(stack, channel=0, ctx=None):
    """``imsegm_stack_median_u8`` on a C-contiguous uint8 stack [N, h, w, C]: twice the per-pixel median of ``stack[..., channel]``
    over the N images as uint16 [h, w], or None for a stack outside the caps (``IMSEGM_E_OBJECT_CAPS``) -- no error"""
    stack = _orient_stack(stack, channel)
    n, h, w, c = stack.shape
    out = np.empty((h, w), dtype=np.uint16)
    ctx = ctx or default_context()
    status = load_library().imsegm_stack_median_u8(ctx._h, _ptr(stack), n, h, w, c, int(channel), _ptr(out))
    if status == IMSEGM_E_OBJECT_CAPS:
        return None
    _check(status)
    return out


def orient_stack(stack, channel=0, mode='cc', template2=None, ctx=None, in_place=False):
    """``imsegm_orient_stack`` on a C-contiguous uint8 stack [N, h, w, C]; ``mode`` 'cc' or 'density'; ``template2``: twice the
    template as integers 0 .. 510 [h, w], or None for the median of the stack.  Returns (template2 uint16 [h, w], flags bool [N],
    sums int64 [N, 9], the stack with the flagged images turned by 180 degrees -- a new array, or ``stack`` itself with
    ``in_place``), or None for a stack outside the caps
    (``IMSEGM_E_OBJECT_CAPS``) -- no error"""
    stack = _orient_stack(stack, channel)
    n, h, w, c = stack.shape
    if template2 is not None:
        template2 = np.ascontiguousarray(template2, dtype=np.uint16)
        if template2.shape != (h, w):
            raise ValueError('template2 %r and the images %r differ in size' % (template2.shape, (h, w)))
    out = np.empty((h, w), dtype=np.uint16)
    flags = np.empty(n, dtype=np.uint8)
    sums = np.empty((n, ORIENT_SUM_WORDS), dtype=np.int64)
    turned = stack if in_place else np.empty_like(stack)
    ctx = ctx or default_context()
    status = load_library().imsegm_orient_stack(ctx._h, _ptr(stack), n, h, w, c, int(channel), ORIENT_MODES[mode], _ptr(template2),
                                                _ptr(out), _ptr(flags), _ptr(sums), _ptr(turned))
    if status == IMSEGM_E_OBJECT_CAPS:
        return None
    _check(status)
    return out, flags != 0, sums, turned


#: ``IMSEGM_DBSCAN_MAX_POINTS`` / ``IMSEGM_DBSCAN_MAX_SETS`` / ``IMSEGM_DBSCAN_MAX_TOTAL``
DBSCAN_MAX_POINTS, DBSCAN_MAX_SETS, DBSCAN_MAX_TOTAL = 4096, 4096, 1 << 20


def dbscan_points(points_concat, offsets, eps, min_samples, ctx=None, out=None):
    """``imsegm_dbscan_points``: DBSCAN of the sets ``offsets`` (int32 [S + 1], not descending) cuts out of the C-contiguous float64
    rows ``points_concat`` [P, 2] as (row, col): (labels int32 [P], cluster counts int32 [S], centres float64 [P, 2] -- row
    ``offsets[s] + c`` is the centre of cluster c of set s, the other rows are 0).  ``out``: the three arrays to write into.  A
    request outside the caps (``IMSEGM_E_OBJECT_CAPS``) gives None -- no error; what scikit-learn refuses raises
    :class:`HipClusterInputError`, a ``ValueError``, and leaves ``out`` as it came."""
    if points_concat.dtype != np.float64 or points_concat.ndim != 2 or points_concat.shape[1] != 2 or not points_concat.flags.c_contiguous:
        raise ValueError('the points must be a C-contiguous float64 array [P, 2]')
    offsets = np.ascontiguousarray(offsets, dtype=np.int32).ravel()
    nb_sets = len(offsets) - 1
    if nb_sets < 0 or (nb_sets and int(offsets[-1]) > len(points_concat)):
        raise ValueError('dbscan_points: the offsets must span the point list')
    total = len(points_concat)
    if out is None:
        out = np.zeros(total, dtype=np.int32), np.zeros(nb_sets, dtype=np.int32), np.zeros((total, 2), dtype=np.float64)
    labels, counts, centres = out
    if (labels.dtype != np.int32 or counts.dtype != np.int32 or centres.dtype != np.float64 or labels.shape != (total, )
            or counts.shape != (nb_sets, ) or centres.shape != (total, 2)
            or not (labels.flags.c_contiguous and counts.flags.c_contiguous and centres.flags.c_contiguous)):
        raise ValueError('out: int32 [P], int32 [S] and float64 [P, 2], C-contiguous')
    ctx = ctx or default_context()
    status = load_library().imsegm_dbscan_points(ctx._h, _ptr(points_concat), _ptr(offsets), nb_sets, float(eps),
                                                 int(np.clip(min_samples, -2 ** 31, 2 ** 31 - 1)), _ptr(labels), _ptr(counts), _ptr(centres))
    if status == IMSEGM_E_OBJECT_CAPS:
        return None
    _check(status)
    return labels, counts, centres


#: ``IMSEGM_ANNOT_MAX_COLORS``: entries of a colour table of the ``imsegm_annot_*`` calls
ANNOT_MAX_COLORS = 256
#: modes of ``imsegm_annot_match``
ANNOT_MATCH_EXACT, ANNOT_MATCH_NEAREST, ANNOT_MATCH_NEAREST_COLOR = 0, 1, 2


def _annot_image(image):
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3 or not image.flags.c_contiguous or image.size == 0:
        raise ValueError('the image must be a non-empty C-contiguous uint8 array [H, W, 3]')
    return image


def _annot_colors(colors):
    colors = np.ascontiguousarray(colors, dtype=np.uint8).reshape(-1, 3)
    if not 1 <= len(colors) <= ANNOT_MAX_COLORS:
        raise ValueError('a colour table holds 1 to %i colours' % ANNOT_MAX_COLORS)
    return colors


def annot_match(image, colors, labels=None, mode=ANNOT_MATCH_EXACT, ctx=None):
    """``imsegm_annot_match`` on a uint8 image [H, W, 3] and a table of colours uint8 [K, 3].  Exact: (int32 [H, W] with ``labels[k]``
    -- none negative, default k -- of the last colour the pixel equals and -1 for none, number of such pixels); nearest: the index of
    the first colour at the smallest L1 distance, int32 [H, W]; nearest colour: that colour, uint8 [H, W, 3]"""
    image, colors = _annot_image(image), _annot_colors(colors)
    if labels is not None:
        labels = np.ascontiguousarray(labels, dtype=np.int32).ravel()
        if len(labels) != len(colors):
            raise ValueError('one label per colour')
    out = np.empty(image.shape if mode == ANNOT_MATCH_NEAREST_COLOR else image.shape[:2], dtype=np.uint8 if mode == ANNOT_MATCH_NEAREST_COLOR else np.int32)
    unmatched = C.c_int64(0)
    ctx = ctx or default_context()
    _check(load_library().imsegm_annot_match(ctx._h, _ptr(image), image.shape[0] * image.shape[1], _ptr(colors), _ptr(labels), len(colors),
                                             int(mode), _ptr(out), C.byref(unmatched)))
    return (out, int(unmatched.value)) if mode == ANNOT_MATCH_EXACT else out


def annot_paint(labels, min_label, table, present=None, out=None, ctx=None):
    """``imsegm_annot_paint``: the C-contiguous int32 map ``labels`` through the colours ``table`` uint8 [T, 3] of the labels
    ``min_label .. min_label + T - 1`` (``present`` uint8 [T]: 0 marks a label without a colour): uint8 labels.shape + (3,).  A label of
    the map without a colour raises ``HipError`` and leaves ``out`` as it came."""
    if labels.dtype != np.int32 or not labels.flags.c_contiguous or labels.size == 0:
        raise ValueError('the label map must be a non-empty C-contiguous int32 array')
    table = _annot_colors(table)
    present = np.ones(len(table), dtype=np.uint8) if present is None else np.ascontiguousarray(present, dtype=np.uint8).ravel()
    if len(present) != len(table):
        raise ValueError('one present flag per colour')
    if out is None:
        out = np.empty(labels.shape + (3, ), dtype=np.uint8)
    elif out.dtype != np.uint8 or out.shape != labels.shape + (3, ) or not out.flags.c_contiguous:
        raise ValueError('out must be a C-contiguous uint8 array of the shape of the map + (3,)')
    ctx = ctx or default_context()
    _check(load_library().imsegm_annot_paint(ctx._h, _ptr(labels), labels.size, int(min_label), len(table), _ptr(table), _ptr(present),
                                             _ptr(out)))
    return out


def annot_color_hist(image, capacity=None, ctx=None):
    """``imsegm_annot_color_hist``: (keys uint32 [n] ascending, ``r << 16 | g << 8 | b``; counts uint32 [n]) of the distinct colours of
    a uint8 image [H, W, 3] in one call: the result arrays have room for ``capacity`` colours, by default for as many as the image
    can hold (one per pixel, 2^24 at the most; pages nothing is written to cost nothing).  An image with more colours than an
    explicit ``capacity`` raises ``ValueError``."""
    image = _annot_image(image)
    ctx = ctx or default_context()
    n_pixels, n = image.shape[0] * image.shape[1], C.c_int(0)
    if capacity is None:
        capacity = min(n_pixels, 1 << 24)
    keys, counts = np.empty(capacity, dtype=np.uint32), np.empty(capacity, dtype=np.uint32)
    _check(load_library().imsegm_annot_color_hist(ctx._h, _ptr(image), n_pixels, int(capacity), C.byref(n), _ptr(keys), _ptr(counts)))
    if n.value > capacity:
        raise ValueError('the image holds %i colours, more than the %i asked for' % (n.value, capacity))
    return keys[:n.value].copy(), counts[:n.value].copy()


def annot_nearest_valid(labels, out=None, ctx=None):
    """``imsegm_annot_nearest_valid``: the C-contiguous 2-D int32 map with every pixel equal to -1 given the label of the nearest
    other pixel (squared Euclidean distance, the smallest row-major index among equals).  A map without such a pixel raises
    ``HipError`` and leaves ``out`` as it came."""
    if labels.ndim != 2 or labels.dtype != np.int32 or not labels.flags.c_contiguous or labels.size == 0:
        raise ValueError('the label map must be a non-empty C-contiguous 2-D int32 array')
    if out is None:
        out = np.empty_like(labels)
    elif out.dtype != np.int32 or out.shape != labels.shape or not out.flags.c_contiguous:
        raise ValueError('out must be a C-contiguous int32 array of the shape of the map')
    ctx = ctx or default_context()
    _check(load_library().imsegm_annot_nearest_valid(ctx._h, _ptr(labels), labels.shape[0], labels.shape[1], _ptr(out)))
    return out


def annot_quantize_nearest_pixel(image, colors, ctx=None):
    """``imsegm_annot_quantize_nearest_pixel``: every pixel of the uint8 image [H, W, 3] replaced by the colour of the nearest pixel
    that has exactly one of ``colors`` uint8 [K, 3] (itself when it has one): uint8 [H, W, 3]"""
    image, colors = _annot_image(image), _annot_colors(colors)
    out = np.empty_like(image)
    ctx = ctx or default_context()
    _check(load_library().imsegm_annot_quantize_nearest_pixel(ctx._h, _ptr(image), image.shape[0], image.shape[1], _ptr(colors), len(colors),
                                                              _ptr(out)))
    return out


#: ``IMSEGM_SCORE_*`` of include/imsegm_hip.h: the label cap of ``imsegm_score_pairs``, the length of its drop list and the geometry of
#: its pixel kernels (lanes of a workgroup, pixels a lane loads per step, steps of a workgroup, last label count with per-wave tables)
SCORE_MAX_LABELS, SCORE_MAX_DROP = 64, 64
SCORE_THREADS, SCORE_RUN, SCORE_CHUNK_STEPS, SCORE_WAVE_TABLE_LABELS = 256, 8, 4, 32
#: pixels of a pair one workgroup owns
SCORE_CHUNK_PIXELS = SCORE_THREADS * SCORE_RUN * SCORE_CHUNK_STEPS
#: what ``score_pairs`` returns in place of ``(labels, table)`` for a pair with more than ``SCORE_MAX_LABELS`` labels
SCORE_TOO_MANY_LABELS = 'too many labels'
#: bytes of maps ``score_pairs`` sends up in one call of ``imsegm_score_pairs``; a longer batch is split between pairs (a single
#: pair above the budget still goes in a call of its own).  1 GiB holds sixteen 4096 x 4096 int32 pairs and keeps the context's scratch,
#: which never shrinks, at a size that leaves the rest of the device's memory to the sessions.
SCORE_BATCH_BYTES = 1 << 30
_SCORE_DTYPES = {np.dtype(np.int32): 0, np.dtype(np.uint8): 1}


def _score_call(annots, segms, dtype, drop, ctx):
    count = len(annots)
    pointers = (_vp * count)(*[_ptr(arr) for arr in annots]), (_vp * count)(*[_ptr(arr) for arr in segms])
    sizes = np.array([arr.size for arr in annots], dtype=np.int64)
    status, n_labels = np.zeros(count, dtype=np.int32), np.zeros(count, dtype=np.int32)
    labels = np.empty((count, SCORE_MAX_LABELS), dtype=np.int32)
    tables = np.empty((count, SCORE_MAX_LABELS * SCORE_MAX_LABELS), dtype=np.int64)
    _check(load_library().imsegm_score_pairs(ctx._h, count, pointers[0], pointers[1], _ptr(sizes), _SCORE_DTYPES[dtype], _ptr(drop), len(drop),
                                             _ptr(status), _ptr(n_labels), _ptr(labels), _ptr(tables)))
    results = []
    for i in range(count):
        if status[i] != 0:
            results.append(SCORE_TOO_MANY_LABELS)
            continue
        used = int(n_labels[i])
        results.append((labels[i, :used].copy(), tables[i, :used * used].reshape(used, used).copy()))
    return results


def score_pairs(annots, segms, drop_labels=None, ctx=None):
    """``imsegm_score_pairs``: per pair of equally sized arrays ``(labels int32 [U] ascending, table int64 [U, U])`` -- the distinct
    values of both arrays over the elements where neither carries one of ``drop_labels``, and ``table[a, b]`` = number of those elements
    with ``annot == labels[a]`` and ``segm == labels[b]`` -- or ``SCORE_TOO_MANY_LABELS`` for a pair with more than ``SCORE_MAX_LABELS``
    of them.  All arrays are C-contiguous and of ONE dtype, int32 or uint8; empty pairs give U = 0.  Batches above
    ``SCORE_BATCH_BYTES`` go up in several calls."""
    annots, segms = list(annots), list(segms)
    if len(annots) != len(segms):
        raise ValueError('one segmentation per annotation')
    drop = np.ascontiguousarray([] if drop_labels is None else drop_labels, dtype=np.int32).ravel()
    if len(drop) > SCORE_MAX_DROP:
        raise ValueError('a drop list holds at most %i labels' % SCORE_MAX_DROP)
    if not annots:
        return []
    dtype = annots[0].dtype
    if dtype not in _SCORE_DTYPES:
        raise ValueError('the arrays must be int32 or uint8')
    for annot, segm in zip(annots, segms):
        for arr in (annot, segm):
            if not isinstance(arr, np.ndarray) or arr.dtype != dtype or not arr.flags.c_contiguous:
                raise ValueError('the arrays must be C-contiguous and of one dtype, int32 or uint8')
        if annot.size != segm.size:
            raise ValueError('the arrays of a pair must have one size')
    ctx = ctx or default_context()
    results, first, held = [], 0, 0
    for i in range(len(annots) + 1):
        here = 2 * annots[i].nbytes if i < len(annots) else 0
        if i == len(annots) or (i > first and held + here > SCORE_BATCH_BYTES):
            results += _score_call(annots[first:i], segms[first:i], dtype, drop, ctx)
            first, held = i, 0
        held += here
    return results


def ray_features_binary2d(seg_binary, positions, directions, edge, ctx=None):
    """``computeRayFeaturesBinary2d`` for a batch of positions (``imsegm_ray_features_binary2d``): float32 [P, A]"""
    ctx = ctx or default_context()
    seg = np.ascontiguousarray(seg_binary, dtype=np.int8)
    positions = np.ascontiguousarray(positions, dtype=np.int32).reshape(-1, 2)
    directions = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 2)
    out = np.empty((len(positions), len(directions)), dtype=np.float32)
    _check(load_library().imsegm_ray_features_binary2d(ctx._h, _ptr(seg), seg.shape[0], seg.shape[1], _ptr(positions), len(positions),
                                                       _ptr(directions), len(directions), int(edge), _ptr(out)))
    return out


#: LDS budgets of the ring kernels (``IMSEGM_RING_MAX_BINS`` / ``IMSEGM_RING_PROBA_MAX_DISCS`` of include/imsegm_hip.h)
RING_MAX_BINS, RING_PROBA_MAX_DISCS = 32, 16
#: ``IMSEGM_RAY_MAX_ANGLES`` / ``IMSEGM_RAY_MAX_BORDER_LABELS``
RAY_MAX_ANGLES, RAY_MAX_BORDER_LABELS = 4096, 64


def ring_hist2d(segm, positions, radii, nb_labels, ctx=None):
    """label histograms under concentric discs for a batch of positions (``imsegm_ring_hist2d``; radii grow strictly):
    uint32 hist [P, D, nb_labels] and the sizes of the clipped discs, uint32 [P, D]; no position: empty tables, no launch"""
    positions = np.ascontiguousarray(positions, dtype=np.int32).reshape(-1, 2)
    radii = np.ascontiguousarray(radii, dtype=np.int32).ravel()
    hist = np.zeros((len(positions), len(radii), int(nb_labels)), dtype=np.uint32)
    size = np.zeros((len(positions), len(radii)), dtype=np.uint32)
    if len(positions) == 0:
        return hist, size
    ctx = ctx or default_context()
    segm = np.ascontiguousarray(segm, dtype=np.int16)
    _check(load_library().imsegm_ring_hist2d(ctx._h, _ptr(segm), segm.shape[0], segm.shape[1], _ptr(positions), len(positions),
                                             _ptr(radii), len(radii), int(nb_labels), _ptr(hist), _ptr(size)))
    return hist, size


def ring_hist_proba2d(proba, positions, radii, ctx=None):
    """sums of the layers of ``proba`` (H x W x C) under concentric discs for a batch of positions (``imsegm_ring_hist_proba2d``):
    float64 [P, D, C] and the sizes of the clipped discs, uint32 [P, D]; no position: empty tables, no launch"""
    proba = np.ascontiguousarray(proba, dtype=np.float64)
    positions = np.ascontiguousarray(positions, dtype=np.int32).reshape(-1, 2)
    radii = np.ascontiguousarray(radii, dtype=np.int32).ravel()
    total = np.zeros((len(positions), len(radii), proba.shape[2]), dtype=np.float64)
    size = np.zeros((len(positions), len(radii)), dtype=np.uint32)
    if len(positions) == 0:
        return total, size
    ctx = ctx or default_context()
    _check(load_library().imsegm_ring_hist_proba2d(ctx._h, _ptr(proba), proba.shape[0], proba.shape[1], proba.shape[2], _ptr(positions),
                                                   len(positions), _ptr(radii), len(radii), _ptr(total), _ptr(size)))
    return total, size


def ray_features_labels2d(segm, border_labels, positions, directions, edge, smooth_taps=None, ctx=None):
    """ray features of a batch of positions against the mask ``segm in border_labels``, optionally smoothed along the angle with
    the half kernel ``smooth_taps`` of :func:`gaussian_taps` (``imsegm_ray_features_labels2d``): float32 [P, A]"""
    positions = np.ascontiguousarray(positions, dtype=np.int32).reshape(-1, 2)
    directions = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 2)
    out = np.empty((len(positions), len(directions)), dtype=np.float32)
    if len(positions) == 0:
        return out
    ctx = ctx or default_context()
    segm = np.ascontiguousarray(segm, dtype=np.int32)
    border = np.ascontiguousarray(border_labels, dtype=np.int32).ravel()
    taps = None if smooth_taps is None else np.ascontiguousarray(smooth_taps, dtype=np.float64)
    _check(load_library().imsegm_ray_features_labels2d(ctx._h, _ptr(segm), segm.shape[0], segm.shape[1], _ptr(border), len(border),
                                                       _ptr(positions), len(positions), _ptr(directions), len(directions), int(edge),
                                                       _ptr(taps), 0 if taps is None else len(taps) - 1, _ptr(out)))
    return out


class RegionGrowing(object):
    """resident state of one region growing on a label session (``imsegm_rg_*``, csrc/region_growing.hip): the label map of
    ``sess`` with the ``edges`` its :meth:`Image2D.graph` returned, for ``n_objects`` objects.  The session must keep its label map
    while the state is open."""

    def __init__(self, sess, edges, n_objects):
        self.sess, self.n_objects, self.n_labels = sess, int(n_objects), int(sess.n_labels)
        edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
        self._h = _vp()
        _check(load_library().imsegm_rg_open(sess._h, _ptr(edges), len(edges), self.n_objects, C.byref(self._h)))
        size = max(self.n_objects * self.n_labels, 1)
        self._cand = (np.empty(size, dtype=np.int32), np.empty(size, dtype=np.int32), np.empty(size, dtype=np.float64))

    def close(self):
        # (the state frees its own buffers without reading the session: either may be closed first)
        if self._h:
            load_library().imsegm_rg_close(self._h)
        self._h = None

    def _handle(self):
        if not self._h or not self.sess._h:
            raise HipError('the region-growing state or its label session is closed')
        return self._h

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _get(self, what, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        _check(load_library().imsegm_rg_get(self._handle(), what, _ptr(out)))
        return out

    def sums(self):
        """int64 [K, 3]: pixel count, row sum and column sum of every superpixel"""
        return self._get(0, (self.n_labels, 3), np.int64)

    def points(self):
        """int32 [K, 2]: ``np.round(superpixel_centers(slic)).astype(int)``"""
        return self._get(1, (self.n_labels, 2), np.int32)

    def shape_costs(self):
        """float64 [K, n_objects + 1]: the resident ``lut_shape_cost``"""
        return self._get(2, (self.n_labels, self.n_objects + 1), np.float64)

    def set_costs(self, lut_data=None, lut_shape=None):
        tables = []
        for table in (lut_data, lut_shape):
            if table is not None:
                table = np.ascontiguousarray(table, dtype=np.float64)
                if table.shape != (self.n_labels, self.n_objects + 1):
                    raise ValueError('cost table %r, expected %r' % (table.shape, (self.n_labels, self.n_objects + 1)))
            tables.append(table)
        _check(load_library().imsegm_rg_set_costs(self._handle(), _ptr(tables[0]), _ptr(tables[1])))

    def _labels(self, labels):
        if labels is None:
            return None
        labels = np.ascontiguousarray(labels, dtype=np.int32).ravel()
        if len(labels) != self.n_labels:
            raise ValueError('%d labels for %d superpixels' % (len(labels), self.n_labels))
        return labels

    @staticmethod
    def _coefs(coef_data, coef_shape, coef_pairwise, pen_bg, pen_fg):
        return np.array([coef_data, coef_shape, coef_pairwise, pen_bg, pen_fg], dtype=np.float64)

    def update_shape_costs(self, objects, centres, shifts, tables, with_proba=False):
        """``lut_shape_cost[:, objects[j] + 1]`` from table ``tables[j]`` (float64 A_j x D_j) around ``centres[j]`` turned by
        ``shifts[j]``; with_proba: returns the priors float64 [len(objects), K]"""
        objects = np.ascontiguousarray(objects, dtype=np.int32).ravel()
        if len(objects) == 0:
            return np.empty((0, self.n_labels)) if with_proba else None
        centres = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1, 2)
        shifts = np.ascontiguousarray(shifts, dtype=np.float64).ravel()
        tables = [np.ascontiguousarray(t, dtype=np.float64) for t in tables]
        if not len(objects) == len(centres) == len(shifts) == len(tables) or any(t.ndim != 2 for t in tables):
            raise ValueError('one centre, one shift and one 2-D table per object')
        dims = np.array([t.shape for t in tables], dtype=np.int32)
        flat = np.concatenate([t.ravel() for t in tables])
        proba = np.empty((len(objects), self.n_labels), dtype=np.float64) if with_proba else None
        _check(load_library().imsegm_rg_shape_costs(self._handle(), len(objects), _ptr(objects), _ptr(centres), _ptr(shifts), _ptr(dims),
                                                    _ptr(flat), _ptr(proba)))
        return proba

    def object_rays(self, labels, positions, directions):
        """'down' ray distances float32 [n_objects, A] of every object's mask ``labels[slic] == i + 1`` from ``positions``"""
        labels = self._labels(labels)
        positions = np.ascontiguousarray(positions, dtype=np.int32).reshape(-1, 2)
        directions = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 2)
        if len(positions) != self.n_objects:
            raise ValueError('one position per object')
        out = np.empty((self.n_objects, len(directions)), dtype=np.float32)
        _check(load_library().imsegm_rg_object_shapes(self._handle(), _ptr(labels), _ptr(positions), _ptr(directions), len(directions), _ptr(out)))
        return out

    def greedy_step(self, labels, allow_obj_swap, coef_data, coef_shape, coef_pairwise, pen_bg, pen_fg, with_scores=True):
        """(objects int32, superpixels int32, changes float64 or None) of the candidates of ``labels``"""
        labels = self._labels(labels)
        coefs = self._coefs(coef_data, coef_shape, coef_pairwise, pen_bg, pen_fg)
        count = C.c_int(0)
        objs, sps, changes = self._cand
        _check(load_library().imsegm_rg_greedy_step(self._handle(), _ptr(labels), int(bool(allow_obj_swap)), _ptr(coefs), C.byref(count),
                                                    _ptr(objs), _ptr(sps), _ptr(changes) if with_scores else None))
        n = count.value
        return objs[:n].copy(), sps[:n].copy(), changes[:n].copy() if with_scores else None

    def criterion(self, labels, coef_data, coef_shape, coef_pairwise, pen_bg, pen_fg):
        labels = self._labels(labels)
        coefs = self._coefs(coef_data, coef_shape, coef_pairwise, pen_bg, pen_fg)
        out = np.empty(1, dtype=np.float64)
        _check(load_library().imsegm_rg_criterion(self._handle(), _ptr(labels), _ptr(coefs), _ptr(out)))
        return float(out[0])
