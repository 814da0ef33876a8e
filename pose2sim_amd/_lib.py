"""ctypes binding of the C-ABI in include/p2s.h, include/p2s_floor.h and include/p2s_tri_frames.h (csrc/libp2s_hip.so).

The library is the only compute path: there is no CPU fallback.  ``load()`` raises if the shared
object is missing; ``Context()`` raises if no MI355X is visible.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('P2S_LIB') or os.path.join(_HERE, 'csrc', 'libp2s_hip.so')   # P2S_LIB: kernel experiments only

P2S_F32, P2S_F64 = 0, 1
P2S_MAX_CAMS = 32
P2S_MAX_PERSONS_TOTAL = 48
P2S_MAX_PERSONS_PER_CAM = 16
P2S_MAX_COMBINATIONS = 1 << 20
P2S_JSON_UNREADABLE, P2S_JSON_NO_PEOPLE_LIST = -1, -2
P2S_ERR_INVALID_ARG = -1
P2S_ERR_GCV_SHORT_RUN, P2S_ERR_GCV_ILL_POSED, P2S_ERR_GCV_NO_MINIMUM, P2S_ERR_GCV_SINGULAR = -6, -7, -8, -9
P2S_JSON_PERSON_NO_LIST, P2S_JSON_PERSON_NOT_NUMERIC = -1, -2
P2S_JSON_DOC_UNREADABLE, P2S_JSON_DOC_PEOPLE, P2S_JSON_DOC_NO_PEOPLE_KEY, P2S_JSON_DOC_PEOPLE_NULL, P2S_JSON_DOC_PEOPLE_OTHER = -1, 0, 1, 2, 3
P2S_JSON_DOC_TYPES = {4: 'list', 5: 'str', 6: 'int', 7: 'float', 8: 'bool', 9: 'NoneType'}    # P2S_JSON_DOC_LIST .. P2S_JSON_DOC_NULL
P2S_LSAP_MAX = 32
P2S_LSAP_ERRORS = {1: 'matrix contains invalid numeric entries', 2: 'cost matrix is infeasible'}   # scipy's messages
P2S_IDS_TOO_MANY = 4
P2S_ERR_SYNC_PADLEN = -10
P2S_REPROJ_DISTORTED = 1
P2S_TRACK_SELECTED, P2S_TRACK_NO_PEOPLE, P2S_TRACK_NO_CANDIDATE = 1, 0, 2
P2S_TRACK_LONG_LIST, P2S_TRACK_BAD_FILE, P2S_TRACK_BAD_CONTENT = -1, -2, -3
P2S_TRACK_MAX_CANDIDATES = 32
P2S_TRACK_MAX_SLOTS = 32   # person slots of p2s_track_persons_*: the rows of its state
P2S_TRACK_TILE = 32      # frames per tile of the map scan in csrc/p2s_extract.hip (T): tests place their cases around it
(P2S_JSON_PERSON_ALL_INTS, P2S_JSON_PERSON_HAS_NULL, P2S_JSON_PERSON_HAS_BOOL, P2S_JSON_PERSON_BIG_INT, P2S_JSON_PERSON_NOT_OBJECT,
 P2S_JSON_PERSON_BAD_LIST) = 1, 2, 4, 8, 16, 32
P2S_GAPS_KINDS = {None: 0, 'linear': 1, 'slinear': 2, 'quadratic': 3, 'cubic': 4}      # P2S_GAPS_KIND_*
P2S_GAPS_FILLS = {'last_value': 1, 'zeros': 2}                                            # P2S_GAPS_FILL_*; anything else: 0
P2S_GAPS_NONFINITE = 1
P2S_MEASURE_SPEED, P2S_MEASURE_ANGLES, P2S_MEASURE_RESTRICT, P2S_MEASURE_FEET_CONST, P2S_MEASURE_HEIGHT, P2S_MEASURE_LEG = 1, 2, 4, 8, 16, 32
P2S_MEASURE_ALL_SLOW, P2S_MEASURE_FEW_SMALL_ANGLES, P2S_MEASURE_ALL_DATA = 1, 2, 4
P2S_REFINE_TILE, P2S_REFINE_MAX_PARTS = 256, 128   # csrc/p2s_refine.hip: points a workgroup pass, partial sums a launch
P2S_RELPOSE_TILE, P2S_RELPOSE_MAX_CHUNKS, P2S_RELPOSE_MAX_PARTS = 256, 64, 128   # csrc/p2s_relpose.hip: points a pass, chunk sums, partial sums
P2S_RELPOSE_MIN_SAMPLE, P2S_RELPOSE_MAX_SAMPLE = 8, 16
P2S_FLOOR_TILE, P2S_FLOOR_MAX_CHUNKS, P2S_FLOOR_MAX_PARTS = 256, 64, 128   # csrc/p2s_floor.hip: points a pass, chunk sums, partial sums
P2S_MEASURE_ROLES =('RShoulder', 'LShoulder', 'RHip', 'LHip', 'Hip', 'Neck', 'RKnee', 'LKnee', 'RAnkle', 'LAnkle')


class TriParams(C.Structure):
    _fields_ = [('reproj_error_threshold', C.c_double),
                ('likelihood_threshold', C.c_double),
                ('min_cameras', C.c_int32),
                ('undistort_points', C.c_int32),
                ('handle_lr_swap', C.c_int32),
                ('reserved', C.c_int32)]


class AssocParams(C.Structure):
    _fields_ = [('reconstruction_error_threshold', C.c_double),
                ('min_affinity', C.c_double),
                ('min_cameras', C.c_int32),
                ('max_iter', C.c_int32),
                ('w_rank', C.c_double),
                ('tol', C.c_double),
                ('w_sparse', C.c_double)]


class SingleParams(C.Structure):
    _fields_ = [('reproj_error_threshold', C.c_double),
                ('likelihood_threshold', C.c_double),
                ('min_cameras', C.c_int32),
                ('reserved', C.c_int32)]


class RefineParams(C.Structure):
    _fields_ = [('lik_thr', C.c_double),
                ('huber_px', C.c_double),
                ('ftol', C.c_double),
                ('min_cams', C.c_int32),
                ('max_iter', C.c_int32)]


class RefineReport(C.Structure):
    _fields_ = [('cost_before', C.c_double),
                ('cost_after', C.c_double),
                ('lambda_final', C.c_double),
                ('kept_points', C.c_int64),
                ('iterations', C.c_int32),
                ('accepted', C.c_int32),
                ('held_coord', C.c_int32),
                ('reserved', C.c_int32),
                ('rms_before', C.c_double * P2S_MAX_CAMS),
                ('rms_after', C.c_double * P2S_MAX_CAMS)]


# name -> (restype, argtypes); every symbol include/p2s.h declares
SIGNATURES = {
    'p2s_version': (C.c_int, []),
    'p2s_last_error': (C.c_char_p, []),
    'p2s_device_count': (C.c_int, [C.POINTER(C.c_int)]),
    'p2s_create': (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    'p2s_destroy': (C.c_int, [C.c_void_p]),
    'p2s_set_stream': (C.c_int, [C.c_void_p, C.c_void_p]),
    'p2s_synchronize': (C.c_int, [C.c_void_p]),
    'p2s_set_calibration': (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 6),
    'p2s_triangulate_device': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.POINTER(TriParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'p2s_triangulate_host': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.POINTER(TriParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'p2s_associate_device': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.POINTER(AssocParams), C.c_void_p]),
    'p2s_associate_host': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.POINTER(AssocParams), C.c_void_p]),
    'p2s_associate_single_device': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.POINTER(SingleParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    'p2s_associate_single_host': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(SingleParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    'p2s_set_tuning': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    'p2s_get_tri_stats': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    'p2s_get_assoc_stats': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    'p2s_butterworth_host': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'p2s_filter_columns_host': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    'p2s_gcv_spline_host': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    'p2s_loess_host': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]),
    'p2s_sync_speeds_host': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    'p2s_lagged_pearson_host': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    'p2s_trc_metrics_host': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'p2s_reproject_host': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int64] + [C.c_void_p] * 6
                           + [C.c_int32, C.c_void_p, C.c_void_p]),
    'p2s_reproject_kernel_ms': (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    'p2s_write_openpose_files': (C.c_int, [C.c_char_p, C.c_void_p, C.c_char_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]),
    'p2s_column_order_stats_host': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    'p2s_jitter_host': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double]
                        + [C.c_void_p] * 7 + [C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]),
    'p2s_jitter_kernel_ms': (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    'p2s_json_select_tracked_person': (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    'p2s_column_mean_std_host': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'p2s_confidence_stats_host': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 5),
    'p2s_confidence_kernel_ms': (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    'p2s_lsap_host': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 4),
    'p2s_id_switch_host': (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 8),
    'p2s_id_switch_kernel_ms': (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    'p2s_track_select_host': (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 3 + [C.c_int32, C.c_double] + [C.c_void_p] * 3),
    'p2s_track_select_kernel_ms': (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    'p2s_track_persons_host': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                        C.c_double] + [C.c_void_p] * 9),
    'p2s_track_persons_device': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                          C.c_double] + [C.c_void_p] * 9),
    'p2s_track_persons_kernel_ms': (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    'p2s_interpolate_gaps': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_void_p]),
    'p2s_fill_gaps': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    'p2s_gap_runs': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_int64, C.c_void_p,
                               C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    'p2s_gaps_kernel_ms': (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    'p2s_timeline_rows_host': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                        C.c_int64] + [C.c_void_p] * 9),
    'p2s_timeline_kernel_ms': (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    'p2s_timeline_write_csv': (C.c_int, [C.c_char_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int32, C.c_char_p, C.c_void_p, C.c_int32]),
    'p2s_refine_extrinsics_host': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 5 + [C.POINTER(RefineParams)]
                                   + [C.c_void_p] * 3 + [C.POINTER(RefineReport)]),
    'p2s_refine_kernel_ms': (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    'p2s_refine_held_coord': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    'p2s_relative_poses_host': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 12),
    'p2s_relpose_kernel_ms': (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    'p2s_json_person_flags': (C.c_int, [C.c_void_p, C.c_void_p]),
    'p2s_write_person_files': (C.c_int, [C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    'p2s_find_peaks_host': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64]
                            + [C.c_void_p] * 5 + [C.POINTER(C.c_int64)]),
    'p2s_gait_contacts_host': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64] + [C.c_void_p] * 5
                               + [C.c_int32, C.c_int32] + [C.c_void_p] * 3 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64]
                               + [C.c_void_p] * 5),
    'p2s_gait_kernel_ms': (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    'p2s_stable_argsort_host': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    'p2s_trimmed_means_host': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]),
    'p2s_body_measure_host': (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 5 + [C.c_int32] + [C.c_void_p] * 4
                              + [C.c_double] * 3 + [C.c_void_p] * 10),
    'p2s_measure_kernel_ms': (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    'p2s_json_person_ids': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'p2s_timing_begin': (C.c_int, [C.c_void_p]),
    'p2s_timing_end': (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    'p2s_json_parse': (C.c_int, [C.c_char_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]),
    'p2s_json_free': (C.c_int, [C.c_void_p]),
    'p2s_json_people_counts': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'p2s_json_person_lengths': (C.c_int, [C.c_void_p, C.c_void_p]),
    'p2s_json_gather_keypoints': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                            C.c_int32, C.c_void_p, C.POINTER(C.c_int64)]),
    'p2s_json_gather_largest_person': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_void_p]),
    'p2s_copy_files': (C.c_int, [C.c_char_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    'p2s_json_gather_people': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                         C.c_void_p, C.POINTER(C.c_int64)]),
    'p2s_assoc_argmax_rows': (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    'p2s_assoc_unique_rows': (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    'p2s_assoc_filter_rows': (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    'p2s_json_rewrite_people': (C.c_int, [C.c_char_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_int32, C.c_void_p]),
    'p2s_trc_append_rows': (C.c_int, [C.c_char_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    'p2s_format_float_repr': (C.c_int, [C.c_double, C.c_char_p, C.c_int32]),
    'p2s_tri_geometry': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int32)]),
}

# the same for include/p2s_floor.h, the floor stage's header
FLOOR_SIGNATURES = {
    'p2s_fit_planes_host': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
                            + [C.c_void_p] * 12),
    'p2s_floor_kernel_ms': (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
}

# and for include/p2s_tri_frames.h, triangulation with per-frame cameras
TRI_FRAMES_SIGNATURES = {
    'p2s_triangulate_frames_device': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                                C.c_void_p, C.c_void_p, C.POINTER(TriParams), C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p]),
    'p2s_triangulate_frames_host': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                              C.c_void_p, C.c_void_p, C.POINTER(TriParams), C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
}

# entry points a library built before them lacks (P2S_LIB may name one): left unbound, and the feature is refused
OPTIONAL = {'p2s_gcv_spline_host', 'p2s_sync_speeds_host', 'p2s_lagged_pearson_host', 'p2s_json_gather_largest_person',
            'p2s_copy_files', 'p2s_reproject_host', 'p2s_reproject_kernel_ms', 'p2s_write_openpose_files',
            'p2s_column_order_stats_host', 'p2s_jitter_host', 'p2s_jitter_kernel_ms', 'p2s_json_select_tracked_person',
            'p2s_column_mean_std_host', 'p2s_confidence_stats_host', 'p2s_confidence_kernel_ms', 'p2s_lsap_host',
            'p2s_id_switch_host', 'p2s_id_switch_kernel_ms', 'p2s_json_person_ids', 'p2s_loess_host',
            'p2s_find_peaks_host', 'p2s_gait_contacts_host', 'p2s_gait_kernel_ms', 'p2s_stable_argsort_host',
            'p2s_trimmed_means_host', 'p2s_body_measure_host', 'p2s_measure_kernel_ms', 'p2s_track_select_host',
            'p2s_track_select_kernel_ms', 'p2s_json_person_flags', 'p2s_write_person_files', 'p2s_track_persons_host',
            'p2s_track_persons_device', 'p2s_track_persons_kernel_ms', 'p2s_interpolate_gaps', 'p2s_fill_gaps', 'p2s_gap_runs',
            'p2s_gaps_kernel_ms', 'p2s_timeline_rows_host', 'p2s_timeline_kernel_ms', 'p2s_timeline_write_csv',
            'p2s_refine_extrinsics_host', 'p2s_refine_kernel_ms', 'p2s_refine_held_coord', 'p2s_relative_poses_host',
            'p2s_relpose_kernel_ms', 'p2s_fit_planes_host', 'p2s_floor_kernel_ms', 'p2s_triangulate_frames_host',
            'p2s_triangulate_frames_device'}

_lib = None


class P2sError(RuntimeError):
    pass


def load():
    """Load libp2s_hip.so and bind every entry point; raises if the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise P2sError(f'{LIB_PATH} is missing: run `python -c "import __graft_entry__ as g; g.build()"` '
                       '(hipcc --offload-arch=gfx950). There is no CPU fallback.')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in {**SIGNATURES, **FLOOR_SIGNATURES, **TRI_FRAMES_SIGNATURES}.items():
        if name in OPTIONAL and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().p2s_last_error()
        raise P2sError(f'p2s error {rc}: {msg.decode() if msg else "?"}')


def device_count():
    n = C.c_int(0)
    check(load().p2s_device_count(C.byref(n)))
    return n.value
