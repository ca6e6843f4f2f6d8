"""ctypes binding of libpyslam_hip.so (C ABI: include/pyslam_hip.h).

There is NO CPU fallback: ``load()`` raises if the library has not been built
and ``DeviceProblem`` raises if no MI355X is visible.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libpyslam_hip.so')
if os.environ.get('PYSLAM_AMD_MEASURE') == '1':       # tools/: the -DPS_MEASURE build (__graft_entry__.build_measure())
    LIB_PATH = os.path.join(_HERE, 'lib', 'libpyslam_hip_measure.so')

c_i32p = C.POINTER(C.c_int32)
c_f64p = C.POINTER(C.c_double)
c_u8p = C.POINTER(C.c_uint8)
PS_NUM_STAGES = 12
STAGE_NAMES = ['landmark_pass', 'pose_pass', 'schur_pairs', 'pose_factors', 'pcg',
               'backsub', 'update', 'cost', 'iteration_total', 'cg_kernel', 'allreduce', 'pack_unpack']


class ProblemDesc(C.Structure):
    _fields_ = [
        ('dof', C.c_int32), ('num_poses', C.c_int32), ('poses', c_f64p), ('pose_rid', c_i32p),
        ('num_points', C.c_int32), ('points', c_f64p), ('point_vid', c_i32p),
        ('num_obs', C.c_int64), ('obs_pose', c_i32p), ('obs_point', c_i32p), ('obs_uvd', c_f64p),
        ('obs_grp', c_i32p),
        ('num_cams', C.c_int32), ('cams', c_f64p), ('num_stiff3', C.c_int32), ('stiff3', c_f64p),
        ('num_obs_groups', C.c_int32), ('obs_groups', c_f64p),
        ('num_edges', C.c_int64), ('e_i', c_i32p), ('e_j', c_i32p), ('e_Tobs_inv', c_f64p), ('e_grp', c_i32p),
        ('num_priors', C.c_int64), ('u_i', c_i32p), ('u_Tobs_inv', c_f64p), ('u_grp', c_i32p),
        ('num_stiffd', C.c_int32), ('stiffd', c_f64p), ('num_edge_groups', C.c_int32), ('edge_groups', c_f64p),
        ('num_extra_pairs', C.c_int64), ('extra_pair_i', c_i32p), ('extra_pair_j', c_i32p),
        ('flags', C.c_uint32),
    ]


PS_DESC_DEVICE_PARAMS, PS_DESC_DEVICE_TABLES = 1, 2


class HostRowsDesc(C.Structure):
    _fields_ = [('num', C.c_int64), ('i', c_i32p), ('j', c_i32p)]


class SolveOptions(C.Structure):
    _fields_ = [('max_iters', C.c_int32), ('allow_nondecreasing_steps', C.c_int32), ('max_nondecreasing_steps', C.c_int32),
                ('linesearch', C.c_int32), ('min_update_norm', C.c_double), ('min_cost', C.c_double),
                ('min_cost_decrease', C.c_double), ('lm_lambda', C.c_double)]


class LmOptions(C.Structure):           # ps_lm_options: 72 bytes
    _fields_ = SolveOptions._fields_ + [('lambda0', C.c_double), ('lambda_min', C.c_double), ('lambda_max', C.c_double)]


class ProblemInfo(C.Structure):
    _fields_ = [
        ('dof', C.c_int32), ('num_poses', C.c_int32), ('num_reduced', C.c_int32),
        ('num_points', C.c_int32), ('num_var_points', C.c_int32),
        ('num_obs', C.c_int64), ('num_edges', C.c_int64), ('num_priors', C.c_int64),
        ('reduced_nnzb', C.c_int64), ('num_pairs', C.c_int64), ('reduce_count', C.c_int64),
        ('device_bytes', C.c_int64), ('cg_restarts', C.c_int64), ('cg_kernel_launches', C.c_int64),
        ('ldi_solves', C.c_int64), ('ldi_fallbacks', C.c_int64), ('ldi_seeds', C.c_int64),
        ('xcg_fused_solves', C.c_int64), ('xcg_fused_fallbacks', C.c_int64),
        ('cg_persist_solves', C.c_int64), ('cg_persist_failures', C.c_int64), ('cg_persist_refused', C.c_int64),
        ('persist_cus', C.c_int32), ('persist_cus_needed', C.c_int32), ('landmark_passes_taken_over', C.c_int64),
    ]


class PhotoDesc(C.Structure):
    _fields_ = [
        ('num_pixels', C.c_int32), ('pt_ref', c_f64p), ('im_ref', c_f64p), ('im_jac', c_f64p), ('tri_jac_d', c_f64p),
        ('height', C.c_int32), ('width', C.c_int32), ('im_track', c_f64p),
        ('cam', C.c_double * 5), ('cam_type', C.c_int32), ('cam_w', C.c_int32), ('cam_h', C.c_int32),
        ('intensity_covar', C.c_double), ('depth_covar', C.c_double), ('loss_id', C.c_int32), ('loss_k', C.c_double),
    ]


class FeatParams(C.Structure):
    _fields_ = [('response_threshold', C.c_int64), ('nms_n', C.c_int32), ('max_features', C.c_int32),
                ('match_radius_u', C.c_int32), ('match_radius_v', C.c_int32), ('disp_max', C.c_int32),
                ('match_cost_max', C.c_int32), ('refinement', C.c_int32), ('reserved', C.c_int32)]


# every symbol include/pyslam_hip.h declares: name -> (restype, argtypes)
H = C.c_void_p
SIGNATURES = {
    'ps_last_error': (C.c_char_p, []),
    'ps_device_count': (C.c_int, []),
    'ps_warm_up': (C.c_int, []),
    'ps_problem_create': (C.c_int, [C.POINTER(ProblemDesc), C.c_void_p, C.POINTER(H)]),
    'ps_problem_create_hybrid': (C.c_int, [C.POINTER(ProblemDesc), C.POINTER(HostRowsDesc), C.c_void_p, C.POINTER(H)]),
    'ps_set_host_rows': (C.c_int, [H, c_f64p, C.c_int64, C.c_double]),
    'ps_problem_destroy': (C.c_int, [H]),
    'ps_get_info': (C.c_int, [H, C.POINTER(ProblemInfo)]),
    'ps_eval_cost': (C.c_int, [H, C.c_int, c_f64p]),
    'ps_linearize': (C.c_int, [H, C.c_double]),
    'ps_reduce_buffer': (C.c_int, [H, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    'ps_shard_pack': (C.c_int, [H]),
    'ps_shard_unpack': (C.c_int, [H]),
    'ps_solve_reduced': (C.c_int, [H, C.c_double, C.c_int, C.POINTER(C.c_int), c_f64p]),
    'ps_backsub': (C.c_int, [H]),
    'ps_get_dx': (C.c_int, [H, c_f64p, c_f64p]),
    'ps_step_norm2': (C.c_int, [H, c_f64p]),
    'ps_apply_update': (C.c_int, [H, C.c_double]),
    'ps_snapshot_params': (C.c_int, [H]),
    'ps_restore_params': (C.c_int, [H]),
    'ps_reset_solver_state': (C.c_int, [H]),
    'ps_build_sha': (C.c_char_p, []),
    'ps_get_params': (C.c_int, [H, c_f64p, c_f64p]),
    'ps_set_params': (C.c_int, [H, c_f64p, c_f64p]),
    'ps_motion_only_solve': (C.c_int, [H, C.POINTER(SolveOptions), c_f64p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                       C.POINTER(C.c_double), c_f64p]),
    'ps_solve': (C.c_int, [H, C.POINTER(SolveOptions), C.c_double, C.c_int, c_f64p, C.c_int32, C.POINTER(C.c_int32),
                           C.POINTER(C.c_int32), C.POINTER(C.c_double), c_i32p, c_f64p, c_f64p]),
    'ps_gn_iteration': (C.c_int, [H, C.c_double, C.c_double, C.c_int, C.c_int, c_f64p, c_f64p,
                                  C.POINTER(C.c_int), c_f64p]),
    'ps_lm_iteration': (C.c_int, [H, C.c_double, C.c_double, C.c_int, C.c_int, c_f64p, c_f64p, c_f64p,
                                  C.POINTER(C.c_int), c_f64p]),
    'ps_solve_lm': (C.c_int, [H, C.POINTER(LmOptions), C.c_double, C.c_int, c_f64p, C.c_int32, C.POINTER(C.c_int32),
                              C.POINTER(C.c_int32), C.POINTER(C.c_double), c_i32p, c_f64p, c_f64p, c_f64p]),
    'ps_gn_finish': (C.c_int, [H, C.c_int, c_f64p, c_f64p, c_f64p]),
    'ps_gn_solve_finish': (C.c_int, [H, C.c_double, C.c_int, C.c_int, c_f64p, c_f64p, c_f64p,
                                     C.POINTER(C.c_int), c_f64p]),
    'ps_set_collective': (C.c_int, [H, C.c_void_p, C.c_void_p]),
    'ps_set_segment_exchange': (C.c_int, [H, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.c_int64,
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'ps_shard_buffer': (C.c_int, [H, C.POINTER(C.c_void_p)]),
    'ps_gn_solve_finish_enqueue': (C.c_int, [H, C.c_double, C.c_int, C.c_int, C.c_int]),
    'ps_gn_result': (C.c_int, [H, C.POINTER(C.c_int), c_f64p, c_f64p, C.POINTER(C.c_int), c_f64p]),
    'ps_covariance_begin': (C.c_int, [H]),
    'ps_covariance_column': (C.c_int, [H, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_int), c_f64p]),
    'ps_covariance_marginals': (C.c_int, [H, c_f64p, c_f64p]),
    'ps_covariance_pose_blocks': (C.c_int, [H, C.c_int64, c_i32p, c_i32p, c_f64p]),
    'ps_covariance_cross_blocks': (C.c_int, [H, C.c_int64, c_i32p, c_i32p, c_i32p, c_i32p, c_f64p]),
    'ps_triangulate': (C.c_int, [H, C.c_int64, c_i32p, C.c_int, C.c_double, C.c_int, c_f64p, c_i32p]),
    'ps_get_reduced_system': (C.c_int, [H, c_i32p, c_i32p, c_f64p, c_f64p]),
    'ps_get_landmark_factors': (C.c_int, [H, c_f64p, c_f64p]),
    'ps_debug_reproj_blocks': (C.c_int, [H, c_f64p, c_f64p, c_f64p]),
    'ps_debug_factor_blocks': (C.c_int, [H, c_f64p, c_f64p, c_f64p]),
    'ps_debug_table_checksums': (C.c_int, [H, C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_int)]),
    'ps_debug_packed_runs': (C.c_int, [H, c_i32p, C.c_int32, c_i32p, c_i32p, c_i32p, c_f64p]),
    'ps_debug_pose_items': (C.c_int, [H, c_i32p, C.c_int32, c_i32p, c_f64p]),
    'ps_set_option': (C.c_int, [H, C.c_char_p, C.c_double]),
    'ps_get_option': (C.c_int, [H, C.c_char_p, c_f64p]),
    'ps_set_profiling': (C.c_int, [H, C.c_int]),
    'ps_get_stage_times': (C.c_int, [H, c_f64p, C.POINTER(C.c_int64), C.c_int]),
    'ps_ransac_transforms': (C.c_int, [c_f64p, c_f64p, C.c_int32, C.c_int32, c_f64p]),
    'ps_ransac_cost': (C.c_int, [c_f64p, C.c_int32, c_f64p, c_f64p, C.c_int32, c_f64p, C.c_double, c_u8p, c_i32p]),
    'ps_ransac_frame_to_frame': (C.c_int, [c_f64p, c_f64p, c_f64p, C.c_int32, c_i32p, C.c_int32, C.c_int32, c_f64p,
                                           C.c_double, c_f64p, c_i32p, c_i32p, c_i32p, c_f64p, c_u8p]),
    'ps_twoview_hypotheses': (C.c_int, [c_f64p, c_f64p, C.c_int32, c_i32p, C.c_int32, c_f64p, C.c_double, c_f64p, c_i32p, c_u8p]),
    'ps_twoview_score': (C.c_int, [c_f64p, C.c_int32, c_f64p, c_f64p, C.c_int32, c_f64p, C.c_double, c_u8p, c_i32p]),
    'ps_twoview_ransac': (C.c_int, [c_f64p, c_f64p, C.c_int32, c_i32p, C.c_int32, c_f64p, C.c_double, C.c_int32, c_f64p, c_f64p,
                                    c_u8p, c_i32p, c_f64p]),
    'ps_pnp_hypotheses': (C.c_int, [c_f64p, c_f64p, C.c_int32, c_i32p, C.c_int32, c_f64p, C.c_double, c_f64p, c_i32p, c_u8p]),
    'ps_pnp_score': (C.c_int, [c_f64p, C.c_int32, c_f64p, c_f64p, C.c_int32, c_f64p, C.c_double, c_u8p, c_i32p]),
    'ps_pnp_ransac': (C.c_int, [c_f64p, c_f64p, C.c_int32, c_i32p, C.c_int32, c_f64p, C.c_double, C.c_int32, c_f64p, c_u8p, c_i32p,
                                c_f64p, c_f64p]),
    'ps_sim3_hypotheses': (C.c_int, [c_f64p, c_f64p, c_f64p, c_f64p, C.c_int32, c_i32p, C.c_int32, c_f64p, C.c_double, C.c_int32,
                                     c_f64p, c_f64p, c_i32p, c_u8p]),
    'ps_sim3_score': (C.c_int, [c_f64p, C.c_int32, c_f64p, c_f64p, c_f64p, c_f64p, C.c_int32, c_f64p, C.c_double, c_u8p, c_i32p]),
    'ps_sim3_ransac': (C.c_int, [c_f64p, c_f64p, c_f64p, c_f64p, C.c_int32, c_i32p, C.c_int32, c_f64p, C.c_double, C.c_int32, C.c_int32,
                                 c_f64p, c_f64p, c_u8p, c_i32p, c_f64p]),
    'ps_sim3pg_create': (C.c_int, [C.c_int32, c_f64p, c_u8p, C.c_int32, c_i32p, c_i32p, c_f64p, c_f64p, C.c_int32, C.c_double, C.c_void_p,
                                   C.POINTER(H)]),
    'ps_sim3pg_destroy': (C.c_int, [H]),
    'ps_sim3pg_set_vertices': (C.c_int, [H, c_f64p]),
    'ps_sim3pg_get_vertices': (C.c_int, [H, c_f64p]),
    'ps_sim3pg_eval_cost': (C.c_int, [H, c_f64p]),
    'ps_sim3pg_linearize': (C.c_int, [H, C.c_double, c_f64p, c_f64p, c_f64p]),
    'ps_sim3pg_iteration': (C.c_int, [H, C.c_double, c_f64p, c_f64p, c_f64p]),
    'ps_sim3pg_solve': (C.c_int, [H, C.POINTER(SolveOptions), c_f64p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_double)]),
    'ps_sim3pg_debug_edges': (C.c_int, [H, c_f64p]),
    'ps_sim3pg_debug_explog': (C.c_int, [C.c_int32, c_f64p, c_f64p, c_f64p, c_f64p]),
    'ps_sim3pg_profile': (C.c_int, [H, C.c_int32, c_f64p]),
    'ps_photometric_create': (C.c_int, [C.POINTER(PhotoDesc), C.c_void_p, C.POINTER(H)]),
    'ps_photometric_destroy': (C.c_int, [H]),
    'ps_photometric_set_pose': (C.c_int, [H, c_f64p]),
    'ps_photometric_get_pose': (C.c_int, [H, c_f64p]),
    'ps_photometric_eval_cost': (C.c_int, [H, c_f64p, C.POINTER(C.c_int64)]),
    'ps_photometric_normal_equations': (C.c_int, [H, c_f64p, c_f64p, c_f64p, C.POINTER(C.c_int64)]),
    'ps_photometric_iteration': (C.c_int, [H, C.c_int32, C.c_int32, c_f64p, c_f64p]),
    'ps_dense_create': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(H)]),
    'ps_dense_destroy': (C.c_int, [H]),
    'ps_dense_upload': (C.c_int, [H, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, c_f64p]),
    'ps_dense_make_tables': (C.c_int, [H, C.c_int32, C.c_int32, c_i32p, c_f64p, C.c_double, C.c_double, C.c_double]),
    'ps_dense_track': (C.c_int, [H, C.c_int32, C.c_int32, C.c_int32, c_i32p, c_i32p, C.POINTER(SolveOptions), C.c_int32,
                                 C.c_double, c_f64p, c_f64p, c_i32p, c_f64p, C.c_int32]),
    'ps_dense_level_shape': (C.c_int, [H, C.c_int32, c_i32p, c_i32p]),
    'ps_dense_read_level': (C.c_int, [H, C.c_int32, C.c_int32, C.c_int32, c_f64p]),
    'ps_dense_num_pixels': (C.c_int, [H, C.c_int32, C.c_int32, c_i32p]),
    'ps_dense_read_tables': (C.c_int, [H, C.c_int32, C.c_int32, C.c_int32, c_f64p, c_f64p, c_f64p, c_f64p]),
    'ps_dense_device_bytes': (C.c_int, [H, C.POINTER(C.c_int64)]),
    'ps_feat_create': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(H)]),
    'ps_feat_destroy': (C.c_int, [H]),
    'ps_feat_push': (C.c_int, [H, C.c_int32, C.c_int32, c_u8p, c_u8p]),
    'ps_feat_match': (C.c_int, [H, C.c_int32, C.POINTER(FeatParams), c_i32p]),
    'ps_feat_read_matches': (C.c_int, [H, C.c_int32, c_f64p, c_i32p]),
    'ps_feat_read_features': (C.c_int, [H, C.c_int32, C.c_int32, c_i32p, c_i32p, C.POINTER(C.c_int64), c_u8p]),
    'ps_feat_set_map': (C.c_int, [H, C.c_int32, c_f64p, c_u8p]),
    'ps_feat_match_map': (C.c_int, [H, c_f64p, c_f64p, C.c_int32, C.POINTER(FeatParams), c_i32p]),
    'ps_feat_read_map_matches': (C.c_int, [H, C.c_int32, c_i32p, c_i32p, c_i32p, c_f64p]),
    'ps_feat_match_map_global': (C.c_int, [H, C.c_int32, C.c_int32, C.POINTER(FeatParams), c_i32p]),
    'ps_feat_read_map_second': (C.c_int, [H, C.c_int32, c_i32p]),
    'ps_feat_db_add': (C.c_int, [H, C.c_int32, c_u8p, c_i32p]),
    'ps_feat_db_clear': (C.c_int, [H]),
    'ps_feat_db_size': (C.c_int, [H, c_i32p, C.POINTER(C.c_int64)]),
    'ps_feat_db_query': (C.c_int, [H, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(FeatParams), c_i32p]),
    'ps_feat_feature_passes': (C.c_int, [H, C.POINTER(C.c_int64)]),
    'ps_feat_device_bytes': (C.c_int, [H, C.POINTER(C.c_int64)]),
    'ps_dense_normal_solve': (C.c_int, [c_f64p, c_f64p, C.c_int32, C.c_int32, c_f64p, c_f64p]),
    'ps_sparse_normal_solve': (C.c_int, [C.c_int32, C.c_int32, c_i32p, c_i32p, c_f64p, c_i32p, c_i32p, c_f64p, c_f64p, c_f64p,
                                         C.c_double, C.c_int32, c_f64p, c_i32p, c_f64p]),
    'ps_sparse_normal_direct': (C.c_int, [C.c_int32, C.c_int32, c_i32p, c_i32p, c_f64p, c_i32p, c_i32p, c_f64p, c_f64p, c_f64p,
                                          C.c_int32, c_f64p, c_f64p]),
    'ps_debug_band_inverse': (C.c_int, [c_f64p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), c_f64p]),
    'ps_debug_coarse_chol': (C.c_int, [c_f64p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_f64p, c_f64p, c_i32p, c_f64p]),
    'ps_debug_coarse_chol_clocks': (C.c_int, [c_f64p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_f64p]),
    'ps_debug_dense_factor': (C.c_int, [c_f64p, C.c_int32, C.c_int32, c_f64p, c_f64p, c_f64p, c_f64p, C.POINTER(C.c_float), c_i32p, c_f64p]),
    'ps_debug_bchol_slab': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, c_i32p, c_i32p, c_i32p, c_i32p]),
    'ps_debug_ldi_gemm': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_float, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_float), C.c_int32,
                                    C.c_float, C.POINTER(C.c_float), C.c_int32, C.c_float, C.POINTER(C.c_float), C.c_int32, c_i32p, C.c_int32,
                                    C.POINTER(C.c_float), C.c_double, c_f64p]),
    'ps_debug_ldi_ritz': (C.c_int, [c_f64p, c_f64p, C.c_int32, C.POINTER(C.c_float)]),
    'ps_debug_ldi_read': (C.c_int, [H, C.c_int32, c_f64p, C.c_int64]),
    'ps_debug_factor_stress': (C.c_int, [c_f64p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_i32p, c_i32p]),
}

_lib = None


class NativeError(RuntimeError):
    pass


def _share_torch_hip_runtime():
    """PyTorch-ROCm ships its own libamdhip64.so.7; the core links /opt/rocm's under the same soname.  Whichever is
    loaded first serves both (the dynamic loader dedups by soname), and torch on top of ROCm's copy finds no GPU
    ("ProcessGroupNCCL is only supported with GPUs").  So when torch is installed its runtime goes in first -- without
    importing torch: the multi-GPU driver and callers' own torch code keep working whatever the import order."""
    import sys
    if 'torch' in sys.modules:
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec('torch')
        if spec is None or not spec.submodule_search_locations:
            return
        path = os.path.join(list(spec.submodule_search_locations)[0], 'lib', 'libamdhip64.so')
        if os.path.exists(path):
            C.CDLL(path, mode=C.RTLD_GLOBAL)
    except Exception:       # noqa: BLE001  (best effort: without it the core still runs on ROCm's runtime)
        pass


_CREATE_ENV = {'PS_CREATE_DEVICE', 'PS_CREATE_KEYS64', 'PS_PAIRS_BY_LANDMARK',
               'PS_SCHUR_TILE_KB', 'PS_SCHUR_TILE_MIN_MB'}       # ps_create_env(): read by every build


# ps_env(): the measurement / debugging switches of the -DPS_MEASURE build (tests/test_host_api.py holds this list against the sources)
_MEASURE_ENV = {'PS_ALLOC_GUARD', 'PS_ARENA_POISON', 'PS_BAND_INV_DOT', 'PS_CP_CLOCKS', 'PS_CREATE_TIMING', 'PS_DIRECT_3LAUNCH',
                'PS_DIRECT_THREADS', 'PS_EVENT_FLAGS', 'PS_F2_ABLATE', 'PS_F2_ROWS', 'PS_HOST_TIMING', 'PS_LAZY_COARSE', 'PS_LDI_SEED_LAG',
                'PS_POSE_CHUNK', 'PS_RS_ABLATE', 'PS_SCALE_NO_PIPE', 'PS_SCHUR_KEEP_TILES', 'PS_SCHUR_LDS_PAD', 'PS_SCHUR_NO_LPT',
                'PS_SCHUR_SPLIT', 'PS_SIDE_CUS', 'PS_SIDE_DELAY', 'PS_SIDE_KICK', 'PS_SIDE_LOWPRIO', 'PS_XCG_ACDONE_LATE', 'PS_XCG_AC_CHECK', 'PS_XCG_AC_MAIN', 'PS_XCG_AC_WAIT', 'PS_XCG_INV_SUM', 'PS_XCG_SIDE_PAD', 'PS_XCG_ROWS_RT', 'PS_XF2_PF', 'PS_XP_CLOCKS'}


def load():
    """dlopen the HIP core; raise loudly if it is missing (no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            "{} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). pyslam_amd has no CPU solver path.".format(LIB_PATH))
    _share_torch_hip_runtime()
    if os.environ.get('PYSLAM_AMD_MEASURE') != '1':
        # the product library compiles the measurement / debugging switches out (csrc/ps_core.hip: ps_env): say so once instead of
        # silently ignoring a variable somebody set (round-4 ADVICE).  The create-time variants below ARE read by it.
        # (only the switches the sources know: procps' PS_FORMAT / PS_PERSONALITY and the like are none of our business)
        ignored = sorted(k for k in os.environ if k in _MEASURE_ENV)
        if ignored:
            import sys
            sys.stderr.write('pyslam_amd: {} ignored by the product library (measurement switches exist only in the -DPS_MEASURE '
                             'build: PYSLAM_AMD_MEASURE=1)\n'.format(', '.join(ignored)))
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise NativeError(load().ps_last_error().decode('utf-8', 'replace'))


def is_resident(a):
    """A torch tensor living in HBM (the C ABI takes its address: ps_problem_desc.flags, ps_set_params, ps_get_params)."""
    return hasattr(a, 'data_ptr') and getattr(a, 'is_cuda', False)


def _resident_ptr(a, ctype, dtype_name):
    if not a.is_contiguous() or str(a.dtype) != 'torch.' + dtype_name:
        raise TypeError('device-resident tables must be contiguous {} tensors'.format(dtype_name))
    return C.cast(C.c_void_p(a.data_ptr()), ctype)


def f64p(a):
    if a is None:
        return None
    return _resident_ptr(a, c_f64p, 'float64') if is_resident(a) else a.ctypes.data_as(c_f64p)


def i32p(a):
    if a is None:
        return None
    return _resident_ptr(a, c_i32p, 'int32') if is_resident(a) else a.ctypes.data_as(c_i32p)


_warm = False


def require_gpu():
    global _warm
    lib = load()
    if lib.ps_device_count() < 1:
        raise NativeError("no HIP device visible: pyslam_amd solves only on an MI355X (no CPU fallback)")
    if not _warm:           # the process-wide one-off costs (code-object load, allocator set-up) here, not in the first solve
        check(lib.ps_warm_up())
        _warm = True
    return lib
